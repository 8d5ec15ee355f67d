"""Float64 NumPy restatement of the Monte Carlo predictive mixture (include/iwvi_hip.h: iwvi_lik_predict_mixture).  TEST INFRASTRUCTURE
ONLY (tests/test_predict_mixture_host.py pins it against a brute-force evaluation; tests/test_gpu_predict_mixture.py compares the HIP
kernels with it).

Per test point n over its S draws s, with (E_s, Var_s) = predict_mean_and_var and predict_density of the likelihood at draw s:
  log_density[n] = logsumexp_s( sum_d predict_density(m_snd, v_snd, Y[n, d]) ) - log S
  mean[n, d]     = (1/S) sum_s E_s[y_d]
  var[n, d]      = (1/S) sum_s (Var_s[y_d] + E_s[y_d]^2) - mean[n, d]^2
The per-draw callables are the existing restatements' (lik_restatement, multiclass_restatement, explink_restatement); the Gaussian is
written out.  Moments are [S, N, Dy] (draw-major, as predict_f_multisample returns them), Y [N, Dy] -- [N, 1] labels for MultiClass."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import explink_restatement as XR   # noqa: E402
import lik_restatement as R   # noqa: E402
import multiclass_restatement as MR   # noqa: E402

U = 2.0 ** -24                                                   # the unit roundoff of float32


class Gaussian:
    name = "gaussian"

    def __init__(self, variance=1.0):
        self.variance = float(variance)

    def predict_density(self, Fmu, Fvar, Y):
        Fmu, Fvar, Y = R._t(Fmu), R._t(Fvar), R._t(Y)
        s = Fvar + self.variance
        return -0.5 * torch.log(2.0 * math.pi * s) - 0.5 * (Y - Fmu) ** 2 / s

    def predict_mean_and_var(self, Fmu, Fvar):
        return R._t(Fmu), R._t(Fvar) + self.variance


def make(kind, **kw):
    """The float64 likelihood of a kind: gaussian / bernoulli / student_t / multiclass / poisson / exponential / gamma."""
    if kind == "gaussian":
        return Gaussian(**kw)
    if kind == "bernoulli":
        return R.Bernoulli()
    if kind == "student_t":
        return R.StudentT(**kw)
    if kind == "multiclass":
        return MR.MultiClass(**kw)
    return XR.make(kind, **kw)


def draw_log_density(ref, m, v, Y):
    """[S, N]: sum_d predict_density of every draw (m, v [S, N, Dy]; Y [N, Dy], or [N, 1] labels)."""
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    Ys = np.broadcast_to(np.asarray(Y, dtype=np.float64), (m.shape[0],) + tuple(np.shape(Y))).copy()
    return ref.predict_density(m, v, Ys).sum(-1).numpy()


def lse_mean(lp):
    """[N]: logsumexp over axis 0 minus log S; -inf where every draw is -inf."""
    lp = np.asarray(lp, dtype=np.float64)
    mx = lp.max(0)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(divide="ignore"):
        return safe + np.log(np.exp(lp - safe).sum(0)) - math.log(lp.shape[0])


def mixture(ref, m, v, Y=None):
    """dict(mean [N, Dy], var [N, Dy][, log_density [N]]) in float64; also 'E' and 'V' [S, N, Dy], the per-draw moments (the tolerance of
    var is written in terms of max_s |E_s|)."""
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    E, V = (a.numpy() for a in ref.predict_mean_and_var(m, v))
    mean = E.mean(0)
    out = {"mean": mean, "var": (V + E ** 2).mean(0) - mean ** 2, "E": E, "V": V}
    if Y is not None:
        out["log_density"] = lse_mean(draw_log_density(ref, m, v, Y))
    return out


def lse_float32(lp32, seg):
    """The device's reduction in plain float32 NumPy on float32 per-draw values lp32 [S, N]: chunks of ``seg`` draws, shift by the running
    float32 maximum, float32 exp, float64 sum -- what tests/test_gpu_predict_mixture.py measures the float32 exp term with."""
    lp32 = np.asarray(lp32, dtype=np.float32)
    S, N = lp32.shape
    m = np.full(N, -np.inf, dtype=np.float32)
    ssum = np.zeros(N, dtype=np.float64)
    for s0 in range(0, S, seg):
        c = lp32[s0:s0 + seg]
        nm = np.maximum(m, c.max(0))
        with np.errstate(invalid="ignore"):
            cs = np.where(np.isfinite(nm), np.exp((c - nm).astype(np.float32)).astype(np.float64).sum(0), 0.0)
            ssum = np.where(np.isfinite(m), ssum * np.exp((m - nm).astype(np.float32)).astype(np.float64), 0.0) + cs
        m = nm
    with np.errstate(divide="ignore"):
        return (m.astype(np.float64) + np.log(ssum) - math.log(S)).astype(np.float32)
