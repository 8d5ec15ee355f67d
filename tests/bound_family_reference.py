"""Float64 statement of the bound family between the K-sample ELBO and the importance-weighted bound (csrc/bound_family.hip; Rainforth et al.
2018, Li & Turner 2016): one triple (groups G, tau, beta), K_g = K / G, group g = the contiguous samples g K_g .. (g + 1) K_g - 1,

    bound_n = beta (1/K) sum_k L_nk + (1 - beta) (1/G) sum_g (1/tau) [ logsumexp_{k in g}(tau L_nk) - log K_g ]
    w_nk    = beta / K + (1 - beta) / G softmax_{k' in group(k)}(tau L_nk')_k
    ess_n   = (sum_k e^(L_nk - m))^2 / sum_k e^(2 (L_nk - m))                         (all K samples, whatever the triple)

and the Gaussian heads under these weights.  TEST INFRASTRUCTURE ONLY: tests/test_bound_family_reference_host.py pins it against float64
autograd and against tests/iw_reduction_reference.py at the special cases; tests/test_gpu_bound_family.py and tests/test_gpu_bound_model.py
compare the HIP kernels and the model with it.  ``L`` is [B, K] NumPy float64; ``tau`` and ``beta`` are used as the float32 values the
descriptor carries (``f32v``).

Tolerances, counted from what the device does (none from what a kernel returned):
  * the device forms x = tau L in float32 (one rounding, ``dx`` = max_k |float32(tau L) - tau L|, computed exactly here; zero when tau is a
    power of two), shifts by the group's maximum of x, takes a hardware exponential per sample, and does everything else -- the sum of the
    exponentials, its logarithm, + max, - log K_g, / tau, the sum over the groups, the mean over k -- in float64.  So the tempered term is off
    by (2 dx + 2e-6) / tau: the rounding of x moves a term and the maximum, and 2e-6 is the relative error of a sum of hardware
    exponentials that ``iw_reduction_reference.tol_reduce`` allows (it stays whole to the hardware: the float32 NumPy restatement below
    needs none of it);
  * the beta term takes ``tol_vi`` (the device's mean is a float64 sum of the float32 L: tol_vi over-covers it);
  * the result is rounded to float32 once: one spacing32 of |bound_n|.
  * ess: the two sums of exponentials are off by 2e-6 relative each (the squared one by twice that: its argument is doubled), the first
    enters squared: (2 + 2) 2e-6 = 8e-6 relative, plus the float32 rounding of the result.
Measured on the CPU (tests/test_bound_family_reference_host.py: ``restate_f32`` against ``bound_n`` over every family, (K, G) pair and
(tau, beta) pair of the GPU test): the worst ratio |restatement - statement| / tolerance is 0.49 (NumPy's float32 exponential in place of
the hardware's); no measured constant is used, so no factor is applied."""
import math

import numpy as np

import iw_reduction_reference as R

REL_SUMEXP = 2e-6                                                # iw_reduction_reference.tol_reduce's allowance for a sum of hardware exponentials
KG_PAIRS = ((1, 1), (4, 2), (6, 3), (16, 16), (64, 2), (65, 5), (65, 13), (66, 2), (130, 2), (130, 65), (128, 4))
ALL_B = (1, 3, 5, 65, 257)
TAU_BETA = ((1.0, 0.0), (0.5, 0.0), (0.05, 0.0), (1.0, 0.3), (1.0, 1.0), (0.5, 0.3))
FAMILIES = ("near_equal", "dominant", "wide", "ties_all", "ties_two")


def f32v(x):
    return float(np.float32(x))


def shape_cases():
    """All (K, G) against B = 5 (two workgroups of the heads kernel, a last wave without a point), all B against (6, 3) and (130, 2)."""
    return [(5, K, G) for K, G in KG_PAIRS] + [(B, K, G) for B in ALL_B if B != 5 for K, G in ((6, 3), (130, 2))]


# ---- the statement --------------------------------------------------------------------------------------------------------------------
def _grouped(L, G):
    L = np.asarray(L, dtype=np.float64)
    B, K = L.shape
    if G < 1 or K % G:
        raise ValueError("groups=%d must be >= 1 and divide K=%d" % (G, K))
    return L.reshape(B, G, K // G)


def tempered(L, G=1, tau=1.0):
    """(1/G) sum_g (1/tau) [logsumexp_{k in g}(tau L) - log K_g] [B]."""
    X = f32v(tau) * _grouped(L, G)
    m = X.max(2)
    lse = m + np.log(np.exp(X - m[..., None]).sum(2)) - math.log(X.shape[2])
    return (lse / f32v(tau)).mean(1)


def bound_n(L, G=1, tau=1.0, beta=0.0):
    b = f32v(beta)
    return b * np.asarray(L, dtype=np.float64).mean(1) + (1.0 - b) * tempered(L, G, tau)


def omega(L, G=1, tau=1.0, beta=0.0):
    """w [B, K] = d bound_n / d L_nk; every row sums to 1."""
    X = f32v(tau) * _grouped(L, G)
    e = np.exp(X - X.max(2, keepdims=True))
    sm = (e / e.sum(2, keepdims=True)).reshape(np.shape(L))
    b = f32v(beta)
    return b / sm.shape[1] + (1.0 - b) / G * sm


def ess(L):
    L = np.asarray(L, dtype=np.float64)
    e = np.exp(L - L.max(1, keepdims=True))
    return e.sum(1) ** 2 / (e * e).sum(1)


def heads(L, fmean, fvar, Y, lik_var, scale, G=1, tau=1.0, beta=0.0):
    """(w = scale omega [B, K], d_mean, d_var [B, K, Dy], d bound / d lik_var): ``iw_reduction_reference.heads`` under the family's weights."""
    fmean, fvar, Y = (np.asarray(a, dtype=np.float64) for a in (fmean, fvar, Y))
    w = scale * omega(L, G, tau, beta)
    e = Y[:, None, :] - fmean
    d_mean = w[..., None] * e / lik_var
    d_var = -0.5 * w[..., None] / lik_var * np.ones_like(e)
    d_lik = (w[..., None] * (-0.5 / lik_var + 0.5 * (e * e + fvar) / lik_var ** 2)).sum()
    return w, d_mean, d_var, d_lik


# ---- tolerances -----------------------------------------------------------------------------------------------------------------------
def dx(L, tau):
    """max_k |float32(tau L) - tau L| [B]: the one float32 rounding in front of the exponential (0 when tau is a power of two)."""
    L = np.asarray(L, dtype=np.float64)
    x32 = (np.float32(tau) * L.astype(np.float32)).astype(np.float64)
    return np.abs(x32 - f32v(tau) * L).max(1)


def tol_bound(L, G=1, tau=1.0, beta=0.0):
    """On bound_n computed from float32 log-weights that are the inputs themselves [B]."""
    b = f32v(beta)
    return (1.0 - b) * (2.0 * dx(L, tau) + REL_SUMEXP) / f32v(tau) + b * R.tol_vi(L) + R.spacing32(bound_n(L, G, tau, beta))


def tol_ess(L):
    e = ess(L)
    return 4 * REL_SUMEXP * e + R.spacing32(e)


def tol_w(w_ref, scale, L, tau, tol_L=0.0):
    """On scale omega: the softmax part carries exp(2 (tau tol_L + dx)) - 1 + 4e-6 relative (a term and its normaliser may move apart by
    the error of x each; 4e-6 as ``iw_reduction_reference.tol_w``), the uniform part beta / K one float32 rounding; written on the whole
    weight, which is at least its softmax part."""
    tol_x = 2.0 * (f32v(tau) * np.broadcast_to(np.asarray(tol_L, dtype=np.float64), (np.shape(L)[0],)) + dx(L, tau))
    return R.tol_w(w_ref, scale, tol_x)


# ---- float32 restatement of the device recurrence ------------------------------------------------------------------------------------
def restate_f32(L, G=1, tau=1.0, beta=0.0):
    """bound_n as the device forms it: x = tau L, the shift and the exponential in float32; sums, logarithm and the rest in float64; one
    rounding to float32 at the end."""
    L32 = np.asarray(L, dtype=np.float32)
    B, K = L32.shape
    X = (np.float32(tau) * L32).astype(np.float32).reshape(B, G, K // G)
    m = X.max(2)
    e = np.exp((X - m[..., None]).astype(np.float32)).astype(np.float32).astype(np.float64)
    lse = m.astype(np.float64) + np.log(e.sum(2)) - math.log(K // G)
    b = f32v(beta)
    return (b * L32.astype(np.float64).mean(1) + (1.0 - b) * (lse / f32v(tau)).mean(1)).astype(np.float32).astype(np.float64)
