"""Float64 restatement of the heteroskedastic Gaussian likelihood (``likelihoods.HeteroskedasticGaussian``; include/iwvi_hip.h:
IWVI_LIK_HETERO_GAUSSIAN) and of the bounds built on it.  TEST INFRASTRUCTURE ONLY (tests/test_hetero_host.py pins it against Monte Carlo,
finite differences and a fine quadrature; tests/test_gpu_hetero.py and tests/test_gpu_hetero_model.py compare the HIP kernels with it).

Moments are [..., 2 Dt]: columns 0 .. Dt-1 the mean function f, columns Dt .. 2 Dt-1 the log noise variance g of the same target column;
Y and every result are [..., Dt].  Per target column:
  logp                     -1/2 log 2pi - g/2 - (y - f)^2 exp(-g) / 2
  variational_expectations -1/2 log 2pi - m_g/2 - q r / 2,   q = (y - m_f)^2 + v_f,  r = exp(a),  a = -m_g + v_g/2
  heads                    dE/dm_f = (y - m_f) r,  dE/dv_f = -r/2,  dE/dm_g = -1/2 + q r/2,  dE/dv_g = -q r/4
  predict_mean_and_var     (m_f, v_f + exp(m_g + v_g/2))
  predict_density          log int N(y; m_f, v_f + exp(g)) N(g; m_g, v_g) dg -- the 20-point Gauss-Hermite rule in log space DEFINES it
                           (v_g floored at 1e-8); ``n=200`` is the fine rule that measures the 20-point rule's own error
  sample_y                 f = m_f + sqrt(v_f) z_1,  g = m_g + sqrt(v_g) z_2,  y = f + exp(g/2) eps
Every exponent is clipped to [-60, 60] (``torch.clamp``: its derivative is zero where the clip is active and passes at the ends, which is
the rule the kernels' heads follow).  The layer stack is the oracle's through ``LikDGP`` of tests/lik_restatement.py: with ONE target
column its broadcast of Y [B, K, 1] against the moments [B, K, 2] is exactly the oracle's own, so nothing there needs restating."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lik_restatement as R   # noqa: E402
from lik_restatement import _t   # noqa: E402

U = 2.0 ** -24                                                   # the unit roundoff of float32
CLIP = 60.0
V_FLOOR = 1e-8                                                   # csrc/likelihood_common.h: LIK_V_FLOOR
HL2P = 0.5 * math.log(2.0 * math.pi)
C_CLOSED = 8.0             # |got - ref| <= 8 x 2^-24 S for the closed forms: tests/test_gpu_explink.py's constant for the same arithmetic
C_QUAD = 16.0              # ... and 16 for the log-space quadrature: tests/bounded_restatement.py's C_BOUND for its densities


def _rule(n):
    x, w = np.polynomial.hermite.hermgauss(n)
    w = w / np.sqrt(np.pi)
    keep = w > 0.0                                               # (the far nodes of a fine rule underflow: they carry nothing)
    return x[keep], w[keep]


def _clip(a):
    return torch.clamp(a, -CLIP, CLIP)


def split(A):
    """[..., 2 Dt] -> (the f columns, the g columns)"""
    A = _t(A)
    Dt = A.shape[-1] // 2
    assert A.shape[-1] == 2 * Dt and Dt >= 1, A.shape
    return A[..., :Dt], A[..., Dt:]


class HeteroskedasticGaussian:
    name = "hetero_gaussian"

    def logp(self, F, Y):
        f, g = split(F)
        return -HL2P - 0.5 * g - 0.5 * (_t(Y) - f) ** 2 * torch.exp(_clip(-g))

    def variational_expectations(self, Fmu, Fvar, Y):
        (mf, mg), (vf, vg) = split(Fmu), split(Fvar)
        q = (_t(Y) - mf) ** 2 + vf
        return -HL2P - 0.5 * mg - 0.5 * q * torch.exp(_clip(-mg + 0.5 * vg))

    def heads(self, Fmu, Fvar, Y):
        """(dE/dFmu, dE/dFvar) [..., 2 Dt], written out from the table (tests/test_hetero_host.py: against central differences)."""
        (mf, mg), (vf, vg) = split(Fmu), split(Fvar)
        e = _t(Y) - mf
        q = e ** 2 + vf
        a = -mg + 0.5 * vg
        r = torch.exp(_clip(a))
        qr = torch.where((a >= -CLIP) & (a <= CLIP), q * r, torch.zeros_like(q))
        return torch.cat([e * r, -0.5 + 0.5 * qr], -1), torch.cat([-0.5 * r, -0.25 * qr], -1)

    def predict_mean_and_var(self, Fmu, Fvar):
        (mf, mg), (vf, vg) = split(Fmu), split(Fvar)
        return mf + 0.0, vf + torch.exp(_clip(mg + 0.5 * vg))

    def _nodes(self, Fmu, Fvar, Y, n):
        """(log N(y; m_f, s_i) + log w_i [..., Dt, n], g_i, s_i)"""
        (mf, mg), (vf, vg) = split(Fmu), split(Fvar)
        x, w = _rule(n)
        gi = mg[..., None] + torch.sqrt(2.0 * torch.clamp(vg, min=V_FLOOR))[..., None] * torch.as_tensor(x)
        s = torch.clamp(vf, min=0.0)[..., None] + torch.exp(_clip(gi))
        e2 = ((_t(Y) - mf) ** 2)[..., None]
        return torch.as_tensor(np.log(w)) - HL2P - 0.5 * torch.log(s) - 0.5 * e2 / s, gi, s

    def predict_density(self, Fmu, Fvar, Y, n=20):
        return torch.logsumexp(self._nodes(Fmu, Fvar, Y, n)[0], -1)

    def sample_y(self, Fmu, Fvar, z_f, eps):
        """(y [..., Dt], the f that was used [..., 2 Dt]): z_f [..., 2 Dt] supplies z_1 and z_2, eps [..., Dt] the target's noise."""
        F = _t(Fmu) + torch.sqrt(torch.clamp(_t(Fvar), min=0.0)) * _t(z_f)
        f, g = split(F)
        return f + torch.exp(_clip(0.5 * g)) * _t(eps), F


def mixture(lik, Fmu, Fvar, Y=None):
    """The Monte Carlo predictive mixture over the S draws of moments [S, N, 2 Dt] -> dict(mean, var [N, Dt][, log_density [N]])."""
    m, v = lik.predict_mean_and_var(Fmu, Fvar)
    mean = m.mean(0)
    out = {"mean": mean.numpy(), "var": ((v + m ** 2).mean(0) - mean ** 2).numpy()}
    if Y is not None:
        lp = lik.predict_density(Fmu, Fvar, _t(Y)[None]).sum(-1)
        out["log_density"] = (torch.logsumexp(lp, 0) - math.log(lp.shape[0])).numpy()
    return out


def bound_and_gradients(spec, zs, mode_vi=False):
    """(bound, per-point log p [B], {name: gradient}) by float64 autodiff through ``LikDGP`` (ONE target column: see the module text)."""
    assert np.asarray(spec["Y"]).shape[1] == 1
    return R.bound_and_gradients(spec, HeteroskedasticGaussian(), zs, mode_vi)


# ---- the inputs of the elementwise and heads tests ---------------------------------------------------------------------------------------
N_BEYOND_RULE = 2


def cases(Dt, seed=0, n=400):
    """(Fmu, Fvar [T, 2 Dt], Y [T, Dt]) float32-representable float64 arrays: ``n`` seeded rows -- m_f, m_g in [-3, 3], v_f, v_g in [1e-4, 4]
    log-spaced, y within 3 predictive standard deviations sqrt(v_f + exp(m_g)) of m_f (targets the model finds plausible: the 20-point rule
    is adequate there, ``rule_error``); f and g differ per column, so a wrong pairing d <-> Dt + d cannot pass -- and then the edges, one row each
    (every column of the row): v_f = 0; v_g = 0; both 0; a = -m_g + v_g/2 at +-60 exactly, just inside (59.99) and just outside (60.01),
    formed with v_g = 0 so that float32 forms a exactly; the same with v_g = 2 (m_g = -+59 .. -+61 + 1); residuals (y - m_f)^2 exp(-g) of
    about 1e6 at v_g = 1e-4 and, as the LAST ``N_BEYOND_RULE`` rows, at v_g = 0.5 and 0.05.  Those last rows are for the closed forms only:
    with a residual of that size the integrand of predict_density lives hundreds of standard deviations out in the tail of N(g; m_g, v_g), where
    no 20-point rule has a node (it misses the fine rule by 315 and 3111 nats there), so the density checks take ``rows[:-N_BEYOND_RULE]``."""
    rng = np.random.default_rng([seed, Dt, 0x6867])
    mf, mg = rng.uniform(-3, 3, (n, Dt)), rng.uniform(-3, 3, (n, Dt))
    vf, vg = (np.exp(rng.uniform(np.log(1e-4), np.log(4.0), (n, Dt))) for _ in range(2))
    y = mf + rng.uniform(-3, 3, (n, Dt)) * np.sqrt(vf + np.exp(mg))
    rows = [(0.3, 0.0, -0.7, 0.5, 1.1), (0.3, 0.4, -0.7, 0.0, 1.1), (0.3, 0.0, -0.7, 0.0, 1.1)]
    for a in (60.0, 59.99, 60.01):
        for sign in (1.0, -1.0):
            rows.append((0.2, 0.3, -sign * a, 0.0, 0.9))             # a = sign * a exactly
            rows.append((0.2, 0.3, -sign * a + 1.0, 2.0, 0.9))       # the same a through v_g / 2 = 1
    rows += [(-5.0, 0.1, -9.2, 1e-4, 5.0), (-5.0, 0.1, -9.2, 0.5, 5.0), (4.0, 1e-3, -11.5, 0.05, 1.0)]
    E = np.array(rows)
    jitter = 1e-3 * np.arange(Dt)[None, :]                           # (columns of an edge row differ too)
    mf, vf, mg, vg, y = (np.concatenate([A, np.repeat(E[:, i:i + 1], Dt, 1) + (jitter if i in (0, 4) else 0.0)]) for i, A in enumerate((mf, vf, mg, vg, y)))
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    return f32(np.concatenate([mf, mg], 1)), f32(np.concatenate([vf, vg], 1)), f32(y)


# ---- the error scales: |got - ref| <= C x 2^-24 x S, S in float64 -------------------------------------------------------------------------
# The closed forms are sums of a few terms and one exponential, as the exp-link family's (tests/explink_restatement.py: _magnitudes): S is 1 +
# the magnitudes of the terms + |x| c exp(x) for the rounding of the exponential's argument x.  Here x = a = -m_g + v_g/2 is itself a rounded
# sum, so |x| is taken as A = |m_g| + v_g/2 (>= |a|), and the factor q is a rounded sum of positive terms (covered by the term's own magnitude).
def _parts(Fmu, Fvar, Y):
    (mf, mg), (vf, vg) = split(Fmu), split(Fvar)
    e = _t(Y) - mf
    return e, e ** 2 + vf, torch.exp(_clip(-mg + 0.5 * vg)), mg.abs() + 0.5 * vg, mg


def var_exp_scale(Fmu, Fvar, Y):
    e, q, r, A, mg = _parts(Fmu, Fvar, Y)
    return 1.0 + HL2P + 0.5 * mg.abs() + 0.5 * q * r * (1.0 + A)


def logp_scale(F, Y):
    f, g = split(F)
    t = 0.5 * (_t(Y) - f) ** 2 * torch.exp(_clip(-g))
    return 1.0 + HL2P + 0.5 * g.abs() + t * (1.0 + g.abs())


def heads_scales(Fmu, Fvar, Y):
    """(S of dE/dFmu, S of dE/dFvar) [..., 2 Dt]"""
    e, q, r, A, _ = _parts(Fmu, Fvar, Y)
    return torch.cat([1.0 + e.abs() * r * (1.0 + A), 1.0 + 0.5 * q * r * (1.0 + A)], -1), \
        torch.cat([1.0 + 0.5 * r * (1.0 + A), 1.0 + 0.25 * q * r * (1.0 + A)], -1)


def var_scale(Fmu, Fvar):
    (mf, mg), (vf, vg) = split(Fmu), split(Fvar)
    return vf + torch.exp(_clip(mg + 0.5 * vg)) * (1.0 + mg.abs() + 0.5 * vg)


def density_scale(lik, Fmu, Fvar, Y):
    """1 + sum_i pi_i (S(node i) + |log w_i|), pi_i the normalised node weights (tests/bounded_restatement.py: density_scale).  A node is
    log w - 1/2 log 2pi - 1/2 log s - e^2 / (2 s) with s = v_f + exp(g_i): S(node) = the magnitudes of its terms + the rounding of exp(g_i)
    -- relative (1 + |g_i|) on the share exp(g_i) / s <= 1 of s -- carried into log s (x 1/2) and into e^2 / s (x e^2 / (2 s))."""
    t, gi, s = lik._nodes(Fmu, Fvar, Y, 20)
    (mf, _), _ = split(Fmu), None
    e2 = ((_t(Y) - mf) ** 2)[..., None]
    logw = torch.as_tensor(np.log(_rule(20)[1]))
    pi = torch.exp(t - torch.logsumexp(t, -1, keepdim=True))
    S = HL2P + 0.5 * torch.log(s).abs() + 0.5 * e2 / s + (0.5 + 0.5 * e2 / s) * (1.0 + gi.abs()) * (torch.exp(_clip(gi)) / s)
    return 1.0 + (pi * (S + logw.abs())).sum(-1)


# ---- the kernels' formulas in plain float32 NumPy (csrc/likelihood_hetero.hip, line by line) ------------------------------------------------
class Float32:
    """var_exp / logp / density / mean_var / heads on float32 arrays [T, 2 Dt] / [T, Dt], every intermediate rounded to float32 (an fmaf is
    written as its two roundings: the bound from this restatement is then no smaller than the kernel's)."""
    f = np.float32

    def __init__(self):
        x, w = np.polynomial.hermite.hermgauss(20)
        self.X, self.LOGW = x[10:].astype(np.float32), np.log(w[10:] / np.sqrt(np.pi)).astype(np.float32)

    @classmethod
    def clip(cls, a):
        return np.minimum(np.maximum(a, cls.f(-CLIP)), cls.f(CLIP)), (a >= cls.f(-CLIP)) & (a <= cls.f(CLIP))

    @staticmethod
    def split(A):
        Dt = A.shape[-1] // 2
        return A[..., :Dt], A[..., Dt:]

    def ve(self, Fmu, Fvar, Y):
        f = self.f
        (mf, mg), (vf, vg) = self.split(Fmu), self.split(Fvar)
        e = Y - mf
        q = e * e + vf
        a, inside = self.clip(f(0.5) * vg - mg)
        r = np.exp(a)
        return (f(-0.5) * q) * r + (f(-0.5) * mg - f(HL2P)), e, q, r, inside

    def var_exp(self, Fmu, Fvar, Y):
        return self.ve(Fmu, Fvar, Y)[0]

    def heads(self, Fmu, Fvar, Y):
        f = self.f
        _, e, q, r, inside = self.ve(Fmu, Fvar, Y)
        qr = np.where(inside, q * r, f(0))
        return np.concatenate([e * r, f(0.5) * qr - f(0.5)], -1), np.concatenate([f(-0.5) * r, f(-0.25) * qr], -1)

    def logp(self, F, Y):
        f = self.f
        mf, g = self.split(F)
        e = Y - mf
        return (f(-0.5) * e * e) * np.exp(self.clip(-g)[0]) + (f(-0.5) * g - f(HL2P))

    def mean_var(self, Fmu, Fvar):
        (mf, mg), (vf, vg) = self.split(Fmu), self.split(Fvar)
        return mf, vf + np.exp(self.clip(self.f(0.5) * vg + mg)[0])

    def density(self, Fmu, Fvar, Y):
        f = self.f
        (mf, mg), (vf, vg) = self.split(Fmu), self.split(Fvar)
        e = Y - mf
        e2 = e * e
        vf = np.maximum(vf, f(0))
        a = np.sqrt(f(2.0) * np.maximum(vg, f(V_FLOOR)))
        terms = []
        with np.errstate(all="ignore"):
            for j in range(10):
                xa = a * self.X[j]
                for gi in (mg + xa, mg - xa):
                    s = vf + np.exp(self.clip(gi)[0])
                    terms.append(self.LOGW[j] - f(HL2P) - f(0.5) * np.log(s) - f(0.5) * e2 / s)
            mx = np.max(terms, 0)
            acc = np.zeros_like(mx)
            for t in terms:
                acc = acc + np.exp(t - mx)
            return mx + np.log(acc)


def measure_float32(Dts=(1, 2, 3)):
    """{name: worst |Float32 - float64| / (2^-24 S)} over ``cases``: tests/test_hetero_host.py asserts 3 x each <= its constant, the factor
    3 being left for the device's expf / logf, as tests/test_gpu_explink.py and tests/test_gpu_bounded.py derive theirs."""
    lik, F32 = HeteroskedasticGaussian(), Float32()
    worst = {}

    def take(name, got, ref, scale):
        m = float((np.abs(got.astype(np.float64) - ref.numpy()) / (U * scale.numpy())).max())
        worst[name] = max(worst.get(name, 0.0), m)

    for Dt in Dts:
        Fmu, Fvar, Y = cases(Dt)
        a32 = [np.asarray(a, dtype=np.float32) for a in (Fmu, Fvar, Y)]
        take("var_exp", F32.var_exp(*a32), lik.variational_expectations(Fmu, Fvar, Y), var_exp_scale(Fmu, Fvar, Y))
        take("logp", F32.logp(a32[0], a32[2]), lik.logp(Fmu, Y), logp_scale(Fmu, Y))
        take("predict_var", F32.mean_var(a32[0], a32[1])[1], lik.predict_mean_and_var(Fmu, Fvar)[1], var_scale(Fmu, Fvar))
        n = Y.shape[0] - N_BEYOND_RULE
        take("predict_density", F32.density(*(a[:n] for a in a32)), lik.predict_density(Fmu[:n], Fvar[:n], Y[:n]), density_scale(lik, Fmu[:n], Fvar[:n], Y[:n]))
        (dm, dv), (rm, rv), (sm, sv) = F32.heads(*a32), lik.heads(Fmu, Fvar, Y), heads_scales(Fmu, Fvar, Y)
        take("d_mean", dm, rm, sm)
        take("d_var", dv, rv, sv)
    return worst


def rule_error(Dts=(1, 2, 3)):
    """max |20-point - 200-point| of predict_density over the density rows of ``cases`` (absolute, in nats): the 20-point rule's own error on
    the test's inputs (DESIGN.md section 6 reports it), and the row where it is attained as (m_f, v_f, m_g, v_g, y)."""
    lik = HeteroskedasticGaussian()
    worst, where = 0.0, None
    for Dt in Dts:
        Fmu, Fvar, Y = (a[:-N_BEYOND_RULE] for a in cases(Dt))
        d = (lik.predict_density(Fmu, Fvar, Y, 20) - lik.predict_density(Fmu, Fvar, Y, 200)).abs().numpy()
        i = np.unravel_index(np.argmax(d), d.shape)
        if d[i] > worst:
            worst, where = float(d[i]), (Fmu[i[0], i[1]], Fvar[i[0], i[1]], Fmu[i[0], Dt + i[1]], Fvar[i[0], Dt + i[1]], Y[i])
    return worst, where
