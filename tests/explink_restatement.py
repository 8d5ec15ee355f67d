"""Float64 restatement of the exp-link likelihoods (GPflow 1.x Poisson, Exponential, Gamma; lambda = exp(F)) and of the bounds built on
them.  TEST INFRASTRUCTURE ONLY (tests/test_explink_host.py pins it against SciPy and against the 20-point rule;
tests/test_gpu_explink.py compares the HIP kernels with it).

``variational_expectations`` is GPflow's closed-form branch for the exp link; ``predict_density`` and ``predict_mean_and_var`` are its
base-class defaults on ``quad`` of tests/lik_restatement.py.  The layer stack is the oracle's through ``LikDGP`` there.

All three log-densities have one shape, logp(f, y) = cm f - ce exp(sg f) + c0(y); ``pieces`` returns (cm, ce, sg, [|terms of c0|]) so the
error scales below are written once."""
import math
import os
import sys

import numpy as np
import torch
from scipy import special

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lik_restatement as R   # noqa: E402
from lik_restatement import GH_W, GH_X, LikDGP, _t, moment_grid, quad   # noqa: E402,F401

U = 2.0 ** -24                                                   # the unit roundoff of float32


class _ExpLink:
    def variational_expectations(self, Fmu, Fvar, Y):
        """The closed form: E exp(sg f) = exp(sg mu + v / 2)."""
        Fmu, Fvar, Y = _t(Fmu), _t(Fvar), _t(Y)
        cm, ce, sg, _ = self.pieces(Y)
        return cm * Fmu - ce * torch.exp(sg * Fmu + 0.5 * Fvar) + self.c0(Y)

    def logp(self, F, Y):
        F, Y = _t(F), _t(Y)
        cm, ce, sg, _ = self.pieces(Y)
        return cm * F - ce * torch.exp(sg * F) + self.c0(Y)

    def predict_density(self, Fmu, Fvar, Y):
        return quad(lambda f: self.logp(f, _t(Y)[..., None]), Fmu, Fvar, logspace=True)

    def predict_mean_and_var(self, Fmu, Fvar):
        m = quad(self.conditional_mean, Fmu, Fvar)
        return m, quad(lambda f: self.conditional_variance(f) + self.conditional_mean(f) ** 2, Fmu, Fvar) - m ** 2


class Poisson(_ExpLink):
    name = "poisson"

    def __init__(self, binsize=1.0):
        self.binsize = binsize

    def pieces(self, Y):
        return Y, self.binsize, 1.0, [torch.lgamma(Y + 1.0), torch.abs(Y * math.log(self.binsize))]

    def c0(self, Y):
        return Y * math.log(self.binsize) - torch.lgamma(Y + 1.0)

    def logp(self, F, Y):                                        # as GPflow writes it: Y log(b l) - b l - lgamma(Y + 1)
        F, Y = _t(F), _t(Y)
        lam = self.binsize * torch.exp(F)
        return Y * torch.log(lam) - lam - torch.lgamma(Y + 1.0)

    def conditional_mean(self, F):
        return self.binsize * torch.exp(F)

    conditional_variance = conditional_mean


class Exponential(_ExpLink):
    name = "exponential"

    def pieces(self, Y):
        return -1.0, Y, -1.0, []

    def c0(self, Y):
        return torch.zeros_like(Y)

    def logp(self, F, Y):                                        # -Y / l - log l
        F, Y = _t(F), _t(Y)
        return -Y / torch.exp(F) - F

    def conditional_mean(self, F):
        return torch.exp(F)

    def conditional_variance(self, F):
        return torch.exp(F) ** 2


class Gamma(_ExpLink):
    name = "gamma"

    def __init__(self, shape=1.0):
        self.shape = shape                                       # may be a tensor that requires grad

    def pieces(self, Y):
        a = _t(self.shape)
        return -a, Y, -1.0, [torch.abs(torch.lgamma(a)) + torch.zeros_like(Y), torch.abs((a - 1.0) * torch.log(Y))]

    def c0(self, Y):
        a = _t(self.shape)
        return (a - 1.0) * torch.log(Y) - torch.lgamma(a)

    def logp(self, F, Y):                                        # -a log l - lgamma(a) + (a - 1) log Y - Y / l
        F, Y, a = _t(F), _t(Y), _t(self.shape)
        return -a * F - torch.lgamma(a) + (a - 1.0) * torch.log(Y) - Y / torch.exp(F)

    def conditional_mean(self, F):
        return _t(self.shape) * torch.exp(F)

    def conditional_variance(self, F):
        return _t(self.shape) * torch.exp(F) ** 2


def make(kind, **kw):
    return {"poisson": Poisson, "exponential": Exponential, "gamma": Gamma}[kind](**kw)


def bound_and_gradients(spec, lik, zs, mode_vi=False):
    """(bound, per-point log p [B], {name: gradient}) by float64 autodiff through ``LikDGP``: tests/lik_restatement.py's own function, plus
    'lik_shape' as a leaf for the Gamma."""
    if not isinstance(lik, Gamma):
        return R.bound_and_gradients(spec, lik, zs, mode_vi)
    a = float(lik.shape)
    lik.shape = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    try:
        val, logp, grads = R.bound_and_gradients(spec, lik, zs, mode_vi)
        grads["lik_shape"] = np.zeros(()) if lik.shape.grad is None else lik.shape.grad.detach().numpy().copy()
    finally:
        lik.shape = a
    return val, logp, grads


def shape_gradient_scale(spec, lik, zs, mode_vi=False):
    """sum |w| (|mu| + |psi(a)| + |log Y|) over (point, sample, output): what the terms of d bound / d shape add up to before they cancel
    (w: the scaled importance weights, or scale / K for the plain bound)."""
    m = LikDGP(spec, lik)
    with torch.no_grad():
        L_NK, _ = m.log_weights_tensor(zs, mode_vi)
        B, K = L_NK.shape
        w = (torch.full_like(L_NK, 1.0 / K) if mode_vi else torch.softmax(L_NK, 1)) * (m.n_data / B)
        mean, _ = m.final_moments()
        per = mean.abs() + abs(float(special.digamma(float(lik.shape)))) + torch.log(m.Y).abs()[:, None, :]
        return float((w[..., None] * per).sum())


def targets(spec, kind):
    """Targets of the right support from the synthetic regression targets, Yz = spec['Y'] standardised per column: counts
    floor(exp(clip(Yz, -2, 2.5))) for the Poisson, exp(clip(Yz, -3, 3)) for the other two; the first row of the Poisson's and the
    Exponential's is 0, so that edge is always present."""
    Y = np.asarray(spec["Y"], dtype=np.float64)
    Yz = (Y - Y.mean(0)) / Y.std(0)
    if kind == "poisson":
        out = np.floor(np.exp(np.clip(Yz, -2.0, 2.5)))
    else:
        out = np.exp(np.clip(Yz, -3.0, 3.0))
    if kind != "gamma":
        out[0] = 0.0
    return out


# ---- the error scales of tests/test_gpu_explink.py: |got - ref| <= 8 U S, S in float64 -----------------------------------------------
def _magnitudes(lik, f, hv, Y):
    """sum |terms| + |x| c exp(x) of cm f - ce exp(x) + c0(Y), x = sg f + hv: the last summand is the rounding of the exponential's argument."""
    f, Y = _t(f), _t(Y)
    cm, ce, sg, c0_terms = lik.pieces(Y)
    x = sg * f + hv
    e = _t(ce) * torch.exp(x)
    return torch.abs(_t(cm) * f) + torch.abs(e) + sum(c0_terms, torch.zeros_like(f)) + torch.abs(x) * torch.abs(e)


def var_exp_scale(lik, Fmu, Fvar, Y):
    return 1.0 + _magnitudes(lik, Fmu, 0.5 * _t(Fvar), Y)


def logp_scale(lik, F, Y):
    return 1.0 + _magnitudes(lik, F, 0.0, Y)


def density_scale(lik, Fmu, Fvar, Y):
    """1 + sum_i pi_i (magnitudes(f_i) + |log w_i|), pi_i = exp(g_i + log w_i - result): the normalised node weights."""
    Fmu, Fvar, Y = _t(Fmu), _t(Fvar), _t(Y)
    f = Fmu[..., None] + torch.sqrt(2.0 * Fvar)[..., None] * torch.as_tensor(GH_X)
    logw = torch.as_tensor(np.log(GH_W))
    g = lik.logp(f, Y[..., None]) + logw
    pi = torch.exp(g - torch.logsumexp(g, -1, keepdim=True))
    return 1.0 + (pi * (_magnitudes(lik, f, 0.0, Y[..., None]) + logw.abs())).sum(-1)


def mean_var_scales(lik, Fmu, Fvar):
    """(A |E_y|, A (E_y2 + E_y^2)), A = 1 + |mu| + 5.4 sqrt(2 v): the largest node argument."""
    Fmu, Fvar = _t(Fmu), _t(Fvar)
    A = 1.0 + Fmu.abs() + 5.4 * torch.sqrt(2.0 * Fvar)
    ey = quad(lik.conditional_mean, Fmu, Fvar)
    ey2 = quad(lambda f: lik.conditional_variance(f) + lik.conditional_mean(f) ** 2, Fmu, Fvar)
    return A * ey.abs(), A * (ey2 + ey ** 2)


def heads(lik, Fmu, Fvar, Y):
    """(dE/dmu, dE/dv, the tolerance scale 1 + |Y| + (1 + |x|) c exp(x) + a) of the closed form."""
    Fmu, Fvar, Y = _t(Fmu), _t(Fvar), _t(Y)
    cm, ce, sg, _ = lik.pieces(Y)
    x = sg * Fmu + 0.5 * Fvar
    e = _t(ce) * torch.exp(x)
    a = float(lik.shape) if isinstance(lik, Gamma) else 0.0
    return _t(cm) - sg * e + torch.zeros_like(Fmu), -0.5 * e, 1.0 + Y.abs() + (1.0 + x.abs()) * e.abs() + a
