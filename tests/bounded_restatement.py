"""Float64 restatement of the bounded-target likelihoods (GPflow 1.x Beta and Ordinal, probit link with GPflow's jitter) and of the bounds
built on them.  TEST INFRASTRUCTURE ONLY (tests/test_bounded_host.py pins it against SciPy and against adaptive quadrature;
tests/test_gpu_bounded.py compares the HIP kernels with it).

``variational_expectations``, ``predict_density`` and ``predict_mean_and_var`` are GPflow's base-class defaults on ``quad`` of
tests/lik_restatement.py.  The layer stack is the oracle's through ``LikDGP`` there.

The error scales S at the end are float64 and follow one rule: the sum of the magnitudes of the terms of a quantity before they cancel,
plus the condition of each transcendental with respect to the rounding of its float32 argument (|x f'(x)| for f(x)).  ``Float32`` evaluates
the kernels' formulas in plain float32 NumPy: the multiple of 2^-24 S it reaches is what the constant C of the GPU tests is derived from."""
import math
import os
import sys

import numpy as np
import torch
from scipy import special

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lik_restatement as R   # noqa: E402
from lik_restatement import GH_W, GH_X, JIT, LikDGP, _t, inv_probit, moment_grid, quad   # noqa: E402,F401

U = 2.0 ** -24                                                   # the unit roundoff of float32
C_JIT = 1.0 - 2.0 * JIT
Y_EPS = 1e-6
SQ2, RS2PI = math.sqrt(2.0), 1.0 / math.sqrt(2.0 * math.pi)
REF_EPS = 2.0 ** -52 / U                                          # a float64 rounding in units of U


def _phi(x):
    return RS2PI * torch.exp(-0.5 * x ** 2)


class _Defaults:
    def variational_expectations(self, Fmu, Fvar, Y):
        return quad(lambda f: self.logp(f, _t(Y)[..., None]), Fmu, Fvar)

    def predict_density(self, Fmu, Fvar, Y):
        return quad(lambda f: self.logp(f, _t(Y)[..., None]), Fmu, Fvar, logspace=True)

    def second_moment(self, F):
        return self.conditional_variance(F) + self.conditional_mean(F) ** 2

    def predict_mean_and_var(self, Fmu, Fvar):
        m = quad(self.conditional_mean, Fmu, Fvar)
        return m, quad(self.second_moment, Fmu, Fvar) - m ** 2


class Beta(_Defaults):
    name, grad_name, par_name = "beta", "lik_scale", "scale"

    def __init__(self, scale=1.0):
        self.scale = scale                                       # may be a tensor that requires grad

    def pieces(self, F, Y):
        """(alpha, beta, log yc, log(1 - yc), s)"""
        F, Y, s = _t(F), _t(Y), _t(self.scale)
        m = inv_probit(F)
        al = m * s
        yc = torch.clamp(Y, Y_EPS, 1.0 - Y_EPS)
        return al, s - al, torch.log(yc), torch.log1p(-yc), s

    def logp(self, F, Y):
        al, be, ly, l1y, s = self.pieces(F, Y)
        return (al - 1.0) * ly + (be - 1.0) * l1y + torch.lgamma(s) - torch.lgamma(al) - torch.lgamma(be)

    def conditional_mean(self, F):
        return inv_probit(F)

    def conditional_variance(self, F):
        m = inv_probit(F)
        return (m - m ** 2) / (_t(self.scale) + 1.0)


class Ordinal(_Defaults):
    name, grad_name, par_name = "ordinal", "lik_sigma", "sigma"

    def __init__(self, bin_edges, sigma=1.0):
        self.bin_edges = np.asarray(bin_edges, dtype=np.float64)
        self.sigma = sigma                                       # may be a tensor that requires grad

    def sides(self, F, Y):
        """(x_hi, x_lo, has_hi, has_lo): the label's scaled edges (e - F) / sigma, 0 where the bin is open on that side."""
        F, Y, sig = _t(F), _t(Y), _t(self.sigma)
        e, n = torch.as_tensor(self.bin_edges), self.bin_edges.size
        yi = Y.long()
        hi, lo = yi < n, yi > 0
        ehi, elo = e[torch.clamp(yi, max=n - 1)], e[torch.clamp(yi - 1, min=0)]
        return (ehi - F) / sig, (elo - F) / sig, hi, lo

    def prob(self, F, Y):
        xa, xb, hi, lo = self.sides(F, Y)
        return torch.where(hi, inv_probit(xa), torch.full_like(xa, 1.0 - JIT)) - torch.where(lo, inv_probit(xb), torch.full_like(xb, JIT))

    def logp(self, F, Y):
        return torch.log(self.prob(F, Y) + Y_EPS)

    def bin_probs(self, F):
        """[..., n + 1]"""
        F, sig = _t(F), _t(self.sigma)
        cdf = inv_probit((torch.as_tensor(self.bin_edges) - F[..., None]) / sig)
        pad = torch.ones_like(F)[..., None]
        return torch.cat([cdf, pad * (1.0 - JIT)], -1) - torch.cat([pad * JIT, cdf], -1)

    def conditional_mean(self, F):
        return (self.bin_probs(F) * torch.arange(self.bin_edges.size + 1.0, dtype=torch.float64)).sum(-1)

    def second_moment(self, F):
        return (self.bin_probs(F) * torch.arange(self.bin_edges.size + 1.0, dtype=torch.float64) ** 2).sum(-1)

    def conditional_variance(self, F):
        return self.second_moment(F) - self.conditional_mean(F) ** 2


def make(kind, **kw):
    return {"beta": Beta, "ordinal": Ordinal}[kind](**kw)


def bound_and_gradients(spec, lik, zs, mode_vi=False):
    """(bound, per-point log p [B], {name: gradient}) by float64 autodiff through ``LikDGP``: tests/lik_restatement.py's own function, plus
    the trained scalar ('lik_scale' / 'lik_sigma') as a leaf."""
    v = float(getattr(lik, lik.par_name))
    leaf = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    setattr(lik, lik.par_name, leaf)
    try:
        val, logp, grads = R.bound_and_gradients(spec, lik, zs, mode_vi)
        grads[lik.grad_name] = np.zeros(()) if leaf.grad is None else leaf.grad.detach().numpy().copy()
    finally:
        setattr(lik, lik.par_name, v)
    return val, logp, grads


STACK_EDGES = (-0.8, 0.0, 0.9)

# ---- the elementwise cases of tests/test_gpu_bounded.py and the constant of their bound -------------------------------------------------
ELEMENTWISE_EDGES = (-1.0, 0.0, 1.5)
ELEMENTWISE_CASES = ([("beta", dict(scale=s), (0.0, 1e-3, 0.3, 0.97, 1.0)) for s in (0.6, 2.0, 50.0)]
                     + [("ordinal", dict(bin_edges=ELEMENTWISE_EDGES, sigma=s), (0.0, 1.0, 2.0, 3.0)) for s in (0.5, 1.3)])
C_BOUND = 16.0            # |got - ref| <= C_BOUND 2^-24 S: 3 x what ``Float32`` reaches on these cases, rounded up (measure_float32 below)


def far_grid(edges, sigma):
    """600 points whose mean runs from 8 sigma below the lowest edge to 8 sigma above the highest (150 values) at four variances: where a
    naive float32 Phi(l) - Phi(r) has lost every digit of a bin's probability."""
    mu = np.linspace(min(edges) - 8.0 * sigma, max(edges) + 8.0 * sigma, 150)
    MU, V = np.meshgrid(mu, np.array([1e-4, 1e-2, 0.3, 4.0]), indexing="ij")
    return MU.reshape(-1).astype(np.float32), V.reshape(-1).astype(np.float32)


def grids(kind, kw):
    MU, V = moment_grid()
    out = [(MU.astype(np.float32), V.astype(np.float32))]
    if kind == "ordinal":
        out.append(far_grid(kw["bin_edges"], kw["sigma"]))
    return out


def measure_float32():
    """{quantity: the worst |Float32 - float64| / (2^-24 S)} over ELEMENTWISE_CASES on their grids (a few seconds on a CPU)."""
    worst = {}

    def note(what, got, ref, scale):
        got, ref, scale = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref, scale))
        assert np.isfinite(got).all(), what
        worst[what] = max(worst.get(what, 0.0), float((np.abs(got - ref) / (U * scale)).max()))
    for kind, kw, ys in ELEMENTWISE_CASES:
        lik = make(kind, **kw)
        F = Float32(lik)
        for mu32, v32 in grids(kind, kw):
            m64, v64 = mu32.astype(np.float64), v32.astype(np.float64)
            (pm, pv), (rm, rv), (sm, sv) = F.mean_var(mu32, v32), lik.predict_mean_and_var(m64, v64), mean_var_scales(lik, m64, v64)
            note("predict_mean", pm, rm.numpy(), sm.numpy())
            note("predict_var", pv, rv.numpy(), sv.numpy())
            for y in ys:
                Y = np.full_like(mu32, y)
                y64 = Y.astype(np.float64)
                E, dm, dv, dp = F.quad(mu32, v32, Y, True)
                rdm, rdv, rdp, Sm, Sv, Sp = heads(lik, m64, v64, y64)
                for what, got, ref, scale in (("var_exp", E, lik.variational_expectations(m64, v64, y64), var_exp_scale(lik, m64, v64, y64)),
                                              ("logp", F.logp(mu32, Y), lik.logp(m64, y64), logp_scale(lik, m64, y64)),
                                              ("predict_density", F.density(mu32, v32, Y), lik.predict_density(m64, v64, y64), density_scale(lik, m64, v64, y64)),
                                              ("d_mean", dm, rdm, Sm), ("d_var", dv, rdv, Sv), ("d_par", dp, rdp, Sp)):
                    note(what, got, ref.numpy(), scale.numpy())
    return worst


def targets(spec, kind, edges=STACK_EDGES):
    """Targets of the right support from the synthetic regression targets, Yz = spec['Y'] standardised per column.  Beta: inv_probit(Yz),
    the first two rows exactly 0 and 1 (the clip's two sides).  Ordinal: the bin of Yz among ``edges``; the first rows are set to the bins
    0 .. n in turn, so that every bin occurs whatever the draw."""
    Y = np.asarray(spec["Y"], dtype=np.float64)
    Yz = (Y - Y.mean(0)) / Y.std(0)
    if kind == "beta":
        out = inv_probit(Yz).numpy()
        out[0], out[1 % len(out)] = 0.0, 1.0
        return out
    out = np.searchsorted(np.asarray(edges), Yz).astype(np.float64)
    for j in range(min(len(edges) + 1, len(out))):
        out[j] = float(j)
    return out


# ---- error scales ---------------------------------------------------------------------------------------------------------------------
def _dg_mag(x):
    """The magnitudes inside the float32 digamma, psi(x) = log(x + 6) - ... - sum_{k < 6} 1 / (x + k), and its condition x psi'(x)."""
    return torch.log(x + 6.0).abs() + sum(1.0 / (x + k) for k in range(6)) + x * torch.special.polygamma(1, x)


def _node_scales(lik, f, Y):
    """(S of logp, S of d logp / df, S of d logp / d par) at the latent values f, elementwise."""
    f, Y = _t(f), _t(Y)
    if isinstance(lik, Beta):
        al, be, ly, l1y, s = lik.pieces(f, Y)
        m, q = al / s, be / s
        cond = (al * torch.digamma(al)).abs() + (be * torch.digamma(be)).abs()
        S = 1.0 + ((al - 1.0) * ly).abs() + ((be - 1.0) * l1y).abs() + torch.lgamma(s).abs() + torch.lgamma(al).abs() + torch.lgamma(be).abs() + cond
        dm = C_JIT * _phi(f) * (1.0 + 0.5 * f ** 2)
        Sg = s * dm * (ly.abs() + l1y.abs() + _dg_mag(al) + _dg_mag(be))
        Sp = 1.0 + torch.digamma(s).abs() + m * (ly.abs() + _dg_mag(al)) + q * (l1y.abs() + _dg_mag(be))
        return S, Sg, Sp
    xa, xb, hi, lo = lik.sides(f, Y)
    sig = _t(lik.sigma)
    den = lik.prob(f, Y) + Y_EPS
    pa, pb = torch.where(hi, _phi(xa), torch.zeros_like(xa)), torch.where(lo, _phi(xb), torch.zeros_like(xb))
    fs = f.abs() / sig
    rel = C_JIT * ((xa.abs() + fs) * pa + (xb.abs() + fs) * pb) / den          # the relative condition of den
    S = 1.0 + torch.log(den).abs() + rel
    # phi(x) and x phi(x) at x = (e - f) / sigma: the exponential's argument x^2 / 2 carries the rounding of x twice, and x that of f
    g1 = C_JIT * (1.0 + fs) * (pa * (1.0 + xa ** 2) + pb * (1.0 + xb ** 2)) / (sig * den)
    g2 = C_JIT * ((xa.abs() + fs) * pa * (1.0 + xa ** 2) + (xb.abs() + fs) * pb * (1.0 + xb ** 2)) / (sig * den)
    return S, g1 * (1.0 + rel), g2 * (1.0 + rel)


def _nodes(Fmu, Fvar):
    Fmu, Fvar = _t(Fmu), _t(Fvar)
    a = torch.sqrt(2.0 * Fvar)[..., None]
    return Fmu[..., None] + a * torch.as_tensor(GH_X), a, torch.as_tensor(GH_W)


def logp_scale(lik, F, Y):
    return _node_scales(lik, F, Y)[0]


def var_exp_scale(lik, Fmu, Fvar, Y):
    f, _, w = _nodes(Fmu, Fvar)
    return (_node_scales(lik, f, _t(Y)[..., None])[0] * w).sum(-1)


def density_scale(lik, Fmu, Fvar, Y):
    """1 + sum_i pi_i (S(f_i) + |log w_i|), pi_i = exp(g_i + log w_i - result): the normalised node weights."""
    f, _, w = _nodes(Fmu, Fvar)
    Y = _t(Y)[..., None]
    g = lik.logp(f, Y) + torch.log(w)
    pi = torch.exp(g - torch.logsumexp(g, -1, keepdim=True))
    return 1.0 + (pi * (_node_scales(lik, f, Y)[0] + torch.log(w).abs())).sum(-1)


def heads(lik, Fmu, Fvar, Y):
    """(dE/dmu, dE/dv, dE/dpar, S_mu, S_v, S_par) of the variational expectation on flat arrays, elementwise; the derivatives by autograd
    (the parameter as one leaf per element, so its derivative comes out elementwise too)."""
    v = float(getattr(lik, lik.par_name))
    mu = torch.tensor(np.asarray(Fmu, dtype=np.float64).reshape(-1), requires_grad=True)
    var = torch.tensor(np.asarray(Fvar, dtype=np.float64).reshape(-1), requires_grad=True)
    par = torch.full((mu.numel(), 1), v, dtype=torch.float64, requires_grad=True)
    Yf = _t(Y).reshape(-1)
    setattr(lik, lik.par_name, par)
    try:
        E = quad(lambda f: lik.logp(f, Yf[..., None]), mu, var)
        dmu, dv, dpar = torch.autograd.grad(E.sum(), (mu, var, par))
    finally:
        setattr(lik, lik.par_name, v)
    f, a, w = _nodes(mu.detach(), var.detach())
    _, Sg, Sp = _node_scales(lik, f, Yf[..., None])
    x = torch.as_tensor(GH_X).abs()
    return dmu, dv, dpar[:, 0], (Sg * w).sum(-1), (Sg * w * x).sum(-1) / a[..., 0], (Sp * w).sum(-1)


def mean_var_scales(lik, Fmu, Fvar):
    """(S of E_y, S of E_y2 - E_y^2)"""
    f, _, w = _nodes(Fmu, Fvar)
    if isinstance(lik, Beta):
        m = inv_probit(f)
        c = C_JIT * f.abs() * _phi(f)                              # the condition of m in f
        s1 = float(lik.scale) + 1.0
        S1, S2 = m + c, lik.second_moment(f) + c * ((1.0 - 2.0 * m).abs() / s1 + 2.0 * m)
    else:
        sig = float(lik.sigma)
        x = (torch.as_tensor(lik.bin_edges) - f[..., None]) / sig
        Q = 0.5 * torch.erfc(x / SQ2)
        c = C_JIT * (Q + (x.abs() + f.abs()[..., None] / sig) * _phi(x))
        j = torch.arange(float(lik.bin_edges.size), dtype=torch.float64)
        # (+ the float64 rounding of the restatement's own sum_j j P_j, whose terms are differences of values near 1: it matters where
        # the mean itself is below 1e-8, far under the lowest edge)
        n = lik.bin_edges.size
        S1, S2 = c.sum(-1) + REF_EPS * n * (n + 1) / 2.0, (c * (2.0 * j + 1.0)).sum(-1) + REF_EPS * n * (n + 1) * (2 * n + 1) / 6.0
    ey = (lik.conditional_mean(f) * w).sum(-1)
    return (S1 * w).sum(-1), (S2 * w).sum(-1) + ey ** 2


# ---- the kernels' formulas in plain float32 NumPy (csrc/likelihood_bounded.hip, line by line) -----------------------------------------
class Float32:
    """var_exp / logp / density / mean_var / heads of one likelihood on float32 arrays, every intermediate rounded to float32."""
    f = np.float32

    def __init__(self, lik):
        self.lik = lik
        self.X, self.W = GH_X[10:].astype(np.float32), GH_W[10:].astype(np.float32)
        self.LOGW = np.log(GH_W[10:]).astype(np.float32)
        f = self.f
        if isinstance(lik, Beta):
            s = np.float64(np.float32(lik.scale))
            self.s, self.lgs, self.psis = f(s), f(special.gammaln(s)), f(special.digamma(s))
        else:
            sig = f(lik.sigma)
            self.rsig = f(1.0) / sig
            self.k = f(1.0 / SQ2) * self.rsig
            self.edges = lik.bin_edges.astype(np.float32)

    @classmethod
    def digamma(cls, x):
        f = cls.f
        r = f(1.0) / x
        for k in range(1, 6):
            r = r + f(1.0) / (x + f(k))
        X = x + f(6.0)
        i = f(1.0) / X
        i2 = i * i
        return np.log(X) - f(0.5) * i - i2 * (f(1.0 / 12.0) - i2 * (f(1.0 / 120.0) - i2 * f(1.0 / 252.0))) - r

    def tgt(self, y):
        f = self.f
        if isinstance(self.lik, Beta):
            lo, hi = y <= f(1e-6), y > f(0.999999)
            ys = np.where(lo | hi, f(0.5), y)
            ly = np.where(lo, f(math.log(1e-6)), np.where(hi, f(math.log1p(-1e-6)), np.log(ys)))
            l1y = np.where(lo, f(math.log1p(-1e-6)), np.where(hi, f(math.log(1e-6)), np.log1p(-ys)))
            return ly.astype(f), l1y.astype(f)
        n = self.edges.size
        yi = np.clip(y.astype(np.int64), 0, n)
        hi, lo = yi < n, yi > 0
        return (np.where(hi, self.edges[np.minimum(yi, n - 1)], f(np.inf)).astype(f), np.where(lo, self.edges[np.maximum(yi - 1, 0)], f(-np.inf)).astype(f),
                hi, lo)

    def eval(self, T, x, grad):
        """(g, g', dg/dpar) without the constants of the rule"""
        f = self.f
        c, jit = f(C_JIT), f(JIT)
        with np.errstate(all="ignore"):
            if isinstance(self.lik, Beta):
                ly, l1y = T
                u = x * f(1.0 / SQ2)
                m = f(0.5) * special.erfc(-u) * c + jit
                q = f(0.5) * special.erfc(u) * c + jit
                al, be = self.s * m, self.s * q
                g = ((al - f(1.0)) * ly + (be - f(1.0)) * l1y) - special.gammaln(al) - special.gammaln(be)
                if not grad:
                    return g.astype(f), None, None
                psa, psb = self.digamma(al), self.digamma(be)
                dm = c * f(RS2PI) * np.exp(f(-0.5) * x * x)
                return g.astype(f), self.s * dm * ((ly - l1y) - (psa - psb)), m * (ly - psa) + q * (l1y - psb)
            ehi, elo, hi, lo = T
            a, b = (ehi - x) * self.k, (elo - x) * self.k
            one = np.where(b >= 0, f(0.5) * (special.erfc(b) - special.erfc(a)),
                           np.where(a <= 0, f(0.5) * (special.erfc(-a) - special.erfc(-b)), f(0.5) * (special.erf(a) + special.erf(-b)))).astype(f)
            den = c * one + f(1e-6)
            g = np.log(den)
            if not grad:
                return g, None, None
            pa, pb = np.where(hi, np.exp(-a * a), f(0)).astype(f), np.where(lo, np.exp(-b * b), f(0)).astype(f)
            xa, xb = np.where(hi, a * pa, f(0)).astype(f), np.where(lo, b * pb, f(0)).astype(f)
            cc = c * f(RS2PI) * self.rsig / den
            return g, cc * (pb - pa), cc * f(SQ2) * (xb - xa)

    def E0(self):
        return self.lgs if isinstance(self.lik, Beta) else self.f(0)

    def DP0(self):
        return self.psis if isinstance(self.lik, Beta) else self.f(0)

    def quad(self, mu, v, y, grad=False):
        f = self.f
        T = self.tgt(y)
        a = np.sqrt(f(2.0) * np.maximum(v, f(1e-8)))
        E = s1 = s2 = sp = np.zeros_like(mu)
        for j in range(10):
            xa = a * self.X[j]
            ga, gpa, qa = self.eval(T, mu + xa, grad)
            gb, gpb, qb = self.eval(T, mu - xa, grad)
            E = self.W[j] * (ga + gb) + E
            if grad:
                s1 = self.W[j] * (gpa + gpb) + s1
                s2 = (self.W[j] * self.X[j]) * (gpa - gpb) + s2
                sp = self.W[j] * (qa + qb) + sp
        if grad:
            return E + self.E0(), s1, s2 / a, sp + self.DP0()
        return E + self.E0()

    def logp(self, mu, y):
        return self.eval(self.tgt(y), mu, False)[0] + self.E0()

    def density(self, mu, v, y):
        f = self.f
        T = self.tgt(y)
        a = np.sqrt(f(2.0) * np.maximum(v, f(0)))
        terms = []
        for j in range(10):
            xa = a * self.X[j]
            terms += [self.LOGW[j] + self.eval(T, mu + xa, False)[0], self.LOGW[j] + self.eval(T, mu - xa, False)[0]]
        mx = np.max(terms, 0)
        s = np.zeros_like(mu)
        for t in terms:
            s = s + np.exp(t - mx)
        return mx + np.log(s) + self.E0()

    def mean_var(self, mu, v):
        f = self.f
        c, jit = f(C_JIT), f(JIT)
        a = np.sqrt(f(2.0) * np.maximum(v, f(0)))
        s1 = s2 = np.zeros_like(mu)
        if isinstance(self.lik, Beta):
            rs1 = f(1.0) / (self.s + f(1.0))
            for j in range(10):
                for x in (mu + a * self.X[j], mu - a * self.X[j]):
                    u = x * f(1.0 / SQ2)
                    m, q = f(0.5) * special.erfc(-u) * c + jit, f(0.5) * special.erfc(u) * c + jit
                    s1 = self.W[j] * m + s1
                    s2 = self.W[j] * (m * q * rs1 + m * m) + s2
            return s1, s2 - s1 * s1
        for e in range(self.edges.size):
            cc, d = (self.edges[e] - mu) * self.k, a * self.k
            qe = np.zeros_like(mu)
            for j in range(10):
                xd = d * self.X[j]
                qe = self.W[j] * (f(0.5) * (special.erfc(cc - xd) + special.erfc(cc + xd))) + qe
            s1 = s1 + qe
            s2 = f(2 * e + 1) * qe + s2
        ey, ey2 = c * s1, c * s2
        return ey, ey2 - ey * ey
