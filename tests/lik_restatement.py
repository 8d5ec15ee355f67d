"""Float64 restatement of the non-Gaussian likelihoods (GPflow 1.x Bernoulli with the probit link, StudentT) and of the bounds built on
them.  TEST INFRASTRUCTURE ONLY (tests/test_likelihoods_host.py pins it against SciPy; tests/test_gpu_likelihoods.py compares the HIP
kernels with it).

The quadrature is GPflow's ``ndiagquad`` with 20 Gauss-Hermite points; the layer stack is the oracle's (oracle/ref_torch_cpu.py), called,
not restated: ``LikDGP`` records the final layer's moments as the oracle computes them and swaps the Gaussian expectation of its
log-weights for the likelihood's."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_torch_cpu import CpuDGP   # noqa: E402

GH_X, GH_W = np.polynomial.hermite.hermgauss(20)
GH_W = GH_W / np.sqrt(np.pi)
JIT = 1e-3


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))


def inv_probit(x):
    return 0.5 * (1.0 + torch.erf(_t(x) / math.sqrt(2.0))) * (1 - 2 * JIT) + JIT


class Bernoulli:
    name = "bernoulli"

    def logp(self, F, Y):
        p = inv_probit(F)
        return torch.where(_t(Y) == 1, torch.log(p), torch.log(1 - p))

    def predict_mean_and_var(self, Fmu, Fvar):
        p = inv_probit(_t(Fmu) / torch.sqrt(1 + _t(Fvar)))
        return p, p - p ** 2

    def predict_density(self, Fmu, Fvar, Y):
        p = self.predict_mean_and_var(Fmu, Fvar)[0]
        return torch.where(_t(Y) == 1, torch.log(p), torch.log(1 - p))

    def variational_expectations(self, Fmu, Fvar, Y):
        return quad(lambda f: self.logp(f, _t(Y)[..., None]), Fmu, Fvar)


class StudentT:
    name = "student_t"

    def __init__(self, scale=1.0, df=3.0):
        self.scale, self.df = scale, df                          # scale may be a tensor that requires grad

    def logp(self, F, Y):
        s, nu = _t(self.scale), self.df
        return (math.lgamma(0.5 * (nu + 1)) - math.lgamma(0.5 * nu) - 0.5 * (torch.log(s ** 2) + math.log(nu) + math.log(math.pi))
                - 0.5 * (nu + 1) * torch.log(1 + ((_t(Y) - _t(F)) / s) ** 2 / nu))

    def variational_expectations(self, Fmu, Fvar, Y):
        return quad(lambda f: self.logp(f, _t(Y)[..., None]), Fmu, Fvar)

    def predict_mean_and_var(self, Fmu, Fvar):
        s, nu = _t(self.scale), self.df
        m = quad(lambda f: f, Fmu, Fvar)
        return m, quad(lambda f: s ** 2 * nu / (nu - 2) + f ** 2, Fmu, Fvar) - m ** 2

    def predict_density(self, Fmu, Fvar, Y):
        return quad(lambda f: self.logp(f, _t(Y)[..., None]), Fmu, Fvar, logspace=True)


def sharded_heads(expect, Fmu, Fvar, kl, scale):
    """The heads of iwvi_lik_elbo_backward for a K-shard against the whole job's normaliser, in float64.  ``expect(mu, var)`` -> [B, K]: a
    sample's expectation summed over its outputs (tensors in, tensor out: the derivatives are autograd's); Fmu, Fvar [B, K, D] and
    kl [B, K, width] hold float32 values.  The job is this shard and a second one that holds the same samples:
      L = expect - sum kl,  lse_global = float32(logsumexp_k L + log 2),  K_total = 2 K,  w = scale exp(L - lse_global),
      d_mean = w dE/dmu,  d_var = w dE/dvar.
    Returns (L, lse_global, w, d_mean, d_var, dE/dmu, dE/dvar) as float64 arrays."""
    mu = torch.tensor(np.asarray(Fmu, dtype=np.float64), requires_grad=True)
    var = torch.tensor(np.asarray(Fvar, dtype=np.float64), requires_grad=True)
    E = expect(mu, var)
    dmu, dvar = (g.numpy() for g in torch.autograd.grad(E.sum(), (mu, var)))
    L = E.detach().numpy() - np.asarray(kl, dtype=np.float64).sum(-1)
    lse = (torch.logsumexp(torch.as_tensor(L), 1).numpy() + math.log(2.0)).astype(np.float32).astype(np.float64)
    w = scale * np.exp(L - lse[:, None])
    return L, lse, w, w[..., None] * dmu, w[..., None] * dvar, dmu, dvar


def quad(g, Fmu, Fvar, logspace=False):
    """sum_i w_i g(mu + sqrt(2 v) x_i), or log sum_i exp(g(.) + log w_i)."""
    Fmu, Fvar = _t(Fmu), _t(Fvar)
    f = Fmu[..., None] + torch.sqrt(2.0 * Fvar)[..., None] * torch.as_tensor(GH_X)
    if logspace:
        return torch.logsumexp(g(f) + torch.as_tensor(np.log(GH_W)), -1)
    return (g(f) * torch.as_tensor(GH_W)).sum(-1)


class LikDGP(CpuDGP):
    """The oracle's DGP with the likelihood's variational expectation in its log-weights."""

    def __init__(self, spec, lik):
        super().__init__(spec, torch.float64)
        self.lik = lik
        self._last = None
        if self.layers[-1]["type"] != "gp" or self.layers[-1]["W"] is not None:
            raise ValueError("the restatement records the moments of a final plain-kernel GP layer")

    def _conditional(self, L, F, full_cov, z):
        out = super()._conditional(L, F, full_cov, z)
        if L is self.layers[-1]:
            self._last = (out[1], out[2])
        return out

    def final_moments(self):
        mean, cov = self._last
        if cov.dim() == 4:
            cov = torch.diagonal(cov, dim1=-2, dim2=-1).transpose(1, 2)
        return mean, cov

    def log_weights_tensor(self, zs, mode_vi=False):
        L_NK, glob = super().log_weights_tensor(zs, mode_vi)          # Gaussian expectation minus the local regularisers
        mean, cov = self.final_moments()
        Yt = self.Y[:, None, :].repeat(1, self.K, 1)
        lik_var = torch.as_tensor(self.lik_var, dtype=self.dtype)
        ve_gauss = -0.5 * math.log(2 * math.pi) - 0.5 * torch.log(lik_var) - 0.5 * ((Yt - mean) ** 2 + cov) / lik_var
        return L_NK - ve_gauss.sum(2) + self.lik.variational_expectations(mean, cov, Yt).sum(2), glob

    def per_point(self, zs, mode_vi=False):
        L_NK, _ = self.log_weights_tensor(zs, mode_vi)
        return L_NK.mean(1) if mode_vi else torch.logsumexp(L_NK, 1) - math.log(self.K)


def bound_and_gradients(spec, lik, zs, mode_vi=False):
    """(bound, per-point log p [B], {name: gradient}) by float64 autodiff, names as oracle/grad_oracle.py plus 'lik_scale' (Student-t)."""
    m = LikDGP(spec, lik)
    params = {}
    leaf = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64)).clone().requires_grad_(True)
    for i, L in enumerate(m.layers):
        if L["type"] == "lv":
            L["W"] = [leaf(w.detach().numpy()) for w in L["W"]]
            L["b"] = [leaf(b.detach().numpy()) for b in L["b"]]
            for j, (w, b) in enumerate(zip(L["W"], L["b"])):
                params["l%d.encW%d" % (i, j)], params["l%d.encb%d" % (i, j)] = w, b
            continue
        for k in ("Z", "ls", "q_mu"):
            L[k] = leaf(L[k].detach().numpy())
            params["l%d.%s" % (i, k)] = L[k]
        raw = leaf(L["q_sqrt"].detach().numpy())
        L["q_sqrt"] = torch.tril(raw)
        params["l%d.q_sqrt" % i] = raw
        L["var"] = leaf(L["var"])
        params["l%d.var" % i] = L["var"]
        if L["W"] is not None:
            L["W"] = leaf(L["W"].detach().numpy())
            params["l%d.W" % i] = L["W"]
        if L["A"] is not None:
            L["A"] = leaf(L["A"].detach().numpy())
            params["l%d.mfA" % i] = L["A"]
    if isinstance(lik, StudentT):
        lik.scale = leaf(float(lik.scale))
        params["lik_scale"] = lik.scale
    val = m.elbo_tensor(zs, mode_vi=mode_vi)
    val.backward()
    grads = {k: (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.detach().numpy().copy()) for k, v in params.items()}
    if isinstance(lik, StudentT):
        lik.scale = float(lik.scale.detach())
    with torch.no_grad():
        logp = m.per_point(zs, mode_vi).numpy()
    return float(val.detach()), logp, grads


def moment_grid():
    """The grid of the issue's tests 2 and 3: mu in [-3, 3], v in [1e-4, 4] (log-spaced), y per likelihood."""
    mu = np.linspace(-3.0, 3.0, 25)
    v = np.geomspace(1e-4, 4.0, 24)
    MU, V = np.meshgrid(mu, v, indexing="ij")
    return MU.reshape(-1), V.reshape(-1)


# ---- the training check's problem (tests/test_gpu_likelihoods.py: test 7) ---------------------------------------------------------
def two_class_problem(seed=41):
    """An L1_G5-style stack (latent-variable layer, one inner layer of 5 latent GPs, final layer) with the reference's initial values
    on a seeded two-class problem: the synthetic regression targets thresholded at 0.  -> (spec, noise(i) -> per-layer arrays)."""
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=2, M=32, B=64, K=5, Dx=4, with_lv=True, seed=seed, parity=False)
    spec["Y"] = (spec["Y"] > 0).astype(np.float64)
    return spec, (lambda i: synthetic.make_noise(spec, seed=1000 + i))


def oracle_trainer(spec, lr=5e-3, gamma=1e-2):
    """The float64 training loop of tests/test_gpu_training.py (gradient restatement + oracle/optim_oracle.py) on the Bernoulli bound.
    (Its parameter list ends in the Gaussian's 'lik_var': a zero gradient leaves that entry where it is.)"""
    import copy
    from test_gpu_training import _OracleTrainer
    ot = _OracleTrainer(copy.deepcopy(spec), lr, gamma)

    def grad(sp, zs):
        val, _, g = bound_and_gradients(sp, Bernoulli(), zs)
        g["lik_var"] = np.zeros(())
        return val, g
    ot.grad = grad
    return ot


def oracle_accuracy(spec):
    """(training accuracy of predict_y > 1/2 at zero noise through the inner layers, majority-class rate) of the float64 model."""
    from oracle.from_spec import build_oracle
    B = spec["B"]
    X, Y = spec["X"][:B], spec["Y"][:B]
    zs = [np.zeros((B, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1])) for l in spec["layers"]]
    m, v = build_oracle(spec, iw=False, num_samples=1).build_predict(X, zs=zs)
    p = Bernoulli().predict_mean_and_var(m, v)[0].numpy()
    return float(((p > 0.5) == (Y == 1)).mean()), float(max(Y.mean(), 1 - Y.mean()))


def oracle_training_record(steps=200):
    """The constants of tests/test_gpu_likelihoods.py's training check, from the float64 loop (about 10 s on a CPU)."""
    from oracle.from_spec import build_oracle
    spec, noise = two_class_problem()
    ot = oracle_trainer(spec)
    v = np.array([ot.step(noise(2 * s), noise(2 * s + 1)) for s in range(steps)])
    acc, maj = oracle_accuracy(ot.spec)
    B = spec["B"]
    zs = [np.zeros((B, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1])) for l in spec["layers"]]
    m, var = build_oracle(ot.spec, iw=False, num_samples=1).build_predict(spec["X"][:B], zs=zs)
    p = Bernoulli().predict_mean_and_var(m, var)[0].numpy()
    return dict(first=float(v[0]), late=float(v[-10:].mean()), late_50_earlier=float(v[-60:-50].mean()), accuracy=acc, majority=maj,
                narrow_points=int((np.abs(p - 0.5) < 0.1).sum()))
