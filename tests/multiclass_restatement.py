"""Float64 restatement of GPflow 1.x ``MultiClass(num_classes)`` with the ``RobustMax`` link and of the bounds built on it.  TEST
INFRASTRUCTURE ONLY (tests/test_multiclass_host.py pins it against a closed form and a Monte Carlo; tests/test_gpu_multiclass.py compares
the HIP kernels of csrc/likelihood_multiclass.hip with it).

Written from the definition, not from the kernels: Y is ONE column of labels, F / Fmu / Fvar have C columns,
  X_i = mu_y + x_i sqrt(max(2 v_y, 1e-10)),  d_ci = (X_i - mu_c) / sqrt(max(v_c, 1e-10)),  Phi~ = Phi(d) (1 - 2e-4) + 1e-4,
  p = sum_i w_i prod_{c != y} Phi~_ci            (x_i, w_i sqrt(pi)) = hermgauss(20)
and the heads of the bound come from autodiff of exactly this.  The layer stack is the oracle's (``lik_restatement.LikDGP``)."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import lik_restatement as R   # noqa: E402
from oracle.ref_torch_cpu import CpuDGP   # noqa: E402

GH_X, GH_W = R.GH_X, R.GH_W
_t = R._t


class MultiClass:
    name = "multiclass"

    def __init__(self, num_classes, epsilon=1e-3, cdf_jitter=1e-4):
        """``cdf_jitter``: GPflow's 1e-4; 0 only in the host test that compares the rule with the jitter-free closed form."""
        self.C, self.eps, self.jit = int(num_classes), float(epsilon), float(cdf_jitter)
        self.eps1 = self.eps / (self.C - 1)

    def prob_is_largest(self, Y, mu, var):
        """[..., 1]: the probability that latent Y is the largest of the C, Y [..., 1] labels, mu / var [..., C]."""
        mu, var = _t(mu), _t(var)
        y = _t(Y).to(torch.int64).expand(*mu.shape[:-1], 1)
        hot = torch.zeros(mu.shape, dtype=torch.bool).scatter_(-1, y, True)
        mu_y, v_y = torch.gather(mu, -1, y), torch.gather(var, -1, y)
        X = mu_y[..., None] + torch.as_tensor(GH_X) * torch.sqrt(torch.clamp(2.0 * v_y, min=1e-10))[..., None]        # [..., 1, 20]
        d = (X - mu[..., None]) / torch.sqrt(torch.clamp(var, min=1e-10))[..., None]                                    # [..., C, 20]
        cdf = 0.5 * torch.erfc(-d / math.sqrt(2.0)) * (1.0 - 2.0 * self.jit) + self.jit
        cdf = torch.where(hot[..., None], torch.ones_like(cdf), cdf)
        return (cdf.prod(-2) * torch.as_tensor(GH_W)).sum(-1, keepdim=True)

    def variational_expectations(self, Fmu, Fvar, Y):
        p = self.prob_is_largest(Y, Fmu, Fvar)
        return p * math.log(1.0 - self.eps) + (1.0 - p) * math.log(self.eps1)

    def logp(self, F, Y):
        F = _t(F)
        idx = torch.arange(self.C).expand(F.shape)
        first = torch.where(F == F.max(-1, keepdim=True)[0], idx, torch.full_like(idx, self.C)).min(-1, keepdim=True)[0]   # tf.argmax: the first
        hit = first == _t(Y).to(torch.int64)
        return torch.where(hit, torch.full(hit.shape, math.log(1.0 - self.eps), dtype=torch.float64),
                           torch.full(hit.shape, math.log(self.eps1), dtype=torch.float64))

    def predict_density(self, Fmu, Fvar, Y):
        p = self.prob_is_largest(Y, Fmu, Fvar)
        return torch.log(p * (1.0 - self.eps) + (1.0 - p) * self.eps1)

    def predict_mean_and_var(self, Fmu, Fvar):
        Fmu = _t(Fmu)
        ps = torch.cat([self.prob_is_largest(torch.full(Fmu.shape[:-1] + (1,), float(k), dtype=torch.float64), Fmu, Fvar)
                        for k in range(self.C)], -1)
        P = ps * (1.0 - self.eps) + (1.0 - ps) * self.eps1
        return P, P - P ** 2


class MultiClassDGP(R.LikDGP):
    """``LikDGP`` with labels of width 1 against C final outputs.  The parent's ``log_weights_tensor`` removes the oracle's Gaussian
    expectation with a Y as wide as the moments; here the same expression is formed with the labels laid out over the C columns
    EXPLICITLY (what the oracle's own broadcast did), so what is subtracted is exactly what the oracle added."""

    def log_weights_tensor(self, zs, mode_vi=False):
        L_NK, glob = CpuDGP.log_weights_tensor(self, zs, mode_vi)
        mean, cov = self.final_moments()
        Yl = self.Y[:, None, :].repeat(1, self.K, 1)                  # [B, K, 1]
        assert Yl.shape[-1] == 1 and mean.shape[-1] == self.lik.C, (Yl.shape, mean.shape)
        Yw = Yl.expand(-1, -1, mean.shape[-1])
        lik_var = torch.as_tensor(self.lik_var, dtype=self.dtype)
        ve_gauss = -0.5 * math.log(2 * math.pi) - 0.5 * torch.log(lik_var) - 0.5 * ((Yw - mean) ** 2 + cov) / lik_var
        return L_NK - ve_gauss.sum(2) + self.lik.variational_expectations(mean, cov, Yl).sum(2), glob


def bound_and_gradients(spec, lik, zs, mode_vi=False):
    """(bound, per-point log p [B], {name: gradient}) by float64 autodiff, names as oracle/grad_oracle.py (MultiClass trains nothing).

    The entry 'final_var_terms' is not a gradient but the SCALE of one: p is unchanged when every latent of a sample is scaled by one
    factor (the arg-max does not move), and the final layer's kernel variance s scales all its means by sqrt(s) and all its variances by
    s.  So d bound / d s = (1/s) sum (mu g_mu / 2 + v g_v) over the final moments is zero up to the 1e-6 jitter on K_uu and the clips: a sum
    of terms that cancel.  'final_var_terms' = (1/s) sum (|mu g_mu| / 2 + |v g_v|) is what its rounding error is relative to."""
    m = MultiClassDGP(spec, lik)
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
    val = m.elbo_tensor(zs, mode_vi=mode_vi)
    mean, cov = m._last
    mean.retain_grad()
    cov.retain_grad()
    val.backward()
    grads = {k: (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.detach().numpy().copy()) for k, v in params.items()}
    s = float(m.layers[-1]["var"].detach())
    grads["final_var_terms"] = np.asarray(float((0.5 * (mean * mean.grad).abs().sum() + (cov * cov.grad).abs().sum()).detach()) / s)
    with torch.no_grad():
        logp = m.per_point(zs, mode_vi).numpy()
    return float(val.detach()), logp, grads


def make_spec(C, L=2, M=16, B=7, K=5, Dx=4, lv=True, seed=3, **kw):
    """``synthetic.make_spec`` with C final outputs, Y replaced by ONE column of labels (the arg-max of its C target functions, so every
    class occurs) and the encoder of a leading latent-variable layer narrowed to its [x, label] input of width Dx + 1."""
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=L, M=M, B=B, K=K, Dx=Dx, Dy=C, with_lv=lv, seed=seed, distinct_y=True, **kw)
    spec["Y"] = np.argmax(spec["Y"], 1).astype(np.float64)[:, None]
    spec["lik_var"] = 1.0                                        # (only the oracle's Gaussian term, which the restatement removes again)
    if lv:
        l0 = spec["layers"][0]
        rng = np.random.default_rng([seed, 0x6d63])
        l0["dims"] = [Dx + 1] + list(l0["dims"][1:])
        l0["enc_W"] = [synthetic._f32(rng.standard_normal((Dx + 1, l0["dims"][1])) * (2.0 / (Dx + 1 + l0["dims"][1])) ** 0.5)] + list(l0["enc_W"][1:])
    return spec


def moment_grid(C, seed=0):
    """Rows of C moments on the issue's ranges: mu in [-3, 3], v in [1e-4, 4] log-spaced; 600 seeded rows, among them rows with every
    variance at an end of the range."""
    rng = np.random.default_rng([seed, C])
    mu = rng.uniform(-3.0, 3.0, (600, C))
    v = np.exp(rng.uniform(np.log(1e-4), np.log(4.0), (600, C)))
    v[:8] = 1e-4
    v[8:16] = 4.0
    return mu, v


# ---- the training check's problem (tests/test_gpu_multiclass.py) ------------------------------------------------------------------
def three_class_problem(seed=17, n=300):
    """Three well-separated Gaussian blobs in the plane (Dx = 2), n points; an L = 2 stack with a leading latent-variable layer and the
    reference's initial values.  -> (spec, noise(i) -> per-layer arrays)."""
    from dgps_with_iwvi_amd import synthetic
    spec = make_spec(3, L=2, M=16, B=n, K=3, Dx=2, lv=True, seed=seed, parity=False, n_data=n)
    rng = np.random.default_rng([seed, 0x626c6f62])
    labels = rng.permutation(np.arange(n) % 3)
    labels[:10] = 0                                              # (a majority class that is not exactly a third)
    centres = np.array([[2.0, 0.0], [-1.0, 1.8], [-1.0, -1.8]])
    X = synthetic._f32(centres[labels] + 0.45 * rng.standard_normal((n, 2)))
    spec["X"], spec["Y"] = X, labels.astype(np.float64)[:, None]
    for l in spec["layers"]:                                     # inducing inputs on the data, as build_models does
        if l["type"] == "gp":
            l["Z"][:, :2] = X[:l["Z"].shape[0]]
    return spec, (lambda i: synthetic.make_noise(spec, seed=1000 + i))


def oracle_trainer(spec, lr=5e-3, gamma=1e-2):
    import copy
    from test_gpu_training import _OracleTrainer
    ot = _OracleTrainer(copy.deepcopy(spec), lr, gamma)

    def grad(sp, zs):
        val, _, g = bound_and_gradients(sp, MultiClass(3), zs)
        g.pop("final_var_terms")
        g["lik_var"] = np.zeros(())
        return val, g
    ot.grad = grad
    return ot


def oracle_accuracy(spec):
    """(training accuracy of arg-max predict_y at zero noise through the inner layers, majority-class rate) of the float64 model."""
    from oracle.from_spec import build_oracle
    B = spec["B"]
    X, Y = spec["X"][:B], spec["Y"][:B]
    zs = [np.zeros((B, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1])) for l in spec["layers"]]
    m, v = build_oracle(spec, iw=False, num_samples=1).build_predict(X, zs=zs)
    P = MultiClass(3).predict_mean_and_var(m, v)[0].numpy()
    maj = max(float((Y == k).mean()) for k in range(3))
    return float((P.argmax(1) == Y[:, 0]).mean()), maj


def oracle_training_record(steps=200):
    """The constants of tests/test_gpu_multiclass.py's training check, from the float64 loop on the CPU."""
    spec, noise = three_class_problem()
    ot = oracle_trainer(spec)
    v = np.array([ot.step(noise(2 * s), noise(2 * s + 1)) for s in range(steps)])
    acc, maj = oracle_accuracy(ot.spec)
    return dict(first=float(v[0]), late=float(v[-10:].mean()), accuracy=acc, majority=maj)
