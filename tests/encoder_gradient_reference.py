"""Float64 references for the encoder-gradient estimators ("iwae" | "dreg" | "stl": include/iwvi_hip.h, IWVI_LV_GRAD_*) and for the
gradient-moments monitor (iwvi_moments_update).  TEST INFRASTRUCTURE ONLY: tests/test_encoder_gradient_reference_host.py pins this module
on the CPU (against oracle/grad_oracle.py and against itself: closed form versus stop-gradient surrogate), tests/test_gpu_encoder_gradient.py
holds the kernels to it.

Two independent statements of each estimator:

  surrogate    autograd of an objective whose gradient w.r.t. the encoder parameters IS the estimator.  With L_nk the log-weights,
               w~_nk = softmax_k(L_nk), scale = n_data / B, sg() = stop-gradient, and L'_nk = L_nk with mu and sigma DETACHED inside log q
               (the sample W = mu + eps sigma still depends on them):
                   iwae   scale sum_n (logsumexp_k L_nk - log K)             (the bound itself)
                   dreg   scale sum_nk sg(w~_nk^2) L'_nk                     (Tucker et al. 2019, eq. 8)
                   stl    scale sum_nk sg(w~_nk)   L'_nk                     (Roeder et al. 2017)
  closed form  the per-sample arithmetic the kernel does (``lv_adjoint_reference``, NumPy), fed with the cotangent of the layer above and
               the weights w = scale w~ taken from autograd of the bound, then pushed through the encoder by a vector-Jacobian product.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_torch_cpu import CpuDGP   # noqa: E402

ESTIMATORS = ("iwae", "dreg", "stl")


class EstimatorDGP(CpuDGP):
    """``CpuDGP`` whose latent-variable layers can hold the encoder's outputs fixed inside log q (``detach_q``) and keep the sample out of
    the regulariser's graph (``detach_kl_sample``: the gradient that then arrives at the sample is the cotangent of the layer above alone).
    Every latent-variable layer leaves dict(H [B, K, 2 Lw] encoder output, W the sample, z the draws) in ``self.lv``."""

    def log_weights_tensor(self, zs, mode_vi=False, detach_q=False, detach_kl_sample=False):
        if mode_vi:
            return super().log_weights_tensor(zs, mode_vi=True)
        K = self.K
        F = self.X[:, None, :].repeat(1, K, 1)
        Yt = self.Y[:, None, :].repeat(1, K, 1)
        XY = torch.cat([F, Yt], -1)
        local, glob, self.lv = [], [], []
        mean = cov = None
        for L, z in zip(self.layers, zs):
            z = None if z is None else torch.as_tensor(z, dtype=self.dtype)
            if L["type"] == "lv":
                H, n = XY, len(L["W"])
                for i, (W, b) in enumerate(zip(L["W"], L["b"])):
                    H0 = H
                    H = H @ W + b
                    if i < n - 1:
                        H = L.get("act", torch.tanh)(H)
                    if W.shape[0] == W.shape[1]:
                        H = H + H0
                mu, raw = H.split(L["Lw"], -1)
                sg = torch.nn.functional.softplus(raw - 3.0)
                Wl = mu + z * sg
                if detach_kl_sample:
                    Wl.retain_grad()
                self.lv.append(dict(H=H, W=Wl, z=z))
                F = torch.cat([F, Wl], -1)
                Wk = Wl.detach() if detach_kl_sample else Wl
                mq, sq = (mu.detach(), sg.detach()) if detach_q else (mu, sg)
                local.append((-0.5 * ((Wk - mq) / sq) ** 2 - torch.log(sq)) - (-0.5 * Wk ** 2))      # log q(W) - log p(W)
                continue
            if L["W"] is not None:
                s, m, v = self._conditional(L, F, False, z)
                s, m, v = s @ L["W"].T, m @ L["W"].T, v @ (L["W"] ** 2).T
                mf = F @ L["A"] if L["A"] is not None else 0.0
                F, mean, cov = s + mf, m + mf, v
            else:
                _, mean, cov = self._conditional(L, F, True, None)
                F = mean
            M, R = L["q_mu"].shape
            Lq = L["q_sqrt"]
            glob.append(0.5 * ((L["q_mu"] ** 2).sum() - M * R - torch.log(torch.diagonal(Lq, dim1=-2, dim2=-1) ** 2).sum() + (Lq ** 2).sum()))
        if cov.dim() == 4:
            cov = torch.diagonal(cov, dim1=-2, dim2=-1).transpose(1, 2)
        lik_var = torch.as_tensor(self.lik_var, dtype=self.dtype)
        ve = -0.5 * math.log(2 * math.pi) - 0.5 * torch.log(lik_var) - 0.5 * ((Yt - mean) ** 2 + cov) / lik_var
        L_NK = ve.sum(2)
        for kl in local:
            L_NK = L_NK - kl.sum(2)
        return L_NK, sum(glob)


def _with_encoder_leaves(spec):
    m = EstimatorDGP(spec, torch.float64)
    params = {}
    for i, L in enumerate(m.layers):
        if L["type"] == "lv":
            L["W"] = [w.clone().requires_grad_(True) for w in L["W"]]
            L["b"] = [b.clone().requires_grad_(True) for b in L["b"]]
            for j, (w, b) in enumerate(zip(L["W"], L["b"])):
                params["l%d.encW%d" % (i, j)], params["l%d.encb%d" % (i, j)] = w, b
    return m, params


def _bound(m, L_NK, glob):
    B, K = L_NK.shape
    return (torch.logsumexp(L_NK, 1) - math.log(K)).sum() * (m.n_data / B) - glob


def surrogate_gradients(spec, zs, estimator):
    """-> (the bound, {'l<i>.encW<j>' / 'l<i>.encb<j>': ndarray}) by autograd of the estimator's surrogate objective."""
    if estimator not in ESTIMATORS:
        raise ValueError(estimator)
    m, params = _with_encoder_leaves(spec)
    L_NK, glob = m.log_weights_tensor(zs, detach_q=estimator != "iwae")
    B = L_NK.shape[0]
    bound = _bound(m, L_NK, glob)
    if estimator == "iwae":
        obj = bound
    else:
        wn = torch.softmax(L_NK.detach(), 1)
        obj = ((wn ** 2 if estimator == "dreg" else wn) * L_NK).sum() * (m.n_data / B)
    names = list(params)
    grads = torch.autograd.grad(obj, [params[n] for n in names], allow_unused=True)
    return float(bound.detach()), {n: (np.zeros(tuple(params[n].shape)) if g is None else g.numpy().copy()) for n, g in zip(names, grads)}


def lv_adjoint_reference(mu, raw, eps, dF, col0, w, K, estimator, w_unit=1.0, sampled=True):
    """The latent-variable layer's adjoint in NumPy float64, as include/iwvi_hip.h states it: mu, raw [B, Lw] (sigma = softplus(raw - 3)),
    eps [B K, Lw], dF [B K, ld] or None (columns col0 ... are the layer's), w [B K] or None -> d (means | raw) [B, 2 Lw]."""
    mu, raw, eps = (np.asarray(a, dtype=np.float64) for a in (mu, raw, eps))
    B, Lw = mu.shape
    sg = np.log1p(np.exp(raw - 3.0))
    e = eps.reshape(B, K, Lw)
    W = mu[:, None, :] + e * sg[:, None, :]
    dfw = np.zeros_like(e) if dF is None else np.asarray(dF, dtype=np.float64)[:, col0:col0 + Lw].reshape(B, K, Lw)
    wt = np.zeros((B, K, 1)) if w is None else np.asarray(w, dtype=np.float64).reshape(B, K, 1)
    s = sg[:, None, :]
    if not sampled:                                              # the analytic regulariser (DGP_VI): "iwae" only
        if estimator != "iwae":
            raise ValueError("the analytic regulariser has the 'iwae' estimator only")
        dmu = (dfw - wt * mu[:, None, :]).sum(1)
        dsg = (dfw * e - wt * (s - 1.0 / s)).sum(1)
    elif estimator == "iwae":
        dW = dfw - wt * W
        dmu, dsg = dW.sum(1), (dW * e + wt / s).sum(1)
    else:
        T = dfw + wt * (e / s - W)
        if estimator == "dreg":
            T = (wt / w_unit) * T
        elif estimator != "stl":
            raise ValueError(estimator)
        dmu, dsg = T.sum(1), (T * e).sum(1)
    return np.concatenate([dmu, dsg * (1.0 - np.exp(-sg))], 1)


def closed_form_gradients(spec, zs, estimator):
    """-> {'l<i>.encW<j>' / 'l<i>.encb<j>': ndarray}: ``lv_adjoint_reference`` on the cotangents and weights autograd gives for the bound,
    then the encoder's vector-Jacobian product."""
    return closed_form_gradients_of(spec, zs, (estimator,))[estimator]


def closed_form_gradients_of(spec, zs, estimators=ESTIMATORS):
    """``closed_form_gradients`` of several estimators from ONE forward and one backward of the bound -> {estimator: {name: ndarray}}."""
    m, params = _with_encoder_leaves(spec)
    L_NK, glob = m.log_weights_tensor(zs, detach_q=True, detach_kl_sample=True)
    B, K = L_NK.shape
    _bound(m, L_NK, glob).backward(retain_graph=True)             # the samples' .grad = the cotangent of the layer above
    for p in params.values():
        p.grad = None
    scale = m.n_data / B
    w = (scale * torch.softmax(L_NK.detach(), 1)).numpy().reshape(-1)
    out, saved = {e: {} for e in estimators}, iter(m.lv)                                  # (m.lv: one entry per latent-variable layer, in layer order)
    for i, L in enumerate(m.layers):
        if L["type"] != "lv":
            continue
        s = next(saved)
        Lw = L["Lw"]
        H = s["H"].detach().numpy()[:, 0, :]                      # (the encoder's rows do not depend on k)
        dfw = s["W"].grad.numpy().reshape(B * K, Lw)
        names = [n for n in params if n.startswith("l%d." % i)]
        for est in estimators:
            d_enc = lv_adjoint_reference(H[:, :Lw], H[:, Lw:], s["z"].numpy().reshape(B * K, Lw), dfw, 0, w, K, est, w_unit=scale)
            # every one of the K copies of a row is the same function of the parameters: the cotangent goes to copy 0
            cot = torch.zeros_like(s["H"])
            cot[:, 0, :] = torch.as_tensor(d_enc)
            gr = torch.autograd.grad(s["H"], [params[n] for n in names], grad_outputs=cot, retain_graph=True)
            out[est].update({n: g.numpy().copy() for n, g in zip(names, gr)})
    return out


def welford_reference(xs):
    """The Welford recurrence of iwvi_moments_update over ``xs`` [R, n] in float64 -> (mean [n], m2 [n], count)."""
    xs = np.asarray(xs, dtype=np.float64)
    mean, m2 = np.zeros(xs.shape[1]), np.zeros(xs.shape[1])
    for c, x in enumerate(xs, 1):
        d = x - mean
        mean = mean + d / c
        m2 = m2 + d * (x - mean)
    return mean, m2, xs.shape[0]
