"""What the importance-sampled held-out log density costs, and what it says about its two proposals, in one session on one box:

  launch     ``iwvi_psis_summary`` (moments mode, one regulariser array: log-weight, raw, ESS, khat, PSIS in ONE launch) against the same
             quantities from torch device ops on the same moments at N = 1000, S = 5000: the log-weight, ``logsumexp``, the ESS, ``sort``,
             the tail gathered, and the generalized-Pareto fit and the smoothed tail as batched float64 torch ops.  Device events, median
             of 20 launches after 3, milliseconds; the largest khat difference between the two is recorded with them.
  call       ``importance_log_density`` (encoder and prior proposals) next to ``predict_log_density`` at N = 1000, S = 5000 on the
             BASELINE configs[2] stack (L = 2, M = 128, a leading latent-variable layer): host clock around calls ending in a
             synchronise, median of 5 after a warm-up, milliseconds per call.
  proposals  one ``L1`` model (M = 32) trained for 2000 iterations on the bimodal toy problem of scripts/run_experiment.py, ONE seed, ONE data
             set: ``evaluate_importance`` with S = 5000 on 500 held-out points from the encoder and from the prior.
No speed threshold: what is measured is reported.
Usage: python scripts/time_importance.py [--out profiles/importance_time.json] [--iterations 2000]"""
import argparse
import json
import math
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from dgps_with_iwvi_amd import build_models, evaluation, psis, synthetic   # noqa: E402

N, S = 1000, 5000
LOG_TINY = math.log(2.0 ** -126)


def torch_composition(fm, fv, Y, kl, s):
    """The launch's outputs from torch ops: float32 up to the sorted log-weights, float64 from the exceedances on (as the kernel)."""
    Nn = Y.shape[0]
    n = fm.shape[0] // Nn
    e = Y[:, None, :] - fm.view(Nn, n, -1)
    tv = fv.view(Nn, n, -1) + s
    lw = (-0.5 * torch.log(2 * math.pi * tv) - 0.5 * e * e / tv).sum(-1) - kl.view(Nn, n, -1).sum(-1)
    mx = lw.max(1, keepdim=True).values
    w = torch.exp(lw - mx).double()
    s1 = w.sum(1)
    raw = mx[:, 0].double() + torch.log(s1) - math.log(n)
    ess = s1 * s1 / (w * w).sum(1)
    x = torch.sort(lw - mx, 1).values.double()
    M = int(math.ceil(min(0.2 * n, 3.0 * math.sqrt(n))))
    cutoff = x[:, n - M - 1:n - M].clamp_min(LOG_TINY)
    tail = x[:, n - M:]                                          # (continuous weights: no ties at the cutoff, every point has M tail entries)
    ec = torch.exp(cutoff)
    ex = torch.exp(tail) - ec
    m = 30 + int(math.floor(math.sqrt(M)))
    j = torch.arange(1, m + 1, dtype=torch.float64, device=x.device)
    b = (1.0 - torch.sqrt(m / (j - 0.5)))[None, :] / (3.0 * ex[:, int(math.floor(M / 4.0 + 0.5)) - 1:int(math.floor(M / 4.0 + 0.5))]) + 1.0 / ex[:, -1:]
    k = torch.log1p(-b[:, :, None] * ex[:, None, :]).mean(2)
    L = M * (torch.log(-b / k) - k - 1.0)
    wj = torch.softmax(L, 1)
    wj = torch.where(wj < 10.0 * 2.0 ** -52, torch.zeros_like(wj), wj)
    wj = wj / wj.sum(1, keepdim=True)
    bp = (wj * b).sum(1, keepdim=True)
    kp = torch.log1p(-bp * ex).mean(1, keepdim=True)
    sigma = -kp / bp
    khat = (M * kp + 5.0) / (M + 10.0)
    p = ((torch.arange(1, M + 1, dtype=torch.float64, device=x.device) - 0.5) / M)[None, :]
    q = sigma * torch.expm1(-khat * torch.log1p(-p)) / khat
    sm = torch.log(q + ec).clamp_max(0.0)
    body = torch.exp(x[:, :n - M]).sum(1)
    ps = mx[:, 0].double() + torch.log(body + torch.exp(sm).sum(1)) - math.log(n)
    return raw, ess, khat[:, 0], ps


def events_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return [float(np.median(ts)), float(min(ts)), float(max(ts))]


def host_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(ts)), float(min(ts)), float(max(ts))]


def launch_part(dev):
    g = torch.Generator(device=dev).manual_seed(0)
    Y = torch.randn(N, 1, device=dev, generator=g)
    fm = (Y[:, None, :] + 0.8 * torch.randn(N, S, 1, device=dev, generator=g)).reshape(N * S, 1).contiguous()
    fv = (0.01 + 0.5 * torch.rand(N * S, 1, device=dev, generator=g)).contiguous()
    kl = torch.randn(N * S, 1, device=dev, generator=g).contiguous()
    s = 0.05
    out = {k: torch.empty(N, device=dev) for k in psis.KEYS}
    kern = lambda: psis.summarise(N, S, S, 1, fmean=fm, fvar=fv, Y=Y, Dy=1, lik_variance=s, kls=[kl], out=out)
    comp = lambda: torch_composition(fm, fv, Y, kl, s)
    kern()
    ref = comp()
    torch.cuda.synchronize()
    res = {"iwvi_psis_summary_ms": events_ms(kern), "torch_composition_ms": events_ms(comp),
           "max_abs_khat_difference": float((out["khat"].double() - ref[2]).abs().max()),
           "max_abs_psis_difference": float((out["psis"].double() - ref[3]).abs().max()),
           "max_abs_raw_difference": float((out["raw"].double() - ref[0]).abs().max())}
    # the launch on ready-made log-weights (terms mode, one column), and its sort-and-sums part alone (no fit below S = 21 -- here: raw and ess only)
    lw = torch.randn(N, S, device=dev, generator=g) * 2.0
    res["iwvi_psis_summary_logw_ms"] = events_ms(lambda: psis.summarise(N, S, S, 1, terms=lw, out=out))
    res["torch_logsumexp_only_ms"] = events_ms(lambda: torch.logsumexp(lw, 1))
    res["torch_sort_only_ms"] = events_ms(lambda: torch.sort(lw, 1))
    return res


def call_part(dev):
    spec = synthetic.make_spec(L=2, M=128, B=1024, K=20, with_lv=True, seed=0, n_data=65536)
    model = synthetic.build_model(spec, dev)
    X, Y = (torch.as_tensor(np.asarray(a[:N], dtype=np.float32), device=dev) for a in (spec["X"], spec["Y"]))
    return {"importance_log_density_encoder_ms": host_ms(lambda: model.importance_log_density(X, Y, S)),
            "importance_log_density_prior_ms": host_ms(lambda: model.importance_log_density(X, Y, S, proposal="prior")),
            "predict_log_density_ms": host_ms(lambda: model.predict_log_density(X, Y, S))}


def proposals_part(dev, iterations):
    from run_experiment import bimodal_data
    seed = 0
    rng = np.random.default_rng(seed)
    np.random.seed(seed)
    X, Y = bimodal_data(2000, rng)
    Xs, Ys = bimodal_data(500, rng)
    mu, sd = Y.mean(), Y.std()
    Y, Ys = (Y - mu) / sd, (Ys - mu) / sd
    ARGS = types.SimpleNamespace(mode="IWAE", configuration="L1", M=32, num_IW_samples=5, minibatch_size=256, likelihood_variance=1e-2,
                                 gamma=1e-2, gamma_decay=0.98, lr=5e-3, lr_decay=0.98, fix_linear=True, use_graph=True)
    model = build_models.build_model(ARGS, X.astype(np.float32), Y.astype(np.float32), device=dev)
    for _ in range(iterations):
        model.train_op()
    torch.cuda.synchronize()
    res = {"model": "L1, M = 32, K = 5, %d iterations, bimodal toy data (2000 training, 500 held-out points), seed %d" % (iterations, seed), "S": S}
    for proposal in ("encoder", "prior"):
        res[proposal] = evaluation.evaluate_importance(model, Xs, Ys, S, proposal=proposal)
    res["predict_log_density_mean"] = float(model.predict_log_density(
        torch.as_tensor(Xs.astype(np.float32), device=dev), torch.as_tensor(Ys.astype(np.float32), device=dev), S).double().mean())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "importance_time.json"))
    ap.add_argument("--iterations", type=int, default=2000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_importance.py measures on the GPU: no device here")
    dev = torch.device("cuda:0")
    res = {"note": "N = %d, S = %d.  launch: device events, [median, min, max] of 20 after 3, ms.  call: host clock around a call ending in a "
                   "synchronise, [median, min, max] of 5 after a warm-up, ms, L2_M128_LV.  proposals: one seed, one data set." % (N, S)}
    res["launch"] = launch_part(dev)
    print("launch", res["launch"], flush=True)
    res["call"] = call_part(dev)
    print("call", res["call"], flush=True)
    res["proposals"] = proposals_part(dev, a.iterations)
    print("proposals", res["proposals"], flush=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
