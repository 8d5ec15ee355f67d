"""Cost of exact predictive draws, ``predict_y_draws``, at the reference's evaluation size (N = 1000 test points, S = 2000 draws) on the
BASELINE configs[2] stack (L = 2, M = 128, latent-variable layer; the shape of profiles/predict_mixture_time.json), for a Poisson, a Gamma,
a Beta and a 4-class model, in one session on one box, against the same draws composed from torch device ops on the same moments:
  draws         ``predict_y_draws``: one precompute, the layer launch without a tail, ONE ``iwvi_lik_sample_y`` launch;
  torch         the same precompute and layer launch, then f = m + sqrt(v) randn and ``torch.poisson`` / ``torch._standard_gamma`` /
                ``torch.bernoulli`` + ``torch.multinomial`` on it;
  tail_launch   the ``iwvi_lik_sample_y`` launch alone, on the stored moments of one batch;
  tail_torch    the torch ops of the second route alone, on the same stored moments.
The routes alternate; a timing is the host clock around CALLS calls that end in a device synchronise; reported are median, min and max of 5
timings after a warm-up, in milliseconds per call.  No ratio is asserted: the file records what came out.
Usage: python scripts/time_lik_sample.py [--out profiles/lik_sample_time.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dgps_with_iwvi_amd import likelihoods, synthetic   # noqa: E402
from dgps_with_iwvi_amd.layers import LatentVariableLayer   # noqa: E402

N, S, CALLS, TIMINGS = 1000, 2000, 3, 5
BINSIZE, SHAPE, SCALE, C, EPS = 1.5, 2.5, 6.0, 4, 1e-3


def models(dev):
    spec = synthetic.make_spec(L=2, M=128, B=1024, K=20, with_lv=True, seed=0, n_data=65536)
    spec_c = synthetic.make_spec(L=2, M=128, B=1024, K=20, with_lv=True, seed=0, n_data=65536, Dy=C, distinct_y=True)
    labels = np.argmax(spec_c["Y"], 1).astype(np.float64)[:, None]
    l0 = spec_c["layers"][0]                                     # the encoder of the latent-variable layer reads [x, label]: Dx + 1 columns
    Dx, rng = spec_c["X"].shape[1], np.random.default_rng(0)
    l0["dims"] = [Dx + 1] + list(l0["dims"][1:])
    l0["enc_W"] = [(rng.standard_normal((Dx + 1, l0["dims"][1])) * (2.0 / (Dx + 1 + l0["dims"][1])) ** 0.5).astype(np.float32)] + list(l0["enc_W"][1:])
    y = np.clip(spec["Y"], -2.0, 2.5)
    build = lambda s, Y, lik: synthetic.build_model(dict(s, Y=Y), dev, likelihood=lik)
    return {"poisson": (build(spec, np.floor(np.exp(y)), likelihoods.Poisson(binsize=BINSIZE)), spec["X"][:N]),
            "gamma": (build(spec, np.exp(y), likelihoods.Gamma(shape=SHAPE)), spec["X"][:N]),
            "beta": (build(spec, 1.0 / (1.0 + np.exp(-y)), likelihoods.Beta(scale=SCALE)), spec["X"][:N]),
            "multiclass_C4": (build(spec_c, labels, likelihoods.MultiClass(C)), spec_c["X"][:N])}


def torch_draws(name, fm, fv):
    """The draws of ``name`` from torch device ops on moments [T, Dy]."""
    f = fm + fv.sqrt() * torch.randn_like(fm)
    if name == "poisson":
        return torch.poisson(BINSIZE * f.exp())
    if name == "gamma":
        return f.exp() * torch._standard_gamma(torch.full_like(f, SHAPE))
    if name == "beta":
        m = likelihoods.inv_probit(f)
        ga, gb = torch._standard_gamma(m * SCALE), torch._standard_gamma(SCALE - m * SCALE)
        return ga / (ga + gb)
    am = f.argmax(1)
    miss = torch.bernoulli(torch.full(am.shape, EPS, device=f.device)).to(torch.int64)
    off = 1 + torch.multinomial(torch.ones(C - 1, device=f.device), am.numel(), replacement=True)
    return ((am + miss * off) % C).to(f.dtype)[:, None]


def moments(model, X, zs):
    """The final layer's moments [N S, Dy] as ``predict_y_draws`` takes them: one precompute, the layer launch without a tail."""
    last = len(model.layers) - 1
    zb = [z.transpose(0, 1).reshape(N * S, -1) for z in zs]
    model.precompute()
    _, outs, _ = model._fused_forward(N * S, S, N, (N * S,), zs=zb, sampled_kl=False, want_layers=True, want_logw=False,
                                      use_encoder=False, X=X, outputs_for={last})
    return outs[last]["mean"], outs[last]["var"]


def timed_ms(fn):
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lik_sample_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lik_sample.py measures on the GPU: no device here")
    dev = torch.device("cuda:0")
    res = {"note": "median, min, max of %d timings of %d calls each, the routes alternating; milliseconds per call; N = %d, S = %d, "
                   "L2_M128_LV; draws / torch: predict_y_draws against the same layer launch + torch ops; tail_launch / tail_torch: the "
                   "iwvi_lik_sample_y launch against those torch ops alone, on stored moments" % (TIMINGS, CALLS, N, S)}
    for name, (model, X) in models(dev).items():
        X = torch.as_tensor(np.asarray(X, dtype=np.float32), device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        zs = [torch.randn(S, N, l.latent_dim if isinstance(l, LatentVariableLayer) else l.num_outputs, device=dev, generator=gen) for l in model.layers]
        fm, fv = (t.clone() for t in moments(model, X, zs))
        lik = model.likelihood
        routes = {"draws": lambda: model.predict_y_draws(X, S, zs=zs),
                  "torch": lambda: torch_draws(name, *moments(model, X, zs)),
                  "tail_launch": lambda: lik.sample_y(fm, fv),
                  "tail_torch": lambda: torch_draws(name, fm, fv)}
        out = {k: f() for k, f in routes.items()}                # warm-up of every shape, and the results to compare
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(TIMINGS):
            for k, f in routes.items():
                times[k].append(timed_ms(f))
        res[name] = {k: [float(np.median(t)), float(min(t)), float(max(t))] for k, t in times.items()}
        res[name]["mean_of_draws"] = {k: float(v.double().mean()) for k, v in out.items()}
        res[name]["launch_no_slower_than_torch"] = bool(res[name]["tail_launch"][0] <= res[name]["tail_torch"][0])
        print(name, res[name], flush=True)
    assert math.isfinite(sum(v for r in res.values() if isinstance(r, dict) for v in r["mean_of_draws"].values()))
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
