"""Cost of ``predict_log_density`` for a non-Gaussian likelihood by its two routes, at the reference's evaluation size (N = 1000 test points,
S = 2000 draws) on the BASELINE configs[2] stack (L = 2, M = 128, latent-variable layer), in one session on one box:
  mixture    ``predict_log_density`` as it is now: per batch one precompute, the layer launch and ONE ``iwvi_lik_predict_mixture`` launch;
  layerwise  ``_predict_log_density_layerwise``, the route it replaces: one launch per layer (``predict_f_multisample``), Y expanded to
             [S, N, .], an elementwise ``iwvi_lik_predict_density`` launch over [S, N, .] and a torch ``logsumexp``.
Both on the same injected noise for a MultiClass (C = 4) and a Poisson model; the two routes alternate, a timing is the host clock around
CALLS calls that end in a device synchronise, reported are median, min and max of 5 timings after a warm-up, in milliseconds per call,
and the largest difference between the two routes' results.  The condition recorded with them: the new route is not slower.
Usage: python scripts/time_predict_mixture.py [--out profiles/predict_mixture_time.json]"""
import argparse
import json
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


def models(dev):
    C = 4
    spec = synthetic.make_spec(L=2, M=128, B=1024, K=20, with_lv=True, seed=0, n_data=65536)
    spec_c = synthetic.make_spec(L=2, M=128, B=1024, K=20, with_lv=True, seed=0, n_data=65536, Dy=C, distinct_y=True)
    labels = np.argmax(spec_c["Y"], 1).astype(np.float64)[:, None]
    l0 = spec_c["layers"][0]                                     # the encoder of the latent-variable layer reads [x, label]: Dx + 1 columns
    Dx, rng = spec_c["X"].shape[1], np.random.default_rng(0)
    l0["dims"] = [Dx + 1] + list(l0["dims"][1:])
    l0["enc_W"] = [(rng.standard_normal((Dx + 1, l0["dims"][1])) * (2.0 / (Dx + 1 + l0["dims"][1])) ** 0.5).astype(np.float32)] + list(l0["enc_W"][1:])
    counts = np.floor(np.exp(np.clip(spec["Y"], -2.0, 2.5)))
    return {"multiclass_C4": (synthetic.build_model(dict(spec_c, Y=labels), dev, likelihood=likelihoods.MultiClass(C)), spec_c["X"][:N], labels[:N]),
            "poisson": (synthetic.build_model(dict(spec, Y=counts), dev, likelihood=likelihoods.Poisson(binsize=1.5)), spec["X"][:N], counts[:N])}


def timed_ms(fn):
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_mixture_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_predict_mixture.py measures on the GPU: no device here")
    dev = torch.device("cuda:0")
    res = {"note": "median, min, max of %d timings of %d calls each, the two routes alternating; milliseconds per predict_log_density call; "
                   "N = %d, S = %d, L2_M128_LV" % (TIMINGS, CALLS, N, S)}
    ok = True
    for name, (model, X, Y) in models(dev).items():
        X, Y = (torch.as_tensor(np.asarray(a_, dtype=np.float32), device=dev) for a_ in (X, Y))
        gen = torch.Generator(device=dev).manual_seed(1)
        zs = [torch.randn(S, N, l.latent_dim if isinstance(l, LatentVariableLayer) else l.num_outputs, device=dev, generator=gen) for l in model.layers]
        routes = {"mixture": lambda: model.predict_log_density(X, Y, S, zs=zs),
                  "layerwise": lambda: model._predict_log_density_layerwise(X, Y, S, zs=zs)}
        out = {k: f() for k, f in routes.items()}                # warm-up of every shape, and the results to compare
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(TIMINGS):
            for k, f in routes.items():
                times[k].append(timed_ms(f))
        res[name] = {k: [float(np.median(t)), float(min(t)), float(max(t))] for k, t in times.items()}
        res[name]["max_abs_difference"] = float((out["mixture"] - out["layerwise"]).abs().max())
        res[name]["max_abs_log_density"] = float(out["layerwise"].abs().max())
        print(name, res[name], flush=True)
        ok = ok and res[name]["mixture"][0] <= res[name]["layerwise"][0]
    res["mixture_route_no_slower_than_layerwise"] = ok
    print("condition (the one-launch mixture route is no slower than the layer-wise one):", ok)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
