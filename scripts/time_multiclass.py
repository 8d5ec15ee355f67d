"""Cost of the MultiClass (robust-max) tail next to the Bernoulli's at one shape, in one session on one box: BASELINE configs[2]
(L = 2, M = 128, K = 20, B = 1024, latent-variable layer) with C = 10 final outputs.  One evaluation (precompute + layer launch +
iwvi_lik_elbo_reduce) and one value + gradient (backward.iw_elbo_and_gradients) per likelihood, each as a hipGraph of 25 calls; a timing
is the mean over 40 replays, reported are median, min and max of 5 timings in microseconds per call.
Usage: python scripts/time_multiclass.py [--out profiles/multiclass_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dgps_with_iwvi_amd import backward, likelihoods, synthetic   # noqa: E402

C, CALLS, REPLAYS, TIMINGS = 10, 25, 40, 5


def models(dev):
    spec = synthetic.make_spec(L=2, M=128, B=1024, K=20, Dy=C, with_lv=True, seed=0, n_data=65536, distinct_y=True)
    bern = dict(spec, Y=(spec["Y"] > 0).astype(np.float64))      # ten 0 / 1 columns: the Bernoulli walks C outputs per sample as well
    mc = dict(spec, Y=np.argmax(spec["Y"], 1).astype(np.float64)[:, None], layers=[dict(l) for l in spec["layers"]])
    l0 = mc["layers"][0]                                         # the encoder reads [x, label]: Dx + 1 columns
    rng = np.random.default_rng(0)
    l0["dims"] = [spec["X"].shape[1] + 1] + list(l0["dims"][1:])
    l0["enc_W"] = [np.float32(rng.standard_normal((l0["dims"][0], l0["dims"][1])) * 0.2).astype(np.float64)] + list(l0["enc_W"][1:])
    return {"bernoulli": synthetic.build_model(bern, dev, likelihood=likelihoods.Bernoulli()),
            "multiclass": synthetic.build_model(mc, dev, likelihood=likelihoods.MultiClass(C))}


def graph_us(fn):
    """Microseconds per call of ``fn`` replayed from a hipGraph of CALLS calls: [median, min, max] of TIMINGS timings."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        keep = [fn() for _ in range(CALLS)]
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(TIMINGS):
        t0 = time.perf_counter()
        for _ in range(REPLAYS):
            g.replay()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / (REPLAYS * CALLS) * 1e6)
    del keep
    return [float(np.median(out)), float(min(out)), float(max(out))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiclass_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"note": "median, min, max of %d timings of %d replays x %d calls; microseconds per call; L2_M128_K20_B1024_LV with %d final outputs"
                   % (TIMINGS, REPLAYS, CALLS, C)}
    for name, model in models(dev).items():
        res[name] = {"evaluation_us": graph_us(lambda: model._build_likelihood()),
                     "value_gradient_us": graph_us(lambda: backward.iw_elbo_and_gradients(model))}
        print(name, res[name], flush=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
