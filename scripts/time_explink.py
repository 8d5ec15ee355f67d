"""Cost of the exp-link likelihoods' tail (Poisson, Exponential, Gamma: csrc/likelihood_explink.hip) next to the Student-t's quadrature
tail and the Gaussian's fused one, at one shape, in one session on one box: BASELINE configs[2] (L = 2, M = 128, K = 20, B = 1024,
latent-variable layer).  One evaluation (precompute + layer launch + iwvi_lik_elbo_reduce; the Gaussian: its one fused launch) and one
value + gradient (backward.iw_elbo_and_gradients) per likelihood, each as a hipGraph of 25 calls; a timing is the mean over 40 replays,
reported are median, min and max of 5 timings in microseconds per call.  The condition recorded with them: an exp-link evaluation does a
twentieth of the Student-t's transcendental work on the same three launches, so it may not be slower than the Student-t's.
Usage: python scripts/time_explink.py [--out profiles/explink_time.json]"""
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

CALLS, REPLAYS, TIMINGS = 25, 40, 5
NEW = ("poisson", "exponential", "gamma")


def models(dev):
    spec = synthetic.make_spec(L=2, M=128, B=1024, K=20, with_lv=True, seed=0, n_data=65536)
    Yz = spec["Y"]                                               # standardised regression targets
    counts = np.floor(np.exp(np.clip(Yz, -2.0, 2.5)))
    positive = np.exp(np.clip(Yz, -3.0, 3.0))
    build = lambda Y, lik: synthetic.build_model(dict(spec, Y=Y), dev, likelihood=lik)
    return {"poisson": build(counts, likelihoods.Poisson(binsize=1.5)), "exponential": build(positive, likelihoods.Exponential()),
            "gamma": build(positive, likelihoods.Gamma(shape=2.5)), "student_t": build(Yz, likelihoods.StudentT(scale=0.7, df=4.0)),
            "gaussian": build(Yz, None)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explink_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_explink.py measures on the GPU: no device here")
    dev = torch.device("cuda:0")
    res = {"note": "median, min, max of %d timings of %d replays x %d calls; microseconds per call; L2_M128_K20_B1024_LV, one output"
                   % (TIMINGS, REPLAYS, CALLS)}
    for name, model in models(dev).items():
        res[name] = {"evaluation_us": graph_us(lambda: model._build_likelihood()),
                     "value_gradient_us": graph_us(lambda: backward.iw_elbo_and_gradients(model))}
        print(name, res[name], flush=True)
    res["new_evaluations_no_slower_than_student_t"] = all(res[k]["evaluation_us"][0] <= res["student_t"]["evaluation_us"][0] for k in NEW)
    print("condition (an exp-link evaluation is no slower than the Student-t's):", res["new_evaluations_no_slower_than_student_t"])
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
