"""Cost of the bounded-target likelihoods' tail (Beta, Ordinal: csrc/likelihood_bounded.hip) next to the Student-t's and the Bernoulli's
quadrature tails, at one shape, in one session on one box: BASELINE configs[2] (L = 2, M = 128, K = 20, B = 1024, latent-variable
layer).  One evaluation (precompute + layer launch + iwvi_lik_elbo_reduce) and one value + gradient (backward.iw_elbo_and_gradients) per
likelihood, each as a hipGraph of 25 calls; a timing is the mean over 40 replays, reported are median, min and max of 5 timings in
microseconds per call.  No threshold: nothing in the project gives one for these two (a Beta node is two erfc, two lgamma and, for the
heads, two digamma -- several times a Bernoulli node).  The file is the record the next change to the tails' speed measures against.
Usage: python scripts/time_bounded.py [--out profiles/bounded_time.json]"""
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
from dgps_with_iwvi_amd import backward, likelihoods, synthetic   # noqa: E402

CALLS, REPLAYS, TIMINGS = 25, 40, 5


def models(dev):
    spec = synthetic.make_spec(L=2, M=128, B=1024, K=20, with_lv=True, seed=0, n_data=65536)
    Yz = spec["Y"]                                               # standardised regression targets
    edges = (-0.8, 0.0, 0.9)
    unit = 0.5 * (1.0 + np.vectorize(math.erf)(Yz / math.sqrt(2.0)))      # in (0, 1)
    grades = np.searchsorted(np.asarray(edges), Yz).astype(np.float64)
    build = lambda Y, lik: synthetic.build_model(dict(spec, Y=Y), dev, likelihood=lik)
    return {"beta": build(unit, likelihoods.Beta(scale=2.5)), "ordinal": build(grades, likelihoods.Ordinal(edges)),
            "student_t": build(Yz, likelihoods.StudentT(scale=0.7, df=4.0)), "bernoulli": build((Yz > 0).astype(np.float64), likelihoods.Bernoulli())}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bounded_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bounded.py measures on the GPU: no device here")
    dev = torch.device("cuda:0")
    res = {"note": "median, min, max of %d timings of %d replays x %d calls; microseconds per call; L2_M128_K20_B1024_LV, one output"
                   % (TIMINGS, REPLAYS, CALLS)}
    for name, model in models(dev).items():
        res[name] = {"evaluation_us": graph_us(lambda: model._build_likelihood()),
                     "value_gradient_us": graph_us(lambda: backward.iw_elbo_and_gradients(model))}
        print(name, res[name], flush=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
