#!/usr/bin/env python3
"""``evaluation.evaluate`` at the reference's evaluation size (1000 test points x 2000 samples per point,
run_conditional_density_estimation.py:27-28), BASELINE configs[2] and configs[3] stacks, three routes:

  host_no_shapiro   evaluate()                 layer-by-layer predict_y_samples + iwvi_kde_loglik; two metrics
  host_shapiro      evaluate(shapiro=True)     the same + every sample copied to the host, scipy.stats.shapiro per test point
  on_device         evaluate(on_device=True)   predict_y_samples_fused + one iwvi_sample_stats launch; all three metrics

Wall time per call from CUDA events around the whole call (the read-back of the results included), median of ``--reps`` after one
warm-up.  The kernel split comes from a ``rocprofv3 --kernel-trace --stats -- python3 scripts/time_evaluate.py --reps 1`` run of the same
script.

  python3 scripts/time_evaluate.py [--reps 5] [--N 1000] [--S 2000] [--out file.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgps_with_iwvi_amd import evaluation, synthetic   # noqa: E402

STACKS = {"configs[2]": dict(L=2, M=128, with_lv=True), "configs[3]": dict(L=3, M=256, with_lv=False)}
ROUTES = {"host_no_shapiro": dict(), "host_shapiro": dict(shapiro=True), "on_device": dict(on_device=True)}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()                                               # (ends in the read-back of its results: the host part is inside the events)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [float(v) for v in ms], out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--S", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    res = dict(N=a.N, S=a.S, reps=a.reps, stacks={})
    for name, kw in STACKS.items():
        spec = synthetic.make_spec(B=1024, K=1, seed=2, n_data=max(1024, a.N), **kw)
        model = synthetic.build_model(spec, dev)
        X = torch.as_tensor(np.asarray(spec["X"][:a.N], np.float32), device=dev)
        Y = torch.as_tensor(np.asarray(spec["Y"][:a.N], np.float32), device=dev)
        row = {}
        for route, opts in ROUTES.items():
            t, all_ms, out = timed(lambda: evaluation.evaluate(model, X, Y, a.S, a.N, **opts), a.reps)
            row[route + "_ms"] = t
            row[route + "_all_ms"] = all_ms
            row[route + "_result"] = {k: float(v) for k, v in out.items()}
        row["on_device_vs_host_no_shapiro"] = row["host_no_shapiro_ms"] / row["on_device_ms"]
        row["on_device_vs_host_shapiro"] = row["host_shapiro_ms"] / row["on_device_ms"]
        res["stacks"][name] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
