#!/usr/bin/env python3
"""``iwvi_kde_density_grid`` against the only route the library had for a density picture, G launches of ``iwvi_kde_loglik`` over the
same samples, at two shapes:

  demo       N = 200 inputs, S = 10 000 samples, G = 200 levels   (the reference's experiments/demo.py: plot_density)
  evaluate   N = 1000, S = 2000, G = 32                           (a grid beside ``evaluate``'s statistics)

Samples are [N, S]-contiguous (what ``predict_y_samples_fused`` writes), levels shared.  Per route: one warm-up, then the median of
``--reps`` runs timed with events around the launches only.  ``sklearn.neighbors.KernelDensity`` is timed on the CPU for ONE point of the
demo shape (fit + the reference's 200 ``score`` calls, and one ``score_samples`` over the 200 levels), when sklearn imports.

  python3 scripts/time_density_grid.py [--reps 7] [--out profiles/kde_grid_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgps_with_iwvi_amd import _abi, evaluation   # noqa: E402

SHAPES = {"demo": dict(N=200, S=10000, G=200), "evaluate": dict(N=1000, S=2000, G=32)}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [float(v) for v in ms]


def sklearn_one_point(x, levels, reps):
    try:
        from sklearn.neighbors import KernelDensity
    except ImportError:
        return None
    x64, l64 = x.astype(np.float64).reshape(-1, 1), levels.astype(np.float64)
    h = 1.06 * x64.std() * len(x64) ** -0.2
    loop, batch = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        kde = KernelDensity(bandwidth=float(h)).fit(x64)
        for level in l64:                                        # the reference's loop: one score call per level
            kde.score(np.array(level).reshape(1, 1))
        loop.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        KernelDensity(bandwidth=float(h)).fit(x64).score_samples(l64.reshape(-1, 1))
        batch.append(1e3 * (time.perf_counter() - t0))
    return dict(per_level_score_calls_ms=float(np.median(loop)), one_score_samples_call_ms=float(np.median(batch)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error("--reps must be at least 5 (the median of at least five runs)")
    dev = torch.device("cuda:0")
    lib = _abi.lib()
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, shapes={})
    for name, sh in SHAPES.items():
        N, S, G = sh["N"], sh["S"], sh["G"]
        rng = np.random.default_rng(S)
        z = rng.standard_normal((N, S))
        host = np.where(rng.random((N, S)) < 0.4, 0.3 * z - 0.5, 0.5 * z + 1.0).astype(np.float32)     # two modes inside [-1, 2]
        levels = np.linspace(-1.0, 2.0, G).astype(np.float32)
        smp = torch.as_tensor(host, device=dev).t()              # [S, N] view of [N, S]
        lev = torch.as_tensor(levels, device=dev)
        ys = lev[:, None].expand(G, N).contiguous()              # the baseline's y per launch
        logp = torch.empty(G, N, dtype=torch.float32, device=dev)
        base_smp = smp.t()                                       # [N, S] contiguous
        ptrs = [(_abi.ptr(ys[g]), _abi.ptr(logp[g])) for g in range(G)]      # (formed once: the loop below is launches only)

        def grid():
            return evaluation.kde_log_density_grid(smp, lev)

        def launches():
            st = _abi.stream_ptr()
            src = _abi.ptr(base_smp)
            for y, out in ptrs:
                _abi.check(lib.iwvi_kde_loglik(src, 1, S, y, N, S, out, None, None, st))

        row = dict(sh)
        row["grid_ms"], row["grid_all_ms"] = timed(grid, a.reps)
        row["g_launches_ms"], row["g_launches_all_ms"] = timed(launches, a.reps)
        row["speedup"] = row["g_launches_ms"] / row["grid_ms"]
        row["kernel_evaluations"] = N * S * G
        row["grid_gevals_per_s"] = N * S * G / row["grid_ms"] * 1e-6
        row["max_abs_difference_of_the_two"] = float((grid()["logdens"].t() - logp).abs().max())
        if name == "demo":
            row["sklearn_cpu_one_point"] = sklearn_one_point(host[0], levels, 5)
        res["shapes"][name] = row
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
