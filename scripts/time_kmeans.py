#!/usr/bin/env python3
"""``iwvi_kmeans`` against ``scipy.cluster.vq.kmeans2`` on the same array and the same start, at two shapes:

  large      N = 500 000, D = 8, M = 128   (the larger regression sets the reference's script accepts)
  workload   N = 45 000,  D = 9, M = 128

Standard normal float32 data (seed 0), the start SciPy's ``minit="points"`` takes after ``np.random.seed(0)``, ten iterations.
Device: one warm-up call, then ``--reps`` calls, each bracketed by a stream synchronisation and timed on the host clock (median, minimum
and maximum are recorded); the upload of X (host float32 -> device, synchronised) is timed the same way and reported separately.  Host:
SciPy on the float64 copy of the same values, ``--host-reps`` calls on this machine's CPU (it runs in one thread).  The comparison the
device route has to win is host against device + upload at the large shape.  The centroids of the two routes are compared too.

  python3 scripts/time_kmeans.py [--reps 20] [--host-reps 3] [--out profiles/kmeans_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.cluster.vq import kmeans2

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgps_with_iwvi_amd import _abi   # noqa: E402

SHAPES = {"large": dict(N=500000, D=8, M=128), "workload": dict(N=45000, D=9, M=128)}
ITERS = 10


def spread(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), repeats=len(ms))


def wall(fn, reps):
    """Each call between two synchronisations, on the host clock."""
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.reps < 5 or a.host_reps < 1:
        ap.error("--reps must be at least 5 (the median of at least five calls), --host-reps at least 1")
    dev = torch.device("cuda:0")
    lib = _abi.lib()
    res = dict(device=torch.cuda.get_device_name(0), iters=ITERS, shapes={})
    for name, sh in SHAPES.items():
        N, D, M = sh["N"], sh["D"], sh["M"]
        X = np.random.RandomState(0).randn(N, D).astype(np.float32)
        np.random.seed(0)
        start = X[np.random.choice(N, size=M, replace=False)].copy()
        state = {}

        def upload():
            state["X"] = torch.as_tensor(X, device=dev)

        upload()
        Z0 = torch.as_tensor(start, device=dev)
        Z = torch.empty(M, D, dtype=torch.float32, device=dev)
        Z64 = torch.empty(M, D, dtype=torch.float64, device=dev)
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.iwvi_kmeans_ws_bytes(N, M, D), dtype=torch.uint8, device=dev)

        def device():
            _abi.check(lib.iwvi_kmeans(_abi.ptr(state["X"]), N, D, _abi.ptr(Z0), M, ITERS, _abi.ptr(Z), _abi.ptr(Z64), _abi.ptr(labels),
                                       None, None, _abi.ptr(ws), _abi.stream_ptr()))

        wall(device, 1)                                           # warm-up: code objects, the LDS attribute
        row = dict(sh, workspace_bytes=int(ws.numel()))
        row["device"] = spread(wall(device, a.reps))
        row["upload"] = spread(wall(upload, a.reps))
        X64, start64 = X.astype(np.float64), start.astype(np.float64)
        host_ms = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            hz, hl = kmeans2(X64, start64, iter=ITERS, minit="matrix")
            host_ms.append(1e3 * (time.perf_counter() - t0))
        row["host_scipy"] = spread(host_ms)
        row["device_plus_upload_ms"] = row["device"]["median_ms"] + row["upload"]["median_ms"]
        row["host_over_device"] = row["host_scipy"]["median_ms"] / row["device"]["median_ms"]
        row["host_over_device_plus_upload"] = row["host_scipy"]["median_ms"] / row["device_plus_upload_ms"]
        row["max_abs_centroid_difference"] = float(np.abs(Z64.cpu().numpy() - hz).max())
        row["labels_differing"] = int((labels.cpu().numpy() != hl).sum())
        row["distance_terms_per_s"] = ITERS * N * M * D / row["device"]["median_ms"] * 1e3
        res["shapes"][name] = row
    res["device_route_faster_at_large"] = bool(res["shapes"]["large"]["host_over_device_plus_upload"] > 1.0)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not res["device_route_faster_at_large"]:
        sys.exit("the device route, upload included, is not faster than SciPy at N = 500 000")
    return res


if __name__ == "__main__":
    main()
