#!/usr/bin/env python3
"""The scoring-rule launches at the evaluation's own size (N = 1000 test points x S = 2000 draws per point), written to
profiles/scores_time.json:

  sample_scores   one ``iwvi_sample_scores`` launch (CRPS in both forms, the PIT's counts, five quantiles and their pinball loss; raw, into
                  preallocated outputs -- ``sample_scores_python_call`` is ``evaluation.sample_scores`` with its allocations and the
                  upload of the quantile levels) against
                  the ``iwvi_sample_stats`` launch on the same samples (the sort's own cost, with its KDE and five quantiles) and against
                  the same scores from torch device ops (``sort``, a weighted sum, comparisons; float64 sums like the kernel's)
  energy_score    one ``iwvi_energy_score`` launch at D = 2, 8, 32 against ``torch.cdist`` over chunks of ``--chunk`` points (its
                  [chunk, S, S] float32 intermediate: 16 MB per point at S = 2000), in both of cdist's modes: the default, which forms
                  the distances from a matrix product (the Gram form: fast, and wrong for tight samples), and the difference form
  evaluate        the whole ``evaluate_scores`` call next to ``evaluate_draws`` on the same model (BASELINE configs[2] stack)

``--compare-lib <path to another build's libiwvi_hip.so>``: also that build's ``iwvi_sample_stats`` launch on the same samples, the two
builds alternating launch by launch (the question the shared sort header raises: did moving the sort slow ``k_sample_stats`` down).

Per launch a pair of device events; the median of ``--reps`` (>= 20) timed launches after ``--warmup`` untimed ones, and the spread
(min, max) beside it.  Samples are stored [N, S] / [N, S, D] (a point's draws contiguous), what ``predict_y_draws`` returns.

  python3 scripts/time_scores.py [--reps 20] [--N 1000] [--S 2000] [--chunk 50] [--out profiles/scores_time.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgps_with_iwvi_amd import _abi, evaluation, synthetic   # noqa: E402

PROBS = [0.05, 0.25, 0.5, 0.75, 0.95]


def timed(fn, reps, warmup):
    for _ in range(warmup):
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
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), launches=reps)


def timed_alternating(fns, reps, warmup):
    """{name: fn}: one launch of each in turn, ``reps`` rounds -- two builds compared under the same neighbours and clocks."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), launches=reps) for k, v in ms.items()}


def torch_scores(x, y, w):
    """x [S, N] float32, y [N], w [S] float64 = 2i - S - 1: the CRPS terms and the counts from torch ops."""
    xs = x.sort(0).values.double()
    G = (w[:, None] * xs).sum(0)
    A = (x.double() - y.double()[None, :]).abs().mean(0)
    S = x.shape[0]
    return A - G / S ** 2, A - G / (S * (S - 1.0)), (x < y[None, :]).sum(0), (x == y[None, :]).sum(0)


def torch_energy(x, Y, chunk, mode):
    """x [N, S, D], Y [N, D]: A - B / S^2 through torch.cdist over chunks of points; the pair sum in float64."""
    N, S, _ = x.shape
    out = torch.empty(N, dtype=torch.float64, device=x.device)
    for lo in range(0, N, chunk):
        xc = x[lo:lo + chunk]
        B = 0.5 * torch.cdist(xc, xc, compute_mode=mode).sum((1, 2), dtype=torch.float64)
        A = (xc - Y[lo:lo + chunk, None, :]).norm(dim=2).mean(1, dtype=torch.float64)
        out[lo:lo + chunk] = A - B / S ** 2
    return out


def stats_launch(lib, smp, y, pr, outs):
    """A raw ``iwvi_sample_stats`` launch of ``lib`` (KDE log density, squared error, mean / std, five quantiles; no Shapiro-Wilk)."""
    S, N = smp.shape
    ss, sn = smp.stride()
    rc = lib.iwvi_sample_stats(ctypes.c_void_p(smp.data_ptr()), ss, sn, _abi.ptr(y), N, S, None, _abi.ptr(pr), len(PROBS), _abi.ptr(outs[0]),
                               _abi.ptr(outs[1]), _abi.ptr(outs[2]), None, _abi.ptr(outs[3]), _abi.stream_ptr())
    assert rc == 0, rc


def scores_launch(lib, smp, y, pr, outs):
    """A raw ``iwvi_sample_scores`` launch (both CRPS, the counts, five quantiles and their pinball loss) into preallocated outputs."""
    S, N = smp.shape
    ss, sn = smp.stride()
    rc = lib.iwvi_sample_scores(ctypes.c_void_p(smp.data_ptr()), ss, sn, _abi.ptr(y), N, S, _abi.ptr(pr), len(PROBS), _abi.ptr(outs[0]),
                                _abi.ptr(outs[1]), _abi.ptr(outs[2]), _abi.ptr(outs[3]), _abi.stream_ptr())
    assert rc == 0, rc


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--S", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=50, help="points per torch.cdist call (its [chunk, S, S] float32 intermediate)")
    ap.add_argument("--compare-lib", default=None, help="another build's libiwvi_hip.so: its iwvi_sample_stats launch, alternating")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.reps < 20:
        ap.error("--reps must be >= 20")
    assert torch.cuda.is_available(), "time_scores.py needs a ROCm device"
    dev = torch.device("cuda:0")
    N, S = a.N, a.S
    g = torch.Generator(device=dev).manual_seed(0)
    res = dict(N=N, S=S, reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               protocol="device events around each launch; median (min, max) of `reps` launches after `warmup` untimed ones")

    # ---- the univariate launch
    smp = torch.randn(N, S, device=dev, generator=g).t()                 # [S, N], a point's draws contiguous
    y = torch.randn(N, device=dev, generator=g)
    pr = torch.as_tensor(PROBS, dtype=torch.float64, device=dev)
    w = 2.0 * torch.arange(1, S + 1, dtype=torch.float64, device=dev) - S - 1.0
    outs = [torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, 2, device=dev), torch.empty(N, len(PROBS), device=dev)]
    lib = _abi.lib()
    row = dict(quantiles=PROBS)
    souts = [torch.empty(N, 2, device=dev), torch.empty(N, 2, dtype=torch.int32, device=dev), torch.empty(N, len(PROBS), device=dev),
             torch.empty(N, len(PROBS), device=dev)]
    row["iwvi_sample_scores"] = timed(lambda: scores_launch(lib, smp, y, pr, souts), a.reps, a.warmup)
    row["sample_scores_python_call"] = timed(lambda: evaluation.sample_scores(smp, y, quantiles=PROBS), a.reps, a.warmup)
    row["iwvi_sample_stats"] = timed(lambda: stats_launch(lib, smp, y, pr, outs), a.reps, a.warmup)
    row["torch_sort_weighted_sum"] = timed(lambda: torch_scores(smp, y, w), a.reps, a.warmup)
    got, want = evaluation.sample_scores(smp, y)["crps"].double(), torch_scores(smp, y, w)[0]
    row["max_abs_gap_to_torch"] = float((got - want).abs().max())
    if a.compare_lib:
        other = ctypes.CDLL(os.path.abspath(a.compare_lib))
        other.iwvi_sample_stats.restype, other.iwvi_sample_stats.argtypes = _abi.PROTOTYPES["iwvi_sample_stats"]
        outs2 = [torch.empty_like(t) for t in outs]
        pair = timed_alternating({"this_build": lambda: stats_launch(lib, smp, y, pr, outs),
                                  "other_build": lambda: stats_launch(other, smp, y, pr, outs2)}, a.reps, a.warmup)
        again = timed_alternating({"other_build_a": lambda: stats_launch(other, smp, y, pr, outs2),
                                   "other_build_b": lambda: stats_launch(other, smp, y, pr, outs2)}, a.reps, a.warmup)
        torch.cuda.synchronize()
        row["iwvi_sample_stats_two_builds"] = dict(
            pair, other_build_against_itself=again, same_bits=all(torch.equal(p, q) for p, q in zip(outs, outs2)),
            note="other_build = the parent commit's library; other_build_against_itself = the spread of repeated runs of that one build")
    res["sample_scores"] = row

    # ---- the pairwise launch
    res["energy_score"] = dict(chunk_points=a.chunk, chunk_intermediate_bytes=a.chunk * S * S * 4,
                               note="max_abs_gap_to_cdist_*: largest |iwvi_energy_score - the torch route| over the N points; the kernel is "
                                    "tested against a float64 restatement (tests/test_gpu_energy_score.py), the torch routes are timed "
                                    "baselines and are not a reference")
    for D in (2, 8, 32):
        x = torch.randn(N, S, D, device=dev, generator=g)
        Y = torch.randn(N, D, device=dev, generator=g)
        xv = x.permute(1, 0, 2)                                          # [S, N, D]
        r = dict(pairs=N * S * (S - 1) // 2)
        r["iwvi_energy_score"] = timed(lambda: evaluation.energy_score(xv, Y), a.reps, a.warmup)
        r["torch_cdist_gram_form"] = timed(lambda: torch_energy(x, Y, a.chunk, "use_mm_for_euclid_dist_if_necessary"), a.reps, a.warmup)
        r["torch_cdist_difference_form"] = timed(lambda: torch_energy(x, Y, a.chunk, "donot_use_mm_for_euclid_dist"), a.reps, a.warmup)
        got = evaluation.energy_score(xv, Y)["energy"].double()
        r["max_abs_gap_to_cdist_gram_form"] = float((got - torch_energy(x, Y, a.chunk, "use_mm_for_euclid_dist_if_necessary")).abs().max())
        r["max_abs_gap_to_cdist_difference_form"] = float((got - torch_energy(x, Y, a.chunk, "donot_use_mm_for_euclid_dist")).abs().max())
        r["giga_pairs_per_second"] = r["pairs"] / r["iwvi_energy_score"]["median_ms"] * 1e-6
        res["energy_score"]["D=%d" % D] = r
        del x, xv

    # ---- the whole evaluation
    spec = synthetic.make_spec(L=2, M=128, B=1024, K=1, seed=2, n_data=max(1024, N), with_lv=True)
    model = synthetic.build_model(spec, dev)
    X = torch.as_tensor(np.asarray(spec["X"][:N], np.float32), device=dev)
    Yt = torch.as_tensor(np.asarray(spec["Y"][:N], np.float32), device=dev)
    ev = dict(stack="configs[2]: LV + 2 GP layers, M = 128, Gaussian, one target column")
    ev["evaluate_scores"] = timed(lambda: evaluation.evaluate_scores(model, X, Yt, S, N), a.reps, a.warmup)
    ev["evaluate_draws"] = timed(lambda: evaluation.evaluate_draws(model, X, Yt, S, N), a.reps, a.warmup)
    out = evaluation.evaluate_scores(model, X, Yt, S, N)
    ev["evaluate_scores_result"] = out
    res["evaluate"] = ev
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
