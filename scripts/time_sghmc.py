#!/usr/bin/env python3
"""The SGHMC mode's two long loops at the reference's sizes, on the G5 stack of BASELINE configs[1]'s shape (2 GP layers, M = 128, 8-D inputs,
1024 points per evaluation), eager against captured graph in one session:

  collect_samples(2000, 5)   10 000 sample ops (value + gradient + one iwvi_sghmc_step launch each), the loop of
                             experiments/run_conditional_density_estimation.py:136-140
  evaluate_sghmc             2000 kept theta x 1000 test points: per theta a q(u) re-pack and one fused y-sample launch, then iwvi_sample_stats

Wall time from a host clock around the whole call, ending in a device synchronise; eager and graph alternate, ``--reps`` times each after a
warm-up of ``--warm`` sample ops per mode (the graph is captured there).  The two modes draw the same noise streams from the same state, so
their samples are compared as a by-product (bit-identical: tests/test_gpu_sghmc.py).

  python3 scripts/time_sghmc.py [--num 2000] [--spacing 5] [--N 1000] [--reps 3] [--out profiles/sghmc_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgps_with_iwvi_amd import evaluation, synthetic   # noqa: E402
from dgps_with_iwvi_amd.models import DGP_VI   # noqa: E402
from dgps_with_iwvi_amd.sghmc import SGHMC   # noqa: E402

STACK = dict(L=2, M=128, B=1024, Dx=8, R=5)                      # BASELINE configs[1]'s shape, configuration 'G5'


def build(dev, use_graph):
    spec = synthetic.make_spec(K=1, seed=2, n_data=8192, parity=False, **STACK)
    model = synthetic.build_model(spec, dev, cls=DGP_VI, num_samples=1)
    for layer in model.layers:
        layer.q_sqrt = None
    opt = SGHMC(model, use_graph=use_graph).generate_update_step(0.01, 0.05)
    return spec, model, opt


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num", type=int, default=2000)
    ap.add_argument("--spacing", type=int, default=5)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    modes = {"eager": build(dev, False), "graph": build(dev, True)}
    for _, _, opt in modes.values():
        for _ in range(a.warm):
            opt.sghmc_step()                                     # burn-in: the sampler's scales leave their initial values
        for _ in range(a.warm):
            opt.sample_op()
    res = dict(stack=STACK, num=a.num, spacing=a.spacing, N=a.N, reps=a.reps, sample_ops=a.num * a.spacing, collect={}, evaluate={})
    kept = {}
    for name in modes:
        res["collect"][name + "_all_ms"] = []
    for _ in range(a.reps):                                      # alternate the two modes
        for name, (_, _, opt) in modes.items():
            ms, kept[name] = wall(lambda: opt.collect_samples(a.num, a.spacing))
            res["collect"][name + "_all_ms"].append(ms)
    for name in modes:
        ms = float(np.median(res["collect"][name + "_all_ms"]))
        res["collect"][name + "_ms"] = ms
        res["collect"][name + "_ms_per_sample_op"] = ms / (a.num * a.spacing)
    res["collect"]["graph_speedup"] = res["collect"]["eager_ms"] / res["collect"]["graph_ms"]
    res["collect"]["graph_equals_eager_bitwise"] = all(bool(torch.equal(x, y)) for x, y in zip(kept["eager"], kept["graph"]))
    spec, model, _ = modes["graph"]
    X = torch.as_tensor(np.asarray(spec["X"][1024:1024 + a.N], np.float32), device=dev)
    Y = torch.as_tensor(np.asarray(spec["Y"][1024:1024 + a.N], np.float32), device=dev)
    evaluation.evaluate_sghmc(model, [k[:8].contiguous() for k in kept["graph"]], X, Y)       # warm-up
    all_ms = []
    for _ in range(a.reps):
        ms, out = wall(lambda: evaluation.evaluate_sghmc(model, kept["graph"], X, Y))
        all_ms.append(ms)
    res["evaluate"] = dict(all_ms=all_ms, ms=float(np.median(all_ms)), ms_per_kept_theta=float(np.median(all_ms)) / a.num,
                           result={k: float(v) for k, v in out.items()})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
