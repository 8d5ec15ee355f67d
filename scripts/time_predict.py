#!/usr/bin/env python3
"""Monte Carlo log predictive density at the reference's evaluation size (1000 test points x 2000 draws,
run_conditional_density_estimation.py:27-28), BASELINE configs[2] and configs[3] stacks: the layer-by-layer route
(predict_f_multisample -> Gaussian.predict_density -> torch.logsumexp: one layer launch per layer, [S, N, D] samples, means and
variances through HBM) against ``predict_log_density`` (one precompute, one fused forward with the predictive tail, one merge).
Wall time per call from CUDA events (the precompute is in both); the kernel split comes from a
``rocprofv3 --kernel-trace --stats -- python3 scripts/time_predict.py`` run of the same script.

  python3 scripts/time_predict.py [--reps 10] [--N 1000] [--S 2000] [--out file.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgps_with_iwvi_amd import synthetic   # noqa: E402

STACKS = {"configs[2]": dict(L=2, M=128, with_lv=True), "configs[3]": dict(L=3, M=256, with_lv=False)}


def layer_by_layer(model, X, Y, S):
    m, v = model.predict_f_multisample(X, S)
    ell = model.likelihood.predict_density(m, v, Y[None].expand(S, *Y.shape)).sum(-1)
    return torch.logsumexp(ell, 0) - np.log(S)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
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
        t_lbl, lp_lbl = timed(lambda: layer_by_layer(model, X, Y, a.S), a.reps)
        t_fused, lp_fused = timed(lambda: model.predict_log_density(X, Y, a.S), a.reps)
        res["stacks"][name] = dict(layer_by_layer_ms=t_lbl, fused_ms=t_fused, speedup=t_lbl / t_fused,
                                   mean_logp_layer_by_layer=float(lp_lbl.double().mean()), mean_logp_fused=float(lp_fused.double().mean()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
