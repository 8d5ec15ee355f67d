"""Cost of the heteroskedastic Gaussian tail next to the Gaussian's fused tail and the Poisson's closed-form tail on the same stack, in one
session on one box: BASELINE configs[2] (L = 2, M = 128, K = 20, B = 1024, latent-variable layer) -- the heteroskedastic model with a
final layer of Dy = 2 outputs over ONE target column, the other two with Dy = 1.  Per likelihood: one evaluation (precompute + layer
launch [+ the tail launch]), one value + gradient (backward.iw_elbo_and_gradients) and one training step (NatGrad op + Adam op), each as
hipGraph replays.  And at N = 1000 points x S = 2000 draws of given final-layer moments: iwvi_lik_predict_mixture and iwvi_lik_sample_y
against the same results formed by torch device ops.

EVERY FIGURE IS ONE FRESH PROCESS (this script with --child), one at a time; the rounds interleave the series, so the spread of a series is
what the same code gives from round to round.  Reported: min / median / max over the rounds, microseconds.  Nothing is promised in advance;
the expectation the figures confirm or refute is that the tail costs what the exp-link tail costs -- the third launch, not a latency chain.
Usage: python scripts/time_hetero.py [--rounds 3] [--out profiles/hetero_time.json]"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("hetero", "gaussian", "poisson")
STACK_FIGURES = ("evaluation", "value_gradient", "train_step")
N, S = 1000, 2000
CALLS, REPLAYS, TIMINGS = 10, 20, 5


def _model(kind, dev):
    import numpy as np
    from dgps_with_iwvi_amd import likelihoods, synthetic
    kw = dict(L=2, M=128, B=1024, K=20, with_lv=True, seed=0, n_data=65536)
    if kind == "hetero":
        return synthetic.build_model(synthetic.make_hetero_spec(Dx=8, parity=True, **kw), dev, likelihood=likelihoods.HeteroskedasticGaussian())
    spec = synthetic.make_spec(**kw)
    if kind == "poisson":
        Yz = (spec["Y"] - spec["Y"].mean(0)) / spec["Y"].std(0)
        return synthetic.build_model(dict(spec, Y=np.floor(np.exp(np.clip(Yz, -2.0, 2.5)))), dev, likelihood=likelihoods.Poisson())
    return synthetic.build_model(spec, dev)


def _graph_us(fn, calls=CALLS):
    """Microseconds per call of ``fn`` replayed from a hipGraph of ``calls`` calls: the mean over REPLAYS replays, TIMINGS times -> the median."""
    import numpy as np
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        keep = [fn() for _ in range(calls)]
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(TIMINGS):
        t0 = time.perf_counter()
        for _ in range(REPLAYS):
            g.replay()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / (REPLAYS * calls) * 1e6)
    del keep
    return float(np.median(out))


def _moments(dev):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(0)
    fm = (torch.rand(N * S, 2, generator=gen) * 4 - 2).to(dev)
    fv = torch.exp(torch.rand(N * S, 2, generator=gen) * math.log(2000.0) + math.log(1e-3)).to(dev)
    Y = (torch.rand(N, 1, generator=gen) * 4 - 2).to(dev)
    return fm, fv, Y


def _rule(fm):
    """(nodes, log weights) of the 20-point rule on the moments' device (made once, outside any capture)"""
    import numpy as np
    import torch
    x, w = np.polynomial.hermite.hermgauss(20)
    return tuple(torch.as_tensor(a, dtype=fm.dtype, device=fm.device) for a in (x, np.log(w / np.sqrt(np.pi))))


def _torch_mixture(fm, fv, Y, rule):
    """What iwvi_lik_predict_mixture computes, by torch device ops (the 20-point rule in log space, the clip, float32)."""
    import torch
    x, logw = rule
    mf, mg, vf, vg = (a.reshape(N, S) for a in (fm[:, 0], fm[:, 1], fv[:, 0], fv[:, 1]))
    gi = mg[..., None] + torch.sqrt(2.0 * vg.clamp(min=1e-8))[..., None] * x
    s = vf[..., None] + torch.exp(gi.clamp(-60.0, 60.0))
    t = logw - 0.5 * math.log(2 * math.pi) - 0.5 * torch.log(s) - 0.5 * ((Y - mf) ** 2)[..., None] / s
    logp = torch.logsumexp(torch.logsumexp(t, -1), 1) - math.log(S)
    mean = mf.mean(1)
    var = (vf + torch.exp((mg + 0.5 * vg).clamp(-60.0, 60.0)) + mf ** 2).mean(1) - mean ** 2
    return logp, mean, var


def _torch_sample(fm, fv):
    import torch
    F = fm + torch.sqrt(fv) * torch.randn_like(fm)
    return F[:, :1] + torch.exp((0.5 * F[:, 1:]).clamp(-60.0, 60.0)) * torch.randn_like(F[:, :1])


def child(kind, figure):
    import torch
    from dgps_with_iwvi_amd import _abi, backward, likelihoods
    from dgps_with_iwvi_amd.training import Trainer
    dev = torch.device("cuda:0")
    if figure in STACK_FIGURES:
        model = _model(kind, dev)
        if figure == "evaluation":
            us = _graph_us(lambda: model._build_likelihood())
        elif figure == "value_gradient":
            us = _graph_us(lambda: backward.iw_elbo_and_gradients(model))
        else:
            tr = Trainer(model, use_graph=True, check_finite=False)
            for _ in range(5):
                tr.step()                                        # (capture and warm-up)
            torch.cuda.synchronize()
            t = []
            for _ in range(TIMINGS):
                t0 = time.perf_counter()
                for _ in range(REPLAYS * 5):
                    tr.step()
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) / (REPLAYS * 5) * 1e6)
            us = sorted(t)[len(t) // 2]
    else:
        fm, fv, Y = _moments(dev)
        lik = likelihoods.HeteroskedasticGaussian()
        if figure == "predict_mixture":
            out = [torch.empty(N, device=dev), torch.empty(N, 1, device=dev), torch.empty(N, 1, device=dev)]

            def ours():
                _abi.check(_abi.lib().iwvi_lik_predict_mixture(lik.lik_desc(), _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(Y), N, S, 2, S, 1,
                                                               _abi.ptr(out[0]), _abi.ptr(out[1]), _abi.ptr(out[2]), _abi.stream_ptr()))
            rule = _rule(fm)
            fn = ours if kind == "hetero" else (lambda: _torch_mixture(fm, fv, Y, rule))
            if kind == "torch":                                  # the two routes give the same numbers
                ours()
                lp, mn, vr = _torch_mixture(fm, fv, Y, rule)
                assert float((lp - out[0]).abs().max()) < 1e-3 and float((mn - out[1][:, 0]).abs().max()) < 1e-5
        else:
            fn = (lambda: lik.sample_y(fm, fv, seed=1, serial=2)) if kind == "hetero" else (lambda: _torch_sample(fm, fv))
        us = _graph_us(fn, calls=2)
    print("RESULT " + json.dumps({"us": us}), flush=True)


def one(kind, figure, limit=240):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--figure", figure], cwd=ROOT, capture_output=True, text=True,
                       timeout=limit)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        print(r.stdout[-2000:], r.stderr[-2000:], flush=True)
        return None
    return json.loads(lines[-1][7:])["us"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hetero_time.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--figure", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.figure)
    order = [(k, f) for f in STACK_FIGURES for k in KINDS] + [(k, f) for f in ("predict_mixture", "sample_y") for k in ("hetero", "torch")]
    series = {}
    for r in range(a.rounds):
        for kind, figure in order:
            us = one(kind, figure)
            if us is None:
                raise SystemExit("%s %s failed in round %d: stopping" % (kind, figure, r))
            series.setdefault(figure, {}).setdefault(kind, []).append(us)
            print("round %d %-16s %-9s %10.2f us" % (r, figure, kind, us), flush=True)
    res = dict(what="microseconds per call; evaluation / value_gradient / train_step at L2_M128_K20_B1024_LV (hetero: Dy = 2 final outputs, one "
                    "target column) as hipGraph replays; predict_mixture / sample_y on given moments at N = %d, S = %d (hetero: the library's one "
                    "launch, torch: the same result from torch device ops), also replayed from a graph; one fresh process per figure, %d rounds "
                    "interleaving the series" % (N, S, a.rounds),
               box=socket.gethostname(), rounds=a.rounds, series=series,
               summary={f: {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v)) for k, v in d.items()} for f, d in series.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
