"""Times of the CVAE baseline on one MI355X, written to profiles/cvae_time.json.

Training step at the workload's own sizes ('100_100', Dx = 8, minibatch 512): the fused step (``cvae.CVAETrainer``: value + gradient in two
launches of csrc/cvae.hip, then ``iwvi_adam_step_dev``) replayed as a hipGraph and launched eagerly, against the same step written in
torch ops with autograd and ``torch.optim.Adam``.  The torch step lives here as a BASELINE only; the package has no such route.  All three
run in one process, alternating in blocks, timed with device events that end in a synchronise, repeated so that the spread shows.

Sampler at N = 1000, S = 2000: ``iwvi_cvae_predict_samples`` against the torch formulation, and against the algorithmic floor: the decoder's
operations over the fp32 peak (157.3 TFLOP/s, MI355X_MICROARCH.md) and the bytes of out_y over the HBM bandwidth (8 TB/s).

    python scripts/time_cvae.py [--steps 2000] [--repeats 3] [--out profiles/cvae_time.json]
"""
import argparse
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dgps_with_iwvi_amd import build_models   # noqa: E402

FP32_PEAK, HBM_PEAK = 157.3e12, 8.0e12
CLIP_LO, CLIP_HI = math.log(1e-12), math.log(1e10)


class TorchCVAE:
    """The same model and step in torch ops (autograd, torch.optim.Adam on the unconstrained variance): the baseline."""

    def __init__(self, model, lr):
        p = lambda t: t.detach().clone().requires_grad_(True)
        self.Ws, self.bs, self.Ws_dec, self.bs_dec = ([p(t) for t in ts] for ts in (model.Ws, model.bs, model.Ws_dec, model.bs_dec))
        v = float(model.variance)
        self.raw_var = torch.tensor([math.log(math.expm1(v - 1e-6))], dtype=torch.float32, device=model.X.device, requires_grad=True)
        self.L = model.latent_dim
        self.opt = torch.optim.Adam(self.Ws + self.bs + self.Ws_dec + self.bs_dec + [self.raw_var], lr=lr, eps=1e-8)

    @staticmethod
    def mlp(h, Ws, bs):
        for i, (W, b) in enumerate(zip(Ws, bs)):
            h = torch.addmm(b, h, W)
            if i < len(Ws) - 1:
                h = torch.tanh(h)
        return h

    def bound(self, X, Y):
        enc = self.mlp(torch.cat([X, Y], 1), self.Ws, self.bs)
        mu, raw = enc[:, :self.L], enc[:, self.L:]
        rc = torch.clamp(raw, CLIP_LO, CLIP_HI)
        sigma = torch.exp(0.5 * rc)
        yhat = self.mlp(torch.cat([mu + torch.randn_like(mu) * sigma, X], 1), self.Ws_dec, self.bs_dec)
        var = torch.nn.functional.softplus(self.raw_var) + 1e-6
        logp = (-0.5 * math.log(2 * math.pi) - 0.5 * torch.log(var) - 0.5 * (Y - yhat) ** 2 / var).sum()
        kl = 0.5 * (sigma * sigma + mu * mu - 1.0 - rc).sum()
        return logp - kl

    def step(self, X, Y):
        self.opt.zero_grad(set_to_none=True)
        loss = -self.bound(X, Y)
        loss.backward()
        self.opt.step()

    def samples(self, Xs, S):
        with torch.no_grad():
            N = Xs.shape[0]
            x = Xs[:, None, :].expand(N, S, Xs.shape[1]).reshape(N * S, -1)
            z = torch.randn(N * S, self.L, device=Xs.device)
            y = self.mlp(torch.cat([z, x], 1), self.Ws_dec, self.bs_dec)
            var = torch.nn.functional.softplus(self.raw_var) + 1e-6
            return (y + var.sqrt() * torch.randn_like(y)).reshape(N, S, -1)


def timed(fn, n):
    """ms per call of n calls between two device events, ending in a synchronise."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=4, help="the steps of a repeat run in this many alternating blocks per variant")
    ap.add_argument("--sampler_calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cvae_time.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "time_cvae.py measures on the GPU; there is no fallback"
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    Dx, B, conf = 8, 512, "100_100"
    X, Y = rng.randn(20000, Dx).astype(np.float32), rng.randn(20000, 1).astype(np.float32)

    def build(use_graph):
        np.random.seed(1)
        ARGS = types.SimpleNamespace(mode="CVAE", configuration=conf, minibatch_size=B, lr=5e-3, use_graph=use_graph)
        m = build_models.build_cvae_model(ARGS, X, Y, device=dev)
        m.init_op()
        return m
    mg, me = build(True), build(False)
    tm = TorchCVAE(me, 5e-3)

    def torch_step():
        me_t.next_minibatch()
        tm.step(me_t.X, me_t.Y)
    me_t = build(False)                                              # the torch baseline's minibatch iterator (the same gather per step)
    variants = {"fused_graph": mg.train_op, "fused_eager": me.train_op, "torch_autograd_adam": torch_step}
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    per = max(1, a.steps // a.blocks)
    train = {k: [] for k in variants}
    for _ in range(a.repeats):
        acc = {k: 0.0 for k in variants}
        for _ in range(a.blocks):
            for k, fn in variants.items():
                acc[k] += timed(fn, per)
        for k in variants:
            train[k].append(acc[k] / a.blocks * 1e3)                 # us per step
    # the gather alone (host-driven, outside the graph, common to all three)
    gather_us = [timed(me_t.next_minibatch, per) * 1e3 for _ in range(a.repeats)]

    # ---- sampler ----
    N, S = 1000, 2000
    Xs = torch.as_tensor(rng.randn(N, Dx).astype(np.float32), device=dev)
    dims = me.dec_dims
    flops = 2.0 * N * S * sum(i * o for i, o in zip(dims[:-1], dims[1:]))
    out_bytes = 4.0 * N * S * me.Y_dim
    floor_compute, floor_bytes = flops / FP32_PEAK * 1e3, out_bytes / HBM_PEAK * 1e3      # ms
    sv = {"fused": lambda: me.predict_y_samples_fused(Xs, S), "torch": lambda: tm.samples(Xs, S)}
    for fn in sv.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samp = {k: [] for k in sv}
    for _ in range(a.repeats):
        for k, fn in sv.items():
            samp[k].append(timed(fn, a.sampler_calls))
    res = {
        "device": torch.cuda.get_device_name(0),
        "train_step": {"configuration": conf, "Dx": Dx, "minibatch": B, "steps_per_repeat": per * a.blocks, "warmup": a.warmup,
                       "us_per_step": train, "minibatch_gather_us": gather_us,
                       "median_us": {k: float(np.median(v)) for k, v in train.items()}},
        "sampler": {"N": N, "S": S, "ms_per_call": samp, "median_ms": {k: float(np.median(v)) for k, v in samp.items()},
                    "flops": flops, "out_bytes": out_bytes, "floor_ms_compute": floor_compute, "floor_ms_bytes": floor_bytes,
                    "bound_by": "compute" if floor_compute >= floor_bytes else "bytes",
                    "share_of_floor": max(floor_compute, floor_bytes) / float(np.median(samp["fused"]))},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return res


if __name__ == "__main__":
    main()
