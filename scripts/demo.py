#!/usr/bin/env python3
"""The conditional density picture of the reference's experiments/demo.py on the device.

A one-dimensional toy problem whose target has two branches, observed on two separated clusters of inputs; a latent-variable DGP
(``L1_G1``, M = 50, K = 5 importance samples) trained in blocks of steps; after every block the model's predictive density on a grid of
200 inputs x 200 levels from 10 000 predictive samples per input (``evaluation.predictive_density_grid``: a Gaussian KDE with Silverman's
bandwidth, one sampling launch and one ``iwvi_kde_density_grid`` launch); and once the ground truth, 10 000 draws of the generator per
input through the same entry point with the fixed bandwidth 0.01.

Written to ``--out``: inputs.npy [200], levels.npy [200], data.npy [200, 2], truth_logdens.npy [200, 200] and per block
density_<block>.npy [200, 200] (log densities, [input, level]); with matplotlib installed also density_<block>.png.

  python3 scripts/demo.py [--blocks 200] [--steps 1000] [--samples 10000] [--out demo_out] [--seed 0]
  python3 scripts/demo.py --blocks 1 --steps 50          # seconds
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgps_with_iwvi_amd import evaluation   # noqa: E402
from dgps_with_iwvi_amd.build_models import build_model   # noqa: E402

TRUTH_BANDWIDTH = 0.01


class ARGS:
    """The reference demo's LV-GP-GP settings."""
    mode = "IWAE"
    configuration = "L1_G1"
    M = 50
    num_IW_samples = 5
    likelihood_variance = 0.1
    minibatch_size = None
    fix_linear = True
    lr, lr_decay = 5e-3, 0.99
    gamma, gamma_decay = 5e-2, 0.99


def two_bumps(x):
    return np.exp(-(x - 1.0) ** 2) + np.exp(-(x + 1.0) ** 2)


def generator(x, rng):
    """y | x: with probability 0.6 the two-bump curve plus log-normal noise (skewed upwards), otherwise the right bump alone plus
    uniform noise."""
    upper = two_bumps(x) + 0.1 * np.exp(rng.standard_normal(x.shape))
    lower = np.exp(-(x - 1.0) ** 2) + rng.uniform(-0.1, 0.1, x.shape)
    return np.where(rng.random(x.shape) < 0.6, upper, lower)


def training_data(rng, per_cluster=100):
    x = np.concatenate([rng.uniform(-3.0, -0.5, (per_cluster, 1)), rng.uniform(1.0, 3.0, (per_cluster, 1))], 0)
    return x, generator(x, rng)


def truth_grid(inputs, levels, S, rng, dev):
    """[n_inputs, G] log density of the generator at every input: S draws each, KDE with the fixed bandwidth, one launch."""
    draws = generator(np.tile(inputs[None, :], (S, 1)), rng).astype(np.float32)       # [S, n_inputs]
    out = evaluation.kde_log_density_grid(torch.as_tensor(draws, device=dev), torch.as_tensor(levels, device=dev), bandwidth=TRUTH_BANDWIDTH)
    return out["logdens"].cpu().numpy()


def save_picture(path, inputs, levels, logdens, X, Y, title):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    fig, ax = plt.subplots(1, 1, figsize=(6, 6))
    ax.pcolormesh(inputs, levels, np.exp(logdens.T), cmap="Blues_r", shading="auto")
    ax.scatter(X, Y, marker=".", color="C1")
    ax.set_xlim(inputs.min(), inputs.max())
    ax.set_ylim(levels.min(), levels.max())
    ax.set_title(title)
    fig.savefig(path)
    plt.close(fig)
    return True


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=200, help="training blocks, a density picture after each")
    ap.add_argument("--steps", type=int, default=1000, help="training steps per block")
    ap.add_argument("--samples", type=int, default=10000, help="predictive samples per input")
    ap.add_argument("--inputs", type=int, default=200)
    ap.add_argument("--levels", type=int, default=200)
    ap.add_argument("--out", default="demo_out")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kmeans", choices=("host", "device"), default="host",
                    help="where the inducing inputs are clustered: SciPy's kmeans2 on the host, or iwvi_kmeans on the device")
    a = ap.parse_args(argv)
    ARGS.kmeans = a.kmeans
    os.makedirs(a.out, exist_ok=True)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    np.random.seed(a.seed)                                       # (the model factory's k-means and initial values)
    X, Y = training_data(rng)
    inputs = np.linspace(-4.0, 4.0, a.inputs)
    levels = np.linspace(-1.0, 2.0, a.levels).astype(np.float32)
    np.save(os.path.join(a.out, "inputs.npy"), inputs)
    np.save(os.path.join(a.out, "levels.npy"), levels)
    np.save(os.path.join(a.out, "data.npy"), np.concatenate([X, Y], 1))

    t0 = time.perf_counter()
    truth = truth_grid(inputs, levels, a.samples, rng, dev)
    print("ground truth: %d inputs x %d draws x %d levels, bandwidth %g: %.2f s" % (a.inputs, a.samples, a.levels, TRUTH_BANDWIDTH, time.perf_counter() - t0))
    np.save(os.path.join(a.out, "truth_logdens.npy"), truth)
    drew = save_picture(os.path.join(a.out, "truth.png"), inputs, levels, truth, X, Y, "generator")

    model = build_model(ARGS, X.astype(np.float32), Y.astype(np.float32), apply_name=None, device=dev)
    Xs = inputs.reshape(-1, 1).astype(np.float32)
    for block in range(a.blocks):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            model.train_op()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        logdens = evaluation.predictive_density_grid(model, Xs, levels, num_samples=a.samples).cpu().numpy()
        t2 = time.perf_counter()
        np.save(os.path.join(a.out, "density_%03d.npy" % block), logdens)
        save_picture(os.path.join(a.out, "density_%03d.png" % block), inputs, levels, logdens, X, Y, "%d steps" % ((block + 1) * a.steps))
        gap = float(np.mean(np.abs(np.exp(logdens) - np.exp(truth))))
        print("block %d: %d steps %.2f s, density grid %.3f s, mean |p_model - p_truth| on the grid %.4f, finite %s" % (
            block, a.steps, t1 - t0, t2 - t1, gap, bool(np.isfinite(logdens).all())))
    print("wrote %s (%s)" % (a.out, "arrays and pictures" if drew else "arrays; matplotlib is not installed, no pictures"))


if __name__ == "__main__":
    main()
