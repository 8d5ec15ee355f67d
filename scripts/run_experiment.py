"""The reference's experiment script (experiments/run_conditional_density_estimation.py) on this framework, end to end
on a synthetic conditional-density problem (no dataset files travel to the GPU box): build the model from a
configuration string, train with the reference's train_op (NatGrad + Adam), evaluate the test log-likelihood by KDE.

    python scripts/run_experiment.py --configuration L1_G5 --mode IWAE --iterations 500
    python scripts/run_experiment.py --configuration G5 --mode SGHMC --iterations 500      (the sampler + Adam on the hyperparameters)
    python scripts/run_experiment.py --configuration 100_100 --mode CVAE --iterations 2000 (the CVAE baseline, Adam)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dgps_with_iwvi_amd import build_models, evaluation   # noqa: E402


def bimodal_data(n, rng):
    """y | x is a two-component mixture whose separation grows with x: a GP with Gaussian noise cannot fit it, a
    latent-variable layer can (the point of the reference's method)."""
    x = rng.uniform(-2, 2, (n, 1))
    side = rng.integers(0, 2, (n, 1)) * 2 - 1
    y = np.sin(2 * x) + side * (0.2 + 0.6 * (x + 2) / 4) + 0.05 * rng.standard_normal((n, 1))
    return x, y


def run_sghmc(ARGS, X, Y, Xs, Ys, dev):
    """--mode SGHMC (reference run_conditional_density_estimation.py:128-156 with build_models.py:306-335): train with sghmc_step +
    train_hypers, collect ``num_predict_samples`` posterior samples ``--sghmc_spacing`` sample ops apart, evaluate over them."""
    model = build_models.build_sghmc_model(ARGS, X.astype(np.float32), Y.astype(np.float32), device=dev)
    model.init_op()
    t0 = time.perf_counter()
    for it in range(ARGS.iterations):
        elbo = model.train_op()
        if it % max(1, ARGS.iterations // 10) == 0:
            print("iteration %5d  bound %.2f" % (it, float(elbo)), flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    t1 = time.perf_counter()
    samples = model.sghmc_optimizer.collect_samples(ARGS.num_predict_samples, ARGS.sghmc_spacing)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res = evaluation.evaluate_sghmc(model, samples, Xs, Ys, ARGS.predict_batch_size)
    res.update(train_seconds=dt, ms_per_iteration=dt / max(ARGS.iterations, 1) * 1e3, collect_seconds=t2 - t1,
               evaluate_seconds=time.perf_counter() - t2)
    res.update(ARGS.__dict__)
    print(res)
    return res


def run_cvae(ARGS, X, Y, Xs, Ys, dev):
    """--mode CVAE (reference build_models.py:148-173): the baseline of the paper's tables -- build, train with its Adam train_op,
    evaluate like every other mode; the reference's ``res`` keys."""
    model = build_models.build_cvae_model(ARGS, X.astype(np.float32), Y.astype(np.float32), device=dev)
    model.init_op()
    before = evaluation.evaluate(model, Xs, Ys, ARGS.num_predict_samples, ARGS.predict_batch_size, on_device=ARGS.device_eval)
    t0 = time.perf_counter()
    for it in range(ARGS.iterations):
        elbo = model.train_op()
        if it % max(1, ARGS.iterations // 10) == 0:
            print("iteration %5d  ELBO %.2f" % (it, float(elbo)), flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = evaluation.evaluate(model, Xs, Ys, ARGS.num_predict_samples, ARGS.predict_batch_size, shapiro=True, on_device=ARGS.device_eval)
    res.update(test_loglik_before_training=before["test_loglik"], train_seconds=dt, ms_per_iteration=dt / max(ARGS.iterations, 1) * 1e3)
    if ARGS.scores:
        res.update(evaluation.evaluate_scores(model, Xs, Ys, ARGS.num_predict_samples, ARGS.predict_batch_size))
    res.update(ARGS.__dict__)
    print(res)
    return res


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--mode", default="IWAE")
    p.add_argument("--configuration", default="L1_G5")
    p.add_argument("--M", type=int, default=64)
    p.add_argument("--num_IW_samples", type=int, default=5)
    p.add_argument("--minibatch_size", type=int, default=256)
    p.add_argument("--iterations", type=int, default=500)
    p.add_argument("--likelihood_variance", type=float, default=1e-2)
    p.add_argument("--gamma", type=float, default=1e-2)
    p.add_argument("--gamma_decay", type=float, default=0.98)
    p.add_argument("--lr", type=float, default=5e-3)
    p.add_argument("--lr_decay", type=float, default=0.98)
    p.add_argument("--fix_linear", type=int, default=1)
    p.add_argument("--num_predict_samples", type=int, default=2000)
    p.add_argument("--predict_batch_size", type=int, default=1000)
    p.add_argument("--n_train", type=int, default=2000)
    p.add_argument("--n_test", type=int, default=500)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--sghmc_spacing", type=int, default=5, help="--mode SGHMC: sample ops between two kept posterior samples")
    p.add_argument("--use_graph", type=int, default=1, help="replay the ops of a step from captured graphs")
    p.add_argument("--device_eval", action="store_true", help="evaluate on the device: fused y-samples + iwvi_sample_stats (evaluate(on_device=True))")
    p.add_argument("--scores", action="store_true",
                   help="add the proper scoring rules of the predictive draws (evaluate_scores: CRPS, pinball loss, PIT histogram and "
                        "calibration error); not with --mode SGHMC")
    p.add_argument("--importance", type=int, nargs="?", const=5000, default=0, metavar="S",
                   help="--mode IWAE / VI: add the importance-sampled held-out log density with S draws per point (default 5000) from the "
                        "encoder proposal and from the prior, each with its Pareto-k and effective sample size (evaluate_importance)")
    p.add_argument("--kmeans", choices=("host", "device"), default="host",
                   help="where the first layer's inducing inputs are clustered: SciPy's kmeans2 on the host, or iwvi_kmeans on the device")
    p.add_argument("--encoder_gradient", choices=("iwae", "dreg", "stl"), default="iwae",
                   help="--mode IWAE: the estimator of the encoders' gradients (reparameterised, doubly reparameterised, sticking the landing)")
    p.add_argument("--bound", default="iwae",
                   help="--mode IWAE: the bound that is trained (models.Bound.parse): iwae | miwae:<groups> | ciwae:<beta> | vr:<alpha>; "
                        "the groups divide --num_IW_samples; anything but iwae goes with --encoder_gradient iwae")
    ARGS = p.parse_args(argv)
    ARGS.fix_linear = bool(ARGS.fix_linear)
    rng = np.random.default_rng(ARGS.seed)
    np.random.seed(ARGS.seed)
    X, Y = bimodal_data(ARGS.n_train, rng)
    Xs, Ys = bimodal_data(ARGS.n_test, rng)
    mu, sd = Y.mean(), Y.std()
    Y, Ys = (Y - mu) / sd, (Ys - mu) / sd
    dev = torch.device("cuda:0")
    if ARGS.mode == "SGHMC":
        return run_sghmc(ARGS, X, Y, Xs, Ys, dev)
    if ARGS.mode == "CVAE":
        return run_cvae(ARGS, X, Y, Xs, Ys, dev)
    model = build_models.build_model(ARGS, X.astype(np.float32), Y.astype(np.float32), device=dev)
    before = evaluation.evaluate(model, Xs, Ys, ARGS.num_predict_samples, ARGS.predict_batch_size)
    t0 = time.perf_counter()
    for it in range(ARGS.iterations):
        elbo = model.train_op()
        if it % max(1, ARGS.iterations // 10) == 0:
            print("iteration %5d  ELBO %.2f" % (it, float(elbo)), flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = evaluation.evaluate(model, Xs, Ys, ARGS.num_predict_samples, ARGS.predict_batch_size, shapiro=True, on_device=ARGS.device_eval)
    res.update(test_loglik_before_training=before["test_loglik"], train_seconds=dt, ms_per_iteration=dt / max(ARGS.iterations, 1) * 1e3)
    if ARGS.scores:
        res.update(evaluation.evaluate_scores(model, Xs, Ys, ARGS.num_predict_samples, ARGS.predict_batch_size))
    if ARGS.importance:
        for proposal in ("encoder", "prior"):
            r = evaluation.evaluate_importance(model, Xs, Ys, ARGS.importance, proposal=proposal)
            res.update({"%s_%s" % (k, proposal): v for k, v in r.items()})
    res.update(ARGS.__dict__)
    print(res)
    return res


if __name__ == "__main__":
    main()
