"""GPflow ``GPModel.predict_y`` / ``predict_density``, ``Gaussian.logp`` / ``predict_density`` and the one-launch Monte Carlo log
predictive density ``predict_log_density`` (iwvi_dgp_predict_density) against the float64 oracle and the device's layer-by-layer route."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.from_spec import build_oracle   # noqa: E402

pytestmark = pytest.mark.gpu

LOG2PI = np.log(2 * np.pi)


def _spec(kind, Dy=1):
    from dgps_with_iwvi_amd import synthetic
    if kind == "single":                                       # one GP layer (SVGP)
        return synthetic.make_spec(L=1, M=32, B=64, K=1, Dy=Dy, seed=11, n_data=1200, distinct_y=True)
    if kind == "cfg2":                                         # BASELINE configs[2]: LV + SharedMixedMok inner (Linear mean) + plain final
        return synthetic.make_spec(L=2, M=128, B=64, K=1, Dy=Dy, with_lv=True, seed=12, n_data=1200, distinct_y=True)
    if kind == "m512":
        return synthetic.make_spec(L=1, M=512, B=64, K=1, Dy=Dy, seed=13, n_data=1200, distinct_y=True)
    if kind in ("f64", "f32s2"):
        return synthetic.make_spec(L=2, M=64, B=64, K=1, Dy=Dy, seed=14, n_data=1200, distinct_y=True)
    if kind == "plain_inner":                                  # inner GPLayer with a plain kernel: 8 latent GPs, no mixing
        spec = synthetic.make_spec(L=2, M=32, B=64, K=1, Dy=Dy, R=8, seed=15, n_data=1200, distinct_y=True)
        spec["layers"][0]["W"] = None
        return spec
    raise KeyError(kind)


def _model(spec, dev, kind=None):
    from dgps_with_iwvi_amd import synthetic
    from dgps_with_iwvi_amd.layers import GPLayer
    m = synthetic.build_model(spec, dev)
    if kind == "f64":
        [l for l in m.layers if isinstance(l, GPLayer)][0].f64_stage1 = True
    return m


def _noise(spec, S, N, seed):
    """One [S, N, dim] N(0,1) array per layer (predict_f_multisample's layout)."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((S, N, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1])).astype(np.float32)
            for l in spec["layers"]]


def _dev(zs, dev):
    return [torch.as_tensor(z, device=dev) for z in zs]


def _oracle_moments(spec, X, zs):
    """The oracle's build_predict on X [..., Dx] with the same noise (the final layer's sample is never consumed)."""
    orc = build_oracle(spec)
    zo = [np.asarray(z, np.float64) for z in zs[:-1]] + [None]
    return orc.build_predict(np.asarray(X, np.float64), zs=zo)


def _logpdf(y, m, v):
    return -0.5 * LOG2PI - 0.5 * np.log(v) - 0.5 * (y - m) ** 2 / v


def _oracle_mc(spec, X, Y, zs, S):
    m, v = _oracle_moments(spec, np.broadcast_to(X, (S,) + X.shape), zs)
    ell = _logpdf(np.asarray(Y, np.float64)[None], m, v + spec["lik_var"]).sum(-1)      # [S, N]
    mx = ell.max(0)
    return mx + np.log(np.exp(ell - mx).mean(0))


def _layer_by_layer(model, X, Y, S, zs):
    m, v = model.predict_f_multisample(X, S, zs=zs)
    ell = model.likelihood.predict_density(m, v, Y[None].expand(S, *Y.shape)).sum(-1)
    return torch.logsumexp(ell.double(), 0) - np.log(S)


def test_gaussian_logp_and_predict_density_match_scipy(gpu_device):
    from scipy.stats import norm
    from dgps_with_iwvi_amd.likelihoods import Gaussian
    rng = np.random.default_rng(1)
    F = rng.standard_normal((37, 3)).astype(np.float32)
    V = rng.uniform(0.01, 2.0, (37, 3)).astype(np.float32)
    Y = (rng.standard_normal((37, 3)) * 2).astype(np.float32)
    t = lambda a: torch.as_tensor(a, device=gpu_device)
    lik = Gaussian(0.3)
    f64 = lambda a: np.asarray(a, np.float64)
    np.testing.assert_allclose(lik.logp(t(F), t(Y)).cpu().numpy(), norm.logpdf(f64(Y), f64(F), np.sqrt(0.3)), rtol=1e-5)
    np.testing.assert_allclose(lik.predict_density(t(F), t(V), t(Y)).cpu().numpy(),
                               norm.logpdf(f64(Y), f64(F), np.sqrt(f64(V) + 0.3)), rtol=1e-5)
    # the variance as the device scalar the class may be bound to (a trainer updates it there)
    lik.bind_device_variance(torch.tensor([0.7], device=gpu_device))
    np.testing.assert_allclose(lik.predict_density(t(F), t(V), t(Y)).cpu().numpy(),
                               norm.logpdf(f64(Y), f64(F), np.sqrt(f64(V) + 0.7)), rtol=1e-5)


@pytest.mark.parametrize("Dy", [1, 3])
def test_predict_y_and_predict_density_match_the_oracle(gpu_device, Dy):
    spec = _spec("cfg2", Dy)
    model = _model(spec, gpu_device)
    X, Y = spec["X"][100:113], spec["Y"][100:113]
    zs = [z[0] for z in _noise(spec, 1, 13, 3)]
    m_ref, v_ref = _oracle_moments(spec, X, zs)
    mean, var = model.predict_y(X, zs=_dev(zs, gpu_device))
    np.testing.assert_allclose(mean.cpu().numpy(), m_ref, rtol=2e-3, atol=1e-3)          # the suite's moment tolerances (test_gpu_parity)
    np.testing.assert_allclose(var.cpu().numpy(), v_ref + spec["lik_var"], rtol=2e-3, atol=1e-4)
    dens = model.predict_density(X, Y, zs=_dev(zs, gpu_device))
    assert tuple(dens.shape) == (13, Dy)
    np.testing.assert_allclose(dens.cpu().numpy(), _logpdf(Y, m_ref, v_ref + spec["lik_var"]), rtol=1e-3, atol=5e-3)


# (stack, N, S, Dy): S inside one chunk of samples (7), exactly one chunk (80), many chunks (2000), a chunk it does not divide (7, 2000)
CASES = [
    ("single", 13, 7, 1), ("single", 1, 2000, 3), ("single", 13, 80, 1),
    ("cfg2", 13, 80, 1), ("cfg2", 13, 7, 3), ("cfg2", 13, 2000, 1), ("cfg2", 1000, 7, 1),
    ("m512", 13, 80, 1), ("f64", 13, 7, 1), ("f32s2", 13, 80, 3), ("plain_inner", 13, 80, 1),
]


@pytest.mark.parametrize("kind,N,S,Dy", CASES)
def test_mc_log_density_matches_oracle_and_layer_by_layer_route(gpu_device, kind, N, S, Dy):
    from dgps_with_iwvi_amd import settings
    spec = _spec(kind, Dy)
    X, Y = spec["X"][:N], spec["Y"][:N]
    zs = _noise(spec, S, N, 7 + N + S)
    old, settings.fw_f32_stage2 = settings.fw_f32_stage2, (kind == "f32s2") or settings.fw_f32_stage2   # a descriptor flag of each call
    try:
        model = _model(spec, gpu_device, kind)
        got = model.predict_log_density(X, Y, S, zs=_dev(zs, gpu_device))
        Xd, Yd = (torch.as_tensor(a, device=gpu_device) for a in (X, Y))
        lbl = _layer_by_layer(model, Xd, Yd, S, _dev(zs, gpu_device))
    finally:
        settings.fw_f32_stage2 = old
    assert got.dtype == torch.float32 and tuple(got.shape) == (N,) and got.is_cuda
    got = got.cpu().numpy()
    err_lbl = np.abs(got - lbl.cpu().numpy()).max()
    err_orc = np.abs(got - _oracle_mc(spec, X, Y, zs, S)).max() if N * S <= 30000 else 0.0     # (float64 oracle on every row)
    print("mc density %s N=%d S=%d Dy=%d: |fused - layer-by-layer| %.2e, |fused - oracle| %.2e" % (kind, N, S, Dy, err_lbl, err_orc))
    assert err_lbl <= 2e-5 * max(1.0, np.abs(got).max())     # (observed <= 3e-6: the same layer arithmetic, another tail)
    assert err_orc <= 3e-4 * max(1.0, np.abs(got).max())     # (observed <= 1e-5; 9e-5 at M = 512)


def test_batches_give_the_same_densities(gpu_device):
    spec = _spec("cfg2")
    model = _model(spec, gpu_device)
    X, Y = spec["X"][:50], spec["Y"][:50]
    zs = _dev(_noise(spec, 33, 50, 5), gpu_device)
    one = model.predict_log_density(X, Y, 33, zs=zs)
    many = model.predict_log_density(X, Y, 33, zs=zs, batch_size=7)       # (other chunk boundaries: other partial sums, same value)
    np.testing.assert_allclose(one.cpu().numpy(), many.cpu().numpy(), rtol=1e-6, atol=1e-5)


def test_one_draw_equals_predict_density_summed(gpu_device):
    spec = _spec("cfg2", 3)
    model = _model(spec, gpu_device)
    X, Y = spec["X"][:13], spec["Y"][:13]
    zs = _noise(spec, 1, 13, 21)
    mc = model.predict_log_density(X, Y, 1, zs=_dev(zs, gpu_device))
    one = model.predict_density(X, Y, zs=_dev([z[0] for z in zs], gpu_device)).sum(-1)
    np.testing.assert_allclose(mc.cpu().numpy(), one.cpu().numpy(), rtol=1e-5, atol=2e-4)


def test_reference_evaluation_size_is_finite_and_reproducible(gpu_device):
    """1000 test points x 2000 draws at configs[2], noise drawn in the kernel: finite, and bit for bit the same on a repeat from the
    same seed and noise counter (the per-point merge runs in a fixed order)."""
    from dgps_with_iwvi_amd import settings
    spec = _spec("cfg2")
    model = _model(spec, gpu_device)
    X, Y = spec["X"][:1000], spec["Y"][:1000]
    runs = []
    for _ in range(2):
        settings.set_seed(5)
        model._words().zero_()
        runs.append(model.predict_log_density(X, Y, 2000))
    assert torch.isfinite(runs[0]).all()
    assert torch.equal(runs[0], runs[1])
    nxt = model.predict_log_density(X, Y, 2000)                # the noise counter advanced: fresh draws
    assert not torch.equal(nxt, runs[0]) and abs(float(nxt.double().mean() - runs[0].double().mean())) < 0.05


def test_bad_arguments_are_refused_before_any_launch(gpu_device):
    spec = _spec("cfg2")
    model = _model(spec, gpu_device)
    X, Y = spec["X"][:10], spec["Y"][:10]
    calls = []
    real = model.precompute
    model.precompute = lambda *a, **k: calls.append(1)
    for bad in (lambda: model.predict_log_density(X, Y[:9], 5),                  # rows of Y
                lambda: model.predict_log_density(X, np.tile(Y, [1, 2]), 5),     # columns of Y
                lambda: model.predict_log_density(X, Y, 0),                      # S < 1
                lambda: model.predict_log_density(X[:, :7], Y, 5)):              # X without D columns
        with pytest.raises(ValueError):
            bad()
    assert not calls
    model.precompute = real
    assert torch.isfinite(model.predict_log_density(X, Y, 5)).all()


def test_evaluate_reports_the_mc_log_likelihood(gpu_device):
    from dgps_with_iwvi_amd import evaluation
    spec = _spec("cfg2")
    model = _model(spec, gpu_device)
    Xt, Yt = spec["X"][200:260], spec["Y"][200:260]
    base = evaluation.evaluate(model, Xt, Yt, num_predict_samples=300, predict_batch_size=25)
    assert "test_loglik_mc" not in base
    res = evaluation.evaluate(model, Xt, Yt, num_predict_samples=300, predict_batch_size=25, mc_loglik=True)
    assert {"test_loglik", "test_rmse", "test_loglik_mc"} <= set(res)
    assert np.isfinite(res["test_loglik_mc"])
    assert abs(res["test_loglik_mc"] - res["test_loglik"]) < 1.0          # two estimates of the same predictive log density
