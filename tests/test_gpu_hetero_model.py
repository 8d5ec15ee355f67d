"""The heteroskedastic Gaussian likelihood through the models on the GPU: the bound of ``DGP_IWVI`` / ``DGP_VI`` and its gradients against
the float64 restatement (tests/hetero_restatement.py on the oracle's stack, the route tests/test_gpu_likelihoods.py takes for the other
families, with that file's tolerances: bound 1e-4 relative, per-point log p rtol 2e-4 + atol 2e-2, gradients 5e-3 of each array's
max-norm); the tail on the layer launch's own moments (tests/test_gpu_hetero.py's tolerance for the reduction); the trainer, eager
against graph replay; a short training run on data whose noise depends on x; the predictive routes; the K-sharded refusal."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import hetero_restatement as H   # noqa: E402

pytestmark = pytest.mark.gpu

ELBO_RTOL = 1e-4
U, C8, C16 = H.U, H.C_CLOSED, H.C_QUAD
REF = H.HeteroskedasticGaussian()


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)), device=dev)


def _n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _lik():
    from dgps_with_iwvi_amd import likelihoods
    return likelihoods.HeteroskedasticGaussian()


def _spec(lv, M=16, B=64, K=5, seed=3, **kw):
    from dgps_with_iwvi_amd import synthetic
    return synthetic.make_hetero_spec(L=2, M=M, B=B, K=K, Dx=3, with_lv=lv, seed=seed, parity=True, **kw)


def _close(name, got, ref, rtol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-12)
    err = np.abs(got - ref).max()
    print("  %-12s max err %.3e of scale %.3e (%.2e relative)" % (name, err, scale, err / scale))
    assert err <= rtol * scale, "%s: max err %.3e vs scale %.3e" % (name, err, scale)


def _vi_noise(zs, B, K):
    """[B, K, dim] (the restatement's layout) -> [S*N, dim], S-major (models.py:50)."""
    return [np.ascontiguousarray(np.asarray(z).transpose(1, 0, 2).reshape(K * B, -1)) for z in zs]


# ---- 1: bound, per-point log p and gradients ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iw", [True, False], ids=["iwvi", "vi"])
@pytest.mark.parametrize("lv", [True, False], ids=["lv", "nolv"])
@pytest.mark.parametrize("M", [16, 32])
def test_bound_logp_and_gradients_match_the_restatement(gpu_device, iw, lv, M):
    from dgps_with_iwvi_amd import synthetic, backward
    from dgps_with_iwvi_amd.models import DGP_IWVI, DGP_VI
    B, K = 64, 5
    spec = _spec(lv, M=M, B=B, K=K, seed=7 + M)
    zs = synthetic.make_noise(spec, seed=2)
    val, logp, gref = H.bound_and_gradients(spec, zs, mode_vi=not iw)
    model = synthetic.build_model(spec, gpu_device, cls=DGP_IWVI if iw else DGP_VI, likelihood=_lik())
    assert model._output_dim() == 2 and tuple(model.Y.shape) == (B, 1)
    zd = [_t(z, gpu_device) for z in (zs if iw else _vi_noise(zs, B, K))]
    got = model.compute_log_likelihood(zd)
    print("iw=%s lv=%s M=%d: bound %.6f vs %.6f (%.2e relative)" % (iw, lv, M, got, val, abs(got - val) / abs(val)))
    assert abs(got - val) <= ELBO_RTOL * abs(val), (got, val)
    assert got == model.compute_log_likelihood(zd)               # the same bits twice
    if iw:
        lp = model.E_log_p_Y(zd).cpu().numpy()
        print("  per-point log p: max abs err %.3e" % np.abs(lp - logp).max())
        np.testing.assert_allclose(lp, logp, rtol=2e-4, atol=2e-2)
        ms, _ = model.lse_partials(zd)
        np.testing.assert_allclose((ms[:, 0] + torch.log(ms[:, 1])).cpu().numpy() - math.log(K), lp, rtol=1e-5, atol=1e-5)
        # the tail alone: the restatement applied to the layer launch's OWN moments and regularisers
        fmean, fvar, local_kls, global_kls, _, _, _ = model._forward_iw(zd)
        m64, v64 = _n64(fmean).reshape(B, K, 2), _n64(fvar).reshape(B, K, 2)
        y64 = np.broadcast_to(_n64(model.Y)[:, None, :], (B, K, 1)).copy()
        klsum = sum((_n64(k).reshape(B, K, -1).sum(-1) for k in local_kls), np.zeros((B, K)))
        L = REF.variational_expectations(m64, v64, y64).sum(-1).numpy() - klsum
        want = torch.logsumexp(torch.as_tensor(L), 1).numpy() - math.log(K)
        S = (H.var_exp_scale(m64, v64, y64).sum(-1).numpy() + np.abs(klsum)).max(1) + np.abs(want)
        mult = float((np.abs(lp - want) / (U * S)).max())
        print("  tail on the launch's own moments: per-point %.2f multiples of 2^-24 S" % mult)
        assert mult <= C8, mult
        glob = sum(float(g.double().sum()) for g in global_kls)
        assert abs(got - (model.num_data / B * want.sum() - glob)) <= C8 * U * model.num_data / B * S.sum()
    elbo, grads = backward.iw_elbo_and_gradients(model, zd)
    assert abs(float(elbo) - val) <= 2e-4 * abs(val), (float(elbo), val)
    assert sorted(grads) == sorted(gref), (sorted(grads), sorted(gref))
    for k, v in grads.items():
        _close(k, v.detach().cpu().numpy().reshape(gref[k].shape), gref[k], rtol=5e-3)
    elbo2, grads2 = backward.iw_elbo_and_gradients(model, zd)
    assert torch.equal(elbo, elbo2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ---- 2: the trainer ------------------------------------------------------------------------------------------------------------------------
def _training_problem(dev, n=256):
    """One input column, 256 points, y = sin(2 x) + sd(x) eps with sd rising from 0.05 on the left to 0.65 on the right; an L = 2 stack
    without a latent-variable layer (which could explain the spread by itself) and the reference's initial values."""
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_hetero_spec(L=2, M=16, B=n, K=5, Dx=1, with_lv=False, seed=41, n_data=n, parity=False)
    return spec, (lambda i: synthetic.make_noise(spec, seed=1000 + i)), synthetic.build_model(spec, dev, likelihood=_lik())


def test_graph_step_equals_eager_step(gpu_device):
    """Trainer(use_graph=True) replays a step with the three-launch evaluation from a hipGraph: the bounds it saw and every parameter are
    bit-identical to the eager trainer's after 6 steps.  The likelihood contributes no Adam scalar; the final layer's q_mu has two columns
    and the NatGrad step moves both."""
    from dgps_with_iwvi_amd import settings
    from dgps_with_iwvi_amd.training import Trainer
    out = []
    for use_graph in (False, True):
        settings.set_seed(3)
        _, _, model = _training_problem(gpu_device, n=64)
        q0 = model.layers[-1].q_mu.clone()
        tr = Trainer(model, use_graph=use_graph, check_finite=False)
        vals = [float(tr.step()) for _ in range(6)]
        out.append((vals, [p.clone() for _, p, _ in tr._entries], model.layers[-1].q_mu.clone(), model.layers[-1].q_sqrt.clone()))
        assert not [n for n, _, _ in tr._entries if n.startswith("lik")]
        moved = (out[-1][2] - q0).abs().amax(0)
        assert tuple(moved.shape) == (2,) and bool((moved > 0).all())
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert all(math.isfinite(v) for v in out[0][0])
    for pa, pb in zip(out[0][1], out[1][1]):
        assert torch.equal(pa, pb)
    assert torch.equal(out[0][2], out[1][2]) and torch.equal(out[0][3], out[1][3])


def _ranks(a):
    r = np.empty(len(a))
    r[np.argsort(a, kind="stable")] = np.arange(len(a))
    return r


def test_training_raises_the_bound_and_learns_where_the_noise_is(gpu_device):
    """200 steps on fixed noise: the bound rises (the mean of the last ten steps above the mean of the first ten), and the fitted noise
    standard deviation exp(m_g / 2) over a grid of inputs is larger where the true one is: a positive rank correlation."""
    from dgps_with_iwvi_amd import synthetic
    from dgps_with_iwvi_amd.training import Trainer
    spec, noise, model = _training_problem(gpu_device)
    tr = Trainer(model, lr=5e-3, gamma=1e-2)
    vals = [float(tr.step([_t(z, gpu_device) for z in noise(2 * s)], [_t(z, gpu_device) for z in noise(2 * s + 1)])) for s in range(200)]
    assert all(math.isfinite(v) for v in vals)
    first, late = float(np.mean(vals[:10])), float(np.mean(vals[-10:]))
    grid = np.linspace(-2.0, 2.0, 41)[:, None]
    zs0 = [torch.zeros(41, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1], device=gpu_device) for l in spec["layers"]]
    m, _ = model.predict_f(grid, zs=zs0)
    fitted = np.exp(0.5 * _n64(m)[:, 1])
    truth = synthetic.hetero_noise_sd(grid)
    rho = float(np.corrcoef(_ranks(fitted), _ranks(truth))[0, 1])
    print("bound %.2f -> %.2f; fitted noise sd %.3f .. %.3f (true %.3f .. %.3f), rank correlation %.3f"
          % (first, late, fitted.min(), fitted.max(), truth.min(), truth.max(), rho))
    assert late > first, (first, late)
    assert rho > 0.0, rho


def test_k_sharded_training_is_refused(gpu_device):
    from dgps_with_iwvi_amd.training import Trainer
    _, _, model = _training_problem(gpu_device, n=64)
    with pytest.raises(NotImplementedError, match="K-sharded"):
        Trainer(model, shard="k")


# ---- 3: the predictive routes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lv", [True, False], ids=["lv", "nolv"])
def test_predictive_routes_agree_with_the_layer_by_layer_route(gpu_device, lv):
    """predict_mixture / predict_log_density at N = 6, S = 33 against the restatement fed the device's own predict_f_multisample moments on
    the same noise (2e-5 relative between the two routes to those moments, as tests/test_gpu_predict_mixture.py allows, on top of
    tests/test_gpu_hetero.py's mixture tolerance); predict_y_draws with z_f given reproduces f = m + sqrt(v) z_f; predict_y /
    predict_density / predict_y_samples have the target's width; evaluate_mixture, evaluate_draws, evaluate and predictive_density_grid run
    on the one-target model."""
    from dgps_with_iwvi_amd import evaluation, settings, synthetic
    N, S = 6, 33
    spec = _spec(lv, M=16, B=12, K=3, seed=9)
    model = synthetic.build_model(spec, gpu_device, likelihood=_lik())
    Xn, Y = spec["X"][:N], spec["Y"][:N]
    rng = np.random.default_rng(3)
    zs = [_t(rng.standard_normal((S, N, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1])), gpu_device) for l in spec["layers"]]
    got = model.predict_mixture(Xn, S, Y=Y, zs=zs)
    assert tuple(got["mean"].shape) == (N, 1) and tuple(got["var"].shape) == (N, 1) and tuple(got["log_density"].shape) == (N,)
    m, v = model.predict_f_multisample(Xn, S, zs=zs)
    assert tuple(m.shape) == (S, N, 2)
    m64, v64 = _n64(m), _n64(v)
    want = H.mixture(REF, m64, v64, Y)
    Ys = np.broadcast_to(np.asarray(Y, dtype=np.float64), (S, N, 1)).copy()
    tm = C8 * U * np.abs(m64[..., :1]).max(0)
    tol = {"log_density": C16 * U * H.density_scale(REF, m64, v64, Ys).numpy().max(0).sum(-1) + 4 * U * (1 + np.abs(want["log_density"])),
           "mean": tm, "var": C8 * U * (H.var_scale(m64, v64).numpy() + m64[..., :1] ** 2).max(0) + 4 * np.abs(m64[..., :1]).max(0) * tm}
    for k, t in tol.items():
        t = t + 2e-5 * np.maximum(1.0, np.abs(want[k]))
        ratio = float((np.abs(_n64(got[k]) - want[k]) / t).max())
        print("lv=%s %-12s worst err / tol %.3f" % (lv, k, ratio))
        assert ratio <= 1.0, (k, ratio)
    lp = model.predict_log_density(Xn, Y, S, zs=zs)
    assert torch.equal(lp, got["log_density"])
    old = model._predict_log_density_layerwise(Xn, Y, S, zs=zs)     # the elementwise entry + torch.logsumexp on the same moments
    np.testing.assert_allclose(_n64(old), want["log_density"], rtol=0, atol=float((tol["log_density"] + 2e-5 * np.maximum(1.0, np.abs(want["log_density"]))).max()))
    # exact draws: f from the given normals, y - f = exp(g / 2) eps
    z_f = _t(rng.standard_normal((S, N, 2)), gpu_device)
    y, f = model.predict_y_draws(Xn, S, zs=zs, z_f=z_f, return_f=True, serial=4)
    assert tuple(y.shape) == (S, N, 1) and tuple(f.shape) == (S, N, 2) and bool(torch.isfinite(y).all())
    fw = m64 + np.sqrt(v64) * _n64(z_f)
    np.testing.assert_allclose(_n64(f), fw, rtol=0, atol=2e-5 * np.maximum(1.0, np.abs(fw)).max())
    y2, _ = model.predict_y_draws(Xn, S, zs=zs, z_f=z_f, return_f=True, serial=4)
    assert torch.equal(y, y2)
    # one draw through the layers: the target's width everywhere
    zs1 = [z[0] for z in zs]
    pm, pv = model.predict_y(Xn, zs=zs1)
    pd = model.predict_density(Xn, Y, zs=zs1)
    ys = model.predict_y_samples(Xn, 5)
    assert tuple(pm.shape) == tuple(pv.shape) == tuple(pd.shape) == (N, 1) and tuple(ys.shape) == (5, N, 1)
    assert bool((pv > 0).all()) and bool(torch.isfinite(pd).all()) and bool(torch.isfinite(ys).all())

    def reset():
        settings.set_seed(21)
        model._words().zero_()
    reset()
    res = evaluation.evaluate_mixture(model, spec["X"][:10], spec["Y"][:10], num_predict_samples=S)
    assert set(res) == {"test_loglik_mc", "test_rmse"} and all(math.isfinite(x) for x in res.values()) and res["test_rmse"] > 0
    reset()
    lp10 = model.predict_mixture(spec["X"][:10], S, Y=spec["Y"][:10])["log_density"]
    assert res["test_loglik_mc"] == float(lp10.double().mean())
    res = evaluation.evaluate_draws(model, spec["X"][:10], spec["Y"][:10], num_predict_samples=64)
    assert {"test_coverage", "test_interval_width", "test_rmse", "test_loglik"} <= set(res) and all(math.isfinite(x) for x in res.values())
    res = evaluation.evaluate(model, spec["X"][:10], spec["Y"][:10], num_predict_samples=64)
    assert math.isfinite(res["test_loglik"]) and math.isfinite(res["test_rmse"])
    levels = np.linspace(-12.0, 12.0, 481)
    grid = evaluation.predictive_density_grid(model, Xn, levels, num_samples=512)
    assert tuple(grid.shape) == (N, 481) and bool(torch.isfinite(grid).all())
    mass = _n64(grid.exp()).sum(1) * (levels[1] - levels[0])
    assert np.all(np.abs(mass - 1.0) < 0.05), mass              # a density over the target: it integrates to one over a wide grid


def test_checkpoint_round_trip_through_a_model(gpu_device, tmp_path):
    from dgps_with_iwvi_amd import build_models, synthetic
    spec = _spec(False, M=16, B=12, K=3, seed=9)
    model = synthetic.build_model(spec, gpu_device, likelihood=_lik())
    path = str(tmp_path / "hetero.npz")
    build_models.save_checkpoint(model, path)
    assert str(np.load(path)["likelihood.type"]) == "HeteroskedasticGaussian"
    other = synthetic.build_model(_spec(False, M=16, B=12, K=3, seed=10), gpu_device, likelihood=_lik())
    build_models.load_checkpoint(other, path)
    assert torch.equal(other.layers[-1].q_mu, model.layers[-1].q_mu)
    with pytest.raises(ValueError, match="HeteroskedasticGaussian"):
        build_models.load_checkpoint(synthetic.build_model(synthetic.make_spec(L=2, M=16, B=12, K=3, Dx=3, Dy=2), gpu_device), path)
