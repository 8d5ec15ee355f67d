"""``DGP_VI.importance_log_density`` / ``evaluation.evaluate_importance`` / ``evaluation.psis_summary`` through small models: 64 training
points, Dx = 2, M = 16; configurations ``L1``, ``L1_G2_L1`` and one without a latent-variable layer (``G2``); 8 held-out points.

  same log-weights   with injected noise, the exported log-weights against a float64 composition of the per-layer outputs of
                     ``DGP_IWVI._forward_iw`` on a model over the SAME layer objects whose data are the held-out rows (the final
                     layer's moments, every latent-variable layer's sampled log q - log p), within tol_logw; the four summaries against
                     the restatement (tests/psis_reference.py) on the exported log-weights, at the bounds of tests/test_gpu_psis.py
  same estimator     ``proposal="prior"`` against ``predict_log_density`` on the same noise, within tol_reduce + tol_logw (Gaussian,
                     and a Poisson model, which goes through ``predict_mixture``)
  same bound         ``kind="bound"`` on the training minibatch against ``E_log_p_Y``: the new kernel against the fused tail
  the two proposals  estimate the same p(y* | x*): |IS - prior MC| <= 5 sqrt(1/ESS_is - 1/S + 1/ESS_mc - 1/S) per point at S = 4096,
                     all 8 points, every restatement ESS >= 50
  model state        minibatch, caches and a following ``compute_log_likelihood`` bit-identical with and without a call in between
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import iw_reduction_reference as IW   # noqa: E402
import psis_reference as R            # noqa: E402
ESS_RTOL, KHAT_TOL = R.GPU_ESS_RTOL, R.GPU_KHAT_TOL

pytestmark = pytest.mark.gpu

N_TRAIN, N_TEST, DX, M = 64, 8, 2, 16
CONFIGS = ("L1", "L1_G2_L1", "G2")


def _data(seed=0):
    rng = np.random.RandomState(seed)
    X = rng.uniform(-2.0, 2.0, (N_TRAIN + N_TEST, DX))
    Y = np.sign(rng.rand(N_TRAIN + N_TEST, 1) - 0.5) * np.sin(2.0 * X[:, :1]) + 0.1 * rng.randn(N_TRAIN + N_TEST, 1)
    f = lambda a: np.asarray(a, dtype=np.float32)
    return f(X[:N_TRAIN]), f(Y[:N_TRAIN]), f(X[N_TRAIN:]), f(Y[N_TRAIN:])


def _model(cfg, dev, K=5, lik_var=0.05, q_scale=0.5, minibatch=None, wide_encoder=False):
    """Layers of build_models.build_layers with q_mu ~ q_scale N(0, 1) (so that the latent variable reaches the output).
    ``wide_encoder``: the encoder's last map times 0.1 and its raw-scale bias at 3 + log(e - 1), so that q(w | x, y) is close to
    N(0, 1), the prior -- an untrained encoder proposes N(mu, 0.05^2), under which p / q has no variance at all."""
    from dgps_with_iwvi_amd import build_models
    from dgps_with_iwvi_amd.layers import LatentVariableLayer
    from dgps_with_iwvi_amd.likelihoods import Gaussian
    from dgps_with_iwvi_amd.models import DGP_IWVI
    X, Y, Xt, Yt = _data()
    np.random.seed(4)                                            # (the encoders' initial weights come from the host generator)
    layers = build_models.build_layers(cfg, X, M, rng=np.random.RandomState(1))
    g = torch.Generator().manual_seed(2)
    for l in layers:
        if isinstance(l, LatentVariableLayer):
            if wide_encoder:
                l.encoder.Ws[-1] = l.encoder.Ws[-1] * 0.1
                l.encoder.bs[-1][l.latent_dim:] = 3.0 + math.log(math.e - 1.0)
        else:
            l.q_mu = q_scale * torch.randn(l.q_mu.shape, generator=g)
    model = DGP_IWVI(X, Y, layers, Gaussian(lik_var), num_samples=K, minibatch_size=minibatch).to(dev)
    t = lambda a: torch.as_tensor(a, device=dev)
    return model, t(Xt), t(Yt)


def _widths(model):
    from dgps_with_iwvi_amd.layers import LatentVariableLayer
    return [l.latent_dim if isinstance(l, LatentVariableLayer) else l.num_outputs for l in model.layers]


def _noise(model, S, N, dev, seed=1):
    """One [S, N, dim] array per layer (the layout of the predictive routes); ``_bk`` turns it into [N, S, dim] (the training layout)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(S, N, w, generator=g).to(dev) for w in _widths(model)]


def _bk(zs):
    return [z.transpose(0, 1).contiguous() for z in zs]


def _n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _layerwise_logw(model, X, Y, S, zs, kind="predictive", prior=False):
    """float64 composition from the per-layer outputs of ``_forward_iw`` on a model over the same layers whose data are (X, Y):
    -> (logw [N, S], big, n_add) with the reference module's rounding count."""
    from dgps_with_iwvi_amd.likelihoods import is_gaussian
    from dgps_with_iwvi_amd.models import DGP_IWVI
    N = X.shape[0]
    if prior:                                                    # latent-variable layers in prior mode, layer by layer; no regulariser
        m, v = model.predict_f_multisample(X, S, zs=zs)
        fmean, fvar, kls = m.transpose(0, 1).contiguous(), v.transpose(0, 1).contiguous(), []
    else:
        ref = DGP_IWVI(X, Y, model.layers, model.likelihood, num_samples=S)
        fmean, fvar, local_kls, _, _, _, _ = ref._forward_iw(_bk(zs))
        kls = [_n64(k).reshape(N, S, -1) for k in local_kls]
    if is_gaussian(model.likelihood):
        return R.logw_moments(_n64(fmean).reshape(N, S, -1), _n64(fvar).reshape(N, S, -1), _n64(Y), float(np.float32(model.likelihood.variance)),
                              1 if kind == "bound" else 0, kls)
    Yx = Y[:, None, :].expand(N, S, Y.shape[1]).contiguous()
    fn = model.likelihood.variational_expectations if kind == "bound" else model.likelihood.predict_density
    terms = fn(fmean.reshape(N, S, -1).contiguous(), fvar.reshape(N, S, -1).contiguous(), Yx)
    return R.logw_terms(_n64(terms).reshape(N, S, -1), kls)


def _check_summaries(res, lw, label):
    ref = R.summary(lw)
    tol_raw = IW.tol_reduce(lw)
    for key, name, tol in (("raw", "log_density", tol_raw), ("psis", "log_density_psis", R.gpu_psis_bound(tol_raw)),
                           ("khat", "khat", np.full_like(tol_raw, KHAT_TOL)), ("ess", "ess", ESS_RTOL * ref["ess"])):
        g, r = _n64(res[name]), ref[key]
        fin = np.isfinite(r)
        assert np.array_equal(g[~fin], r[~fin]), (label, key, g, r)
        gap = np.abs(g - r)[fin]
        print("  %s %s: worst gap / bound %.3g%s" % (label, key, float((gap / tol[fin]).max()) if fin.any() else 0.0,
                                                     "  (%.3g of the raw bound)" % float((gap / tol_raw[fin]).max()) if key == "psis" and fin.any() else ""))
        assert (gap <= tol[fin]).all(), (label, key, g, r, tol)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("kind", ["predictive", "bound"])
def test_log_weights_are_the_layerwise_composition(gpu_device, cfg, kind):
    S = 33
    model, Xt, Yt = _model(cfg, gpu_device)
    zs = _noise(model, S, N_TEST, gpu_device)
    res = model.importance_log_density(Xt, Yt, S, kind=kind, zs=zs, return_logw=True)
    assert set(res) == {"log_density", "log_density_psis", "khat", "ess", "logw"} and res["logw"].shape == (N_TEST, S)
    l64, big, n_add = _layerwise_logw(model, Xt, Yt, S, zs, kind=kind)
    lw = _n64(res["logw"])
    tol = IW.tol_logw(big, n_add)
    gap = np.abs(lw - l64).max(1)
    print("  %s %s: logw worst gap / bound %.3g" % (cfg, kind, float((gap / tol).max())))
    assert (gap <= tol).all(), (gap, tol)
    _check_summaries(res, lw, "%s %s" % (cfg, kind))
    # batches of three points: the same bits
    res3 = model.importance_log_density(Xt, Yt, S, kind=kind, zs=zs, return_logw=True, batch_size=3)
    for k in res:
        assert torch.equal(res[k], res3[k]), k


@pytest.mark.parametrize("cfg", CONFIGS)
def test_prior_proposal_is_predict_log_density_with_diagnostics(gpu_device, cfg):
    S = 40
    model, Xt, Yt = _model(cfg, gpu_device)
    zs = _noise(model, S, N_TEST, gpu_device, seed=5)
    res = model.importance_log_density(Xt, Yt, S, proposal="prior", zs=zs, return_logw=True)
    want = _n64(model.predict_log_density(Xt, Yt, S, zs=zs))
    l64, big, n_add = _layerwise_logw(model, Xt, Yt, S, zs, prior=True)
    tol = IW.tol_reduce(l64) + IW.tol_logw(big, n_add)
    gap = np.abs(_n64(res["log_density"]) - want)
    print("  %s: worst gap / bound %.3g" % (cfg, float((gap / tol).max())))
    assert (gap <= tol).all(), (gap, tol)
    _check_summaries(res, _n64(res["logw"]), cfg + " prior")


def _poisson_model(dev):
    from dgps_with_iwvi_amd import likelihoods, synthetic
    spec = synthetic.make_spec(L=2, M=16, B=16, K=4, Dx=3, Dy=2, with_lv=True, seed=21, n_data=N_TRAIN + N_TEST, distinct_y=True)
    spec["Y"] = np.floor(np.abs(spec["Y"]) * 3.0)
    Xt, Yt = np.asarray(spec["X"][N_TRAIN:], dtype=np.float32), np.asarray(spec["Y"][N_TRAIN:], dtype=np.float32)
    spec["X"], spec["Y"], spec["n_data"] = spec["X"][:N_TRAIN], spec["Y"][:N_TRAIN], N_TRAIN
    model = synthetic.build_model(spec, dev, likelihood=likelihoods.Poisson(binsize=1.5))
    return model, torch.as_tensor(Xt, device=dev), torch.as_tensor(Yt, device=dev)


def test_prior_proposal_of_a_poisson_model_is_predict_mixture(gpu_device):
    S = 40
    model, Xt, Yt = _poisson_model(gpu_device)
    zs = _noise(model, S, N_TEST, gpu_device, seed=6)
    res = model.importance_log_density(Xt, Yt, S, proposal="prior", zs=zs, return_logw=True)
    want = _n64(model.predict_log_density(Xt, Yt, S, zs=zs))       # (through predict_mixture)
    l64, big, n_add = _layerwise_logw(model, Xt, Yt, S, zs, prior=True)
    tol = IW.tol_reduce(l64) + IW.tol_logw(big, n_add)
    gap = np.abs(_n64(res["log_density"]) - want)
    print("  poisson: worst gap / bound %.3g" % float((gap / tol).max()))
    assert (gap <= tol).all(), (gap, tol)


@pytest.mark.parametrize("cfg", ["L1", "L1_G2_L1"])
def test_bound_kind_on_the_minibatch_is_the_training_bound(gpu_device, cfg):
    K = 7
    model, _, _ = _model(cfg, gpu_device, K=K, minibatch=16)
    B = model.X.shape[0]
    zs = _noise(model, K, B, gpu_device, seed=7)
    want = _n64(model.E_log_p_Y(_bk(zs)))
    res = model.importance_log_density(model.X, model.Y, K, kind="bound", zs=zs, return_logw=True)
    l64, big, n_add = _layerwise_logw(model, model.X, model.Y, K, zs, kind="bound")
    tol = IW.tol_reduce(l64) + IW.tol_logw(big, n_add)
    gap = np.abs(_n64(res["log_density"]) - want)
    print("  %s: worst gap / bound %.3g" % (cfg, float((gap / tol).max())))
    assert (gap <= tol).all(), (gap, tol)
    # ... and the exported log-weights are the training log-weights
    lw_train = _n64(model._logw(_bk(zs))).reshape(B, K)
    assert (np.abs(_n64(res["logw"]) - lw_train).max(1) <= IW.tol_logw(big, n_add)).all()


def test_encoder_and_prior_proposals_agree(gpu_device):
    """Likelihood variance 0.25, q_mu scale 0.3 and the encoder widened to about N(0, 1) (``_model``: wide_encoder): the values at which
    every one of the 8 points has a restatement ESS of at least 50 under BOTH proposals at S = 4096."""
    from dgps_with_iwvi_amd import settings
    S = 4096
    model, Xt, Yt = _model("L1", gpu_device, lik_var=0.25, q_scale=0.3, wide_encoder=True)
    settings.set_seed(11)
    model._words().zero_()
    a = model.importance_log_density(Xt, Yt, S, proposal="encoder", return_logw=True)
    b = model.importance_log_density(Xt, Yt, S, proposal="prior", return_logw=True)
    ra, rb = R.summary(_n64(a["logw"])), R.summary(_n64(b["logw"]))
    print("  ESS encoder", np.round(ra["ess"], 1), "prior", np.round(rb["ess"], 1))
    print("  khat encoder", np.round(ra["khat"], 3), "prior", np.round(rb["khat"], 3))
    assert (ra["ess"] >= 50).all() and (rb["ess"] >= 50).all(), (ra["ess"], rb["ess"])
    gap = np.abs(_n64(a["log_density"]) - _n64(b["log_density"]))
    bound = 5.0 * np.sqrt(1.0 / ra["ess"] - 1.0 / S + 1.0 / rb["ess"] - 1.0 / S)
    print("  |IS - MC| / bound", np.round(gap / bound, 3))
    assert gap.shape == (N_TEST,) and (gap <= bound).all(), (gap, bound)
    assert not torch.equal(a["logw"], b["logw"])                 # (two different proposals did run)


@pytest.mark.parametrize("kind", ["poisson", "multiclass", "hetero"])
def test_other_likelihoods_take_the_terms_route(gpu_device, kind):
    from dgps_with_iwvi_amd import likelihoods, synthetic
    S = 21
    if kind == "poisson":
        model, Xt, Yt = _poisson_model(gpu_device)
    elif kind == "multiclass":
        import multiclass_restatement as MR
        spec, _ = MR.three_class_problem()                       # (the reference's initial values; its first rows stand in as held-out points)
        model = synthetic.build_model(spec, gpu_device, likelihood=likelihoods.MultiClass(3))
        Xt = torch.as_tensor(np.asarray(spec["X"][:N_TEST], dtype=np.float32), device=gpu_device)
        Yt = torch.as_tensor(np.asarray(spec["Y"][:N_TEST], dtype=np.float32), device=gpu_device)
    else:
        spec = synthetic.make_hetero_spec(L=2, M=16, B=16, K=4, Dx=3, with_lv=True, seed=23, n_data=N_TRAIN + N_TEST, parity=True)
        Xt, Yt = np.asarray(spec["X"][N_TRAIN:], dtype=np.float32), np.asarray(spec["Y"][N_TRAIN:], dtype=np.float32)
        spec["X"], spec["Y"], spec["n_data"] = spec["X"][:N_TRAIN], spec["Y"][:N_TRAIN], N_TRAIN
        model = synthetic.build_model(spec, gpu_device, likelihood=likelihoods.HeteroskedasticGaussian())
        Xt, Yt = torch.as_tensor(Xt, device=gpu_device), torch.as_tensor(Yt, device=gpu_device)
    zs = _noise(model, S, N_TEST, gpu_device, seed=8)
    for k in ("predictive", "bound"):
        res = model.importance_log_density(Xt, Yt, S, kind=k, zs=zs, return_logw=True)
        l64, big, n_add = _layerwise_logw(model, Xt, Yt, S, zs, kind=k)
        lw = _n64(res["logw"])
        tol = IW.tol_logw(big, n_add)
        gap = np.abs(lw - l64).max(1)
        print("  %s %s: logw worst gap / bound %.3g" % (kind, k, float((gap / tol).max())))
        assert (gap <= tol).all(), (kind, k, gap, tol)
        _check_summaries(res, lw, "%s %s" % (kind, k))


def _state(model):
    from dgps_with_iwvi_amd.layers import LatentVariableLayer
    lv = [l for l in model.layers if isinstance(l, LatentVariableLayer)]
    return dict(X=model.X, Y=model.Y, Xb=model.X.clone(), Yb=model.Y.clone(), serial=model._mb_serial, key=model._mb_key(),
                xy=getattr(model, "_xy_cache", None), xyb=None if getattr(model, "_xy_cache", None) is None else model._xy_cache.clone(),
                xy_key=getattr(model, "_xy_key", None), enc=[getattr(l, "_enc_out", None) for l in lv],
                encb=[None if getattr(l, "_enc_out", None) is None else l._enc_out.clone() for l in lv],
                enc_key=[getattr(l, "_enc_key", None) for l in lv])


@pytest.mark.parametrize("cfg", ["L1", "L1_G2_L1"])
def test_the_models_state_is_as_it_was(gpu_device, cfg):
    K = 5
    model, Xt, Yt = _model(cfg, gpu_device, K=K, minibatch=16)
    zs = _bk(_noise(model, K, 16, gpu_device, seed=9))
    first = model.compute_log_likelihood(zs)
    lw0 = model._logw(zs).clone()
    before = _state(model)
    model.importance_log_density(Xt, Yt, 25, zs=_noise(model, 25, N_TEST, gpu_device, seed=10), batch_size=5)
    model.importance_log_density(Xt, Yt, 25, proposal="prior", kind="bound")
    after = _state(model)
    assert after["X"] is before["X"] and after["Y"] is before["Y"] and after["xy"] is before["xy"]
    assert (after["serial"], after["key"], after["xy_key"], after["enc_key"]) == (before["serial"], before["key"], before["xy_key"], before["enc_key"])
    assert torch.equal(after["Xb"], before["Xb"]) and torch.equal(after["Yb"], before["Yb"]) and torch.equal(after["xyb"], before["xyb"])
    for a, b, ab, bb in zip(after["enc"], before["enc"], after["encb"], before["encb"]):
        assert a is b and (ab is None and bb is None or torch.equal(ab, bb))
    assert model.compute_log_likelihood(zs) == first
    assert torch.equal(model._logw(zs), lw0)
    # a refused call leaves it as it was too
    with pytest.raises(ValueError):
        model.importance_log_density(Xt, Yt[:, :0], 25)
    assert model._mb_key() == before["key"] and model.compute_log_likelihood(zs) == first


def test_evaluate_importance_and_psis_summary_of_the_training_weights(gpu_device):
    from dgps_with_iwvi_amd import evaluation, settings
    K = 32
    model, Xt, Yt = _model("L1", gpu_device, K=K, minibatch=16)
    settings.set_seed(3)
    model._words().zero_()
    res = evaluation.evaluate_importance(model, Xt.cpu().numpy(), Yt.cpu().numpy(), num_importance_samples=200, predict_batch_size=3)
    assert set(res) == {"test_loglik_is", "test_loglik_psis", "test_khat_median", "test_khat_max", "test_khat_bad_share",
                        "test_ess_median", "test_ess_min"}
    assert all(math.isfinite(v) for k, v in res.items() if "khat" not in k) and 0.0 <= res["test_khat_bad_share"] <= 1.0
    assert 1.0 <= res["test_ess_min"] <= res["test_ess_median"] <= 200.0 and res["test_khat_median"] <= res["test_khat_max"]
    settings.set_seed(3)
    model._words().zero_()
    per = model.importance_log_density(Xt, Yt, 200, batch_size=3)
    assert res["test_loglik_is"] == float(per["log_density"].double().mean())
    assert res["test_loglik_psis"] == float(per["log_density_psis"].double().mean())
    assert res["test_khat_bad_share"] == float((per["khat"] > 0.7).double().mean())
    pr = evaluation.evaluate_importance(model, Xt, Yt, num_importance_samples=64, proposal="prior")
    assert math.isfinite(pr["test_loglik_is"])
    # the training log-weights: the ESS of the new kernel is importance_ess
    zs = _bk(_noise(model, K, 16, gpu_device, seed=12))
    s = evaluation.psis_summary(model._logw(zs).view(16, K))
    ess = model.importance_ess(zs)
    np.testing.assert_allclose(_n64(s["ess"]), _n64(ess), rtol=ESS_RTOL, atol=0)
    assert torch.isfinite(s["khat"]).all() and torch.isfinite(s["log_mean_psis"]).all()
    np.testing.assert_allclose(_n64(s["log_mean"]), _n64(model.E_log_p_Y(zs)), rtol=0, atol=float(IW.tol_reduce(_n64(model._logw(zs)).reshape(16, K)).max()) * 2)


def test_refusals_name_their_limits(gpu_device):
    model, Xt, Yt = _model("L1", gpu_device)
    with pytest.raises(ValueError, match="16384"):
        model.importance_log_density(Xt, Yt, 16385)
    with pytest.raises(ValueError, match="S must be"):
        model.importance_log_density(Xt, Yt, 0)
    with pytest.raises(ValueError, match="proposal"):
        model.importance_log_density(Xt, Yt, 10, proposal="posterior")
    with pytest.raises(ValueError, match="kind"):
        model.importance_log_density(Xt, Yt, 10, kind="elbo")
    five, Xt5, Yt5 = _model("L1_L1_L1_L1_L1", gpu_device)
    with pytest.raises(ValueError, match="IWVI_MAX_KL") as ei:
        five.importance_log_density(Xt5, Yt5, 10)
    assert "5 latent-variable layers" in str(ei.value) and "at most 4" in str(ei.value)
    assert torch.isfinite(five.importance_log_density(Xt5, Yt5, 10, proposal="prior")["log_density"]).all()   # (no weights, no limit)
