"""``sghmc.SGHMC`` (the reference's experiments/sghmc.py over ``q_sqrt = None`` layers), the factory ``build_models.build_sghmc_model`` and
``evaluation.evaluate_sghmc`` on a tiny model: N = 64 points, M = 16 inducing points, configuration 'G5', minibatches of 32."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, M, D = 64, 16, 4


def _data(seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)).astype(np.float32)
    Y = (np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))).astype(np.float32)
    return X, Y


def _args(**kw):
    a = dict(mode="SGHMC", configuration="G5", M=M, likelihood_variance=0.01, minibatch_size=32, num_IW_samples=1, lr=5e-3,
             fix_linear=True, use_graph=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _model(dev, **kw):
    from dgps_with_iwvi_amd import build_models as bm
    np.random.seed(3)                                            # the factory's k-means and N(0, 1) inducing inputs
    X, Y = _data()
    return bm.build_sghmc_model(_args(**kw), X, Y, device=dev)


def _sampler(dev, window_size=5, use_graph=False, **kw):
    """The factory's model with a sampler of our own window size (the factory's is the reference's 100)."""
    from dgps_with_iwvi_amd.sghmc import SGHMC
    model = _model(dev)
    opt = SGHMC(model, window_size=window_size, lr=5e-3, use_graph=use_graph, **kw)
    opt.generate_update_step(0.01, 0.05)
    return model, opt


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def test_factory_attaches_the_reference_attributes(gpu_device):
    from dgps_with_iwvi_amd.sghmc import SGHMC
    model = _model(gpu_device)
    assert all(l.q_sqrt is None for l in model.layers) and len(model.layers) == 2
    assert isinstance(model.sghmc_optimizer, SGHMC) and model.sghmc_optimizer.window_size == 100
    with pytest.raises(RuntimeError):
        model.sghmc_optimizer.sample_op()                        # before init_op: no update step yet
    model.init_op()
    assert model.global_step == 0 and (model.sghmc_optimizer.epsilon, model.sghmc_optimizer.mdecay) == (0.01, 0.05)
    for step in (1, 2):
        elbo = model.train_op()
        assert model.global_step == step and np.isfinite(float(elbo))
    assert model.sghmc_optimizer.window_len == 2


def test_refusals_come_before_any_work(gpu_device):
    from dgps_with_iwvi_amd import build_models as bm, synthetic
    from dgps_with_iwvi_amd.models import DGP_VI
    from dgps_with_iwvi_amd.sghmc import SGHMC
    X, Y = _data()
    with pytest.raises(NotImplementedError, match="latent-variable"):
        bm.build_sghmc_model(_args(configuration="L1_G5"), X, Y, device=gpu_device)
    with pytest.raises(NotImplementedError, match="build_sghmc_model"):
        bm.build_model(_args(), X, Y, device=gpu_device)
    iw = synthetic.build_model(synthetic.make_spec(L=2, M=16, B=9, K=2, seed=1), gpu_device)
    with pytest.raises(NotImplementedError, match="DGP_IWVI"):
        SGHMC(iw)
    lv = synthetic.build_model(synthetic.make_spec(L=2, M=16, B=9, K=1, seed=1, with_lv=True), gpu_device, cls=DGP_VI, num_samples=1)
    with pytest.raises(NotImplementedError, match="latent-variable"):
        SGHMC(lv)
    vi = synthetic.build_model(synthetic.make_spec(L=2, M=16, B=9, K=1, seed=1), gpu_device, cls=DGP_VI, num_samples=1)
    with pytest.raises(ValueError, match="q_sqrt = None"):
        SGHMC(vi)
    for l in vi.layers:
        l.q_sqrt = None
    with pytest.raises(NotImplementedError, match="sharded"):
        SGHMC(vi, group=object())


def test_twelve_steps_window_and_untouched_chain(gpu_device):
    model, opt = _sampler(gpu_device, window_size=5)
    Z0 = [l._Z().clone() for l in model.layers]
    for step in range(1, 13):
        e1 = opt.sghmc_step()
        assert opt.window_len == min(step, 5)
        theta = [t.clone() for t in opt.vars]
        e2 = opt.train_hypers()
        for t, t0, l in zip(opt.vars, theta, model.layers):
            assert torch.equal(t, t0), "train_hypers moved the chain's theta"
            assert l.q_mu.data_ptr() == t.data_ptr()
        assert _finite(e1, e2, *opt.vars)
    for st, t in zip(opt.state, opt.vars):
        assert _finite(*st.values())
        assert torch.equal(st["theta64"].float(), t)             # theta is the float32 rounding of its master
    assert all(not torch.equal(l._Z(), z0) for l, z0 in zip(model.layers, Z0)), "the hyper step trained nothing"
    assert float(opt.vars[0].abs().max()) > 0.0                  # the chain left q_mu = 0
    assert int(opt.adam.t_dev.item()) == 12 and opt.burn_in_op_count == 12 and opt.hyper_step_count == 12
    # the window holds the last five theta, the newest at position (12 - 1) % 5
    assert torch.equal(opt.window[0][(12 - 1) % 5], opt.vars[0])


def test_state_dict_round_trip_continues_bit_identically(gpu_device):
    from dgps_with_iwvi_amd import build_models as bm
    model, opt = _sampler(gpu_device, window_size=5)
    for _ in range(6):
        opt.sghmc_step()
        opt.train_hypers()
    sd_model, sd = bm.state_dict(model), opt.state_dict()

    def one_more():
        opt.sghmc_step()
        opt.train_hypers()
        opt.sample_op()
        return [t.clone() for t in opt.vars] + [l._Z().clone() for l in model.layers] + [st["p"].clone() for st in opt.state]

    a = one_more()
    bm.load_state_dict(model, sd_model)
    opt.load_state_dict(sd)
    b = one_more()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_graph_replay_equals_eager_bit_for_bit(gpu_device):
    out = []
    for use_graph in (False, True):
        from dgps_with_iwvi_amd import settings
        settings.set_seed(0)
        model, opt = _sampler(gpu_device, use_graph=use_graph)
        for _ in range(4):
            opt.sample_op()
        torch.cuda.synchronize()
        out.append([t.clone() for t in opt.vars] + [opt.rng_state.clone()])
        assert opt.sample_op_count == 4
    for x, y in zip(*out):
        assert torch.equal(x, y)
    assert float(out[0][0].abs().max()) > 0.0


def test_collect_samples_shapes_and_distinct_samples(gpu_device):
    model, opt = _sampler(gpu_device)
    samples = opt.collect_samples(3, 2)
    assert opt.sample_op_count == 6 and len(samples) == len(model.layers)
    for s, l in zip(samples, model.layers):
        assert tuple(s.shape) == (3, l.num_inducing, l.num_outputs) and s.is_cuda and _finite(s)
        for i in range(3):
            for j in range(i):
                assert not torch.equal(s[i], s[j])
    assert torch.equal(samples[0][2], model.layers[0].q_mu)


def test_evaluate_sghmc_columns_and_result(gpu_device):
    from dgps_with_iwvi_amd import evaluation
    model, opt = _sampler(gpu_device)
    for _ in range(3):
        opt.sghmc_step()
    Nt, S = 7, 8
    rng = np.random.default_rng(4)
    Xt = rng.standard_normal((Nt, D)).astype(np.float32)
    Yt = rng.standard_normal((Nt, 1)).astype(np.float32)
    t = lambda a: torch.as_tensor(a.astype(np.float32), device=gpu_device)
    zs = [t(rng.standard_normal((S, Nt, l.num_outputs))) for l in model.layers]
    z_y = t(rng.standard_normal((S, Nt, 1)))
    theta = [l.q_mu.clone() for l in model.layers]
    same = [q[None].repeat(S, 1, 1).contiguous() for q in theta]  # every kept theta = the current one
    res = evaluation.evaluate_sghmc(model, same, Xt, Yt, zs=zs, z_y=z_y, return_samples=True)
    assert tuple(res["samples"].shape) == (Nt, S)
    for j in range(S):
        want = model.predict_y_samples_fused(Xt, 1, zs=[z[j:j + 1] for z in zs], z_y=z_y[j:j + 1])      # [1, Nt, 1]
        assert torch.equal(res["samples"][:, j], want[0, :, 0]), j
    for l, q in zip(model.layers, theta):
        assert torch.equal(l.q_mu, q)                            # the chain's theta is back
    # results dict: the keys of evaluate(on_device=True), finite, from collected samples and in-kernel noise
    kept = opt.collect_samples(S, 1)
    got = evaluation.evaluate_sghmc(model, kept, Xt, Yt, predict_batch_size=4)       # two batches of points
    ref_keys = set(evaluation.evaluate(model, Xt, Yt, num_predict_samples=S, on_device=True))
    assert set(got) == ref_keys == {"test_loglik", "test_rmse", "test_shapiro_W_median"}
    assert all(np.isfinite(v) for v in got.values()), got
    with pytest.raises(ValueError):
        evaluation.evaluate_sghmc(model, kept[:1], Xt, Yt)
