"""``DGP_IWVI.bound`` (models.Bound: MIWAE, CIWAE, VR-alpha) through the model, the backward driver and the trainer, on small stacks
(M = 16, B = 7, K = 6, Dx = 4; one with a leading latent-variable layer, one without) with fixed noise:

  value      the model's bound against the float64 statement (tests/bound_family_reference.py) applied to the model's own log-weights;
  gradient   miwae:G against the mean over the groups of the importance-weighted gradients of K / G-sample models over the SAME layer objects
             (code that tests/test_gpu_backward.py verifies against the oracle), ciwae:beta against the convex combination of its two ends --
             every gradient name, at twice the tolerance tests/test_gpu_backward.py applies to that name against the oracle (5e-3 of the
             largest entry, so 1e-2);
  trainer    use_graph=True bit-identical to eager, across a change of ``model.bound`` between steps;
  the default bound takes the launches it took, every refusal comes before any launch, ``importance_ess`` lies in [1, K]."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bound_family_reference as F   # noqa: E402
import iw_reduction_reference as R   # noqa: E402

pytestmark = pytest.mark.gpu

K, B = 6, 7
STACKS = [True, False]                                           # with / without the leading latent-variable layer
GRAD_RTOL = 2 * 5e-3


def _spec(lv, seed=3):
    from dgps_with_iwvi_amd import synthetic
    return synthetic.make_spec(L=2, M=16, B=B, K=K, Dx=4, with_lv=lv, seed=seed)


def _model_and_noise(dev, lv, seed=3):
    from dgps_with_iwvi_amd import synthetic
    spec = _spec(lv, seed)
    zs = [torch.as_tensor(np.asarray(z, dtype=np.float32), device=dev) for z in synthetic.make_noise(spec, seed=2)]
    return synthetic.build_model(spec, dev), zs


def _close(name, got, ref, rtol=GRAD_RTOL):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64).reshape(np.shape(got))
    scale = max(np.abs(ref).max(), 1e-12)
    err = np.abs(got - ref).max()
    assert err <= rtol * scale, "%s: max err %.3e vs scale %.3e" % (name, err, scale)


def _grads(model, zs, **kw):
    from dgps_with_iwvi_amd import backward
    elbo, g = backward.iw_elbo_and_gradients(model, zs, **kw)
    return float(elbo), {k: v.detach().cpu().numpy().astype(np.float64) for k, v in g.items()}


class _Calls:
    """Counts the calls of the named entry points of the loaded library while active (the Python side looks them up on the handle)."""

    def __init__(self, *names):
        self.names, self.n = names, {k: 0 for k in names}

    def __enter__(self):
        from dgps_with_iwvi_amd import _abi
        self.lib = _abi.lib()
        self.orig = {k: getattr(self.lib, k) for k in self.names}
        for k in self.names:
            def wrap(*a, _k=k):
                self.n[_k] += 1
                return self.orig[_k](*a)
            setattr(self.lib, k, wrap)
        return self.n

    def __exit__(self, *exc):
        for k, f in self.orig.items():
            setattr(self.lib, k, f)


_ENTRIES = ("iwvi_model_precompute", "iwvi_gp_precompute", "iwvi_dgp_forward", "iwvi_iw_elbo_backward_dev", "iwvi_logw_reduce",
            "iwvi_bound_logw_reduce", "iwvi_bound_elbo_backward", "iwvi_gp_layer_backward")


@pytest.mark.parametrize("lv", STACKS)
@pytest.mark.parametrize("text", ["miwae:2", "miwae:3", "ciwae:0.3", "vr:0.5"])
def test_value_is_the_float64_statement_on_the_models_own_log_weights(gpu_device, lv, text):
    from dgps_with_iwvi_amd.models import Bound
    model, zs = _model_and_noise(gpu_device, lv)
    L = model._logw(zs).detach().cpu().numpy().astype(np.float64).reshape(B, K)
    kl = [g.detach().cpu().numpy().astype(np.float64).reshape(-1) for g in model._global_kls()]
    model.bound = text
    b = model.bound
    assert b == Bound.parse(text) and not b.is_default
    lp = model.E_log_p_Y(zs).detach().cpu().numpy().astype(np.float64)
    ref, tol = F.bound_n(L, b.groups, b.tau, b.beta), F.tol_bound(L, b.groups, b.tau, b.beta)
    print("  %s lv=%s: bound_n max err %.3e (allowed %.3e)" % (text, lv, np.abs(lp - ref).max(), tol.min()))
    assert np.all(np.abs(lp - ref) <= tol), (text, float(np.abs(lp - ref).max()))
    scale = float(model.num_data) / B
    val = model.compute_log_likelihood(zs)
    assert abs(val - R.bound(lp, scale, kl)) <= R.bound_tol(lp, scale) + 64 * 2.0 ** -52 * sum(float(np.abs(k).sum()) for k in kl), (val, R.bound(lp, scale, kl))
    assert abs(val - R.bound(ref, scale, kl)) <= scale * float(tol.sum()) + 1e-9 * abs(val)
    # the value the backward driver returns is the same bound, from the other kernel
    e, _ = _grads(model, zs)
    assert abs(e - val) <= 1e-5 * abs(val), (e, val)            # (two float32 routes to L_nk: the figure tests/test_gpu_likelihoods.py allows between them)


@pytest.mark.parametrize("lv", STACKS)
@pytest.mark.parametrize("G", [2, 3])
def test_miwae_gradient_is_the_mean_of_the_groups_importance_weighted_gradients(gpu_device, lv, G):
    from dgps_with_iwvi_amd.models import DGP_IWVI
    model, zs = _model_and_noise(gpu_device, lv)
    Kg = K // G
    vals, parts = [], []
    for g in range(G):
        sub = DGP_IWVI(model.X, model.Y, model.layers, model.likelihood, num_samples=Kg)
        sub.num_data = model.num_data
        v, gr = _grads(sub, [z[:, g * Kg:(g + 1) * Kg].contiguous() for z in zs])
        vals.append(v)
        parts.append(gr)
    model.bound = "miwae:%d" % G
    val, grads = _grads(model, zs)
    assert abs(val - np.mean(vals)) <= 2e-4 * abs(val), (val, vals)
    assert sorted(grads) == sorted(parts[0])
    for k in grads:
        _close(k, grads[k], np.mean([p[k].reshape(grads[k].shape) for p in parts], 0))
    # wrt="final_q" follows the bound: the same value and the same two entries, bit for bit
    from dgps_with_iwvi_amd import backward
    e_q, g_q = backward.iw_elbo_and_gradients(model, zs, wrt="final_q")
    e_a, g_a = backward.iw_elbo_and_gradients(model, zs)
    assert float(e_q) == float(e_a) and len(g_q) == 2
    for k in g_q:
        assert torch.equal(g_q[k], g_a[k]), k


@pytest.mark.parametrize("lv", STACKS)
def test_ciwae_gradient_is_the_convex_combination_of_its_ends(gpu_device, lv):
    model, zs = _model_and_noise(gpu_device, lv)
    beta = 0.3
    v_iw, g_iw = _grads(model, zs)
    model.bound = "ciwae:1"
    v_el, g_el = _grads(model, zs)
    model.bound = "ciwae:%r" % beta
    val, grads = _grads(model, zs)
    assert abs(val - (beta * v_el + (1 - beta) * v_iw)) <= 2e-4 * abs(val)
    assert sorted(grads) == sorted(g_iw)
    for k in grads:
        _close(k, grads[k], beta * g_el[k] + (1 - beta) * g_iw[k])
    assert any(np.abs(g_el[k] - g_iw[k]).max() > 2 * GRAD_RTOL * np.abs(g_iw[k]).max() for k in grads), "the two ends do not differ: the test shows nothing"


def test_trainer_graph_mode_equals_eager_and_follows_a_change_of_bound(gpu_device):
    from dgps_with_iwvi_amd import synthetic, settings
    from dgps_with_iwvi_amd.training import Trainer
    spec = _spec(True, seed=11)
    out = []
    for use_graph in (False, True):
        settings.set_seed(5)
        model = synthetic.build_model(spec, gpu_device)
        model.bound = "miwae:2"
        tr = Trainer(model, use_graph=use_graph, check_finite=False)
        vals = [float(tr.step()) for _ in range(3)]
        after3 = [p.clone() for _, p, _ in tr._entries] + [model.layers[-1].q_mu.clone(), model.layers[-1].q_sqrt.clone()]
        n_graphs = len(tr._graphs)
        model.bound = "vr:0.5"                                   # between steps: the captured launches hold the old triple
        vals += [float(tr.step()) for _ in range(2)]
        model.bound = "iwae"                                     # and back to the default route (fused heads)
        vals.append(float(tr.step()))
        out.append((vals, after3, [p.clone() for _, p, _ in tr._entries] + [model.layers[-1].q_mu.clone(), model.layers[-1].q_sqrt.clone()], n_graphs))
    assert out[1][3] >= 1 and out[0][3] == 0
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert all(np.isfinite(v) for v in out[0][0])
    for i in (1, 2):
        for pa, pb in zip(out[0][i], out[1][i]):
            assert torch.equal(pa, pb)
    # the bound did change what was trained: the same three steps under the default bound end elsewhere
    settings.set_seed(5)
    model = synthetic.build_model(spec, gpu_device)
    tr = Trainer(model, check_finite=False)
    for _ in range(3):
        tr.step()
    assert not all(torch.equal(p, q) for (_, p, _), q in zip(tr._entries, out[0][1]))


@pytest.mark.parametrize("lv", STACKS)
def test_default_bound_takes_the_launches_it_took(gpu_device, lv):
    """Under ``Bound.iwae()`` -- never set, or set back after another member -- value and value + gradient make the same library calls (none of
    them an iwvi_bound_* entry: one layer launch per evaluation, the heads out of its tail) and give the same bits; another member adds
    exactly its two entries.  At M = 32, K = 8, B = 520, where the library fuses the heads (tests/test_gpu_fused_tail_reduction.py: at
    K = 6 the launch's chunk does not hold whole points and both routes would take the separate heads launch)."""
    from dgps_with_iwvi_amd import synthetic
    from dgps_with_iwvi_amd.models import Bound
    spec = synthetic.make_spec(L=1 if lv else 2, M=32, B=520, K=8, with_lv=lv, seed=4)
    zs = [torch.as_tensor(np.asarray(z, dtype=np.float32), device=gpu_device) for z in synthetic.make_noise(spec, seed=2)]
    fresh, back = synthetic.build_model(spec, gpu_device), synthetic.build_model(spec, gpu_device)
    back.bound = "miwae:2"
    back.bound = Bound.iwae()
    assert fresh.bound == Bound.iwae() and back.bound.is_default
    seen = []
    for m in (fresh, back):
        with _Calls(*_ENTRIES) as n:
            v = m._build_likelihood(zs).clone()
            lp = m.E_log_p_Y(zs).clone()
            from dgps_with_iwvi_amd import backward
            e, g = backward.iw_elbo_and_gradients(m, zs)
        seen.append((dict(n), v, lp, e.clone(), {k: t.clone() for k, t in g.items()}))
    n0 = seen[0][0]
    assert n0 == seen[1][0] and n0["iwvi_bound_logw_reduce"] == 0 and n0["iwvi_bound_elbo_backward"] == 0 and n0["iwvi_logw_reduce"] == 0, n0
    assert n0["iwvi_dgp_forward"] == 3 and n0["iwvi_iw_elbo_backward_dev"] == 0, n0     # one launch per evaluation: the fused tail, the fused heads
    assert torch.equal(seen[0][1], seen[1][1]) and torch.equal(seen[0][2], seen[1][2]) and torch.equal(seen[0][3], seen[1][3])
    for k in seen[0][4]:
        assert torch.equal(seen[0][4][k], seen[1][4][k]), k
    back.bound = "miwae:2"
    with _Calls(*_ENTRIES) as n:
        back._build_likelihood(zs)
        back.E_log_p_Y(zs)
        backward.iw_elbo_and_gradients(back, zs)
    assert n["iwvi_bound_logw_reduce"] == 2 and n["iwvi_bound_elbo_backward"] == 1 and n["iwvi_iw_elbo_backward_dev"] == 0, dict(n)
    assert n["iwvi_dgp_forward"] == 3 and n["iwvi_gp_layer_backward"] == n0["iwvi_gp_layer_backward"], dict(n)


def test_every_refusal_comes_before_any_launch(gpu_device):
    from dgps_with_iwvi_amd import backward, likelihoods, synthetic
    from dgps_with_iwvi_amd.models import DGP_VI
    from dgps_with_iwvi_amd.training import Trainer
    model, zs = _model_and_noise(gpu_device, True)
    model.bound = "miwae:2"
    ms_exchange = lambda ms: ms[:, 0]
    student = synthetic.build_model(_spec(True), gpu_device, likelihood=likelihoods.StudentT(scale=0.5, df=4.0))
    student.bound = "ciwae:0.5"
    literal, _ = _model_and_noise(gpu_device, True)
    literal.bound, literal.full_cov_over_samples = "vr:0.5", True
    odd, _ = _model_and_noise(gpu_device, True)
    odd.bound = "miwae:4"                                        # 6 % 4: refused where it is used
    ktrainer = Trainer(_model_and_noise(gpu_device, True)[0], shard="k")
    ktrainer.model.bound = "miwae:2"
    vi = synthetic.build_model(_spec(True), gpu_device, cls=DGP_VI)
    with _Calls(*_ENTRIES) as n:
        with pytest.raises(NotImplementedError, match="shard"):
            backward.iw_elbo_and_gradients(model, zs, exchange=ms_exchange)
        with pytest.raises(NotImplementedError, match="shard"):
            backward.iw_elbo_and_gradients(model, zs, K_total=2 * K)
        with pytest.raises(NotImplementedError, match="sharded training"):
            ktrainer.step()
        with pytest.raises(ValueError, match="mode_vi"):
            backward.iw_elbo_and_gradients(model, zs, mode_vi=True)
        with pytest.raises(ValueError, match="DGP_VI"):
            vi.bound = "miwae:2"
        with pytest.raises(ValueError, match="'dreg' and 'stl'"):
            backward.iw_elbo_and_gradients(model, zs, encoder_gradient="dreg")
        model.encoder_gradient = "stl"
        with pytest.raises(ValueError, match="'dreg' and 'stl'"):
            backward.iw_elbo_and_gradients(model, zs)
        model.encoder_gradient = "iwae"
        for call in (lambda: backward.iw_elbo_and_gradients(student, zs), student.compute_log_likelihood, student.E_log_p_Y):
            with pytest.raises(NotImplementedError, match="Gaussian policy only"):
                call()
        for call in (literal.compute_log_likelihood, lambda: literal.E_log_p_Y(zs)):
            with pytest.raises(NotImplementedError, match="full_cov_over_samples"):
                call()
        with pytest.raises(NotImplementedError, match="lse_partials"):
            model.lse_partials(zs)
        for call in (odd.compute_log_likelihood, lambda: odd.E_log_p_Y(zs), lambda: backward.iw_elbo_and_gradients(odd, zs)):
            with pytest.raises(ValueError, match="does not divide num_samples=6"):
                call()
    assert all(v == 0 for v in n.values()), dict(n)
    assert vi.bound.is_default
    vi.bound = "iwae"                                            # the default is everybody's


@pytest.mark.parametrize("lv", STACKS)
def test_importance_ess_lies_in_1_K_under_every_bound(gpu_device, lv):
    model, zs = _model_and_noise(gpu_device, lv)
    L = model._logw(zs).detach().cpu().numpy().astype(np.float64).reshape(B, K)
    e0 = model.importance_ess(zs)
    assert tuple(e0.shape) == (B,)
    got = e0.detach().cpu().numpy().astype(np.float64)
    assert np.all(got >= 1.0) and np.all(got <= K), got
    assert np.all(np.abs(got - F.ess(L)) <= F.tol_ess(L)), (got, F.ess(L))
    for text in ("miwae:2", "ciwae:0.3", "vr:0.5"):
        model.bound = text
        assert torch.equal(model.importance_ess(zs), e0), text    # over all K, whatever the bound
    drawn = model.importance_ess().detach().cpu().numpy()         # device noise
    assert np.all(drawn >= 1.0) and np.all(drawn <= K)
