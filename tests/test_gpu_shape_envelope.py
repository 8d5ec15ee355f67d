"""The shape envelope the C-ABI accepts (include/iwvi_hip.h: M <= 512; D, R, P <= 32; 8 layers per fused launch) against the float64
oracles, at the shapes where the kernels switch code: the second 16-wide q(u) block and output block of the forward, K_uf at 9 MFMA steps,
the fast ELBO tail on both sides of kl_total = 64, full-depth stacks, an LDS plan below 5 sub-tiles, every backward route pinned by
iwvi_debug_last_backward_routes, and one past every cap (refused before any launch).

Tolerances are the suites' stated ones: ELBO relative 1e-4 (2e-4 beside gradients), per-point log p rtol 3e-4, gradients max-norm
relative 5e-3.  Every inner mixing matrix is dense (``make_spec(mixing="dense")``): latent GPs beyond Dx reach the output."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.from_spec import build_oracle, oracle_noise   # noqa: E402

pytestmark = pytest.mark.gpu

ELBO_RTOL, LOGP_RTOL = 1e-4, 3e-4


def _t(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)


def _variant():
    from dgps_with_iwvi_amd import _abi
    return int(_abi.lib().iwvi_debug_last_forward_variant())


def _close(name, got, ref, rtol=5e-3):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-12)
    err = np.abs(got - ref).max()
    assert err <= rtol * scale, "%s: max err %.3e vs scale %.3e" % (name, err, scale)


def _kl_total(spec):
    return sum(l["q_mu"].shape[1] for l in spec["layers"] if l["type"] == "gp")


def _forward_vs_oracle(dev, spec, seed):
    """Injected draws through the fused forward + ELBO tail: the bound and the per-point log p against the oracle.  -> (elbo, variant)"""
    from dgps_with_iwvi_amd import synthetic
    zs = synthetic.make_noise(spec, seed=seed)
    model = synthetic.build_model(spec, dev)
    zd = [_t(z, dev) for z in zs]
    elbo = float(model.compute_log_likelihood(zd))
    torch.cuda.synchronize()
    variant = _variant()
    om = build_oracle(spec)
    ref = om.build_likelihood(oracle_noise(spec, zs))
    assert np.isfinite(elbo) and abs(elbo - ref) <= ELBO_RTOL * abs(ref), (spec["name"], elbo, ref)
    L_NK = om.log_weights(oracle_noise(spec, zs))[0]
    m_o = L_NK.max(1)
    logp_o = m_o + np.log(np.exp(L_NK - m_o[:, None]).sum(1)) - np.log(spec["K"])
    np.testing.assert_allclose(model.E_log_p_Y(zd).double().cpu().numpy(), logp_o, rtol=LOGP_RTOL, atol=100 * LOGP_RTOL)
    return elbo, variant


# ------------------------------------------------------------------------------------------------------------------------------------
# b. model-level forward, general variant
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why,kw", [
    ("16-wide blocks, inside edge", dict(L=2, M=128, B=24, K=5, Dx=16, R=16, Dy=16)),
    ("16-wide blocks, first past the edge", dict(L=2, M=128, B=24, K=5, Dx=17, R=17, Dy=17, distinct_y=True)),
    ("every cap, M > 128, kl_total = 64", dict(L=2, M=200, B=16, K=4, Dx=32, R=32, Dy=32, distinct_y=True)),
    ("kl_total = 65, Dx + Lw = 32", dict(L=3, M=96, B=16, K=4, Dx=31, R=32, Dy=1, with_lv=True, latent_dim=1)),
    ("LV latent_dim = 4", dict(L=2, M=64, B=20, K=6, Dx=28, R=9, Dy=3, with_lv=True, latent_dim=4, distinct_y=True)),
    ("LV + 7 GP layers", dict(L=7, M=32, B=12, K=3, Dx=6, R=3, Dy=2, with_lv=True)),
    ("8 GP layers", dict(L=8, M=32, B=12, K=3, Dx=5, R=4, Dy=1)),
])
def test_wide_and_deep_models_match_the_oracle(gpu_device, why, kw):
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(mixing="dense", seed=sum(v for v in kw.values() if isinstance(v, int)), **kw)
    _, variant = _forward_vs_oracle(gpu_device, spec, seed=5)
    assert not variant & (3 << 10), (why, hex(variant))
    assert bool(variant >> 9 & 1) == (kw["M"] > 128), (why, hex(variant))


@pytest.mark.parametrize("kw", [dict(L=2, M=200, B=16, K=4, Dx=32, R=32, Dy=32, distinct_y=True),                        # kl_total = 64
                                dict(L=3, M=96, B=16, K=4, Dx=31, R=32, Dy=1, with_lv=True, latent_dim=1)],               # kl_total = 65
                         ids=["kl64", "kl65"])
def test_both_elbo_tails_agree_at_the_kl_bound(gpu_device, kw):
    """The fast ELBO tail is taken while kl_total <= 64: on both sides of the bound the stored-partials tail (IWVI_FW_SLOW_TAIL) gives
    the same bound, and both hold the oracle's tolerance."""
    from dgps_with_iwvi_amd import _abi, synthetic
    spec = synthetic.make_spec(mixing="dense", seed=kw["M"], **kw)
    assert _kl_total(spec) in (64, 65)
    out = []
    for slow in (0, 1):
        _abi.set_debug_option("IWVI_FW_SLOW_TAIL", slow)
        try:
            out.append(_forward_vs_oracle(gpu_device, spec, seed=9)[0])
        finally:
            _abi.set_debug_option("IWVI_FW_SLOW_TAIL", 0)
    assert abs(out[0] - out[1]) <= 1e-6 * abs(out[1]), out


def test_wide_stack_with_a_lowered_lds_plan(gpu_device):
    """A wide stack at 16 400 samples: the LDS planner steps the sub-tiles per workgroup below 5, and the bound still matches."""
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=2, M=128, B=820, K=20, Dx=32, R=32, Dy=1, mixing="dense", seed=31, n_data=820)
    _, variant = _forward_vs_oracle(gpu_device, spec, seed=3)
    assert (variant & 0xff) < 5, hex(variant)


# ------------------------------------------------------------------------------------------------------------------------------------
# d. backward against float64 autograd, every case pinned to its route
# ------------------------------------------------------------------------------------------------------------------------------------
def _layer_case(dev, spec, li, T, Tr, seed):
    """One GP layer's adjoint on T rows against float64 autograd -> the routes that ran.  Tr < T: the cotangents are live on
    ``live_rows(T)`` only (tests/adjoint_reference.py: a live row in every 16-row tile, so in every workgroup and every split-K chunk),
    and the reference is evaluated on those rows."""
    from dgps_with_iwvi_amd import _abi, backward, synthetic
    from adjoint_reference import live_rows, mask_rows
    from test_gpu_backward import _layer_reference
    model = synthetic.build_model(spec, dev)
    layer = model.layers[li]
    rng = np.random.default_rng(seed)
    D, R = layer._Z().shape[1], layer.num_outputs
    P = spec["layers"][li]["W"].shape[0] if spec["layers"][li]["W"] is not None else R
    F = rng.standard_normal((T, D)).astype(np.float32)
    z = rng.standard_normal((T, R)).astype(np.float32)
    cs, cm, cv = (rng.standard_normal((T, P)).astype(np.float32) for _ in range(3))
    rows = np.arange(T) if Tr >= T else live_rows(T)
    mask_rows(rows, cs, cm, cv)
    saved = backward.gp_forward_saved(layer, _t(F, dev), _t(z, dev))
    _abi.backward_routes()                                           # (empties the log)
    out = backward.gp_backward(layer, saved, _t(cs, dev), _t(cm, dev), _t(cv, dev), kl_weight=0.7)
    torch.cuda.synchronize()
    routes = _abi.backward_routes()
    ref = _layer_reference(spec, li, F[rows], z[rows], cs[rows], cm[rows], cv[rows], 0.7)
    dF = out["dF"].cpu().numpy()
    _close("dF", dF[rows], ref["F"])
    dead = np.setdiff1d(np.arange(T), rows)
    assert len(dead) == 0 or float(np.abs(dF[dead]).max()) == 0.0
    _close("dq_mu", out["dq_mu"].cpu(), ref["q_mu"])
    _close("dq_sqrt", out["dq_sqrt"].cpu(), np.tril(ref["q_sqrt"]))
    _close("dZ", out["dZ"].cpu(), ref["Z"])
    _close("dls", out["dls"].cpu(), ref["ls"])
    _close("dvariance", out["dvariance"].cpu()[0], ref["var"])
    return routes


CHAIN, MID, GEMM = 1, 2, 3


@pytest.mark.parametrize("why,M,Dx,R,li,T,Tr,fused,route", [
    ("chain, D = 16", 128, 16, 5, 0, 2048, 2048, 0, (CHAIN, 16, 16)),
    ("chain, D = 17", 128, 17, 5, 0, 2048, 2048, 0, (CHAIN, 32, 16)),
    ("chain, D = 32", 128, 32, 5, 0, 2048, 2048, 0, (CHAIN, 32, 16)),
    ("chain, R = 17: second q_mu block", 128, 8, 17, 0, 2048, 2048, 0, (CHAIN, 8, 16)),
    ("chain, final layer Dy = 17", 128, 12, 17, 1, 2048, 2048, 0, (CHAIN, 16, 16)),
    ("GEMM, D = R = P = 32: the chain does not fit", 128, 32, 32, 0, 16400, 512, 0, (GEMM, 32, 16)),
    ("fused k_bw_mid<1, 32>, M = 64, D = 24", 64, 24, 32, 0, 20480, 512, 1, (MID, 32, 64)),
    ("fused k_bw_mid<4, 32>, M = 256, D = 20", 256, 20, 20, 0, 8192, 512, 1, (MID, 32, 64)),
    ("GEMM at M = 256, D = 20 without the fused kernel", 256, 20, 20, 0, 8192, 512, 0, (GEMM, 32, 16)),
    ("32-sample chain at M = 256, D = 20", 256, 20, 2, 0, 16384, 512, 0, (CHAIN, 32, 32)),
    ("64-sample chain at M = 176 (odd block count: two tiles), D = 20", 176, 20, 2, 0, 16384, 512, 0, (CHAIN, 32, 64)),
])
def test_wide_layer_adjoints_match_autodiff(gpu_device, why, M, Dx, R, li, T, Tr, fused, route):
    from dgps_with_iwvi_amd import _abi, synthetic
    Dy = R if li == 1 else 1
    spec = synthetic.make_spec(L=2, M=M, B=8, K=2, Dx=Dx, R=R if li == 0 else 5, Dy=Dy, mixing="dense", seed=M + Dx + R)
    _abi.set_debug_option("IWVI_BW_FUSED", fused)
    try:
        routes = _layer_case(gpu_device, spec, li, T, Tr, seed=T + Dx)
    finally:
        _abi.set_debug_option("IWVI_BW_FUSED", 0)
    assert routes == [route], (why, routes)


def _model_grads_vs_oracle(dev, spec, zs, mode_vi=False, S=None):
    from dgps_with_iwvi_amd import _abi, backward, synthetic
    from dgps_with_iwvi_amd.models import DGP_VI
    from oracle.grad_oracle import iw_elbo_and_gradients
    val, ref = iw_elbo_and_gradients(spec, zs, mode_vi=mode_vi)
    if mode_vi:
        model = synthetic.build_model(spec, dev, cls=DGP_VI, num_samples=S)
        zd = [_t(np.asarray(z).transpose(1, 0, 2).reshape(S * spec["B"], -1), dev) for z in zs]
    else:
        model = synthetic.build_model(spec, dev)
        zd = [_t(z, dev) for z in zs]
    _abi.backward_routes()
    elbo, grads = backward.iw_elbo_and_gradients(model, zd)
    torch.cuda.synchronize()
    routes = _abi.backward_routes()
    assert abs(float(elbo) - val) <= 2e-4 * abs(val), (float(elbo), val)
    assert sorted(grads) == sorted(ref)
    for k, v in grads.items():
        _close(k, v.detach().cpu().numpy().reshape(ref[k].shape), ref[k])
    return routes


@pytest.mark.parametrize("why,kw,routes", [
    ("LV latent_dim = 3, Dx = 29 (D = 32)", dict(L=2, M=64, B=16, K=4, Dx=29, R=7, Dy=1, with_lv=True, latent_dim=3),
     [(CHAIN, 32, 16), (CHAIN, 32, 16)]),
    ("final layer Dy = 17", dict(L=2, M=64, B=16, K=4, Dx=10, R=17, Dy=17, distinct_y=True), [(CHAIN, 16, 16), (CHAIN, 16, 16)]),
])
def test_wide_model_gradients_match_oracle(gpu_device, why, kw, routes):
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(mixing="dense", seed=kw["Dx"], **kw)
    zs = synthetic.make_noise(spec, seed=2)
    assert _model_grads_vs_oracle(gpu_device, spec, zs) == routes, why


def test_wide_vi_bound_gradients_match_oracle(gpu_device):
    from dgps_with_iwvi_amd import synthetic
    S, B = 3, 16
    spec = synthetic.make_spec(L=2, M=48, B=B, K=S, Dx=24, R=20, Dy=2, with_lv=True, latent_dim=2, mixing="dense", distinct_y=True, seed=43)
    zs = synthetic.make_noise(spec, seed=44)
    routes = _model_grads_vs_oracle(gpu_device, spec, zs, mode_vi=True, S=S)
    assert routes == [(CHAIN, 32, 16), (CHAIN, 32, 16)], routes


# ------------------------------------------------------------------------------------------------------------------------------------
# e. training at width: one Trainer step on a Dy = 17 model against the oracle loop
# ------------------------------------------------------------------------------------------------------------------------------------
def test_training_step_with_a_wide_final_layer_follows_the_oracle_loop(gpu_device):
    import copy
    from dgps_with_iwvi_amd import _abi, synthetic
    from dgps_with_iwvi_amd.training import Trainer
    from test_gpu_training import _OracleTrainer
    spec = synthetic.make_spec(L=2, M=32, B=12, K=3, Dx=6, R=5, Dy=17, mixing="dense", distinct_y=True, seed=17)
    model = synthetic.build_model(spec, gpu_device)
    ospec = copy.deepcopy(spec)
    tr = Trainer(model, lr=5e-3, gamma=1e-2, fix_linear=True)
    ot = _OracleTrainer(ospec, 5e-3, 1e-2, True)
    assert sorted(n for n, _, _ in tr._entries) == sorted(ot.names)
    zs_a, zs_b = synthetic.make_noise(spec, seed=100), synthetic.make_noise(spec, seed=101)
    e_gpu = float(tr.step([_t(z, gpu_device) for z in zs_a], [_t(z, gpu_device) for z in zs_b]))
    e_ref = ot.step(zs_a, zs_b)
    assert abs(e_gpu - e_ref) <= 3e-4 * abs(e_ref), (e_gpu, e_ref)
    assert _abi.lib().iwvi_debug_last_natgrad_route() == 1        # R = Dy = 17 > 8: one workgroup per latent GP
    f, fo = model.layers[-1], ospec["layers"][-1]
    np.testing.assert_allclose(f.q_mu.cpu().numpy(), fo["q_mu"], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(f.q_sqrt.cpu().numpy(), fo["q_sqrt"], rtol=2e-3, atol=2e-4)
    sig = dict(zip(ot.names, ot.signif))
    for name, p, _ in tr._entries:
        ref = np.asarray(ot.get(name), dtype=np.float64).reshape(-1)
        got = p.detach().cpu().numpy().astype(np.float64).reshape(-1)
        m = np.asarray(sig[name]).reshape(-1)
        np.testing.assert_allclose(got[m], ref[m], rtol=2e-4, atol=2e-4, err_msg=name)


# ------------------------------------------------------------------------------------------------------------------------------------
# f. one past each cap: refused before any launch, and no error state sticks
# ------------------------------------------------------------------------------------------------------------------------------------
def _refusal_case(which):
    from dgps_with_iwvi_amd import synthetic
    base = dict(L=2, M=32, B=8, K=2, Dx=6, R=3, Dy=1, mixing="dense", seed=1, n_data=64)
    if which == "D = 33":
        return synthetic.make_spec(**dict(base, Dx=33))
    if which == "Dx + Lw = 33":
        return synthetic.make_spec(**dict(base, Dx=31, with_lv=True, latent_dim=2))
    if which == "R = 33":
        return synthetic.make_spec(**dict(base, R=33))
    if which == "Dy = 33":
        return synthetic.make_spec(**dict(base, Dy=33))
    if which == "M = 513":
        return synthetic.make_spec(**dict(base, M=513, n_data=513))
    if which == "9 layers":
        return synthetic.make_spec(**dict(base, L=9))
    if which == "encoder width 65":
        spec = synthetic.make_spec(**dict(base, with_lv=True))
        lv = spec["layers"][0]
        rng = np.random.default_rng(0)
        lv["dims"] = [lv["dims"][0], 65, lv["dims"][2], lv["dims"][3]]
        lv["enc_W"] = [rng.standard_normal((a, b)) * 0.1 for a, b in zip(lv["dims"][:-1], lv["dims"][1:])]
        lv["enc_b"] = [np.zeros(b) for b in lv["dims"][1:]]
        return spec
    raise AssertionError(which)


_CAPS = {"D = 33": "33", "Dx + Lw = 33": "33", "R = 33": "33", "Dy = 33": "33", "M = 513": "513", "9 layers": "8", "encoder width 65": "65"}


def test_one_past_each_cap_is_refused_and_nothing_sticks(gpu_device):
    from dgps_with_iwvi_amd import _abi, synthetic
    for which, size in _CAPS.items():
        spec = _refusal_case(which)
        zs = synthetic.make_noise(spec, seed=1)
        with pytest.raises((ValueError, _abi.IwviError)) as ei:
            model = synthetic.build_model(spec, gpu_device)
            model.compute_log_likelihood([_t(z, gpu_device) for z in zs])
            torch.cuda.synchronize()
        e = ei.value
        assert not isinstance(e, _abi.IwviError) or e.rc == _abi.ERR_ARG, (which, e.rc, str(e))
        assert size in str(e), (which, str(e))
    torch.cuda.synchronize()
    spec = synthetic.make_spec(L=2, M=32, B=8, K=3, Dx=6, R=3, with_lv=True, mixing="dense", seed=2)
    _forward_vs_oracle(gpu_device, spec, seed=3)
