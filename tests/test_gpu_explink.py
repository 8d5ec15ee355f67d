"""Poisson, Exponential and Gamma likelihoods (exp link) on the GPU against the float64 restatement (tests/explink_restatement.py, pinned
by tests/test_explink_host.py), with injected noise.

Elementwise callables and heads: |got - ref| <= 8 x 2^-24 x S with the scale S computed in float64 from the magnitudes of the terms
(explink_restatement.var_exp_scale and its neighbours).  The constant is derived, not fitted: a plain float32 NumPy evaluation of the
formulas over these cases stays within 2.6 x 2^-24 S, and 8 leaves a factor 3 for the device's expf / logf / lgammaf.  Through the stack
the tolerances are tests/test_gpu_likelihoods.py's own for the same comparisons (the layers are the same kernels)."""
import copy
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import explink_restatement as X   # noqa: E402

pytestmark = pytest.mark.gpu

U = X.U
C8 = 8.0
ELBO_RTOL = 1e-4
STACK = {"poisson": dict(binsize=1.5), "exponential": {}, "gamma": dict(shape=2.5)}       # the parameters of the tests through the stack
ELEMENTWISE_CASES = [("poisson", dict(binsize=1.0), (0.0, 1.0, 3.0, 40.0)), ("poisson", dict(binsize=2.5), (0.0, 7.0)),
                     ("exponential", {}, (0.0, 0.05, 1.3, 9.0)),
                     ("gamma", dict(shape=2.5), (0.05, 1.3, 9.0)), ("gamma", dict(shape=50.0), (0.5, 30.0)), ("gamma", dict(shape=0.6), (0.5, 3.0))]
_IDS = ["%s-%s" % (k, "-".join("%g" % v for v in kw.values()) or "none") for k, kw, _ in ELEMENTWISE_CASES]


def _t(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)


def _n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _liks(kind, **kw):
    from dgps_with_iwvi_amd import likelihoods
    cls = {"poisson": likelihoods.Poisson, "exponential": likelihoods.Exponential, "gamma": likelihoods.Gamma}[kind]
    return cls(**kw), X.make(kind, **kw)


def _spec(kind, L=2, M=32, B=12, K=4, lv=True, Dy=1, seed=3, **kw):
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=L, M=M, B=B, K=K, with_lv=lv, Dy=Dy, seed=seed, distinct_y=Dy > 1, **kw)
    spec["Y"] = X.targets(spec, kind)
    return spec


def _multiple(got, ref, scale):
    """max |got - ref| / (2^-24 S)"""
    got, ref, scale = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref, scale))
    assert got.shape == ref.shape == scale.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / (U * scale)).max())


def _close(name, got, ref, rtol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-12)
    err = np.abs(got - ref).max()
    print("  %-12s max err %.3e of scale %.3e (%.2e relative)" % (name, err, scale, err / scale))
    assert err <= rtol * scale, "%s: max err %.3e vs scale %.3e" % (name, err, scale)


def _grid32():
    MU, V = X.moment_grid()
    return MU.astype(np.float32), V.astype(np.float32)


# ---- 1: the elementwise callables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw,ys", ELEMENTWISE_CASES, ids=_IDS)
def test_elementwise_callables_match_the_restatement(gpu_device, kind, kw, ys):
    lik, ref = _liks(kind, **kw)
    mu32, v32 = _grid32()
    m64, v64 = mu32.astype(np.float64), v32.astype(np.float64)
    m, v = _t(mu32.reshape(-1, 1), gpu_device), _t(v32.reshape(-1, 1), gpu_device)
    worst = {}
    pm, pv = lik.predict_mean_and_var(m, v)
    rm, rv = ref.predict_mean_and_var(m64, v64)
    sm, sv = X.mean_var_scales(ref, m64, v64)
    worst["predict_mean"] = _multiple(_n64(pm), rm.numpy(), sm.numpy())
    worst["predict_var"] = _multiple(_n64(pv), rv.numpy(), sv.numpy())
    assert float(pm.min()) > 0.0
    for y in ys:
        Y = np.full_like(mu32, y)
        yy, y64 = _t(Y.reshape(-1, 1), gpu_device), Y.astype(np.float64)
        for what, got, want, scale in (
                ("var_exp", lik.variational_expectations(m, v, yy), ref.variational_expectations(m64, v64, y64), X.var_exp_scale(ref, m64, v64, y64)),
                ("logp", lik.logp(m, yy), ref.logp(m64, y64), X.logp_scale(ref, m64, y64)),
                ("predict_density", lik.predict_density(m, v, yy), ref.predict_density(m64, v64, y64), X.density_scale(ref, m64, v64, y64))):
            assert tuple(got.shape) == (600, 1)
            worst[what] = max(worst.get(what, 0.0), _multiple(_n64(got), want.numpy(), scale.numpy()))
    print("%s %r: worst multiples of 2^-24 S: " % (kind, kw) + "  ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    for what, w in worst.items():
        assert w <= C8, (what, w)


# ---- 2: the heads directly ----------------------------------------------------------------------------------------------------------
def _backward_call(dev, desc, fm, fv, Y, B, K, Dy, scale=1.0, mode_vi=1, kls=(), glob=None, lse_global=None, K_total=0):
    """kls: local regularisers [B K, width] each; glob: one float64 array of global KL shares; lse_global [B] with K_total: the heads of a
    K-shard against the whole job's normaliser."""
    from dgps_with_iwvi_amd import _abi
    T = B * K
    w, dm, dv = torch.empty(T, device=dev), torch.empty(T, Dy, device=dev), torch.empty(T, Dy, device=dev)
    sums = torch.empty(3, dtype=torch.float64, device=dev)
    ws = torch.empty(2 * B, dtype=torch.float64, device=dev)
    kls = list(kls)
    kd = (ctypes.c_int32 * max(len(kls), 1))(*[k.shape[-1] for k in kls])
    gl = [] if glob is None else [glob]
    gn = (ctypes.c_int32 * 1)(glob.numel() if gl else 0)
    _abi.check(_abi.lib().iwvi_lik_elbo_backward(desc, _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(Y), Dy, _abi.ptr_array(kls) if kls else None, kd, len(kls),
                                                 B, K, scale, mode_vi, _abi.ptr(w), _abi.ptr(dm), _abi.ptr(dv), _abi.ptr_array(gl) if gl else None, gn,
                                                 len(gl), _abi.ptr(lse_global), K_total or K,
                                                 ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(ws.data_ptr()), _abi.stream_ptr()))
    return w, dm, dv, sums


@pytest.mark.parametrize("kind,kw,ys", ELEMENTWISE_CASES, ids=_IDS)
def test_heads_are_the_derivatives_of_the_closed_form(gpu_device, kind, kw, ys):
    """iwvi_lik_elbo_backward with K = 1, the plain bound, scale = 1 and no regularisers: d_mean and d_var ARE dE/dmu and dE/dv;
    out_sums[1] = sum_b (-mu_b - psi(a) + log Y_b) for the Gamma -- the check of the device digamma -- and 0 for the other two."""
    from scipy import special
    lik, ref = _liks(kind, **kw)
    mu32, v32 = _grid32()
    B = mu32.size
    Y32 = np.asarray([ys[b % len(ys)] for b in range(B)], dtype=np.float32)
    m64, v64, y64 = (a.astype(np.float64) for a in (mu32, v32, Y32))
    fm, fv, Yd = (_t(a.reshape(-1, 1), gpu_device) for a in (mu32, v32, Y32))
    w, dm, dv, sums = _backward_call(gpu_device, lik.lik_desc(), fm, fv, Yd, B, 1, 1)
    rdm, rdv, scale = X.heads(ref, m64, v64, y64)
    mult = {"d_mean": _multiple(_n64(dm), rdm.numpy(), scale.numpy()), "d_var": _multiple(_n64(dv), rdv.numpy(), scale.numpy())}
    assert torch.equal(w, torch.ones_like(w))
    sums = sums.cpu().numpy()
    ve = ref.variational_expectations(m64, v64, y64).numpy()
    mult["sum of E"] = abs(sums[0] - ve.sum()) / (U * X.var_exp_scale(ref, m64, v64, y64).numpy().sum())
    assert sums[2] == sums[0]                                    # scale = 1, no global KL
    if kind == "gamma":
        psi = float(special.digamma(kw["shape"]))
        want = float((-m64 - psi + np.log(y64)).sum())
        mult["d_shape"] = abs(sums[1] - want) / (U * float((1.0 + np.abs(m64) + abs(psi) + np.abs(np.log(y64))).sum()))
    else:
        assert sums[1] == 0.0
    print("%s %r heads: worst multiples of 2^-24 S: " % (kind, kw) + "  ".join("%s %.2f" % kv for kv in sorted(mult.items())))
    for what, x in mult.items():
        assert x <= C8, (what, x)


@pytest.mark.parametrize("K", [3, 70])
def test_gamma_heads_of_a_k_shard_against_the_jobs_normaliser(gpu_device, K):
    """iwvi_lik_elbo_backward with lse_global (the K-sharded weights scale exp(L - lse_global), the constant c0 taken off the job's normaliser
    and added back to out_sums[0]) at K = 3 and K = 70 -- past the one-sample-per-lane shortcut --, B = 5, Dy = 2, one regulariser of width 2,
    scale 2.75, against X.R.sharded_heads in float64.  L carries 8 x 2^-24 x S (S: the expectation's scales of the sample's outputs and its
    regulariser entries, the worst sample of the point) plus half a spacing of the float32 normaliser; the weights follow
    iw_reduction_reference.tol_w from that; a head adds 8 x 2^-24 x its own scale (X.heads) per unit weight; d shape likewise."""
    from scipy import special
    import iw_reduction_reference as IR
    lik, ref = _liks("gamma", **STACK["gamma"])
    B, Dy, scale = 5, 2, 2.75
    rng = np.random.default_rng(23 + K)
    mu32 = rng.uniform(-1.5, 1.5, (B, K, Dy)).astype(np.float32)
    v32 = rng.uniform(0.05, 0.5, (B, K, Dy)).astype(np.float32)
    kl32 = rng.uniform(0.0, 1.0, (B, K, 2)).astype(np.float32)
    Y32 = rng.uniform(0.3, 4.0, (B, Dy)).astype(np.float32)
    glob = np.array([1.25, 0.5])
    m64, v64, kl64 = (a.astype(np.float64) for a in (mu32, v32, kl32))
    y64 = np.broadcast_to(Y32.astype(np.float64)[:, None, :], (B, K, Dy)).copy()
    L, lse, wr, dmr, dvr, _, _ = X.R.sharded_heads(lambda m, v: ref.variational_expectations(m, v, y64).sum(-1), m64, v64, kl64, scale)
    Kt = 2 * K
    fm, fv, kl = (_t(a, gpu_device).reshape(B * K, -1) for a in (mu32, v32, kl32))
    w, dm, dv, sums = _backward_call(gpu_device, lik.lik_desc(), fm, fv, _t(Y32, gpu_device), B, K, Dy, scale=scale, mode_vi=0, kls=[kl],
                                     glob=torch.as_tensor(glob, dtype=torch.float64, device=gpu_device), lse_global=_t(lse, gpu_device), K_total=Kt)
    w, dm, dv, sums = _n64(w).reshape(B, K), _n64(dm).reshape(B, K, Dy), _n64(dv).reshape(B, K, Dy), sums.cpu().numpy()
    S_L = (X.var_exp_scale(ref, m64, v64, y64).sum(-1).numpy() + kl64.sum(-1)).max(1) + np.abs(L).max(1)
    tol_L = C8 * U * S_L + 0.5 * IR.spacing32(lse)
    tw = IR.tol_w(wr, scale, tol_L)
    print("gamma K=%d lse_global: w max err / allowed %.3f" % (K, float((np.abs(w - wr) / tw).max())))
    assert np.isfinite(w).all() and np.all(np.abs(w - wr) <= tw), float((np.abs(w - wr) / tw).max())
    _, _, S_h = X.heads(ref, m64, v64, y64)
    for nm, got, want in (("d_mean", dm, dmr), ("d_var", dv, dvr)):
        tol = np.abs(want) * (tw / wr)[..., None] + wr[..., None] * C8 * U * S_h.numpy()
        print("gamma K=%d lse_global: %s max err / allowed %.3f" % (K, nm, float((np.abs(got - want) / tol).max())))
        assert np.all(np.abs(got - want) <= tol), (nm, float((np.abs(got - want) / tol).max()))
    want0 = float((lse - math.log(Kt)).sum())
    assert abs(sums[0] - want0) <= float(tol_L.sum()), (sums[0], want0)
    assert abs(sums[2] - (scale * sums[0] - glob.sum())) <= 4 * 2.0 ** -52 * (abs(scale * sums[0]) + glob.sum()), sums
    psi = float(special.digamma(STACK["gamma"]["shape"]))
    term = -m64 - psi + np.log(y64)
    want1 = float((wr[..., None] * term).sum())
    tol1 = float(((tw[..., None] + wr[..., None] * C8 * U) * (1.0 + np.abs(m64) + abs(psi) + np.abs(np.log(y64)))).sum())
    print("gamma K=%d lse_global: d_shape err %.3e allowed %.3e" % (K, abs(sums[1] - want1), tol1))
    assert abs(sums[1] - want1) <= tol1, (sums[1], want1, tol1)


@pytest.mark.parametrize("kind", sorted(STACK))
@pytest.mark.parametrize("mode_vi", [0, 1], ids=["iw", "vi"])
def test_reduction_where_a_workgroup_takes_a_second_pass(gpu_device, kind, mode_vi):
    """iwvi_lik_elbo_reduce directly at B = 4100, K = 33: 64 lanes per point, 4 points per pass, 1025 passes for a grid capped at 1024
    workgroups -- the one shape class at which a workgroup of k_xl_elbo walks on to a second pass (and K > 32 the widest segment).
    Per point: |got - ref| <= 8 x 2^-24 x (max_k (S_bk + |kl_bk|) + |ref|), S the variational expectation's scale; the bound: the sum of those."""
    from dgps_with_iwvi_amd import _abi
    lik, ref = _liks(kind, **STACK[kind])
    B, K, scale = 4100, 33, 3.5
    rng = np.random.default_rng(17)
    mu32 = rng.uniform(-3.0, 3.0, (B, K, 1)).astype(np.float32)
    v32 = np.exp(rng.uniform(np.log(1e-4), np.log(4.0), (B, K, 1))).astype(np.float32)
    kl32 = rng.uniform(0.0, 2.0, (B, K, 2)).astype(np.float32)
    Y32 = (np.floor(rng.uniform(0.0, 9.0, (B, 1))) if kind == "poisson" else rng.uniform(0.05, 9.0, (B, 1))).astype(np.float32)
    glob = np.array([1.25, 0.5])
    m64, v64, kl64 = (a.astype(np.float64) for a in (mu32, v32, kl32))
    y64 = np.broadcast_to(Y32.astype(np.float64)[:, None, :], (B, K, 1)).copy()
    L = ref.variational_expectations(m64, v64, y64).sum(-1) - torch.as_tensor(kl64.sum(-1))
    want = (L.mean(1) if mode_vi else torch.logsumexp(L, 1) - math.log(K)).numpy()
    S = (X.var_exp_scale(ref, m64, v64, y64).sum(-1).numpy() + kl64.sum(-1)).max(1) + np.abs(want)
    fm, fv, kl = (_t(a, gpu_device).reshape(B * K, -1) for a in (mu32, v32, kl32))
    Yd = _t(Y32, gpu_device)
    gl = torch.as_tensor(glob, dtype=torch.float64, device=gpu_device)
    ms = torch.full((B, 2), float("nan"), device=gpu_device)
    logp = torch.full((B,), float("nan"), device=gpu_device)
    elbo = torch.full((1,), float("nan"), dtype=torch.float64, device=gpu_device)
    ticket = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    kl_dims, gl_n = (ctypes.c_int32 * 1)(2), (ctypes.c_int32 * 1)(2)
    for _ in range(2):                                           # the second call finds the ticket re-armed
        _abi.check(_abi.lib().iwvi_lik_elbo_reduce(lik.lik_desc(), _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(Yd), B, K, 1, K, 1, _abi.ptr_array([kl]), kl_dims, 1,
                                                   _abi.ptr_array([gl]), gl_n, 1, scale, K, mode_vi, None if mode_vi else _abi.ptr(ms), _abi.ptr(logp),
                                                   ctypes.c_void_p(elbo.data_ptr()), ctypes.c_void_p(ticket.data_ptr()), _abi.stream_ptr()))
        assert int(ticket) == 0
    got = _n64(logp)
    mult = _multiple(got, want, S)
    e_got, e_want = float(elbo), scale * want.sum() - glob.sum()
    e_mult = abs(e_got - e_want) / (U * scale * S.sum())
    print("%s mode_vi=%d B=%d K=%d: per-point %.2f, bound %.2f multiples of 2^-24 S" % (kind, mode_vi, B, K, mult, e_mult))
    assert mult <= C8 and e_mult <= C8, (mult, e_mult)
    assert abs(e_got - (scale * got.sum() - glob.sum())) <= 1e-12 * abs(e_got)      # the float64 sum of the stored per-point values
    if not mode_vi:
        np.testing.assert_allclose(_n64(ms[:, 0]) + np.log(_n64(ms[:, 1])) - math.log(K), got, rtol=1e-5, atol=1e-5)


# ---- 3: row tiling and the device scalar --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(STACK))
def test_row_tiling_of_the_elementwise_entries(gpu_device, kind):
    """row_div / row_mod: 24 rows, 4 per target row, read Y[t // 4] -- bit-equal to the call on the expanded targets."""
    from dgps_with_iwvi_amd import _abi
    lik, _ = _liks(kind, **STACK[kind])
    Fm, Fv = _t(np.linspace(-2, 2, 48).reshape(24, 2), gpu_device), _t(np.linspace(0.01, 1.5, 48).reshape(24, 2), gpu_device)
    Y6 = _t(np.array([[0.0, 3.0], [1.0, 7.0], [2.0, 1.0], [5.0, 0.0], [1.0, 1.0], [4.0, 2.0]]) + (0.25 if kind == "gamma" else 0.0), gpu_device)
    big = Y6.repeat_interleave(4, 0)
    for entry, fv, want in (("iwvi_lik_var_exp", Fv, lik.variational_expectations(Fm, Fv, big)),
                            ("iwvi_lik_predict_density", Fv, lik.predict_density(Fm, Fv, big)),
                            ("iwvi_lik_predict_density", None, lik.logp(Fm, big))):
        out = torch.full_like(Fm, float("nan"))
        _abi.check(getattr(_abi.lib(), entry)(lik.lik_desc(), _abi.ptr(Fm), _abi.ptr(fv), _abi.ptr(Y6), 24, 2, 4, 6, _abi.ptr(out), _abi.stream_ptr()))
        assert torch.equal(out, want), entry
    assert not torch.equal(lik.logp(Fm, big), lik.logp(Fm, big.flip(0)))      # (the targets do matter)


def test_device_scalar_is_honoured_for_the_gamma_and_ignored_for_the_poisson(gpu_device):
    from dgps_with_iwvi_amd import _abi, likelihoods
    mu32, v32 = _grid32()
    m, v = _t(mu32.reshape(-1, 1), gpu_device), _t(v32.reshape(-1, 1), gpu_device)
    yy = torch.full_like(m, 1.3)
    dev_shape = torch.full((1,), 4.0, device=gpu_device)
    bound, plain, stale = likelihoods.Gamma(shape=2.5), likelihoods.Gamma(shape=4.0), likelihoods.Gamma(shape=2.5)
    bound.bind_device_variance(dev_shape)
    d = bound.lik_desc()
    assert d.param[0] == 2.5 and d.param0_dev == dev_shape.data_ptr()
    for f in (lambda l: l.variational_expectations(m, v, yy), lambda l: l.predict_density(m, v, yy), lambda l: l.logp(m, yy),
              lambda l: l.predict_mean_and_var(m, v)[0], lambda l: l.predict_mean_and_var(m, v)[1]):
        assert torch.equal(f(bound), f(plain)) and not torch.equal(f(bound), f(stale))
    Yd = torch.full_like(m, 1.3)
    a = _backward_call(gpu_device, d, m, v, Yd, 600, 1, 1)
    b = _backward_call(gpu_device, plain.lik_desc(), m, v, Yd, 600, 1, 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the Poisson's binsize is a host parameter: a device pointer in its descriptor is not read
    p = likelihoods.Poisson(binsize=2.5)
    dp = p.lik_desc()
    dp.param0_dev = dev_shape.data_ptr()
    out = torch.empty_like(m)
    cnt = torch.full_like(m, 3.0)
    _abi.check(_abi.lib().iwvi_lik_var_exp(dp, _abi.ptr(m), _abi.ptr(v), _abi.ptr(cnt), 600, 1, 1, 600, _abi.ptr(out), _abi.stream_ptr()))
    assert torch.equal(out, p.variational_expectations(m, v, cnt))


# ---- 4: bound, per-point log p and gradients through the stack ----------------------------------------------------------------------
def _vi_noise(zs, B, K):
    """[B, K, dim] (the restatement's layout) -> [S*N, dim], S-major (models.py:50)."""
    return [np.ascontiguousarray(np.asarray(z).transpose(1, 0, 2).reshape(K * B, -1)) for z in zs]


@pytest.mark.parametrize("kind", sorted(STACK))
@pytest.mark.parametrize("iw", [True, False], ids=["iwvi", "vi"])
@pytest.mark.parametrize("lv", [True, False], ids=["lv", "nolv"])
@pytest.mark.parametrize("B,K,Dy", [(7, 1, 1), (7, 20, 3), (67, 5, 1), (12, 70, 1)])
def test_bound_logp_and_gradients_match_the_restatement(gpu_device, kind, iw, lv, B, K, Dy):
    """B = 67 crosses a workgroup's 64 points, K = 70 a wave's lanes (and the K <= 64 single-evaluation path of the heads), Dy = 3 walks the
    outputs.  'lik_shape' is a sum of cancelling terms (as the final layer's 'var' is for MultiClass): its error is taken relative to
    sum |w| (|mu| + |psi(a)| + |log Y|), not to its own value."""
    from dgps_with_iwvi_amd import synthetic, backward
    from dgps_with_iwvi_amd.models import DGP_IWVI, DGP_VI
    spec = _spec(kind, B=B, K=K, lv=lv, Dy=Dy, seed=7 + K + Dy + B)
    zs = synthetic.make_noise(spec, seed=2)
    lik, ref = _liks(kind, **STACK[kind])
    val, logp, gref = X.bound_and_gradients(spec, ref, zs, mode_vi=not iw)
    model = synthetic.build_model(spec, gpu_device, cls=DGP_IWVI if iw else DGP_VI, likelihood=lik)
    zd = [_t(z, gpu_device) for z in (zs if iw else _vi_noise(zs, B, K))]
    got = model.compute_log_likelihood(zd)
    print("%s iw=%s lv=%s B=%d K=%d Dy=%d: bound %.6f vs %.6f (%.2e relative)" % (kind, iw, lv, B, K, Dy, got, val, abs(got - val) / abs(val)))
    assert abs(got - val) <= ELBO_RTOL * abs(val), (got, val)
    if iw:
        lp = model.E_log_p_Y(zd).cpu().numpy()
        print("  per-point log p: max abs err %.3e" % np.abs(lp - logp).max())
        np.testing.assert_allclose(lp, logp, rtol=2e-4, atol=2e-2)
        ms, _ = model.lse_partials(zd)                           # the K-shard exchange unit carries the same numbers, the targets' terms included
        np.testing.assert_allclose((ms[:, 0] + torch.log(ms[:, 1])).cpu().numpy() - math.log(K), lp, rtol=1e-5, atol=1e-5)
    elbo, grads = backward.iw_elbo_and_gradients(model, zd)
    assert abs(float(elbo) - val) <= 2e-4 * abs(val), (float(elbo), val)
    assert sorted(grads) == sorted(gref), (sorted(grads), sorted(gref))
    assert ("lik_shape" in grads) == (kind == "gamma")
    for k, v in grads.items():
        if k == "lik_shape":
            scale = X.shape_gradient_scale(spec, ref, zs, mode_vi=not iw)
            err = abs(float(v) - float(gref[k]))
            print("  %-12s %.6e vs %.6e: err %.3e of the terms' %.3e (%.2e relative)" % (k, float(v), float(gref[k]), err, scale, err / scale))
            assert err <= 5e-3 * scale, (float(v), float(gref[k]), scale)
            continue
        _close(k, v.detach().cpu().numpy().reshape(gref[k].shape), gref[k], rtol=5e-3)


# ---- 5: finite differences ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(STACK))
def test_gradient_agrees_with_central_differences_of_the_forward(gpu_device, kind):
    """One finite-difference spot check per likelihood (the pattern of tests/test_gpu_likelihoods.py): directional derivatives of the HIP
    adjoint against central differences of the HIP bound on the same injected noise; for the Gamma also d / d shape."""
    from dgps_with_iwvi_amd import synthetic, backward
    spec = _spec(kind, L=2, M=64, B=64, K=8, lv=True, seed=13)
    lik, _ = _liks(kind, **STACK[kind])
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    zs = [_t(z, gpu_device) for z in synthetic.make_noise(spec, seed=1)]
    elbo0, grads = backward.iw_elbo_and_gradients(model, zs)
    f0 = model.compute_log_likelihood(zs)
    assert abs(float(elbo0) - f0) <= 1e-5 * abs(f0)
    gen = torch.Generator(device="cpu").manual_seed(5)
    params = dict(backward.parameter_list(model))
    noise = 2e-6 * abs(f0)
    for pname in ("l2.q_mu", "l1.Z", "l0.encW0", "l2.ls"):
        p, g = params[pname], grads[pname].reshape(params[pname].shape).double()
        d = torch.randn(p.shape, generator=gen).to(gpu_device)
        d = d / d.norm()
        gd = float((g * d.double()).sum())
        eps = min(0.02, 100.0 * noise / max(abs(gd), 1e-30))
        with torch.no_grad():
            p.add_(eps * d); fp = model.compute_log_likelihood(zs)
            p.add_(-2 * eps * d); fm = model.compute_log_likelihood(zs)
            p.add_(eps * d)
        fd = (fp - fm) / (2 * eps)
        print("%s %s: fd %.6e adjoint %.6e eps %.3g" % (kind, pname, fd, gd, eps))
        assert abs(fd - gd) <= 0.02 * abs(gd) + noise / eps, (pname, fd, gd, eps)
    if kind == "gamma":
        gd, s0 = float(grads["lik_shape"]), lik.shape
        eps = min(0.02, 100.0 * noise / max(abs(gd), 1e-30))
        lik.shape = s0 + eps; fp = model.compute_log_likelihood(zs)
        lik.shape = s0 - eps; fm = model.compute_log_likelihood(zs)
        lik.shape = s0
        fd = (fp - fm) / (2 * eps)
        print("gamma lik_shape: fd %.6e adjoint %.6e eps %.3g" % (fd, gd, eps))
        assert abs(fd - gd) <= 0.02 * abs(gd) + noise / eps, (fd, gd, eps)
    else:
        assert not [k for k in grads if k.startswith("lik")]


# ---- 6: the headline shape ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(STACK))
def test_full_headline_shape_matches_the_restatement(gpu_device, kind):
    """BASELINE configs[2] (L=2, M=128, K=20, B=1024, latent-variable layer): bound and per-point log p at the tolerance the Gaussian test
    of that shape uses; one evaluation is one layer launch and one iwvi_lik_elbo_reduce."""
    from dgps_with_iwvi_amd import synthetic
    from test_gpu_likelihoods import _Calls, _TAILS
    spec = _spec(kind, L=2, M=128, B=1024, K=20, lv=True, seed=0, n_data=65536)
    zs = synthetic.make_noise(spec, seed=1)
    lik, ref = _liks(kind, **STACK[kind])
    m = X.LikDGP(spec, ref)
    with torch.no_grad():
        val, logp = float(m.elbo_tensor(zs)), m.per_point(zs).numpy()
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    zd = [_t(z, gpu_device) for z in zs]
    with _Calls(*_TAILS) as n:
        got = model.compute_log_likelihood(zd)
    print("%s full shape: entry points of one evaluation: %r" % (kind, n))
    assert n == dict(iwvi_dgp_forward=1, iwvi_iw_elbo_reduce_dev=0, iwvi_iw_elbo_backward_dev=0, iwvi_lik_elbo_reduce=1, iwvi_lik_elbo_backward=0), n
    lp = model.E_log_p_Y(zd).cpu().numpy()
    print("%s full shape: bound %.4f vs %.4f (%.2e relative); log p max abs err %.3e" % (kind, got, val, abs(got - val) / abs(val), np.abs(lp - logp).max()))
    assert abs(got - val) <= ELBO_RTOL * abs(val), (got, val)
    np.testing.assert_allclose(lp, logp, rtol=2e-4, atol=2e-2)


# ---- 7: prediction ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(STACK))
def test_predictions_match_the_restatement(gpu_device, kind):
    """predict_y, predict_density and predict_log_density(X, Y, S=8) on 20 points against the restatement fed the device's own
    predict_f / predict_f_multisample moments, at the elementwise bounds."""
    from dgps_with_iwvi_amd import synthetic
    N, S, Dy = 20, 8, 2
    spec = _spec(kind, B=N, K=3, lv=True, Dy=Dy, seed=9)
    lik, ref = _liks(kind, **STACK[kind])
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    rng = np.random.default_rng(3)
    Xn, Y = spec["X"][:N], spec["Y"][:N]
    dims = [l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1] for l in spec["layers"]]
    z1 = [_t(rng.standard_normal((N, d)), gpu_device) for d in dims]
    m1, v1 = model.predict_f(Xn, zs=z1)
    m64, v64 = _n64(m1), _n64(v1)
    P, PV = model.predict_y(Xn, zs=z1)
    rP, rV = ref.predict_mean_and_var(m64, v64)
    sP, sV = X.mean_var_scales(ref, m64, v64)
    assert tuple(P.shape) == (N, Dy) and float(P.min()) > 0.0 and float(PV.min()) > 0.0
    pd = model.predict_density(Xn, Y, zs=z1)
    assert tuple(pd.shape) == (N, Dy)
    mult = {"predict_y mean": _multiple(_n64(P), rP.numpy(), sP.numpy()), "predict_y var": _multiple(_n64(PV), rV.numpy(), sV.numpy()),
            "predict_density": _multiple(_n64(pd), ref.predict_density(m64, v64, Y).numpy(), X.density_scale(ref, m64, v64, Y).numpy())}
    print("%s predictions: worst multiples of 2^-24 S: " % kind + "  ".join("%s %.2f" % kv for kv in sorted(mult.items())))
    for what, x in mult.items():
        assert x <= C8, (what, x)
    zs = [_t(rng.standard_normal((S, N, d)), gpu_device) for d in dims]
    got = model.predict_log_density(Xn, Y, S, zs=zs).cpu().numpy()
    m, v = model.predict_f_multisample(Xn, S, zs=zs)
    Ys = np.broadcast_to(Y, (S, N, Dy)).copy()
    lp = ref.predict_density(_n64(m), _n64(v), Ys).sum(-1)
    want = (torch.logsumexp(lp, 0) - math.log(S)).numpy()
    bound = float(C8 * U * X.density_scale(ref, _n64(m), _n64(v), Ys).max())
    assert got.shape == (N,)
    np.testing.assert_allclose(got, want, rtol=0, atol=3 * bound + 1e-5 * np.abs(want).max())


# ---- 8: training --------------------------------------------------------------------------------------------------------------------
def test_training_steps_follow_the_oracle_loop(gpu_device):
    """Three Trainer.step calls on a Gamma model against the float64 loop of tests/test_gpu_training.py with this restatement's gradients;
    the oracle's 'lik_var' entry (positive, last) holds the shape.  Tolerances: test_training_steps_follow_the_oracle_loop's."""
    from dgps_with_iwvi_amd import synthetic
    from dgps_with_iwvi_amd.training import Trainer
    from test_gpu_training import _OracleTrainer
    spec = _spec("gamma", L=2, M=32, B=12, K=4, lv=True, seed=11)
    lik, _ = _liks("gamma", shape=2.5)
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    ospec = copy.deepcopy(spec)
    ospec["lik_var"] = 2.5
    tr = Trainer(model, lr=5e-3, gamma=1e-2)
    ot = _OracleTrainer(ospec, 5e-3, 1e-2)

    def grad(sp, zs):
        val, _, g = X.bound_and_gradients(sp, X.Gamma(shape=float(sp["lik_var"])), zs)
        g["lik_var"] = g.pop("lik_shape")
        return val, g
    ot.grad = grad
    assert sorted(n for n, _, _ in tr._entries) == sorted("lik_shape" if n == "lik_var" else n for n in ot.names)
    for s in range(3):
        zs_a, zs_b = synthetic.make_noise(spec, seed=100 + 2 * s), synthetic.make_noise(spec, seed=101 + 2 * s)
        e_gpu = float(tr.step([_t(z, gpu_device) for z in zs_a], [_t(z, gpu_device) for z in zs_b]))
        e_ref = ot.step(zs_a, zs_b)
        print("step %d: bound %.6f vs %.6f" % (s, e_gpu, e_ref))
        assert abs(e_gpu - e_ref) <= 3e-4 * abs(e_ref), (s, e_gpu, e_ref)
    sig = dict(zip(ot.names, ot.signif))
    n_sig = 0
    for name, p, _ in tr._entries:
        oname = "lik_var" if name == "lik_shape" else name
        want = np.asarray(ot.get(oname), dtype=np.float64).reshape(-1)
        got = p.detach().cpu().numpy().astype(np.float64).reshape(-1)
        msk = np.asarray(sig[oname]).reshape(-1)
        n_sig += int(msk.sum())
        np.testing.assert_allclose(got[msk], want[msk], rtol=2e-4, atol=2e-4, err_msg=name)
        np.testing.assert_allclose(got, want, rtol=0, atol=2 * 3.5 * 5e-3, err_msg=name)  # each side moves at most ~3 Adam steps of lr
    assert n_sig >= 100, n_sig
    f, fo = model.layers[-1], ospec["layers"][-1]
    np.testing.assert_allclose(f.q_mu.cpu().numpy(), fo["q_mu"], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(f.q_sqrt.cpu().numpy(), fo["q_sqrt"], rtol=2e-3, atol=2e-4)
    print("shape after 3 steps: %.6f vs %.6f" % (model.likelihood.shape, ospec["lik_var"]))
    assert model.likelihood.shape != 2.5 and model.likelihood.shape == pytest.approx(ospec["lik_var"], rel=1e-3)


def _problem(kind, dev, likelihood=None):
    """An L1_G5-style stack (latent-variable layer, one inner layer of 5 latent GPs, final layer) with the reference's initial values."""
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=2, M=32, B=64, K=5, Dx=4, with_lv=True, seed=41, parity=False)
    spec["Y"] = X.targets(spec, kind)
    return spec, synthetic.build_model(spec, dev, likelihood=likelihood or _liks(kind, **STACK[kind])[0])


@pytest.mark.parametrize("kind", ["poisson", "gamma"])
def test_graph_step_equals_eager_step_and_resume_is_exact(gpu_device, kind, tmp_path):
    """Trainer(use_graph=True) replays a step with the three-launch evaluation as ONE hipGraph: parameters bit-identical to the eager
    trainer's after 6 steps; 3 steps, checkpoint, restore into a fresh model + trainer, 3 more == 6 uninterrupted, bit for bit.  The
    Gamma's shape is an Adam scalar on the device and moves: lgamma and digamma of it are evaluated by the replayed kernels."""
    from dgps_with_iwvi_amd import build_models, settings
    from dgps_with_iwvi_amd.training import Trainer

    def fresh(use_graph):
        settings.set_seed(3)
        _, model = _problem(kind, gpu_device)
        return model, Trainer(model, use_graph=use_graph, check_finite=False)

    out = []
    for use_graph in (False, True):
        model, tr = fresh(use_graph)
        vals = [float(tr.step()) for _ in range(6)]
        assert all(math.isfinite(x) for x in vals), vals
        out.append((vals, [p.clone() for _, p, _ in tr._entries], model.layers[-1].q_sqrt.clone(), model, tr))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    for pa, pb in zip(out[0][1], out[1][1]):
        assert torch.equal(pa, pb)
    assert torch.equal(out[0][2], out[1][2])
    assert len(out[1][4]._graphs) >= 1                           # the graph trainer did replay graphs
    names = [n for n, _, _ in out[0][4]._entries]
    if kind == "gamma":
        assert "lik_shape" in names and out[0][3].likelihood.shape == out[1][3].likelihood.shape != 2.5
    else:
        assert not [n for n in names if n.startswith("lik")]
    b, tb = fresh(False)
    for _ in range(3):
        tb.step()
    path = str(tmp_path / "ckpt_explink.npz")
    build_models.save_checkpoint(b, path, tb)
    assert str(np.load(path)["likelihood.type"]) == type(b.likelihood).__name__
    c, tc = fresh(False)
    tc.step()                                                    # disturb the fresh state: everything must come from the file
    build_models.load_checkpoint(c, path, tc)
    for _ in range(3):
        tc.step()
    for (n, pa, _), (_, pc, _) in zip(out[0][4]._entries, tc._entries):
        assert torch.equal(pa, pc), n
    assert torch.equal(out[0][3].layers[-1].q_sqrt, c.layers[-1].q_sqrt) and torch.equal(out[0][3].layers[-1].q_mu, c.layers[-1].q_mu)
    if kind == "gamma":
        assert out[0][3].likelihood.shape == c.likelihood.shape


def test_training_raises_the_bound_on_fixed_noise(gpu_device):
    from dgps_with_iwvi_amd import synthetic
    from dgps_with_iwvi_amd.training import Trainer
    spec = _spec("poisson", L=2, M=32, B=64, K=5, lv=True, seed=5)
    model = synthetic.build_model(spec, gpu_device, likelihood=_liks("poisson", **STACK["poisson"])[0])
    zs = [_t(z, gpu_device) for z in synthetic.make_noise(spec, seed=1)]
    before = model.compute_log_likelihood(zs)
    tr = Trainer(model, lr=5e-3, gamma=1e-2)
    for _ in range(25):
        tr.step()
    after = model.compute_log_likelihood(zs)
    print("Poisson bound on fixed noise: %.4f -> %.4f" % (before, after))
    assert after > before, (before, after)


@pytest.mark.parametrize("kind", sorted(STACK))
def test_k_sharded_training_refuses_the_new_likelihoods(gpu_device, kind):
    from dgps_with_iwvi_amd.training import Trainer
    _, model = _problem(kind, gpu_device)
    with pytest.raises(NotImplementedError, match="K-sharded"):
        Trainer(model, shard="k")
