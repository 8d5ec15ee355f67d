"""The heteroskedastic Gaussian likelihood on the GPU, direct through the C-ABI, against the float64 restatement
(tests/hetero_restatement.py, pinned by tests/test_hetero_host.py).

Tolerances are the project's own for the same arithmetic.  Closed forms (one exp per column: variational expectation, logp, predictive
variance, heads): |got - ref| <= 8 x 2^-24 x S, tests/test_gpu_explink.py's constant, S the float64 magnitude of the terms
(hetero_restatement.var_exp_scale and its neighbours).  The log-space quadrature (predict_density): 16 x 2^-24 x S,
tests/test_gpu_bounded.py's constant for its densities.  Both are three times what a plain float32 evaluation of the kernels' formulas
reaches on these inputs (tests/test_hetero_host.py asserts that on the CPU).  The reductions, weights and mixtures take the forms of
tests/test_gpu_explink.py / tests/test_gpu_bounded.py with those constants."""
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
import hetero_restatement as H   # noqa: E402
import iw_reduction_reference as IR   # noqa: E402

pytestmark = pytest.mark.gpu

U, C8, C16 = H.U, H.C_CLOSED, H.C_QUAD
REF = H.HeteroskedasticGaussian()


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)), device=dev)


def _n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _lik():
    from dgps_with_iwvi_amd import likelihoods
    return likelihoods.HeteroskedasticGaussian()


def _multiple(got, ref, scale):
    """max |got - ref| / (2^-24 S)"""
    got, ref, scale = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref, scale))
    assert got.shape == ref.shape == scale.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / (U * scale)).max())


# ---- 1: the elementwise modes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dt", [1, 2, 3])
def test_elementwise_modes_match_the_restatement(gpu_device, Dt):
    """var_exp, logp (Fvar = NULL), predict_density and predict_mean_and_var on hetero_restatement.cases: the seeded rows and every edge
    (v_f = 0, v_g = 0, a at and around the clip, residuals of 1e6); the density on the rows the 20-point rule reaches."""
    lik = _lik()
    Fmu, Fvar, Y = H.cases(Dt)
    T, n = Y.shape[0], Y.shape[0] - H.N_BEYOND_RULE
    m, v, y = (_t(a, gpu_device) for a in (Fmu, Fvar, Y))
    worst = {}
    ve = lik.variational_expectations(m, v, y)
    lp = lik.logp(m, y)
    pd = lik.predict_density(m[:n], v[:n], y[:n])
    pm, pv = lik.predict_mean_and_var(m, v)
    for t in (ve, lp, pm, pv):
        assert tuple(t.shape) == (T, Dt)
    worst["var_exp"] = _multiple(_n64(ve), REF.variational_expectations(Fmu, Fvar, Y).numpy(), H.var_exp_scale(Fmu, Fvar, Y).numpy())
    worst["logp"] = _multiple(_n64(lp), REF.logp(Fmu, Y).numpy(), H.logp_scale(Fmu, Y).numpy())
    worst["predict_var"] = _multiple(_n64(pv), REF.predict_mean_and_var(Fmu, Fvar)[1].numpy(), H.var_scale(Fmu, Fvar).numpy())
    dens = _multiple(_n64(pd), REF.predict_density(Fmu[:n], Fvar[:n], Y[:n]).numpy(), H.density_scale(REF, Fmu[:n], Fvar[:n], Y[:n]).numpy())
    assert torch.equal(pm, m[:, :Dt])                            # the predictive mean IS m_f
    print("Dt=%d: worst multiples of 2^-24 S: " % Dt + "  ".join("%s %.2f" % kv for kv in sorted(worst.items())) + "  predict_density %.2f" % dens)
    for what, w in worst.items():
        assert w <= C8, (what, w)
    assert dens <= C16, dens
    # a second call gives the same bits
    assert torch.equal(ve, lik.variational_expectations(m, v, y)) and torch.equal(pd, lik.predict_density(m[:n], v[:n], y[:n]))


def test_row_tiling_of_the_elementwise_entries(gpu_device):
    """row_div / row_mod at Dt = 2: 24 rows, 4 per target row, read Y[t // 4] -- bit-equal to the call on the expanded targets."""
    from dgps_with_iwvi_amd import _abi
    lik = _lik()
    Fm, Fv = _t(np.linspace(-2, 2, 96).reshape(24, 4), gpu_device), _t(np.linspace(0.01, 1.5, 96).reshape(24, 4), gpu_device)
    Y6 = _t(np.array([[0.0, 3.0], [1.0, -0.7], [2.0, 1.0], [-1.5, 0.0], [1.0, 1.0], [0.4, 2.0]]), gpu_device)
    big = Y6.repeat_interleave(4, 0)
    for entry, fv, want in (("iwvi_lik_var_exp", Fv, lik.variational_expectations(Fm, Fv, big)),
                            ("iwvi_lik_predict_density", Fv, lik.predict_density(Fm, Fv, big)),
                            ("iwvi_lik_predict_density", None, lik.logp(Fm, big))):
        out = torch.full((24, 2), float("nan"), device=gpu_device)
        _abi.check(getattr(_abi.lib(), entry)(lik.lik_desc(), _abi.ptr(Fm), _abi.ptr(fv), _abi.ptr(Y6), 24, 4, 4, 6, _abi.ptr(out), _abi.stream_ptr()))
        assert torch.equal(out, want), entry
    assert not torch.equal(lik.logp(Fm, big), lik.logp(Fm, big.flip(0)))      # (the targets do matter)
    # the column pairing: swapping the two g columns changes both outputs, swapping f and g halves changes everything
    swapped = Fm[:, [0, 1, 3, 2]].contiguous()
    a, b = lik.variational_expectations(Fm, Fv, big), lik.variational_expectations(swapped, Fv, big)
    assert not torch.equal(a[:, 0], b[:, 0]) and not torch.equal(a[:, 1], b[:, 1])


# ---- 2: the heads directly ---------------------------------------------------------------------------------------------------------------
def _backward_call(dev, desc, fm, fv, Y, B, K, Dy, scale=1.0, mode_vi=1, kls=(), glob=None, want_heads=True):
    from dgps_with_iwvi_amd import _abi
    T = B * K
    w = torch.full((T,), float("nan"), device=dev)
    dm, dv = (torch.full((T, Dy), float("nan"), device=dev) if want_heads else None for _ in range(2))
    sums = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.empty(2 * B, dtype=torch.float64, device=dev)
    kls = list(kls)
    kd = (ctypes.c_int32 * max(len(kls), 1))(*[k.shape[-1] for k in kls])
    gl = [] if glob is None else [glob]
    gn = (ctypes.c_int32 * 1)(glob.numel() if gl else 0)
    _abi.check(_abi.lib().iwvi_lik_elbo_backward(desc, _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(Y), Dy, _abi.ptr_array(kls) if kls else None, kd, len(kls),
                                                 B, K, scale, mode_vi, _abi.ptr(w), _abi.ptr(dm), _abi.ptr(dv), _abi.ptr_array(gl) if gl else None, gn,
                                                 len(gl), None, K, ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(ws.data_ptr()), _abi.stream_ptr()))
    return w, dm, dv, sums


@pytest.mark.parametrize("Dt", [1, 2, 3])
def test_heads_are_the_derivatives_of_the_closed_form(gpu_device, Dt):
    """iwvi_lik_elbo_backward with K = 1, the plain bound, scale = 1 and no regularisers: d_mean and d_var ARE dE/dmoments, on every row of
    hetero_restatement.cases -- at a = +-60 the derivative passes, beyond it the m_g / v_g parts through r are exactly -1/2 and 0."""
    lik = _lik()
    Fmu, Fvar, Y = H.cases(Dt)
    B = Y.shape[0]
    fm, fv, yd = (_t(a, gpu_device) for a in (Fmu, Fvar, Y))
    w, dm, dv, sums = _backward_call(gpu_device, lik.lik_desc(), fm, fv, yd, B, 1, 2 * Dt)
    (rm, rv), (sm, sv) = REF.heads(Fmu, Fvar, Y), H.heads_scales(Fmu, Fvar, Y)
    mult = {"d_mean": _multiple(_n64(dm), rm.numpy(), sm.numpy()), "d_var": _multiple(_n64(dv), rv.numpy(), sv.numpy())}
    assert torch.equal(w, torch.ones_like(w))
    a = -Fmu[:, Dt:] + 0.5 * Fvar[:, Dt:]
    beyond = np.abs(a) > H.CLIP
    assert beyond.any() and (np.abs(a) == H.CLIP).any()
    assert np.all(_n64(dm)[:, Dt:][beyond] == -0.5) and np.all(_n64(dv)[:, Dt:][beyond] == 0.0)
    sums = sums.cpu().numpy()
    ve = REF.variational_expectations(Fmu, Fvar, Y).numpy()
    mult["sum of E"] = abs(sums[0] - ve.sum()) / (U * H.var_exp_scale(Fmu, Fvar, Y).numpy().sum())
    assert sums[1] == 0.0 and sums[2] == sums[0]                 # nothing is trained; scale = 1, no global KL
    print("Dt=%d heads: worst multiples of 2^-24 S: " % Dt + "  ".join("%s %.2f" % kv for kv in sorted(mult.items())))
    for what, x in mult.items():
        assert x <= C8, (what, x)


# ---- 3: the reduction and the weighted heads ---------------------------------------------------------------------------------------------
def _reduction_case(B, K, Dt, n_kl, seed):
    """Moments [B, K, 2 Dt], regularisers [B, K, width] (widths 2 and 1), Y [B, Dt]: seeded, moderate (m in [-1.5, 1.5], v in [0.05, 0.5]);
    with B >= 3 three edge samples: (0, 0) has v_f = v_g = 0, (1, 0) a residual of 1e6, (2, 0) a = -60.01 (beyond the clip) and
    (2, K - 1) a = -60 exactly (its end)."""
    rng = np.random.default_rng([seed, B, K, Dt])
    mu = rng.uniform(-1.5, 1.5, (B, K, 2 * Dt))
    var = rng.uniform(0.05, 0.5, (B, K, 2 * Dt))
    Y = rng.uniform(-2.0, 2.0, (B, Dt))
    kls = [rng.uniform(0.0, 1.0, (B, K, wd)) for wd in (2, 1)[:n_kl]]
    if B >= 3:
        var[0, 0] = 0.0
        mu[1, 0, :Dt], mu[1, 0, Dt:], var[1, 0, Dt:] = Y[1] - 10.0, -9.2, 1e-4
        mu[2, 0, Dt:], var[2, 0, Dt:] = 60.01, 0.0
        mu[2, K - 1, Dt:], var[2, K - 1, Dt:] = 60.0, 0.0
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    return f32(mu), f32(var), f32(Y), [f32(k) for k in kls]


def _reduce_call(dev, desc, fm, fv, Yd, B, K, Dy, sb, sk, kls, gl, scale, mode_vi):
    from dgps_with_iwvi_amd import _abi
    ms = torch.full((B, 2), float("nan"), device=dev)
    logp = torch.full((B,), float("nan"), device=dev)
    elbo = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int64, device=dev)
    kd = (ctypes.c_int32 * max(len(kls), 1))(*[k.shape[-1] for k in kls])
    gn = (ctypes.c_int32 * 1)(gl.numel())
    _abi.check(_abi.lib().iwvi_lik_elbo_reduce(desc, _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(Yd), B, K, Dy, sb, sk, _abi.ptr_array(kls) if kls else None, kd,
                                               len(kls), _abi.ptr_array([gl]), gn, 1, scale, K, mode_vi, None if mode_vi else _abi.ptr(ms), _abi.ptr(logp),
                                               ctypes.c_void_p(elbo.data_ptr()), ctypes.c_void_p(ticket.data_ptr()), _abi.stream_ptr()))
    assert int(ticket) == 0                                      # re-armed by the last workgroup
    return ms, logp, elbo


@pytest.mark.parametrize("mode_vi", [0, 1], ids=["iw", "vi"])
@pytest.mark.parametrize("B,K,Dt,n_kl", [(1, 1, 1, 0), (3, 5, 2, 1), (65, 20, 3, 2), (257, 64, 1, 1), (3, 65, 2, 0), (65, 130, 1, 2),
                                         (257, 5, 3, 0), (1, 130, 3, 1)])
def test_reduction_and_weighted_heads(gpu_device, B, K, Dt, n_kl, mode_vi):
    """iwvi_lik_elbo_reduce in both tilings (point-major stride_b = K, stride_k = 1; sample-major stride_b = 1, stride_k = B) and
    iwvi_lik_elbo_backward on the same case.  K: a segment narrower than a wave, a full wave, and the striding edge 64 / 65 / 130 of the
    heads' core; B: a partial pass, several workgroups.  Per point |got - ref| <= 8 x 2^-24 x (max_k (S_bk + |kl_bk|) + |ref|); the weights
    iw_reduction_reference.tol_w of that; a head adds 8 x 2^-24 of its own scale per unit weight (tests/test_gpu_explink.py).  Two calls of
    either entry give the same bits."""
    lik = _lik()
    Dy, scale = 2 * Dt, 2.75
    mu32, v32, Y32, kl32 = _reduction_case(B, K, Dt, n_kl, 11)
    glob = np.array([1.25, 0.5])
    m64, v64 = mu32.astype(np.float64), v32.astype(np.float64)
    y64 = np.broadcast_to(Y32.astype(np.float64)[:, None, :], (B, K, Dt)).copy()
    klsum = sum((k.astype(np.float64).sum(-1) for k in kl32), np.zeros((B, K)))
    E = REF.variational_expectations(m64, v64, y64).sum(-1).numpy()
    L = E - klsum
    want = L.mean(1) if mode_vi else torch.logsumexp(torch.as_tensor(L), 1).numpy() - math.log(K)
    S_L = (H.var_exp_scale(m64, v64, y64).sum(-1).numpy() + klsum).max(1) + np.abs(want)
    gl = torch.as_tensor(glob, dtype=torch.float64, device=gpu_device)
    Yd = _t(Y32, gpu_device)
    results = []
    for sample_major in (False, True):
        lay = (lambda a: np.transpose(a, (1, 0, 2))) if sample_major else (lambda a: a)
        fm, fv = (_t(lay(a), gpu_device).reshape(B * K, -1) for a in (mu32, v32))
        kls = [_t(lay(k), gpu_device).reshape(B * K, -1) for k in kl32]
        sb, sk = (1, B) if sample_major else (K, 1)
        first = _reduce_call(gpu_device, lik.lik_desc(), fm, fv, Yd, B, K, Dy, sb, sk, kls, gl, scale, mode_vi)
        again = _reduce_call(gpu_device, lik.lik_desc(), fm, fv, Yd, B, K, Dy, sb, sk, kls, gl, scale, mode_vi)
        assert torch.equal(first[1], again[1]) and torch.equal(first[2], again[2])                # determinism
        results.append(first)
    (ms, logp, elbo), other = results
    assert torch.equal(logp, other[1]) and torch.equal(elbo, other[2])                            # the tiling does not change the arithmetic
    got = _n64(logp)
    mult = _multiple(got, want, S_L)
    e_got, e_want = float(elbo), scale * want.sum() - glob.sum()
    e_mult = abs(e_got - e_want) / (U * scale * S_L.sum())
    print("B=%d K=%d Dt=%d n_kl=%d mode_vi=%d: per-point %.2f, bound %.2f multiples of 2^-24 S" % (B, K, Dt, n_kl, mode_vi, mult, e_mult))
    assert mult <= C8 and e_mult <= C8, (mult, e_mult)
    assert abs(e_got - (scale * got.sum() - glob.sum())) <= 1e-12 * max(abs(e_got), 1.0)
    if not mode_vi:
        np.testing.assert_allclose(_n64(ms[:, 0]) + np.log(_n64(ms[:, 1])) - math.log(K), got, rtol=1e-5, atol=1e-5)
    # the heads
    fm, fv = (_t(a, gpu_device).reshape(B * K, -1) for a in (mu32, v32))
    kls = [_t(k, gpu_device).reshape(B * K, -1) for k in kl32]
    w, dm, dv, sums = _backward_call(gpu_device, lik.lik_desc(), fm, fv, Yd, B, K, Dy, scale=scale, mode_vi=mode_vi, kls=kls, glob=gl)
    again = _backward_call(gpu_device, lik.lik_desc(), fm, fv, Yd, B, K, Dy, scale=scale, mode_vi=mode_vi, kls=kls, glob=gl)
    assert all(torch.equal(a, b) for a, b in zip((w, dm, dv, sums), again))                       # determinism
    w_only = _backward_call(gpu_device, lik.lik_desc(), fm, fv, Yd, B, K, Dy, scale=scale, mode_vi=mode_vi, kls=kls, glob=gl, want_heads=False)
    assert torch.equal(w_only[0], w) and torch.equal(w_only[3], sums)                             # d_mean = d_var = NULL: the weights alone
    w, dm, dv, sums = _n64(w).reshape(B, K), _n64(dm).reshape(B, K, Dy), _n64(dv).reshape(B, K, Dy), sums.cpu().numpy()
    wr = np.full((B, K), scale / K) if mode_vi else scale * torch.softmax(torch.as_tensor(L), 1).numpy()
    tol_L = C8 * U * S_L
    tw = np.full((B, K), 4 * U * scale / K) if mode_vi else IR.tol_w(wr, scale, tol_L)
    assert np.isfinite(w).all() and np.all(np.abs(w - wr) <= tw), float((np.abs(w - wr) / tw).max())
    (rm, rv), (sm, sv) = REF.heads(m64, v64, y64), H.heads_scales(m64, v64, y64)
    for nm, g, r, Sh in (("d_mean", dm, rm.numpy(), sm.numpy()), ("d_var", dv, rv.numpy(), sv.numpy())):
        tol = np.abs(r) * tw[..., None] + wr[..., None] * C8 * U * Sh
        ratio = float((np.abs(g - r * wr[..., None]) / tol).max())
        print("  %s max err / allowed %.3f" % (nm, ratio))
        assert ratio <= 1.0, (nm, ratio)
    assert sums[1] == 0.0
    assert abs(sums[0] - want.sum()) <= float(tol_L.sum()), (sums[0], want.sum())
    assert abs(sums[2] - (scale * sums[0] - glob.sum())) <= 4 * 2.0 ** -52 * (abs(scale * sums[0]) + glob.sum()), sums


# ---- 4: the predictive mixture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N,Dt", [(1, 70, 2), (7, 9, 3), (64, 5, 1), (65, 9, 2)])
def test_mixture_entry_point_matches_the_restatement(gpu_device, S, N, Dt):
    """iwvi_lik_predict_mixture, both layouts: S = 1 (the elementwise result; N = 70: two workgroups of 64 points), 7 (a ragged segment of 8),
    64 and 65 (one full chunk of 64 lanes, and one more draw).  Tolerances: tests/test_gpu_bounded.py's _mixture_tol with this file's
    constants -- C 2^-24 S of the worst draw, the target columns added, + 4 x 2^-24 (1 + |result|) for the log-sum-exp; the variance also
    carries the mean's error through 2 E dE."""
    from dgps_with_iwvi_amd import _abi
    lik = _lik()
    rng = np.random.default_rng([S, N, Dt])
    Dy = 2 * Dt
    mu32 = rng.uniform(-2.0, 2.0, (S, N, Dy)).astype(np.float32)
    v32 = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), (S, N, Dy))).astype(np.float32)
    m64, v64 = mu32.astype(np.float64), v32.astype(np.float64)
    # targets the mixture finds plausible (the 20-point rule's reach: hetero_restatement.cases)
    Y32 = (m64[0, :, :Dt] + rng.uniform(-2, 2, (N, Dt)) * np.sqrt(v64[0, :, :Dt] + np.exp(m64[0, :, Dt:]))).astype(np.float32)
    Y64 = Y32.astype(np.float64)
    want = H.mixture(REF, m64, v64, Y64)
    Ys = np.broadcast_to(Y64, (S, N, Dt)).copy()
    tm = C8 * U * np.abs(m64[..., :Dt]).max(0)
    tol = {"log_density": C16 * U * H.density_scale(REF, m64, v64, Ys).numpy().max(0).sum(-1) + 4 * U * (1 + np.abs(want["log_density"])),
           "mean": tm + U * 1e-30,
           "var": C8 * U * (H.var_scale(m64, v64).numpy() + m64[..., :Dt] ** 2).max(0) + 4 * np.abs(m64[..., :Dt]).max(0) * tm}
    for sample_major in (False, True):
        lay = (lambda a: a) if sample_major else (lambda a: np.transpose(a, (1, 0, 2)))
        fm, fv, yd = _t(lay(mu32), gpu_device), _t(lay(v32), gpu_device), _t(Y32, gpu_device)
        got = {"log_density": torch.full((N,), float("nan"), device=gpu_device), "mean": torch.full((N, Dt), float("nan"), device=gpu_device),
               "var": torch.full((N, Dt), float("nan"), device=gpu_device)}
        sn, ss = (1, N) if sample_major else (S, 1)
        _abi.check(_abi.lib().iwvi_lik_predict_mixture(lik.lik_desc(), _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(yd), N, S, Dy, sn, ss,
                                                       _abi.ptr(got["log_density"]), _abi.ptr(got["mean"]), _abi.ptr(got["var"]), _abi.stream_ptr()))
        for k in tol:
            g = _n64(got[k])
            assert g.shape == want[k].shape and np.isfinite(g).all(), (k, g.shape)
            ratio = float((np.abs(g - want[k]) / tol[k]).max())
            print("S=%d sample_major=%s %-12s max err %.3e, worst err / tol %.3f" % (S, sample_major, k, float(np.abs(g - want[k]).max()), ratio))
            assert ratio <= 1.0, (k, ratio)
        # the density alone, and the moments alone: the same bits
        lp = torch.full((N,), float("nan"), device=gpu_device)
        _abi.check(_abi.lib().iwvi_lik_predict_mixture(lik.lik_desc(), _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(yd), N, S, Dy, sn, ss, _abi.ptr(lp), None, None,
                                                       _abi.stream_ptr()))
        mn, vr = (torch.full((N, Dt), float("nan"), device=gpu_device) for _ in range(2))
        _abi.check(_abi.lib().iwvi_lik_predict_mixture(lik.lik_desc(), _abi.ptr(fm), _abi.ptr(fv), None, N, S, Dy, sn, ss, None, _abi.ptr(mn), _abi.ptr(vr),
                                                       _abi.stream_ptr()))
        assert torch.equal(lp, got["log_density"]) and torch.equal(mn, got["mean"]) and torch.equal(vr, got["var"])
        if S == 1:                                               # one draw: the elementwise entries' own numbers
            pm, pv = lik.predict_mean_and_var(fm.reshape(N, Dy), fv.reshape(N, Dy))
            assert torch.equal(mn, pm) and torch.equal(vr, pv)


# ---- 5: the sampler --------------------------------------------------------------------------------------------------------------------------
def test_sample_y_is_f_plus_scaled_unit_noise(gpu_device):
    """With z_f given and return_f: f = m_f + sqrt(v_f) z_1 and g = m_g + sqrt(v_g) z_2 to float32 rounding, and (y - f) exp(-g / 2) is a
    unit-variance eps: its sample variance over 2 x 20 000 draws at fixed moments lies within 4 standard errors sqrt(2 / (n - 1)) of 1, its mean
    within 4 / sqrt(n) of 0.  The same (seed, serial) gives the same bits, another serial other draws."""
    lik = _lik()
    T, Dt = 20000, 2
    rng = np.random.default_rng(8)
    mu = np.tile(np.array([[0.5, -1.0, -1.2, 0.8]]), (T, 1))
    var = np.tile(np.array([[0.3, 0.0, 0.6, 0.25]]), (T, 1))
    z = rng.standard_normal((T, 4)).astype(np.float32)
    m, v, zd = _t(mu, gpu_device), _t(var, gpu_device), _t(z, gpu_device)
    y, f = lik.sample_y(m, v, z_f=zd, return_f=True, seed=5, serial=9)
    assert tuple(y.shape) == (T, Dt) and tuple(f.shape) == (T, 4)
    fw = mu + np.sqrt(var) * z.astype(np.float64)
    np.testing.assert_allclose(_n64(f), fw, rtol=0, atol=4 * U * (np.abs(mu) + np.sqrt(var) * np.abs(z)).max())
    eps = (_n64(y) - _n64(f)[:, :Dt]) * np.exp(-0.5 * _n64(f)[:, Dt:])
    n = eps.size
    s2, mean = eps.var(ddof=1), eps.mean()
    print("eps: mean %.4f (allowed %.4f), variance %.4f (allowed 1 +- %.4f)" % (mean, 4 / math.sqrt(n), s2, 4 * math.sqrt(2.0 / (n - 1))))
    assert abs(s2 - 1.0) <= 4 * math.sqrt(2.0 / (n - 1)) and abs(mean) <= 4 / math.sqrt(n)
    for d in range(Dt):                                          # ... in each column by itself too (n = T there)
        assert abs(eps[:, d].var(ddof=1) - 1.0) <= 4 * math.sqrt(2.0 / (T - 1)), d
    y2, f2 = lik.sample_y(m, v, z_f=zd, return_f=True, seed=5, serial=9)
    assert torch.equal(y, y2) and torch.equal(f, f2)
    y3 = lik.sample_y(m, v, z_f=zd, seed=5, serial=10)
    assert not torch.equal(y, y3)
    # drawn z: f and g are standardised normals of their own, uncorrelated with each other and with eps
    y4, f4 = lik.sample_y(m, v, return_f=True, seed=5, serial=11)
    sd = np.sqrt(var[0])
    lim = 4 / math.sqrt(T)
    for c in (0, 2, 3):                                          # (column 1 has v_f = 0: f = m_f exactly)
        zc = (_n64(f4)[:, c] - mu[0, c]) / sd[c]
        assert abs(zc.mean()) <= lim and abs(zc.var(ddof=1) - 1.0) <= 4 * math.sqrt(2.0 / (T - 1)), c
    assert np.all(_n64(f4)[:, 1] == np.float32(-1.0))
    e4 = (_n64(y4) - _n64(f4)[:, :Dt]) * np.exp(-0.5 * _n64(f4)[:, Dt:])
    z1, z2 = (_n64(f4)[:, 0] - mu[0, 0]) / sd[0], (_n64(f4)[:, 2] - mu[0, 2]) / sd[2]
    for a, b in ((z1, z2), (z1, e4[:, 0]), (z2, e4[:, 0])):
        assert abs(np.corrcoef(a, b)[0, 1]) <= lim
    assert abs(e4.var(ddof=1) - 1.0) <= 4 * math.sqrt(2.0 / (e4.size - 1))
    # Fvar = None: f = m_f, g = m_g; a NaN moment gives a NaN y in its own column only
    y5, f5 = lik.sample_y(m, None, return_f=True, seed=5, serial=12)
    assert torch.equal(f5, m)
    bad = m[:4].clone()
    bad[1, 2] = float("nan")                                     # g of column 0, row 1
    y6 = lik.sample_y(bad, v[:4], seed=5, serial=13)
    assert bool(torch.isnan(y6[1, 0])) and int(torch.isnan(y6).sum()) == 1
