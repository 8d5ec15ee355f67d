"""Beta and Ordinal likelihoods (probit link) on the GPU against the float64 restatement (tests/bounded_restatement.py, pinned by
tests/test_bounded_host.py), with injected noise.

Elementwise callables and heads: |got - ref| <= C x 2^-24 x S with the scale S computed in float64 from the magnitudes of the terms
(bounded_restatement.var_exp_scale and its neighbours).  C = 16 is derived, not fitted: a plain float32 NumPy evaluation of the kernels'
formulas (bounded_restatement.Float32) over these very cases stays within 5.16 x 2^-24 S (the Beta's predictive variance at scale 50;
tests/test_bounded_host.py asserts 3 x the measured multiple <= C), and the factor 3 is left for the device's erfcf / lgammaf / digamma.
On an MI355X the worst multiple over these cases is 6.56 (the Beta's variational expectation at scale 2), 2.36 for the heads.
Through the stack the tolerances are tests/test_gpu_likelihoods.py's own for the same comparisons (the layers are the same kernels)."""
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
import bounded_restatement as X   # noqa: E402
import iw_reduction_reference as IR   # noqa: E402
import mixture_restatement as MX   # noqa: E402

pytestmark = pytest.mark.gpu

U = X.U
C = X.C_BOUND
ELBO_RTOL = 1e-4
STACK = {"beta": dict(scale=2.5), "ordinal": dict(bin_edges=X.STACK_EDGES, sigma=0.8)}     # the parameters of the tests through the stack
_IDS = ["%s-%g" % (k, kw.get("scale", kw.get("sigma"))) for k, kw, _ in X.ELEMENTWISE_CASES]


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)), device=dev)


def _n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _liks(kind, **kw):
    from dgps_with_iwvi_amd import likelihoods
    if kind == "beta":
        return likelihoods.Beta(**kw), X.make(kind, **kw)
    lik = likelihoods.Ordinal(kw["bin_edges"])
    lik.sigma = kw.get("sigma", 1.0)
    return lik, X.make(kind, **kw)


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


_grids = X.grids          # moment_grid(), 600 points; the Ordinal also on far_grid: f up to 8 sigma past the outer edges


# ---- 1: the elementwise callables and the heads -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw,ys", X.ELEMENTWISE_CASES, ids=_IDS)
def test_elementwise_callables_match_the_restatement(gpu_device, kind, kw, ys):
    lik, ref = _liks(kind, **kw)
    worst = {}
    for mu32, v32 in _grids(kind, kw):
        assert mu32.size == 600
        m64, v64 = mu32.astype(np.float64), v32.astype(np.float64)
        m, v = _t(mu32.reshape(-1, 1), gpu_device), _t(v32.reshape(-1, 1), gpu_device)
        pm, pv = lik.predict_mean_and_var(m, v)
        rm, rv = ref.predict_mean_and_var(m64, v64)
        sm, sv = X.mean_var_scales(ref, m64, v64)
        worst["predict_mean"] = max(worst.get("predict_mean", 0.0), _multiple(_n64(pm), rm.numpy(), sm.numpy()))
        worst["predict_var"] = max(worst.get("predict_var", 0.0), _multiple(_n64(pv), rv.numpy(), sv.numpy()))
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
        assert w <= C, (what, w)


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


@pytest.mark.parametrize("kind,kw,ys", X.ELEMENTWISE_CASES, ids=_IDS)
def test_heads_are_the_derivatives_of_the_rule(gpu_device, kind, kw, ys):
    """iwvi_lik_elbo_backward with K = 1, the plain bound, scale = 1 and no regularisers: d_mean and d_var ARE dE/dmu and dE/dv, and
    out_sums[1] = sum_b dE_b / d scale (Beta: the check of the device digamma) or d sigma (Ordinal), against its own scale sum_b S_b."""
    lik, ref = _liks(kind, **kw)
    mult = {}
    for mu32, v32 in _grids(kind, kw):
        B = mu32.size
        Y32 = np.asarray([ys[b % len(ys)] for b in range(B)], dtype=np.float32)
        m64, v64, y64 = (a.astype(np.float64) for a in (mu32, v32, Y32))
        fm, fv, Yd = (_t(a.reshape(-1, 1), gpu_device) for a in (mu32, v32, Y32))
        w, dm, dv, sums = _backward_call(gpu_device, lik.lik_desc(), fm, fv, Yd, B, 1, 1)
        rdm, rdv, rdp, Sm, Sv, Sp = X.heads(ref, m64, v64, y64)
        assert torch.equal(w, torch.ones_like(w))
        sums = sums.cpu().numpy()
        ve = ref.variational_expectations(m64, v64, y64).numpy()
        for what, x in (("d_mean", _multiple(_n64(dm), rdm.numpy(), Sm.numpy())), ("d_var", _multiple(_n64(dv), rdv.numpy(), Sv.numpy())),
                        ("sum of E", abs(sums[0] - ve.sum()) / (U * X.var_exp_scale(ref, m64, v64, y64).numpy().sum())),
                        ("d_par", abs(sums[1] - float(rdp.sum())) / (U * float(Sp.sum())))):
            mult[what] = max(mult.get(what, 0.0), x)
        assert sums[2] == sums[0]                                # scale = 1, no global KL
    print("%s %r heads: worst multiples of 2^-24 S: " % (kind, kw) + "  ".join("%s %.2f" % kv for kv in sorted(mult.items())))
    for what, x in mult.items():
        assert x <= C, (what, x)


# ---- 2: the reduction and the heads where the layout changes ------------------------------------------------------------------------
def _direct_case(kind, B, K, Dy, seed):
    rng = np.random.default_rng(seed)
    mu32 = rng.uniform(-2.0, 2.0, (B, K, Dy)).astype(np.float32)
    v32 = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), (B, K, Dy))).astype(np.float32)
    kl32 = rng.uniform(0.0, 1.0, (B, K, 2)).astype(np.float32)
    if kind == "beta":
        Y32 = rng.uniform(0.02, 0.98, (B, Dy)).astype(np.float32)
        Y32.reshape(-1)[0] = 0.0
        Y32.reshape(-1)[-1] = 1.0
    else:
        Y32 = rng.integers(0, len(X.STACK_EDGES) + 1, (B, Dy)).astype(np.float32)
    return mu32, v32, kl32, Y32


SHAPES = [(65, 5), (3, 65), (64, 33), (1, 4)]


@pytest.mark.parametrize("Dy", [1, 2])
@pytest.mark.parametrize("B,K", SHAPES)
@pytest.mark.parametrize("kind", sorted(STACK))
def test_reduction_and_heads_at_the_layout_switches(gpu_device, kind, B, K, Dy):
    """iwvi_lik_elbo_reduce and iwvi_lik_elbo_backward directly: B = 65 a second workgroup with one live point (and a partly filled wave of
    the heads' workgroup), K = 65 a second trip of the sample loop and the heads' second evaluation, K = 33 the widest segment, (1, 4) the
    narrowest with a single point; both bounds, with and without a local regulariser (width 2).  Per point: |got - ref| <= C 2^-24
    (max_k (S_bk + |kl_bk|) + |ref|); weights: iw_reduction_reference.tol_w of that; a head adds C 2^-24 of its own scale per unit weight."""
    from dgps_with_iwvi_amd import _abi
    lik, ref = _liks(kind, **STACK[kind])
    mu32, v32, kl32, Y32 = _direct_case(kind, B, K, Dy, 100 * B + K + Dy)
    scale, glob = 3.5, np.array([1.25, 0.5])
    m64, v64, kl64 = (a.astype(np.float64) for a in (mu32, v32, kl32))
    y64 = np.broadcast_to(Y32.astype(np.float64)[:, None, :], (B, K, Dy)).copy()
    fm, fv, kl = (_t(a, gpu_device).reshape(B * K, -1) for a in (mu32, v32, kl32))
    Yd = _t(Y32, gpu_device)
    gl = torch.as_tensor(glob, dtype=torch.float64, device=gpu_device)
    E = ref.variational_expectations(m64, v64, y64).sum(-1)
    S_E = X.var_exp_scale(ref, m64, v64, y64).sum(-1).numpy()
    rdm, rdv, rdp, Sm, Sv, Sp = (a.numpy().reshape(B, K, Dy) for a in X.heads(ref, m64, v64, y64))
    kl_dims, gl_n = (ctypes.c_int32 * 1)(2), (ctypes.c_int32 * 1)(2)
    for with_kl in (False, True):
        L = (E - torch.as_tensor(kl64.sum(-1)) * (1.0 if with_kl else 0.0)).numpy()
        for mode_vi in (0, 1):
            tag = "%s B=%d K=%d Dy=%d kl=%d vi=%d" % (kind, B, K, Dy, with_kl, mode_vi)
            want = IR.logp(L, mode_vi=bool(mode_vi))
            S = (S_E + (kl64.sum(-1) if with_kl else 0.0)).max(1) + np.abs(want)
            ms = torch.full((B, 2), float("nan"), device=gpu_device)
            logp = torch.full((B,), float("nan"), device=gpu_device)
            elbo = torch.full((1,), float("nan"), dtype=torch.float64, device=gpu_device)
            ticket = torch.zeros(1, dtype=torch.int64, device=gpu_device)
            _abi.check(_abi.lib().iwvi_lik_elbo_reduce(lik.lik_desc(), _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(Yd), B, K, Dy, K, 1,
                                                       _abi.ptr_array([kl]) if with_kl else None, kl_dims, int(with_kl),
                                                       _abi.ptr_array([gl]), gl_n, 1, scale, K, mode_vi, None if mode_vi else _abi.ptr(ms), _abi.ptr(logp),
                                                       ctypes.c_void_p(elbo.data_ptr()), ctypes.c_void_p(ticket.data_ptr()), _abi.stream_ptr()))
            assert int(ticket) == 0
            got = _n64(logp)
            mult = _multiple(got, want, S)
            e_got, e_want = float(elbo), scale * want.sum() - glob.sum()
            e_mult = abs(e_got - e_want) / (U * scale * S.sum())
            assert mult <= C and e_mult <= C, (tag, mult, e_mult)
            assert abs(e_got - (scale * got.sum() - glob.sum())) <= 1e-12 * abs(e_got) + 1e-12
            if not mode_vi:
                np.testing.assert_allclose(_n64(ms[:, 0]) + np.log(_n64(ms[:, 1])) - math.log(K), got, rtol=1e-5, atol=1e-5)
            # the heads
            w, dm, dv, sums = _backward_call(gpu_device, lik.lik_desc(), fm, fv, Yd, B, K, Dy, scale=scale, mode_vi=mode_vi, kls=[kl] if with_kl else (), glob=gl)
            w, dm, dv, sums = _n64(w).reshape(B, K), _n64(dm).reshape(B, K, Dy), _n64(dv).reshape(B, K, Dy), sums.cpu().numpy()
            wr = np.full((B, K), scale / K) if mode_vi else scale * np.exp(L - IR.logp(L)[:, None] - math.log(K))
            tol_L = C * U * (S_E + (kl64.sum(-1) if with_kl else 0.0) + np.abs(L)).max(1)
            tw = np.full((B, K), 4 * U * scale / K) if mode_vi else IR.tol_w(wr, scale, tol_L)
            assert np.isfinite(w).all() and np.all(np.abs(w - wr) <= tw), (tag, float((np.abs(w - wr) / tw).max()))
            for nm, g, r, Sh in (("d_mean", dm, rdm, Sm), ("d_var", dv, rdv, Sv)):
                tol = np.abs(r) * (tw / wr)[..., None] + wr[..., None] * C * U * Sh
                assert np.all(np.abs(g - r * wr[..., None]) <= tol), (tag, nm, float((np.abs(g - r * wr[..., None]) / tol).max()))
            want1 = float((wr[..., None] * rdp).sum())
            tol1 = float(((tw[..., None] + wr[..., None] * C * U) * Sp).sum())
            assert abs(sums[1] - want1) <= tol1, (tag, sums[1], want1, tol1)
            assert abs(sums[0] - want.sum()) <= C * U * S.sum(), (tag, sums[0], want.sum())
            print("%s: per-point %.2f, bound %.2f multiples of 2^-24 S; w err / allowed %.3f" % (tag, mult, e_mult, float((np.abs(w - wr) / tw).max())))


@pytest.mark.parametrize("B,K", [(3, 65), (1, 4)])
@pytest.mark.parametrize("kind", sorted(STACK))
def test_heads_of_a_k_shard_against_the_jobs_normaliser(gpu_device, kind, B, K):
    """iwvi_lik_elbo_backward with lse_global and K_total = 2 K > K (the K-sharded weights scale exp(L - lse_global)), Dy = 2, one regulariser
    of width 2, scale 2.75, against lik_restatement.sharded_heads in float64; tolerances as tests/test_gpu_explink.py's test of the same."""
    lik, ref = _liks(kind, **STACK[kind])
    Dy, scale = 2, 2.75
    mu32, v32, kl32, Y32 = _direct_case(kind, B, K, Dy, 23 + K)
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
    tol_L = C * U * S_L + 0.5 * IR.spacing32(lse)
    tw = IR.tol_w(wr, scale, tol_L)
    assert np.isfinite(w).all() and np.all(np.abs(w - wr) <= tw), float((np.abs(w - wr) / tw).max())
    _, _, rdp, Sm, Sv, Sp = (a.numpy().reshape(B, K, Dy) for a in X.heads(ref, m64, v64, y64))
    for nm, got, want, Sh in (("d_mean", dm, dmr, Sm), ("d_var", dv, dvr, Sv)):
        tol = np.abs(want) * (tw / wr)[..., None] + wr[..., None] * C * U * Sh
        print("%s K=%d lse_global: %s max err / allowed %.3f" % (kind, K, nm, float((np.abs(got - want) / tol).max())))
        assert np.all(np.abs(got - want) <= tol), (nm, float((np.abs(got - want) / tol).max()))
    want0 = float((lse - math.log(Kt)).sum())
    assert abs(sums[0] - want0) <= float(tol_L.sum()), (sums[0], want0)
    assert abs(sums[2] - (scale * sums[0] - glob.sum())) <= 4 * 2.0 ** -52 * (abs(scale * sums[0]) + glob.sum()), sums
    want1 = float((wr[..., None] * rdp).sum())
    tol1 = float(((tw[..., None] + wr[..., None] * C * U) * Sp).sum())
    assert abs(sums[1] - want1) <= tol1, (sums[1], want1, tol1)


# ---- 3: bound, per-point log p and gradients through the stack ----------------------------------------------------------------------
def _vi_noise(zs, B, K):
    """[B, K, dim] (the restatement's layout) -> [S*N, dim], S-major (models.py:50)."""
    return [np.ascontiguousarray(np.asarray(z).transpose(1, 0, 2).reshape(K * B, -1)) for z in zs]


@pytest.mark.parametrize("kind", sorted(STACK))
@pytest.mark.parametrize("iw,lv,Dy", [(True, True, 1), (False, True, 1), (True, False, 2)], ids=["iwvi-lv", "vi-lv", "iwvi-nolv-Dy2"])
def test_bound_logp_and_gradients_match_the_restatement(gpu_device, kind, iw, lv, Dy):
    from dgps_with_iwvi_amd import synthetic, backward
    from dgps_with_iwvi_amd.models import DGP_IWVI, DGP_VI
    B, K = 12, 4
    spec = _spec(kind, L=2, M=32, B=B, K=K, lv=lv, Dy=Dy)
    zs = synthetic.make_noise(spec, seed=2)
    lik, ref = _liks(kind, **STACK[kind])
    val, logp, gref = X.bound_and_gradients(spec, ref, zs, mode_vi=not iw)
    model = synthetic.build_model(spec, gpu_device, cls=DGP_IWVI if iw else DGP_VI, likelihood=lik)
    zd = [_t(z, gpu_device) for z in (zs if iw else _vi_noise(zs, B, K))]
    got = model.compute_log_likelihood(zd)
    print("%s iw=%s lv=%s Dy=%d: bound %.6f vs %.6f (%.2e relative)" % (kind, iw, lv, Dy, got, val, abs(got - val) / abs(val)))
    assert abs(got - val) <= ELBO_RTOL * abs(val), (got, val)
    if iw:
        lp = model.E_log_p_Y(zd).cpu().numpy()
        print("  per-point log p: max abs err %.3e" % np.abs(lp - logp).max())
        np.testing.assert_allclose(lp, logp, rtol=2e-4, atol=2e-2)
    elbo, grads = backward.iw_elbo_and_gradients(model, zd)
    assert abs(float(elbo) - val) <= 2e-4 * abs(val), (float(elbo), val)
    assert sorted(grads) == sorted(gref), (sorted(grads), sorted(gref))
    assert ref.grad_name in grads
    for k, v in grads.items():
        _close(k, v.detach().cpu().numpy().reshape(gref[k].shape), gref[k], rtol=5e-3)


# ---- 4: the predictive mixture ------------------------------------------------------------------------------------------------------
def _mixture_tol(ref, m64, v64, Y, want):
    """C 2^-24 S per draw (the worst draw of a point), the outputs of a point added; + 4 x 2^-24 (1 + |result|) for the float32 exponentials
    of the log-sum-exp and its rounding; the variance also carries the mean's error through 2 E dE (twice: E_s and the mixture mean)."""
    S, N, Dy = m64.shape
    Ys = np.broadcast_to(np.asarray(Y, dtype=np.float64), (S, N, Dy)).copy()
    sm, sv = (a.numpy() for a in X.mean_var_scales(ref, m64, v64))
    tm = C * U * sm.max(0)
    return {"log_density": C * U * X.density_scale(ref, m64, v64, Ys).numpy().max(0).sum(-1) + 4 * U * (1 + np.abs(want["log_density"])),
            "mean": tm, "var": C * U * sv.max(0) + 4 * np.abs(want["E"]).max(0) * tm}


def _assert_within(tag, got, want, tol):
    for k in tol:
        g, w = _n64(got[k]), want[k]
        assert g.shape == w.shape and np.isfinite(g).all(), (tag, k, g.shape, w.shape)
        ratio = float((np.abs(g - w) / tol[k]).max())
        print("%s %-12s max err %.3e, worst err / tol %.3f" % (tag, k, float(np.abs(g - w).max()), ratio))
        assert ratio <= 1.0, (tag, k, ratio)


@pytest.mark.parametrize("kind", sorted(STACK))
def test_mixture_entry_point_matches_the_restatement(gpu_device, kind):
    """iwvi_lik_predict_mixture at N = 4, S = 33 (one full chunk of 32 lanes and a ragged one), Dy = 2, both layouts."""
    from dgps_with_iwvi_amd import _abi
    lik, ref = _liks(kind, **STACK[kind])
    N, S, Dy = 4, 33, 2
    mu32, v32, _, Y32 = _direct_case(kind, N, S, Dy, 5)
    mu32, v32 = mu32.transpose(1, 0, 2).copy(), v32.transpose(1, 0, 2).copy()          # [S, N, Dy]
    m64, v64 = mu32.astype(np.float64), v32.astype(np.float64)
    want = MX.mixture(ref, m64, v64, Y32.astype(np.float64))
    tol = _mixture_tol(ref, m64, v64, Y32, want)
    for sample_major in (False, True):
        lay = (lambda a: a) if sample_major else (lambda a: np.transpose(a, (1, 0, 2)))
        fm, fv, yd = _t(lay(mu32), gpu_device), _t(lay(v32), gpu_device), _t(Y32, gpu_device)
        got = {"log_density": torch.full((N,), float("nan"), device=gpu_device), "mean": torch.full((N, Dy), float("nan"), device=gpu_device),
               "var": torch.full((N, Dy), float("nan"), device=gpu_device)}
        sn, ss = (1, N) if sample_major else (S, 1)
        _abi.check(_abi.lib().iwvi_lik_predict_mixture(lik.lik_desc(), _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(yd), N, S, Dy, sn, ss,
                                                       _abi.ptr(got["log_density"]), _abi.ptr(got["mean"]), _abi.ptr(got["var"]), _abi.stream_ptr()))
        _assert_within("%s sample_major=%s" % (kind, sample_major), got, want, tol)


@pytest.mark.parametrize("kind", sorted(STACK))
def test_predict_mixture_and_evaluate_mixture_through_the_stack(gpu_device, kind):
    """model.predict_mixture at N = 4, S = 33 against the restatement fed the device's own predict_f_multisample moments (2e-5 relative for
    the two routes to those moments, as tests/test_gpu_predict_mixture.py allows); evaluation.evaluate_mixture reports test_loglik_mc
    -- the mean of predict_mixture's log densities on the same noise -- and test_rmse for both likelihoods, unchanged."""
    from dgps_with_iwvi_amd import evaluation, settings, synthetic
    N, S = 4, 33
    spec = _spec(kind, L=2, M=16, B=10, K=3, lv=True, Dy=2, seed=9)
    lik, ref = _liks(kind, **STACK[kind])
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    Xn, Y = spec["X"][:N], spec["Y"][:N]
    rng = np.random.default_rng(3)
    zs = [_t(rng.standard_normal((S, N, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1])), gpu_device) for l in spec["layers"]]
    got = model.predict_mixture(Xn, S, Y=Y, zs=zs)
    m, v = model.predict_f_multisample(Xn, S, zs=zs)
    m64, v64 = _n64(m), _n64(v)
    want = MX.mixture(ref, m64, v64, Y)
    tol = {k: t + 2e-5 * np.maximum(1.0, np.abs(want[k])) for k, t in _mixture_tol(ref, m64, v64, Y, want).items()}
    _assert_within("%s through the stack" % kind, got, want, tol)

    def reset():
        settings.set_seed(21)
        model._words().zero_()
    reset()
    res = evaluation.evaluate_mixture(model, spec["X"][:10], spec["Y"][:10], num_predict_samples=S)
    assert set(res) == {"test_loglik_mc", "test_rmse"} and all(math.isfinite(x) for x in res.values()) and res["test_rmse"] > 0
    reset()
    lp = model.predict_mixture(spec["X"][:10], S, Y=spec["Y"][:10])["log_density"]
    assert res["test_loglik_mc"] == float(lp.double().mean())


# ---- 5: training --------------------------------------------------------------------------------------------------------------------
def _problem(kind, dev):
    """An L1_G5-style stack (latent-variable layer, one inner layer of 5 latent GPs, final layer) with the reference's initial values."""
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=2, M=32, B=64, K=5, Dx=4, with_lv=True, seed=41, parity=False)
    spec["Y"] = X.targets(spec, kind)
    return spec, synthetic.build_model(spec, dev, likelihood=_liks(kind, **STACK[kind])[0])


def _par(lik):
    return lik.scale if hasattr(lik, "scale") else lik.sigma


@pytest.mark.parametrize("kind", sorted(STACK))
def test_graph_step_equals_eager_step_and_resume_is_exact(gpu_device, kind, tmp_path):
    """Trainer(use_graph=True) replays a step with the three-launch evaluation as ONE hipGraph: parameters bit-identical to the eager
    trainer's after 6 steps; 3 steps, checkpoint, restore into a fresh model + trainer, 3 more == 6 uninterrupted, bit for bit.  The
    trained scalar is an Adam scalar on the device and moves; the Ordinal's edges, which share its buffer, do not."""
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
    gname = "lik_scale" if kind == "beta" else "lik_sigma"
    start = STACK[kind].get("scale", STACK[kind].get("sigma"))
    assert gname in names and _par(out[0][3].likelihood) == _par(out[1][3].likelihood) != start
    if kind == "ordinal":
        for _, _, _, model, _ in out:
            buf = model.likelihood._buffer()
            assert torch.equal(buf[1:].cpu(), torch.as_tensor(np.asarray(X.STACK_EDGES, dtype=np.float32)))
            assert float(buf[0]) == model.likelihood.sigma
    b, tb = fresh(False)
    for _ in range(3):
        tb.step()
    path = str(tmp_path / "ckpt_bounded.npz")
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
    assert _par(out[0][3].likelihood) == _par(c.likelihood)


@pytest.mark.parametrize("kind", sorted(STACK))
def test_training_moves_the_scalar_and_raises_the_bound_on_fixed_noise(gpu_device, kind):
    from dgps_with_iwvi_amd import synthetic
    from dgps_with_iwvi_amd.training import Trainer
    spec = _spec(kind, L=2, M=32, B=64, K=5, lv=True, seed=5)
    lik = _liks(kind, **STACK[kind])[0]
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    zs = [_t(z, gpu_device) for z in synthetic.make_noise(spec, seed=1)]
    before, p0 = model.compute_log_likelihood(zs), _par(lik)
    tr = Trainer(model, lr=5e-3, gamma=1e-2)
    for _ in range(25):
        tr.step()
    after = model.compute_log_likelihood(zs)
    print("%s bound on fixed noise: %.4f -> %.4f; trained scalar %.6f -> %.6f" % (kind, before, after, p0, _par(lik)))
    assert after > before, (before, after)
    assert _par(lik) != p0
    if kind == "ordinal":
        assert torch.equal(lik._buffer()[1:].cpu(), torch.as_tensor(np.asarray(X.STACK_EDGES, dtype=np.float32)))


@pytest.mark.parametrize("kind", sorted(STACK))
def test_k_sharded_training_refuses_the_new_likelihoods(gpu_device, kind):
    from dgps_with_iwvi_amd.training import Trainer
    _, model = _problem(kind, gpu_device)
    with pytest.raises(NotImplementedError, match="K-sharded"):
        Trainer(model, shard="k")


# ---- 6: the device master -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(STACK))
def test_device_master_is_read_by_the_next_launch(gpu_device, kind):
    """ONE descriptor, made once: writing the scale / sigma on the device changes what the next launch of every entry computes, to the
    bits of a likelihood constructed with that value."""
    from dgps_with_iwvi_amd import _abi
    MU, V = X.moment_grid()
    m, v = _t(MU.reshape(-1, 1), gpu_device), _t(V.reshape(-1, 1), gpu_device)
    yy = torch.full_like(m, 0.3 if kind == "beta" else 2.0)
    a, _ = _liks(kind, **STACK[kind])
    moved = dict(STACK[kind], **({"scale": 4.0} if kind == "beta" else {"sigma": 1.7}))
    b, _ = _liks(kind, **moved)
    if kind == "beta":
        master = torch.full((1,), STACK[kind]["scale"], device=gpu_device)
        a.bind_device_variance(master)
    else:
        master = a.trained_scalar_view(gpu_device)
    d = a.lik_desc()
    assert d.param0_dev == master.data_ptr()

    def var_exp(desc):
        out = torch.empty_like(m)
        _abi.check(_abi.lib().iwvi_lik_var_exp(desc, _abi.ptr(m), _abi.ptr(v), _abi.ptr(yy), 600, 1, 1, 600, _abi.ptr(out), _abi.stream_ptr()))
        return out
    first = var_exp(d)
    h0 = _backward_call(gpu_device, d, m, v, yy, 600, 1, 1)
    master.fill_(4.0 if kind == "beta" else 1.7)
    second = var_exp(d)                                          # the SAME descriptor
    h1 = _backward_call(gpu_device, d, m, v, yy, 600, 1, 1)
    assert not torch.equal(first, second) and torch.equal(second, var_exp(b.lik_desc()))
    hb = _backward_call(gpu_device, b.lik_desc(), m, v, yy, 600, 1, 1)
    assert all(torch.equal(x, y) for x, y in zip(h1, hb)) and not torch.equal(h0[1], h1[1])
    a.mark_device_variance_changed()
    assert _par(a) == pytest.approx(4.0 if kind == "beta" else 1.7, rel=1e-6)
