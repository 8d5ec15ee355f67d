"""Every stand-alone HIP form of the importance-weight reduction, fed chosen log-weights and compared with the float64 reference of
tests/iw_reduction_reference.py (pinned on the CPU by tests/test_iw_reduction_reference_host.py):

  k_elbo<SEG>      iwvi_logw_reduce, iwvi_iw_elbo_reduce, iwvi_iw_elbo_reduce_dev          (csrc/lv_elbo.hip)
  k_elbo_final     iwvi_lse_merge, iwvi_lse_merge_steps
  k_elbo_bwd/_finish  iwvi_iw_elbo_backward, iwvi_iw_elbo_backward_dev                      (csrc/backward.hip)
  k_lik_elbo<SEG>, k_lik_elbo_bwd   iwvi_lik_elbo_reduce, iwvi_lik_elbo_backward            (csrc/likelihood_tail.hip)

Inputs: the families of the reference module (near-equal, one dominant sample at k = 0 / SEG-1 / SEG / K-1 / 64, rising, wide range,
ties) at K in {1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 100, 128, 130} against B = 65 and B in {1, 3, 63, 64, 65, 257} against
K in {5, 65}; the rest (Dy, regularisers, global KL arrays, layouts, modes) pairwise.

Tolerances (all from the reference module, none from what a kernel returned):
  logp from float32 log-weights that ARE the inputs     4 spacing32(max(|m|, log K_total)) + 2e-6     (tol_reduce)
      the float32 NumPy restatement of the recurrence (restate_f32) stays within the spacing term alone on every family (host test),
      so the 2e-6 term is left whole to the hardware's exp and log; it has not needed measuring.
  the VI mean                                            half a spacing32 of sum_k |L| + one of the result  (tol_vi)
  logp from a log-weight summed on the device            (additions per sample + 4) spacing32(largest |partial sum|)   (tol_logw)
      plus tol_reduce.  tol_logw alone is the error of L; the reduction's own three float32 operations act at the magnitude of
      max(|m|, log K_total), which the partial sums of L do not reach when |L| < 1 < log K.  Measured on an MI355X with tol_logw alone:
      all samples equal, K = 64, K_total = 71, |L| = 0.5: 4.72e-7 against 4.17e-7 (s = 64 and its logarithm are exact there: what is left is
      the rounding of m + log s - log K_total at magnitude 4.2, half a spacing of 4.8e-7 twice, which the float32 restatement has too);
      near-equal, K = 65: 4.95e-7 against 4.77e-7.  iwvi_lik_elbo_reduce adds the same two terms.
  the generic (quadrature) tail                          Dy 1.5e-6 on top of both of the above
  weights                                                scale (w_ref / scale (exp(tol_L) - 1 + 4e-6) + 1e-30)          (tol_w)
  the bound                                              B 2^-52 of scale sum |logp_device|: float64 arithmetic on what the device wrote
"""
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
import iw_reduction_reference as R   # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ("bk", "kb")


def _f(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _d(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _lay(a, layout):
    """[B, K, ...] -> the array as the device reads it, (stride_b, stride_k) in rows."""
    B, K = a.shape[:2]
    if layout == "bk":
        return np.ascontiguousarray(a), K, 1
    return np.ascontiguousarray(np.swapaxes(a, 0, 1)), 1, B


def _glob(kls, dev):
    g = [_d(k, dev) for k in kls]
    return g, _abi().ptr_array(g), (ctypes.c_int32 * max(len(g), 1))(*[k.numel() for k in g])


def _abi():
    from dgps_with_iwvi_amd import _abi
    return _abi


class _Out:
    """Result buffers of one reduction call, run TWICE on the same ticket word: the two bounds are bit-identical, the word reads zero
    after each, and the bound is float64 arithmetic on the logp the device published."""

    def __init__(self, dev, B, want_ms=True):
        self.dev, self.B = dev, B
        self.ticket = torch.zeros(1, dtype=torch.int64, device=dev)
        self.logp = torch.full((B,), float("nan"), device=dev)
        self.ms = torch.full((B, 2), float("nan"), device=dev) if want_ms else None
        self.elbo = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)

    def twice(self, call, scale, kls, what):
        first = None
        for _ in range(2):
            self.logp.fill_(float("nan")); self.elbo.fill_(float("nan"))
            _abi().check(call(self))
            assert int(self.ticket.item()) == 0, "%s: ticket word left at %d" % (what, int(self.ticket.item()))
            got = (float(self.elbo.item()), self.logp.clone())
            if first is None:
                first = got
            else:
                assert got[0] == first[0] and torch.equal(got[1], first[1]), "%s: not bit-identical on the second call" % what
        lp = _np(self.logp)
        assert np.all(np.isfinite(lp)), what
        _check_bound(first[0], lp, scale, kls, what)
        return lp, (None if self.ms is None else _np(self.ms))


def _check_bound(elbo, lp_dev, scale, kls, what):
    want = R.bound(lp_dev, scale, kls)
    kl_abs = sum(float(np.abs(k).sum()) for k in kls)
    tol = R.bound_tol(lp_dev, scale) + sum(np.size(k) for k in kls) * 2.0 ** -52 * kl_abs
    print("  %s: bound %.17g vs %.17g (|d| %.3e, allowed %.3e)" % (what, elbo, want, abs(elbo - want), tol))
    assert abs(elbo - want) <= tol, (what, elbo, want, tol)


def _check_logp(lp, ref, tol, what):
    err = np.abs(lp - ref)
    i = int(np.argmax(err - tol))
    print("  %s: logp max err %.3e (worst point %d: err %.3e, allowed %.3e)" % (what, err.max(), i, err[i], tol[i]))
    assert np.all(err <= tol), (what, i, lp[i], ref[i], err[i], tol[i])


def _check_ms(ms, L, K_total, tol, what):
    """The published (m, s) pair recombines to the same logp; m is the maximum itself."""
    assert np.array_equal(ms[:, 0], L.max(1)), what
    _check_logp(ms[:, 0] + np.log(ms[:, 1]) - math.log(K_total), R.logp(L, K_total), tol, what + " (from ms)")


# ---- iwvi_logw_reduce ------------------------------------------------------------------------------------------------------------------
def _logw_reduce(dev, L, layout="bk", K_total=0, mode_vi=False, kls=(), scale=1.0, want_ms=True, what=""):
    a = _abi()
    B, K = L.shape
    arr, sb, sk = _lay(L, layout)
    lw = _f(arr, dev)
    g, gp, gn = _glob(kls, dev)
    out = _Out(dev, B, want_ms and not mode_vi)
    call = lambda o: a.lib().iwvi_logw_reduce(a.ptr(lw), B, K, sb, sk, gp, gn, len(g), scale, K_total, 1 if mode_vi else 0,
                                              a.ptr(o.ms), a.ptr(o.logp), a.ptr(o.elbo), a.ptr(o.ticket), a.stream_ptr())
    return out.twice(call, scale, kls, what)


@pytest.mark.parametrize("name", R.FAMILIES)
def test_logw_reduce_every_K_and_every_B(gpu_device, name):
    for n, (B, K) in enumerate(R.shape_cases()):
        L = R.family(name, B, K, seed=20)
        what = "%s B=%d K=%d" % (name, B, K)
        lp, ms = _logw_reduce(gpu_device, L, layout=LAYOUTS[n % 2], scale=1.0 + n, kls=R.global_kls(n % 3, 1 + n % 2 * (R.MAX_R - 1), seed=n),
                              what=what)
        _check_logp(lp, R.logp(L), R.tol_reduce(L), what)
        _check_ms(ms, L, K, R.tol_reduce(L), what)
        if name == "wide":                                       # finite and equal to the maximum up to float32 spacing
            assert np.all(np.abs(lp + math.log(K) - L.max(1)) <= R.spacing32(L.max(1))), what
            assert np.array_equal(ms[:, 1], np.ones(B)), what


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["vi", "k_total"])
def test_logw_reduce_modes_layouts_and_global_terms(gpu_device, layout, mode):
    """The VI mean and K_total > K in both layouts, with zero, one and the maximum number of global KL arrays of 1 and IWVI_MAX_R entries."""
    glob = [(0, 1), (1, 1), (1, R.MAX_R), (R.MAX_GLOB, 1), (R.MAX_GLOB, R.MAX_R)]
    n = 0
    for name in ("near_equal", "dominant", "rising", "ties_two"):
        for B, K in ((65, 5), (3, 65), (257, 17), (64, 130), (63, 8), (1, 33)):
            L = R.family(name, B, K, seed=21)
            kls = R.global_kls(*glob[n % len(glob)], seed=n)
            what = "%s %s %s B=%d K=%d glob=%s" % (mode, layout, name, B, K, glob[n % len(glob)])
            n += 1
            if mode == "vi":
                lp, _ = _logw_reduce(gpu_device, L, layout, mode_vi=True, kls=kls, scale=0.75, what=what)
                _check_logp(lp, R.logp(L, mode_vi=True), R.tol_vi(L), what)
            else:
                Kt = K + 1 + n
                lp, ms = _logw_reduce(gpu_device, L, layout, K_total=Kt, kls=kls, scale=3.5, what=what)
                _check_logp(lp, R.logp(L, Kt), R.tol_reduce(L, Kt), what)
                _check_ms(ms, L, Kt, R.tol_reduce(L, Kt), what)


# ---- iwvi_iw_elbo_reduce / _dev --------------------------------------------------------------------------------------------------------
def _moment_inputs(target, Dy, lik_var, rng):
    """fmean, fvar [B, K, Dy] float32-valued and Y [B, Dy] whose Gaussian expectation sums to about ``target`` [B, K] (<= Dy c0)."""
    B, K = target.shape
    c0 = -0.5 * math.log(2 * math.pi) - 0.5 * math.log(lik_var)
    q = (Dy * c0 - target) / Dy                                   # ((y - f)^2 + v) / (2 s) per output
    assert np.all(q >= 0), "target above the Gaussian's maximum"
    split = rng.uniform(0.2, 0.8, (B, K, Dy))
    Y = R.f32(rng.standard_normal((B, Dy)))
    fvar = R.f32(split * q[..., None] * 2 * lik_var)
    e = np.sqrt((1 - split) * q[..., None] * 2 * lik_var) * rng.choice([-1.0, 1.0], (B, K, Dy))
    return R.f32(Y[:, None, :] - e), fvar, Y


def _elbo_reduce(dev, fm, fv, Y, lik_var, kls_local, layout, K_total, mode_vi, glob, scale, lik_var_dev=None, what=""):
    a = _abi()
    B, K, Dy = fm.shape
    fma, sb, sk = _lay(fm, layout)
    tm, tv, tY = _f(fma, dev), _f(_lay(fv, layout)[0], dev), _f(Y, dev)
    tk = [_f(_lay(k, layout)[0], dev) for k in kls_local]
    kd = (ctypes.c_int32 * max(len(tk), 1))(*[k.shape[-1] for k in kls_local])
    g, gp, gn = _glob(glob, dev)
    out = _Out(dev, B, not mode_vi)
    if lik_var_dev is None:
        call = lambda o: a.lib().iwvi_iw_elbo_reduce(a.ptr(tm), a.ptr(tv), a.ptr(tY), lik_var, B, K, Dy, sb, sk, a.ptr_array(tk), kd, len(tk),
                                                     gp, gn, len(g), scale, K_total, 1 if mode_vi else 0, a.ptr(o.ms), a.ptr(o.logp),
                                                     a.ptr(o.elbo), a.ptr(o.ticket), a.stream_ptr())
    else:                                                        # the device scalar wins over the host argument
        ts = _f([lik_var_dev], dev)
        call = lambda o: a.lib().iwvi_iw_elbo_reduce_dev(a.ptr(tm), a.ptr(tv), a.ptr(tY), lik_var, a.ptr(ts), B, K, Dy, sb, sk, a.ptr_array(tk), kd,
                                                         len(tk), gp, gn, len(g), scale, K_total, 1 if mode_vi else 0, a.ptr(o.ms), a.ptr(o.logp),
                                                         a.ptr(o.elbo), a.ptr(o.ticket), a.stream_ptr())
    return out.twice(call, scale, glob, what)


def _f32v(x):
    return float(np.float32(x))


REG_SHAPES = [(0, 1)] + [(n, w) for n in (1, R.MAX_KL) for w in (1, 3)]


@pytest.mark.parametrize("channel", ["moments", "regularisers"])
@pytest.mark.parametrize("name", R.FAMILIES)
def test_iw_elbo_reduce_families_through_both_channels(gpu_device, name, channel):
    """The same families delivered through fmean / fvar / Y (a small likelihood variance gives the wide range) and through kl_local with
    fmean = Y, fvar = 0 (exact control); every second case goes through the _dev entry point with a device likelihood variance that differs
    from the host argument."""
    rng = np.random.default_rng(30)
    cases = [(65, K) for K in (1, 4, 5, 9, 17, 33, 64, 65, 130)] + [(B, K) for B in (1, 3, 63, 64, 257) for K in (5, 65)]
    for n, (B, K) in enumerate(cases):
        Dy = (1, 3)[n % 2]
        lik_var = _f32v(1e-3 if name == "wide" else 0.4)
        L = R.family(name, B, K, seed=31)
        layout = LAYOUTS[(n // 2) % 2]
        if channel == "moments":
            c0 = -0.5 * math.log(2 * math.pi) - 0.5 * math.log(lik_var)
            n_kl, width = REG_SHAPES[n % 3] if name != "wide" else (0, 1)
            # (the Gaussian part cannot exceed Dy c0: a per-point constant regulariser carries the rest, the pattern stays in the moments)
            shift = np.maximum(L.max(1, keepdims=True) - Dy * c0 + 0.5, 0.0) if name != "wide" else 0.0
            if not n_kl:
                L = L - shift
            fm, fv, Y = _moment_inputs(L - shift if n_kl else L, Dy, lik_var, rng)
            kls = R.split_regularisers(np.broadcast_to(-shift, L.shape), n_kl, width, seed=n) if n_kl else []
        else:
            if name == "wide":
                continue                                         # (the regulariser channel adds nothing to it: the range comes from the moments)
            n_kl, width = REG_SHAPES[1 + n % 4]
            Y = R.f32(rng.standard_normal((B, Dy)))
            fm, fv = np.repeat(Y[:, None, :], K, 1), np.zeros((B, K, Dy))
            c0 = -0.5 * math.log(2 * math.pi) - 0.5 * math.log(lik_var)
            kls = R.split_regularisers(Dy * c0 - L, n_kl, width, seed=n)
        dev_var = _f32v(lik_var) if n % 2 == 0 else None
        host_var = lik_var if dev_var is None else _f32v(7.0 * lik_var)
        Lref, big, n_add = R.gaussian_logw(fm, fv, Y, lik_var, kls)
        tol = R.tol_logw(big, n_add)
        if name in ("near_equal", "dominant", "ties_all", "ties_two"):
            assert tol.max() < 1e-4, tol.max()
        Kt = 0 if n % 3 else K + 7
        glob = R.global_kls(n % 3, 2, seed=n)
        what = "%s %s %s B=%d K=%d Dy=%d n_kl=%dx%d Kt=%d dev=%s" % (channel, name, layout, B, K, Dy, n_kl, width, Kt, dev_var is not None)
        lp, ms = _elbo_reduce(gpu_device, fm, fv, Y, host_var, kls, layout, Kt, False, glob, 2.0 + n, lik_var_dev=dev_var, what=what)
        tol_lp = tol + R.tol_reduce(Lref, Kt or K)
        _check_logp(lp, R.logp(Lref, Kt or K), tol_lp, what)
        _check_logp(ms[:, 0] + np.log(ms[:, 1]) - math.log(Kt or K), R.logp(Lref, Kt or K), tol_lp, what + " (from ms)")
        if name == "wide":
            assert np.all(np.abs(lp + math.log(Kt or K) - Lref.max(1)) <= tol + R.spacing32(Lref.max(1))) and np.array_equal(ms[:, 1], np.ones(B)), what
        if n % 4 == 1:                                           # the VI mean of the same inputs
            lpv, _ = _elbo_reduce(gpu_device, fm, fv, Y, host_var, kls, layout, 0, True, glob, 0.5, lik_var_dev=dev_var, what=what + " vi")
            _check_logp(lpv, R.logp(Lref, mode_vi=True), tol + R.tol_vi(Lref), what + " vi")


# ---- iwvi_lse_merge / iwvi_lse_merge_steps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 1024, 1025])
def test_lse_merge_of_uneven_shards_and_its_batched_form(gpu_device, G, B):
    """G shards of uneven size -- one holds a single sample, one lies 200 nats below another -- merged per evaluation and in the batched
    form: the reference's merge within the reduction tolerance, the bound exact on the published logp, the two forms bit for bit."""
    a = _abi()
    from dgps_with_iwvi_amd.sharding import merge_lse
    S, scale = 3, 4.25
    rng = np.random.default_rng(40 + G)
    sizes = [1] + [int(s) for s in rng.integers(2, 40, G - 1)]
    Kt = sum(sizes)
    ms_all, Ls = np.empty((G, S, B, 2)), []
    for e in range(S):
        shards = [R.family(("near_equal", "dominant", "rising")[e], B, K, seed=50 + 7 * e + i) for i, K in enumerate(sizes)]
        if G > 1:
            shards[1] = R.f32(shards[1] - 200.0)
        for r, sh in enumerate(shards):
            m, s = R.partials(sh)
            ms_all[r, e, :, 0], ms_all[r, e, :, 1] = m, R.f32(s)
        Ls.append(np.concatenate(shards, 1))
    ms32 = R.f32(ms_all)
    t = _f(ms32, gpu_device)
    kls = R.global_kls(2, R.MAX_R, seed=G)
    g, gp, gn = _glob(kls, gpu_device)
    logp = torch.empty(S, B, device=gpu_device)
    elbo = torch.empty(S, dtype=torch.float64, device=gpu_device)
    a.check(a.lib().iwvi_lse_merge_steps(a.ptr(t), G, S, B, Kt, gp, gn, len(g), scale, a.ptr(logp), a.ptr(elbo), a.stream_ptr()))
    for e in range(S):
        what = "merge G=%d B=%d evaluation %d" % (G, B, e)
        lp, el = merge_lse(t[:, e].contiguous(), Kt, g, scale)
        assert torch.equal(lp, logp[e]) and float(el) == float(elbo[e]), what
        ref = R.merge(ms32[:, e], Kt)                             # the published float32 partials, merged in float64
        tol = 4 * R.spacing32(np.maximum(np.abs(ms32[:, e, :, 0]).max(0), math.log(Kt))) + 2e-6
        _check_logp(_np(lp), ref, tol, what)
        _check_logp(_np(lp), R.logp(Ls[e], Kt), tol + 2.0 ** -23, what + " (against the unsharded samples)")   # + the float32 rounding of each s
        _check_bound(float(el), _np(lp), scale, kls, what)


# ---- iwvi_iw_elbo_backward / _dev ------------------------------------------------------------------------------------------------------
def _backward(dev, fm, fv, Y, lik_var, kls_local, mode_vi, glob, scale, lse_global=None, K_total=0, lik_var_dev=None, lik=None):
    a = _abi()
    B, K, Dy = fm.shape
    tm, tv, tY = _f(fm, dev), _f(fv, dev), _f(Y, dev)
    tk = [_f(k, dev) for k in kls_local]
    kd = (ctypes.c_int32 * max(len(tk), 1))(*[k.shape[-1] for k in kls_local])
    g, gp, gn = _glob(glob, dev)
    w = torch.full((B, K), float("nan"), device=dev)
    dm, dv = torch.full((B, K, Dy), float("nan"), device=dev), torch.full((B, K, Dy), float("nan"), device=dev)
    sums = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.empty(2 * B, dtype=torch.float64, device=dev)
    tl = None if lse_global is None else _f(lse_global, dev)
    if lik is not None:
        a.check(a.lib().iwvi_lik_elbo_backward(lik, a.ptr(tm), a.ptr(tv), a.ptr(tY), Dy, a.ptr_array(tk), kd, len(tk), B, K, scale, 1 if mode_vi else 0,
                                               a.ptr(w), a.ptr(dm), a.ptr(dv), gp, gn, len(g), a.ptr(tl), K_total or K, a.ptr(sums), a.ptr(ws),
                                               a.stream_ptr()))
    elif lik_var_dev is None:
        a.check(a.lib().iwvi_iw_elbo_backward(a.ptr(tm), a.ptr(tv), a.ptr(tY), Dy, a.ptr_array(tk), kd, len(tk), B, K, lik_var, scale,
                                              1 if mode_vi else 0, a.ptr(w), a.ptr(dm), a.ptr(dv), gp, gn, len(g), a.ptr(tl), K_total or K,
                                              a.ptr(sums), a.ptr(ws), a.stream_ptr()))
    else:
        ts = _f([lik_var_dev], dev)
        a.check(a.lib().iwvi_iw_elbo_backward_dev(a.ptr(tm), a.ptr(tv), a.ptr(tY), Dy, a.ptr_array(tk), kd, len(tk), B, K, lik_var, a.ptr(ts), scale,
                                                  1 if mode_vi else 0, a.ptr(w), a.ptr(dm), a.ptr(dv), gp, gn, len(g), a.ptr(tl), K_total or K,
                                                  a.ptr(sums), a.ptr(ws), a.stream_ptr()))
    return _np(w), _np(dm), _np(dv), _np(sums)


def _check_heads(got, Lref, tol_L, fm, fv, Y, lik_var, scale, mode_vi, glob, what, lse_global=None, K_total=None, name="", d_extra=0.0, gaussian=True):
    """w under the weight rule; d_mean, d_var: the same relative error plus four float32 roundings; the three sums."""
    w, dm, dv, sums = got
    B, K = Lref.shape
    wr, dmr, dvr, dlr = R.heads(Lref, fm, fv, Y, lik_var, scale, mode_vi, lse_global)
    tw = R.tol_w(wr, scale, tol_L)
    if mode_vi:
        tw = np.full_like(wr, 2.0 ** -23 * scale / K)
    ew = np.abs(w - wr)
    print("  %s: w max err %.3e (max of err / allowed %.3f)" % (what, ew.max(), (ew / tw).max()))
    assert np.all(np.isfinite(w)) and np.all(ew <= tw), (what, float((ew / tw).max()))
    if lse_global is None:
        assert np.all(np.abs(w.sum(1) - scale) <= K * 2.0 ** -23 * scale), (what, float(np.abs(w.sum(1) - scale).max()))
    if name == "wide":                                           # one live weight per point, equal to scale in float32
        assert np.all((w != 0).sum(1) == 1) and np.all(w.max(1) == float(np.float32(scale))), what
    if gaussian:
        rel = tw / np.maximum(wr, 1e-300)
        for nm, a_, r_ in (("d_mean", dm, dmr), ("d_var", dv, dvr)):
            tol = np.abs(r_) * (rel[..., None] + 4 * 2.0 ** -23) + 1e-30 * np.abs(r_ / np.maximum(wr[..., None], 1e-300)) + d_extra
            assert np.all(np.abs(a_ - r_) <= tol), (what, nm, float(np.abs(a_ - r_).max()))
        e = Y[:, None, :] - fm
        term = np.abs(-0.5 / lik_var + 0.5 * (e * e + fv) / lik_var ** 2)
        tol_dl = float(((tw[..., None] + 2.0 ** -23 * wr[..., None]) * term).sum())
        assert abs(sums[1] - dlr) <= tol_dl + 1e-300, (what, sums[1], dlr, tol_dl)
    lpr = R.logp(Lref, K_total or K, mode_vi) if lse_global is None else np.asarray(lse_global) - math.log(K_total)
    assert abs(sums[0] - lpr.sum()) <= float(np.sum(tol_L + (0 if lse_global is not None else R.tol_reduce(Lref, K_total or K)))), (what, sums[0], lpr.sum())
    want = scale * sums[0] - math.fsum(v for k in glob for v in k)
    assert abs(sums[2] - want) <= 4 * 2.0 ** -52 * (abs(scale * sums[0]) + sum(float(np.abs(k).sum()) for k in glob)), (what, sums[2], want)


@pytest.mark.parametrize("name", R.FAMILIES)
def test_iw_elbo_backward_weights_heads_and_sums(gpu_device, name):
    rng = np.random.default_rng(60)
    cases = [(5, K) for K in (1, 2, 5, 9, 33, 63, 64, 65, 100, 130)] + [(B, K) for B in (1, 3, 4, 65, 257) for K in (5, 65)]
    for n, (B, K) in enumerate(cases):
        Dy = (1, 3)[n % 2]
        lik_var = _f32v(1e-3 if name == "wide" else 0.4)
        c0 = -0.5 * math.log(2 * math.pi) - 0.5 * math.log(lik_var)
        L = R.family(name, B, K, seed=61)
        if name == "wide" or n % 2:                              # through the moments
            if name != "wide":
                L = L - np.maximum(L.max(1, keepdims=True) - Dy * c0 + 0.5, 0.0)
            fm, fv, Y = _moment_inputs(L, Dy, lik_var, rng)
            kls = []
        else:                                                    # through the regulariser channel
            Y = R.f32(rng.standard_normal((B, Dy)))
            fm, fv = np.repeat(Y[:, None, :], K, 1), np.zeros((B, K, Dy))
            kls = R.split_regularisers(Dy * c0 - L, *REG_SHAPES[1 + n % 4], seed=n)
        Lref, big, n_add = R.gaussian_logw(fm, fv, Y, lik_var, kls)
        tol_L = R.tol_logw(big, n_add)
        glob = R.global_kls((0, 1, R.MAX_GLOB_BWD)[n % 3], (1, R.MAX_R)[n % 2], seed=n)
        scale = 1.5 + n
        dev_var = _f32v(lik_var) if n % 2 == 0 else None
        host_var = lik_var if dev_var is None else _f32v(3.0 * lik_var)
        what = "%s B=%d K=%d Dy=%d n_kl=%d" % (name, B, K, Dy, len(kls))
        got = _backward(gpu_device, fm, fv, Y, host_var, kls, False, glob, scale, lik_var_dev=dev_var)
        _check_heads(got, Lref, tol_L, fm, fv, Y, lik_var, scale, False, glob, what, name=name)
        if n % 3 == 0:
            got = _backward(gpu_device, fm, fv, Y, host_var, kls, True, glob, scale, lik_var_dev=dev_var)
            _check_heads(got, Lref, tol_L + R.tol_vi(Lref), fm, fv, Y, lik_var, scale, True, glob, what + " vi")
        if n % 3 == 1 and name != "wide":                        # a K-shard against the whole job's normaliser (float32, as the exchange leaves it)
            other = R.family(name, B, 7, seed=62) - (3.0 if name != "rising" else 0.0)
            Kt = K + 7
            lse = R.f32(R.logp(np.concatenate([Lref, other], 1), Kt) + math.log(Kt))
            got = _backward(gpu_device, fm, fv, Y, host_var, kls, False, glob, scale, lse_global=lse, K_total=Kt, lik_var_dev=dev_var)
            _check_heads(got, Lref, tol_L + 0.5 * R.spacing32(lse), fm, fv, Y, lik_var, scale, False, glob, what + " lse_global", lse_global=lse, K_total=Kt)


# ---- iwvi_lik_elbo_reduce / iwvi_lik_elbo_backward -------------------------------------------------------------------------------------
def _lik(kind):
    """struct iwvi_lik_desc with host parameters: Gaussian(0.4), Bernoulli (probit), StudentT(scale 0.7, df 4)."""
    a = _abi()
    d = a.LikDesc()
    if kind == "gaussian":
        d.type, d.param[0] = a.LIK_GAUSSIAN, 0.4
    elif kind == "bernoulli":
        d.type = a.LIK_BERNOULLI_PROBIT
    else:
        d.type, d.param[0], d.param[1], d.lgc = a.LIK_STUDENT_T, 0.7, 4.0, math.lgamma(2.5) - math.lgamma(2.0)
    return d


def _lik_constant(kind, mu, v, Y):
    """sum_d of the likelihood's variational expectation, float64 [B] (tests/lik_restatement.py; the Gaussian's closed form)."""
    if kind == "gaussian":
        return (-0.5 * math.log(2 * math.pi * _f32v(0.4)) - 0.5 * ((Y - mu) ** 2 + v) / _f32v(0.4)).sum(-1)
    import lik_restatement as LR
    ref = LR.Bernoulli() if kind == "bernoulli" else LR.StudentT(scale=_f32v(0.7), df=4.0)
    return ref.variational_expectations(mu, v, Y).numpy().sum(-1)


# B on both sides of 256 / SEG for every SEG, K on both sides of 64
LIK_CASES = [(K, B) for K, bs in ((3, (63, 64, 65)), (7, (31, 32, 33)), (12, (15, 16, 17)), (20, (7, 8, 9)), (33, (3, 4, 5)), (64, (4, 5)), (65, (3, 4, 5)), (130, (9,)))
             for B in bs]


@pytest.mark.parametrize("kind", ["gaussian", "bernoulli", "student_t"])
def test_generic_tail_reduction_and_weights(gpu_device, kind):
    """k_lik_elbo / k_lik_elbo_bwd: the pattern travels through the regulariser channel, the moments are constant over k, so the
    quadrature contributes one constant per point.  Gaussian on every case, Bernoulli and Student-t on one family each."""
    a = _abi()
    rng = np.random.default_rng(70)
    desc = _lik(kind)
    fams = ("near_equal", "dominant", "rising", "ties_all", "ties_two") if kind == "gaussian" else (("dominant",) if kind == "bernoulli" else ("near_equal",))
    for name in fams:
        for n, (K, B) in enumerate(LIK_CASES):
            Dy = (1, 3)[n % 2]
            L = R.family(name, B, K, seed=71)
            Y = R.f32(rng.integers(0, 2, (B, Dy))) if kind == "bernoulli" else R.f32(rng.standard_normal((B, Dy)))
            mu, v = R.f32(rng.standard_normal((B, Dy))), R.f32(rng.uniform(0.05, 0.5, (B, Dy)))
            cst = _lik_constant(kind, mu, v, Y)
            fm, fv = np.repeat(mu[:, None, :], K, 1), np.repeat(v[:, None, :], K, 1)
            n_kl, width = REG_SHAPES[1 + n % 4]
            kls = R.split_regularisers(-L, n_kl, width, seed=n)
            # reference: the float64 constant minus the float32 regulariser entries, in the device's order
            Lref, big = np.repeat(cst[:, None], K, 1), np.repeat(np.abs(cst)[:, None], K, 1) + 2.0
            for k in kls:
                for j in range(width):
                    Lref = Lref - k[..., j]
                    big = np.maximum.reduce([big, np.abs(k[..., j]), np.abs(Lref)])
            tol_L = R.tol_logw(big, Dy + n_kl * width) + Dy * 1.5e-6
            layout = LAYOUTS[n % 2]
            Kt = 0 if n % 3 else K + 5
            glob = R.global_kls(n % 3, 2, seed=n)
            scale = 1.25 + n
            what = "%s %s %s B=%d K=%d Dy=%d n_kl=%dx%d Kt=%d" % (kind, name, layout, B, K, Dy, n_kl, width, Kt)
            fma, sb, sk = _lay(fm, layout)
            tm, tv, tY = _f(fma, gpu_device), _f(_lay(fv, layout)[0], gpu_device), _f(Y, gpu_device)
            tk = [_f(_lay(k, layout)[0], gpu_device) for k in kls]
            kd = (ctypes.c_int32 * len(tk))(*[width] * len(tk))
            g, gp, gn = _glob(glob, gpu_device)
            out = _Out(gpu_device, B)
            call = lambda o: a.lib().iwvi_lik_elbo_reduce(desc, a.ptr(tm), a.ptr(tv), a.ptr(tY), B, K, Dy, sb, sk, a.ptr_array(tk), kd, len(tk), gp, gn,
                                                          len(g), scale, Kt, 0, a.ptr(o.ms), a.ptr(o.logp), a.ptr(o.elbo), a.ptr(o.ticket),
                                                          a.stream_ptr())
            lp, ms = out.twice(call, scale, glob, what)
            tol = tol_L + R.tol_reduce(Lref, Kt or K)
            _check_logp(lp, R.logp(Lref, Kt or K), tol, what)
            _check_logp(ms[:, 0] + np.log(ms[:, 1]) - math.log(Kt or K), R.logp(Lref, Kt or K), tol, what + " (from ms)")
            if n % 4 == 0:
                outv = _Out(gpu_device, B, want_ms=False)
                callv = lambda o: a.lib().iwvi_lik_elbo_reduce(desc, a.ptr(tm), a.ptr(tv), a.ptr(tY), B, K, Dy, sb, sk, a.ptr_array(tk), kd, len(tk), gp,
                                                               gn, len(g), scale, 0, 1, None, a.ptr(o.logp), a.ptr(o.elbo), a.ptr(o.ticket),
                                                               a.stream_ptr())
                lpv, _ = outv.twice(callv, scale, glob, what + " vi")
                _check_logp(lpv, R.logp(Lref, mode_vi=True), tol_L + R.tol_vi(Lref), what + " vi")
            # the heads ([B, K] layout only): the weights follow the weight rule
            got = _backward(gpu_device, fm, fv, Y, None, kls, False, glob[:R.MAX_GLOB_BWD], scale, lik=desc)
            _check_heads(got, Lref, tol_L, fm, fv, Y, _f32v(0.4), scale, False, glob, what + " heads", gaussian=False)


@pytest.mark.parametrize("K", [3, 70])
def test_generic_tail_heads_of_a_k_shard_against_the_jobs_normaliser(gpu_device, K):
    """k_lik_elbo_bwd with lse_global (Student-t): the K-sharded weights scale exp(L - lse_global) and out_sums[0] = sum (lse_global -
    log K_total), at K = 3 and K = 70 -- past the one-sample-per-lane shortcut --, B = 5, Dy = 2, one regulariser of width 2, scale 2.75,
    moments that differ from sample to sample; the reference is lik_restatement.sharded_heads in float64.  L: the generic tail's tol_L plus
    half a spacing of the float32 normaliser, as the Gaussian test above; w, out_sums[0] and [2]: _check_heads.  d_mean and d_var carry the
    weight's relative error, four float32 roundings, and per unit weight the error of the rule's derivative sums: a node's g' = (nu + 1) e /
    (s^2 nu + e^2) is off by at most |g''| <= (nu + 1) / (s^2 nu) = 2.55 times half a spacing32 of |f| < 8 plus four roundings of |g'| <= 1.79
    -- 1.65e-6 --, and the ten fused accumulations add 10 x 2^-24 x 1.79 = 1.1e-6: under 4e-6 for dE/dmu (the weights sum to 1), and 4e-6 x
    sum_i w_i |x_i| / sqrt(2 v) = 4e-6 x 0.5642 / sqrt(2 v) for dE/dv = sum_i w_i x_i g'(f_i) / sqrt(2 v)."""
    import lik_restatement as LR
    B, Dy, scale = 5, 2, 2.75
    rng = np.random.default_rng(80 + K)
    desc = _lik("student_t")
    ref = LR.StudentT(scale=_f32v(0.7), df=4.0)
    fm, fv = R.f32(rng.standard_normal((B, K, Dy))), R.f32(rng.uniform(0.05, 0.5, (B, K, Dy)))
    Y, kl = R.f32(rng.standard_normal((B, Dy))), R.f32(rng.uniform(0.0, 1.0, (B, K, 2)))
    Lref, lse, wr, dmr, dvr, _, _ = LR.sharded_heads(lambda m, v: ref.variational_expectations(m, v, Y[:, None, :]).sum(-1), fm, fv, kl, scale)
    E = Lref + kl.sum(-1)
    big = np.maximum.reduce([np.abs(E) + 2.0, kl[..., 0], np.abs(E - kl[..., 0]), kl[..., 1], np.abs(Lref)])
    tol_L = R.tol_logw(big, Dy + 2) + Dy * 1.5e-6 + 0.5 * R.spacing32(lse)
    glob = R.global_kls(2, 2, seed=K)
    what = "student_t B=%d K=%d Dy=%d lse_global" % (B, K, Dy)
    got = _backward(gpu_device, fm, fv, Y, None, [kl], False, glob, scale, lse_global=lse, K_total=2 * K, lik=desc)
    _check_heads(got, Lref, tol_L, fm, fv, Y, _f32v(0.4), scale, False, glob, what, lse_global=lse, K_total=2 * K, gaussian=False)
    rel = R.tol_w(wr, scale, tol_L) / wr
    extra = {"d_mean": 4e-6 * np.ones_like(fv), "d_var": 4e-6 * 0.5642 / np.sqrt(2.0 * fv)}
    for nm, a_, r_ in (("d_mean", got[1], dmr), ("d_var", got[2], dvr)):
        tol = np.abs(r_) * (rel[..., None] + 4 * 2.0 ** -23) + wr[..., None] * extra[nm]
        print("  %s: %s max of err / allowed %.3f" % (what, nm, float((np.abs(a_ - r_) / tol).max())))
        assert np.all(np.abs(a_ - r_) <= tol), (what, nm, float((np.abs(a_ - r_) / tol).max()))
