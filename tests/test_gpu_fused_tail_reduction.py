"""The reductions inside the forward launch (csrc/dgp_forward.hip), each against the float64 reduction of the launch's OWN float32
log-weights (tests/iw_reduction_reference.py): ``model._fused_forward(..., elbo=...)`` returns ``logw`` together with
``(elbo, logp, ms)``, so nothing but the reduction stands between the two.  Tolerance: that of iwvi_logw_reduce,
4 spacing32(max(|m|, log K_total)) + 2e-6 (tol_reduce), half a spacing of sum |L| plus one of the result for the VI mean (tol_vi); the
bound is float64 arithmetic on the published logp (B 2^-52 of scale sum |logp|).  The dynamic range is widened by lik_var = 1e-3
and a few outliers in Y.

Which case reaches which tail (host dispatch of iwvi_dgp_forward: a workgroup takes 16 ns samples, ns = ceil(T / 4096) capped at 5 and
by the LDS; the low byte of iwvi_debug_last_forward_variant is ns, bit 10 the LEAN variant, bit 11 the shaped variant with the general tail):

  rows       the last arriver's loop over out_logw rows (fw_arrive): K does not divide the chunk (K = 5, B = 40: 13 chunks, the last one
             partial), the [K, B] layout (K = 4, B = 37), the VI mean ([K, B], K = 4, B = 37); K_total > K with want_ms on the first
  local      per-chunk log-sum-exp, partials stored and re-read by the last arriver (local_lse without the packed arrival): [B, K] with
             K | 16 at ns = 1, where the scratch has one slot per chunk and the packed arrival is therefore off (K = 4, B = 37; K = 16, B = 5)
  packed     the same with the packed arrival (fw_arrive_fast): needs ns >= 2, i.e. T > 4096, and at most 511 chunks: K = 8, B = 520
             (T = 4160, 130 chunks of 32).  IWVI_FW_SLOW_TAIL = 1 sends the same launch through `local`: logp and ms bit for bit.
             local_lse's loop for K > 32 needs a chunk that holds such a point: K = 40 | 80, so ns = 5, so T > 16384: K = 40, B = 420
             (T = 16800, 210 chunks), the smallest that reaches it; the packed arrival is on there.
  heads      the fused adjoint heads (adj_* of iwvi_elbo_desc) in the local_lse tail need two scratch slots per chunk, so ns >= 2 as well
             (at ns = 1 the library refuses them -- asserted): K = 8, B = 520 with and without the latent-variable layer, and the shaped variant
  lean       the LEAN variant's half-wave tail + packed arrival: the headline layer shape M = 128, K = 20, T % 80 == 0 AND ns == 5, which
             T <= 16384 does not give: B = 820 (T = 16400, 205 chunks) is the smallest B that reaches it (B = 40 runs the generic variant
             with ns = 1 -- asserted below); the same model with per-layer outputs takes the shaped variant with the general tail (bit 11)

The packed arrival carries each workgroup's partial sum as fixed point in units of 2^-20 (csrc/dgp_forward.hip: fw_arrive_fast; a partial
of 2^16 or more is stored exactly instead).  A float32 logp of magnitude 8 or more is a multiple of 2^-20, so on these inputs (lik_var = 1e-3:
every |logp| is in the hundreds or thousands) the packed bound, too, is exact arithmetic on the published logp and is held to the exact
rule; were a |logp| below 8 the format's own resolution, 2^-21 scale per chunk, is added."""
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

#        id                L  lv     M    K   B    layout mode_vi K_total ns   tail
CASES = {"rows_K5":       (2, True,  32,  5,  40,  "bk", False, 9,    1, "rows"),
         "rows_kb":       (1, True,  32,  4,  37,  "kb", False, 0,    1, "rows"),
         "rows_vi":       (2, False, 32,  4,  37,  "kb", True,  0,    1, "rows"),
         "local_K4":      (2, True,  32,  4,  37,  "bk", False, 11,   1, "local"),
         "local_K16":     (1, False, 32,  16, 5,   "bk", False, 0,    1, "local"),
         "packed_K40":    (1, False, 32,  40, 420, "bk", False, 0,    5, "packed"),
         "packed_K8":     (1, True,  32,  8,  520, "bk", False, 0,    2, "packed"),
         "packed_K8_ms":  (2, False, 32,  8,  520, "bk", False, 13,   2, "packed")}


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _variant():
    from dgps_with_iwvi_amd import _abi
    return int(_abi.lib().iwvi_debug_last_forward_variant())


_MODELS = {}


def _model(dev, L, lv, M, K, B):
    """A small synthetic model with a wide dynamic range of log-weights, its injected noise in the [B, K] layout (built once per shape)."""
    key = (L, lv, M, K, B)
    if key not in _MODELS:
        from dgps_with_iwvi_amd import synthetic
        spec = synthetic.make_spec(L=L, M=M, B=B, K=K, with_lv=lv, seed=5 + K, n_data=max(4 * B, 64))
        spec["lik_var"] = 1e-3
        Y = np.array(spec["Y"], copy=True)
        Y[::7] += 2.0; Y[3::11] -= 1.0                            # a few outliers
        spec["Y"] = Y
        _MODELS[key] = (synthetic.build_model(spec, dev), synthetic.make_noise(spec, seed=6), spec)
    return _MODELS[key]


def _forward(model, zs, K, B, layout, mode_vi, K_total, dev, **kw):
    """-> (logw [B, K] float64, (elbo, logp, ms), outs)."""
    T = B * K
    model.precompute(with_encoders=True)
    el = dict(B=B, K=K, mode_vi=mode_vi, want_ms=not mode_vi, K_total=K_total or None, **kw.pop("elbo_extra", {}))
    if layout == "bk":
        zd = None if zs is None else [_t(z.reshape(T, -1), dev) for z in zs]
        logw, outs, red = model._fused_forward(T, K, B, (T,), zs=zd, sampled_kl=not mode_vi, elbo=dict(el, stride_b=K, stride_k=1), **kw)
        lw = _np(logw).reshape(B, K)
    else:                                                        # rows t = k B + b (the VI tiling, models.py:50)
        zd = [_t(np.asarray(z).transpose(1, 0, 2).reshape(T, -1), dev) for z in zs]
        logw, outs, red = model._fused_forward(T, 1, B, (T,), zs=zd, sampled_kl=not mode_vi, elbo=dict(el, stride_b=1, stride_k=B), **kw)
        lw = _np(logw).reshape(K, B).T
    return lw, red, outs


def _check(lw, red, K, K_total, mode_vi, what):
    el, lp, ms = float(red[0].item()), _np(red[1]), (None if red[2] is None else _np(red[2]))
    assert np.all(np.isfinite(lw)) and np.all(np.isfinite(lp)), what
    ref = R.logp(lw, K_total or K, mode_vi)
    tol = R.tol_vi(lw) if mode_vi else R.tol_reduce(lw, K_total or K)
    err = np.abs(lp - ref)
    print("%s: |L| up to %.3g, range within a point up to %.3g; logp max err %.3e (allowed %.3e at that point)"
          % (what, np.abs(lw).max(), (lw.max(1) - lw.min(1)).max(), err.max(), tol[int(np.argmax(err))]))
    assert np.all(err <= tol), (what, float((err / tol).max()))
    if ms is not None:
        assert np.array_equal(ms[:, 0], lw.max(1)), what
        assert np.all(np.abs(ms[:, 0] + np.log(ms[:, 1]) - math.log(K_total or K) - ref) <= tol), what
    return el, lp


def _kl_terms(model):
    return [_np(g).reshape(-1) for g in model._global_kls()]


def _bound_err(el, lp, model, B, packed_chunks=0):
    """|bound - (scale sum logp_device - kl)| and what the exact rule allows (``packed_chunks``: + the fixed point's resolution when
    some |logp| < 8 is not a multiple of 2^-20)."""
    scale, kls = float(model.num_data) / B, _kl_terms(model)
    want = R.bound(lp, scale, kls)
    tol = R.bound_tol(lp, scale) + sum(k.size for k in kls) * 2.0 ** -52 * sum(float(np.abs(k).sum()) for k in kls)
    if packed_chunks and np.abs(lp).min() < 8.0:
        tol += packed_chunks * 2.0 ** -21 * scale
    return abs(el - want), tol, scale


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_tail_against_the_float64_reduction_of_its_own_logw(gpu_device, case):
    L, lv, M, K, B, layout, mode_vi, Kt, ns, tail = CASES[case]
    model, zs, _ = _model(gpu_device, L, lv, M, K, B)
    words = model._words()
    lw, red, _ = _forward(model, zs, K, B, layout, mode_vi, Kt, gpu_device)
    v = _variant()
    assert v & 0xff == ns and not (v >> 10) & 3, hex(v)           # the generic variant at the chunk size the case was chosen for
    el, lp = _check(lw, red, K, Kt, mode_vi, case)
    chunks = (B * K + 16 * ns - 1) // (16 * ns)
    err, tol, scale = _bound_err(el, lp, model, B, chunks if tail == "packed" else 0)
    print("%s: bound off the float64 sum of the published logp by %.3e (exact rule %.3e; %d chunks)" % (case, err, tol, chunks))
    if tail == "packed":
        assert chunks <= 511 and 2 * chunks <= (B * K + 15) // 16   # the host's conditions for the packed arrival
    assert err <= tol, (case, err, tol)
    assert int(words[2].item()) == 0                              # the arrival word is left at zero
    lw2, red2, _ = _forward(model, zs, K, B, layout, mode_vi, Kt, gpu_device)
    assert np.array_equal(lw, lw2) and float(red2[0].item()) == el and torch.equal(red2[1], red[1]), case
    if tail == "packed":                                         # the same launch through the stored partials: the per-point results bit for bit
        from dgps_with_iwvi_amd import _abi
        _abi.set_debug_option("IWVI_FW_SLOW_TAIL", 1)
        try:
            lw3, red3, _ = _forward(model, zs, K, B, layout, mode_vi, Kt, gpu_device)
        finally:
            _abi.set_debug_option("IWVI_FW_SLOW_TAIL", 0)
        assert np.array_equal(lw, lw3) and torch.equal(red3[1], red[1]) and torch.equal(red3[2], red[2]), case
        err3, tol3, _ = _bound_err(float(red3[0].item()), _np(red3[1]), model, B)
        assert err3 <= tol3, (case, err3, tol3)                   # ... and their sum exact


LEAN = dict(L=2, lv=True, M=128, K=20)


def _lean_model(dev, B):
    from dgps_with_iwvi_amd import synthetic
    key = ("lean", B)
    if key not in _MODELS:
        spec = synthetic.make_spec(L=2, M=128, B=B, K=20, with_lv=True, seed=2, n_data=4 * B)
        spec["lik_var"] = 1e-3
        Y = np.array(spec["Y"], copy=True)
        Y[::7] += 2.0
        spec["Y"] = Y
        _MODELS[key] = synthetic.build_model(spec, dev)
    return _MODELS[key]


def test_lean_and_shaped_variants(gpu_device):
    """M = 128, K = 20, device-drawn noise.  B = 40 does not reach the shaped variants (ns = 1); B = 820 does: bound-only -> LEAN (bit 10),
    with per-layer outputs -> the shaped variant with the general tail (bit 11)."""
    small = _lean_model(gpu_device, 40)
    lw, red, _ = _forward(small, None, 20, 40, "bk", False, 0, gpu_device)
    assert _variant() & 0xff == 1 and not (_variant() >> 10) & 3, hex(_variant())
    el, lp = _check(lw, red, 20, 0, False, "M=128 B=40")
    err, tol, _ = _bound_err(el, lp, small, 40)
    assert err <= tol, (err, tol)                                # (the row loop: 20 does not divide 16)
    model = _lean_model(gpu_device, 820)
    lw, red, _ = _forward(model, None, 20, 820, "bk", False, 0, gpu_device)
    assert _variant() & 0xff == 5 and (_variant() >> 10) & 3 == 1, hex(_variant())
    el, lp = _check(lw, red, 20, 0, False, "lean")
    err, tol, scale = _bound_err(el, lp, model, 820, 205)
    print("lean: bound off the float64 sum of the published logp by %.3e (exact rule %.3e; 205 chunks)" % (err, tol))
    assert err <= tol, (err, tol)
    lw, red, _ = _forward(model, None, 20, 820, "bk", False, 23, gpu_device, want_layers=True)
    assert _variant() & 0xff == 5 and (_variant() >> 10) & 3 == 2, hex(_variant())
    el, lp = _check(lw, red, 20, 23, False, "shaped, general tail")
    err, tol, scale = _bound_err(el, lp, model, 820, 205)
    assert err <= tol, (err, tol)
    assert int(model._words()[2].item()) == 0                     # the arrival word is left at zero


def test_fused_heads_are_refused_where_the_scratch_has_one_slot_per_chunk(gpu_device):
    from dgps_with_iwvi_amd import _abi
    L, lv, M, K, B = CASES["local_K4"][:5]
    model, zs, _ = _model(gpu_device, L, lv, M, K, B)
    T = B * K
    adj = dict(w=torch.empty(T, device=gpu_device), d_mean=torch.empty(T, 1, device=gpu_device), d_var=torch.empty(T, 1, device=gpu_device),
               sums=torch.empty(3, dtype=torch.float64, device=gpu_device))
    with pytest.raises(_abi.IwviError) as e:
        _forward(model, zs, K, B, "bk", False, 0, gpu_device, want_layers=True, elbo_extra=dict(adj=adj))
    assert e.value.rc == _abi.ERR_UNSUPPORTED


@pytest.mark.parametrize("case", ["packed_K8", "packed_K8_ms", "shaped"])
def test_fused_heads_against_the_float64_softmax_of_the_launch_logw(gpu_device, case):
    """adj_w / adj_dmean / adj_dvar / adj_sums from the launch's tail: w under the weight rule (tol_L = 0: the log-weights are the
    launch's own), the sums from the reference, and iwvi_iw_elbo_backward on the final moments of the same launch (the fuse_heads=False
    route) at the route comparison's tolerance (5e-3 of each array's largest entry, tests/test_gpu_likelihoods.py)."""
    import ctypes
    from dgps_with_iwvi_amd import _abi
    if case == "shaped":
        K, B, model, zs = 20, 820, _lean_model(gpu_device, 820), None
    else:
        L, lv, M, K, B = CASES[case][:5]
        model, zs, _ = _model(gpu_device, L, lv, M, K, B)
    T, dev = B * K, gpu_device
    adj = dict(w=torch.full((T,), float("nan"), device=dev), d_mean=torch.full((T, 1), float("nan"), device=dev),
               d_var=torch.full((T, 1), float("nan"), device=dev), sums=torch.full((3,), float("nan"), dtype=torch.float64, device=dev))
    lw, red, outs = _forward(model, zs, K, B, "bk", False, 0, dev, want_layers=True, elbo_extra=dict(adj=adj))
    v = _variant()
    assert (v >> 10) & 3 == (2 if case == "shaped" else 0) and v & 0xff == (5 if case == "shaped" else CASES[case][8]), hex(v)
    el, lp = _check(lw, red, K, 0, False, case + " heads")
    scale = float(model.num_data) / B
    lik_var = float(np.float32(model.likelihood.variance))
    fm, fv = _np(outs[-1]["mean"]).reshape(B, K, 1), _np(outs[-1]["var"]).reshape(B, K, 1)
    Y = _np(model.Y)
    wr, dmr, dvr, dlr = R.heads(lw, fm, fv, Y, lik_var, scale)
    w, dm, dv, sums = _np(adj["w"]).reshape(B, K), _np(adj["d_mean"]).reshape(B, K, 1), _np(adj["d_var"]).reshape(B, K, 1), _np(adj["sums"])
    tw = R.tol_w(wr, scale, np.zeros(B))
    print("%s: w max err %.3e, max err / allowed %.3f" % (case, np.abs(w - wr).max(), (np.abs(w - wr) / tw).max()))
    assert np.all(np.abs(w - wr) <= tw)
    assert np.all(np.abs(w.sum(1) - scale) <= K * 2.0 ** -23 * scale)
    rel = (tw / np.maximum(wr, 1e-300))[..., None] + 4 * 2.0 ** -23
    assert np.all(np.abs(dm - dmr) <= np.abs(dmr) * rel + 1e-30 / lik_var * np.abs(Y[:, None, :] - fm))
    assert np.all(np.abs(dv - dvr) <= np.abs(dvr) * rel + 1e-30 / lik_var)
    e = Y[:, None, :] - fm
    term = np.abs(-0.5 / lik_var + 0.5 * (e * e + fv) / lik_var ** 2)
    assert abs(sums[1] - dlr) <= float(((tw[..., None] + 2.0 ** -23 * wr[..., None]) * term).sum())
    assert sums[0] == math.fsum(lp.tolist()) or abs(sums[0] - math.fsum(lp.tolist())) <= B * 2.0 ** -52 * np.abs(lp).sum()
    kl = math.fsum(x for k in _kl_terms(model) for x in k)
    assert abs(sums[2] - (scale * sums[0] - kl)) <= 4 * 2.0 ** -52 * (abs(scale * sums[0]) + abs(kl)) and sums[2] == el
    # the two-launch route on the same final moments
    tm, tv = outs[-1]["mean"].reshape(T, 1).contiguous(), outs[-1]["var"].reshape(T, 1).contiguous()
    kls = [o["kl_local"].reshape(T, -1).contiguous() for o in outs if o is not None and "kl_local" in o]
    kd = (ctypes.c_int32 * max(len(kls), 1))(*[k.shape[1] for k in kls])
    glob = [g.reshape(-1) for g in model._global_kls()]
    gn = (ctypes.c_int32 * max(len(glob), 1))(*[g.numel() for g in glob])
    w2, dm2, dv2 = torch.empty(T, device=dev), torch.empty(T, 1, device=dev), torch.empty(T, 1, device=dev)
    sums2, ws = torch.empty(3, dtype=torch.float64, device=dev), torch.empty(2 * B, dtype=torch.float64, device=dev)
    _abi.check(_abi.lib().iwvi_iw_elbo_backward(_abi.ptr(tm), _abi.ptr(tv), _abi.ptr(model.Y), 1, _abi.ptr_array(kls), kd, len(kls), B, K, lik_var, scale, 0,
                                                _abi.ptr(w2), _abi.ptr(dm2), _abi.ptr(dv2), _abi.ptr_array(glob), gn, len(glob), None, K,
                                                _abi.ptr(sums2), _abi.ptr(ws), _abi.stream_ptr()))
    for nm, a, b in (("w", adj["w"], w2), ("d_mean", adj["d_mean"], dm2), ("d_var", adj["d_var"], dv2), ("sums", adj["sums"], sums2)):
        a, b = _np(a).reshape(-1), _np(b).reshape(-1)
        assert np.abs(a - b).max() <= 5e-3 * np.abs(b).max(), (case, nm, float(np.abs(a - b).max()), float(np.abs(b).max()))
