"""The encoder MLP at its four kernel sites (tests/encoder_cases.py: A layer kernel per sample, B layer kernel per data point, C precompute
launch with its sampling tail, D adjoint) against the float64 restatement, for every case of the table on every site it applies to.

Bounds: ``encoder_cases.bound`` = 8 x the case's recorded float32-versus-float64 error + 1e-6 x max |reference| (gradients: the same,
relative to each tensor's maximum).  Bit-for-bit checks only where two paths run the same instruction stream on the same inputs: the Philox
draws of site C's sampling tail against the layer kernel's, the copied X columns, and site C with and without ``sample_z``.  The draws
are also held to ``philox_reference.layer_normal``, which shares no code with either kernel.  Every
comparison prints its error / bound ratio before it asserts; ``test_error_ratios_report`` prints the largest per site."""
import ctypes

import numpy as np
import pytest
import torch

import encoder_cases as ec
import philox_reference as pr

pytestmark = pytest.mark.gpu

CANARY = -7.25e11                                                # an exact float32 no result comes near
PAD = 64                                                         # canary floats on either side of every output buffer
SEED, STEP = (7 << 32) | 12345, 5                                # Philox key (both halves in use) and evaluation number of the sampling tail
# as tests/test_gpu_fill_normal.py: tells streams apart (a wrong counter, key or quad moves a draw by O(1)); the hardware log2 / sin / cos
# leave ~3e-7 between the device and the float64 restatement
STREAM_ATOL = 1e-4
RATIOS = {}                                                      # site -> (largest error / bound, where)

_ALL = pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.id)
_FIT_C = pytest.mark.parametrize("case", [c for c in ec.CASES if ec.expect(c.id, "C") == "evaluate"], ids=lambda c: c.id)
_OVER_C = pytest.mark.parametrize("case", [c for c in ec.CASES if ec.expect(c.id, "C") == "refuse"], ids=lambda c: c.id)


def _dev(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)


def _np(t):
    return t.detach().double().cpu().numpy()


def _check(site, what, got, ref, limit):
    """max |got - ref| against ``limit``; the ratio is printed and kept for the report before the assertion."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(ref).all(), what
    err = float(np.abs(got - ref).max()) if np.isfinite(got).all() else float("inf")
    ratio = err / limit
    print("%s %-44s err %.3e bound %.3e ratio %.3f" % (site, what, err, limit, ratio))
    if ratio >= RATIOS.get(site, (0.0, ""))[0]:
        RATIOS[site] = (ratio, what)
    assert err <= limit, "%s %s: max error %.3e > bound %.3e" % (site, what, err, limit)


class _Guarded:
    """An output buffer with PAD canary floats in front of it and behind it, itself filled with the canary."""

    def __init__(self, shape, dev):
        self.n = int(np.prod(shape))
        self.full = torch.full((self.n + 2 * PAD,), CANARY, dtype=torch.float32, device=dev)
        self.t = self.full[PAD:PAD + self.n].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def pads_intact(self):
        return bool((self.full[:PAD] == CANARY).all()) and bool((self.full[PAD + self.n:] == CANARY).all())

    def untouched(self):
        return bool((self.full == CANARY).all())


_INPUTS, _REF = {}, {}


def _inputs(case):
    if case.id not in _INPUTS:
        inp = ec.make_inputs(case)
        _INPUTS[case.id] = inp
        _REF[case.id] = ec.mlp(inp["XY"], inp["Ws"], inp["bs"], case.dims, case.act)       # computed once, read-only
        _REF[case.id].setflags(write=False)
    return _INPUTS[case.id], _REF[case.id]


def _encoder(case, dev):
    """The library's Encoder with the case's weights; ``bs = None`` / entries None are the missing biases."""
    from dgps_with_iwvi_amd.layers import Encoder
    inp, _ = _inputs(case)
    enc = Encoder(ec.latent_dim(case), case.dims[0], list(case.dims[1:-1]), activation_func=case.act)
    enc.Ws = [_dev(w, dev) for w in inp["Ws"]]
    enc.bs = None if inp["bs"] is None else [None if b is None else _dev(b, dev) for b in inp["bs"]]
    return enc


# ---- site A ---------------------------------------------------------------------------------------------------------------------------
def _run_a(case, dev, rows, sampled):
    from dgps_with_iwvi_amd.layers import LatentVariableLayer
    inp, _ = _inputs(case)
    lv = LatentVariableLayer(ec.latent_dim(case), encoder=_encoder(case, dev))
    s, m, v, kl = lv.propagate(_dev(inp["F"][:rows], dev), _dev(inp["XY"][:rows], dev), bool(sampled), z=_dev(inp["z"][:rows], dev))
    return _np(s), _np(m), _np(v), _np(kl)


@_ALL
def test_site_a_layer_kernel_one_row_per_sample(gpu_device, case):
    inp, ref = _inputs(case)
    e, Lw = ec.ERR32[case.id], ec.latent_dim(case)
    enc = _encoder(case, gpu_device)
    for rows in ec.A_ROWS:
        out = ref[:rows]
        q_mu, q_sqrt = enc(_dev(inp["XY"][:rows], gpu_device))
        _check("A", "%s rows=%d q_mu" % (case.id, rows), _np(q_mu), out[:, :Lw], ec.bound(e["out"], out[:, :Lw]))
        sg = np.logaddexp(0.0, out[:, Lw:] - 3.0)
        _check("A", "%s rows=%d q_sqrt" % (case.id, rows), _np(q_sqrt), sg, ec.bound(e["sg"], sg))
        for sampled in (0, 1):
            got = _run_a(case, gpu_device, rows, sampled)
            want = ec.lv_tail(out, inp["F"][:rows], inp["z"][:rows], sampled)
            for name, key, g, w in zip(("sample", "mean", "var", "kl"), ("sample", "out", "var", "kl"), got, want):
                _check("A", "%s rows=%d skl=%d %s" % (case.id, rows, sampled, name), g, w, ec.bound(e[key], w))


# ---- site B ---------------------------------------------------------------------------------------------------------------------------
def _run_b(case, dev, sampled):
    """iwvi_dgp_forward as a model calls it: B_POINTS data points, B_SAMPLES samples each (row t reads data row t // K), the weights in the
    descriptor.  -> the layer's exported sample, mean, var [T, D + Lw] and kl [T, Lw]."""
    from dgps_with_iwvi_amd import _abi
    from dgps_with_iwvi_amd.layers import LatentVariableLayer
    inp, _ = _inputs(case)
    Bp, K, D, Lw = ec.B_POINTS, ec.B_SAMPLES, ec.layer_width(case), ec.latent_dim(case)
    T = Bp * K
    lv = LatentVariableLayer(Lw, encoder=_encoder(case, dev))
    X, XY, z = _dev(inp["F"][:Bp], dev), _dev(inp["XY"][:Bp], dev), _dev(inp["z"][:T], dev)
    outs = {k: _Guarded((T, D + Lw), dev) for k in ("sample", "mean", "var")}
    outs["kl_local"] = _Guarded((T, Lw), dev)
    d, keep = lv.fused_desc(D, z=z, outputs={k: g.t for k, g in outs.items()}, sampled_kl=bool(sampled), draw=False)
    _abi.check(_abi.lib().iwvi_dgp_forward((_abi.LayerDesc * 1)(d), 1, _abi.ptr(X), D, _abi.ptr(XY), XY.shape[1], None, 0, T, K, Bp,
                                           1.0, 0, None, None, None, _abi.stream_ptr()))
    torch.cuda.synchronize()
    assert all(g.pads_intact() for g in outs.values())
    return tuple(_np(outs[k].t) for k in ("sample", "mean", "var", "kl_local"))


@_ALL
def test_site_b_layer_kernel_one_row_per_data_point(gpu_device, case):
    inp, ref = _inputs(case)
    e, Bp, K = ec.ERR32[case.id], ec.B_POINTS, ec.B_SAMPLES
    rep = lambda a: np.repeat(a[:Bp], K, axis=0)
    for sampled in (0, 1):
        got = _run_b(case, gpu_device, sampled)
        want = ec.lv_tail(rep(ref), rep(inp["F"]), inp["z"][:Bp * K], sampled)
        for name, key, g, w in zip(("sample", "mean", "var", "kl"), ("sample", "out", "var", "kl"), got, want):
            _check("B", "%s skl=%d %s" % (case.id, sampled, name), g, w, ec.bound(e[key], w))


# ---- site C ---------------------------------------------------------------------------------------------------------------------------
_GP = {}


def _gp_desc(dev):
    """The smallest GP layer: iwvi_model_precompute wants one beside the encoders."""
    if "d" not in _GP:
        from dgps_with_iwvi_amd import kernels, settings
        from dgps_with_iwvi_amd.temp_workaround import GpState
        rng = np.random.default_rng(0)
        M, D, R = 16, 2, 1
        st = GpState(M, R, dev)
        keep = (_dev(rng.standard_normal((M, D)), dev), kernels.RBF(D, variance=1.0, lengthscales=np.ones(D, np.float32)).to(dev),
                _dev(rng.standard_normal((M, R)), dev), _dev(np.eye(M)[None], dev))
        _GP["d"], _GP["keep"] = st.desc(keep[0], keep[1], keep[2], keep[3], settings.jitter_level), (st, keep)
    return _GP["d"]


class _SiteC:
    """One encoder descriptor of a precompute launch with guarded outputs; ``tail``: also the sampling tail (K, sampled_kl, want_z)."""

    def __init__(self, case, dev, rows, tail=None, words=None):
        from dgps_with_iwvi_amd import _abi
        inp, _ = _inputs(case)
        self.case, self.rows, Lw = case, rows, ec.latent_dim(case)
        self.enc = _encoder(case, dev)
        self.XY = _dev(inp["XY"][:rows], dev)
        self.out = _Guarded((rows, 2 * Lw), dev)
        Wp, bp, dims, n, keep = self.enc.abi_args()
        e = _abi.EncDesc()
        e.XY, e.rows, e.enc_W, e.enc_b, e.dims, e.n_enc = self.XY.data_ptr(), rows, Wp, bp, dims, n
        e.latent_dim, e.out, e.act = Lw, self.out.ptr(), self.enc.act
        self.keep, self.bufs = (Wp, bp, dims, keep), [self.out]
        self.smp_X = self.smp_kl = self.smp_z = None
        if tail is not None:
            K, Dx = tail["K"], ec.layer_width(case)
            self.X = _dev(inp["F"][:rows], dev)
            self.smp_X, self.smp_kl = _Guarded((rows * K, Dx + Lw), dev), _Guarded((rows * K,), dev)
            self.bufs += [self.smp_X, self.smp_kl]
            e.X, e.Dx, e.K, e.sampled_kl, e.layer_index = self.X.data_ptr(), Dx, K, tail["sampled_kl"], 0
            e.seed, e.rng_state = SEED, words.data_ptr() + 8
            self.keep += (words,)                               # the launch reads the step from it: it lives as long as the descriptor
            e.sample_X, e.sample_kl = self.smp_X.ptr(), self.smp_kl.ptr()
            if tail["want_z"]:
                self.smp_z = _Guarded((rows * K, Lw), dev)
                self.bufs.append(self.smp_z)
                e.sample_z = self.smp_z.ptr()
        self.desc = e


def _words(dev):
    w = torch.zeros(4, dtype=torch.int64, device=dev)             # [ticket, rng step, rng ticket, -] as a model keeps them
    w[1] = STEP
    return w


def _precompute(dev, encs):
    """-> (status, message) of one iwvi_model_precompute call with the small GP layer and these encoder descriptors."""
    from dgps_with_iwvi_amd import _abi
    arr = (_abi.GpDesc * 1)(_gp_desc(dev))
    earr = (_abi.EncDesc * len(encs))(*[s.desc for s in encs])
    rc = _abi.lib().iwvi_model_precompute(arr, 1, earr, len(encs), _abi.stream_ptr())
    msg = _abi.lib().iwvi_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    return rc, msg


def _check_c_out(s, tag):
    _, ref = _inputs(s.case)
    want = ref[:s.rows]
    assert all(b.pads_intact() for b in s.bufs), tag
    got = _np(s.out.t)
    blocks = sorted({0, s.rows - 1} | {r for b in range(0, s.rows, 256) for r in (b, min(b + 255, s.rows - 1))})
    assert np.isfinite(got[blocks]).all() and (got[blocks] != CANARY).all(), tag      # first and last row of every 256-row block are written
    _check("C", "%s out" % tag, got, want, ec.bound(ec.ERR32[s.case.id]["out"], want))


@_FIT_C
def test_site_c_precompute_launch_output(gpu_device, case):
    for rows in ec.C_ROWS:
        s = _SiteC(case, gpu_device, rows)
        rc, msg = _precompute(gpu_device, [s])
        assert rc == 0, msg
        _check_c_out(s, "%s rows=%d" % (case.id, rows))


def _layer_kernel_draws(case, dev, rows, K):
    """The draws the in-kernel layer exports (noise_out) for the same seed, step and layer index, and its sample rows."""
    from dgps_with_iwvi_amd import _abi
    from dgps_with_iwvi_amd.layers import LatentVariableLayer
    inp, _ = _inputs(case)
    D, Lw, T = ec.layer_width(case), ec.latent_dim(case), rows * K
    lv = LatentVariableLayer(Lw, encoder=_encoder(case, dev))
    X, XY = _dev(inp["F"][:rows], dev), _dev(inp["XY"][:rows], dev)
    noise, sample = _Guarded((T, Lw), dev), _Guarded((T, D + Lw), dev)
    d, keep = lv.fused_desc(D, z=None, outputs=dict(noise_out=noise.t, sample=sample.t), sampled_kl=True, draw=True)
    words = _words(dev)
    _abi.check(_abi.lib().iwvi_dgp_forward((_abi.LayerDesc * 1)(d), 1, _abi.ptr(X), D, _abi.ptr(XY), XY.shape[1], None, 0, T, K, rows,
                                           1.0, SEED, ctypes.c_void_p(words.data_ptr() + 8), None, None, _abi.stream_ptr()))
    torch.cuda.synchronize()
    assert noise.pads_intact() and sample.pads_intact()
    return noise.t.clone(), sample.t.clone()


@_FIT_C
def test_site_c_sampling_tail(gpu_device, case):
    inp, ref = _inputs(case)
    e, Lw, Dx, K = ec.ERR32[case.id], ec.latent_dim(case), ec.layer_width(case), case.K
    for rows in (ec.C_ROWS[2], ec.C_ROWS[3]) if case.K == 3 else ec.C_ROWS:
        tag = "%s rows=%d K=%d skl=%d" % (case.id, rows, K, case.sampled_kl)
        runs = {}
        for want_z in (True, False):
            s = _SiteC(case, gpu_device, rows, tail=dict(K=K, sampled_kl=case.sampled_kl, want_z=want_z), words=_words(gpu_device))
            rc, msg = _precompute(gpu_device, [s])
            assert rc == 0, msg
            _check_c_out(s, tag)
            runs[want_z] = s
        s, s0 = runs[True], runs[False]
        # without sample_z: the same bits everywhere else
        for a, b in ((s.out, s0.out), (s.smp_X, s0.smp_X), (s.smp_kl, s0.smp_kl)):
            assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)), tag
        # the draws: the layer kernel's stream for (seed, step, layer 0, sample, quad), bit for bit
        z_k, _ = _layer_kernel_draws(case, gpu_device, rows, K)
        assert torch.equal(s.smp_z.t.view(torch.int32), z_k.view(torch.int32)), tag
        z = _np(s.smp_z.t)
        # ... and a restatement of that stream which shares no code with draw_normal4 (the quad handling for Lw % 4 != 0 included)
        z_ref = pr.layer_normal(SEED, STEP, 0, np.arange(rows * K), Lw)
        assert z.shape == z_ref.shape and np.abs(z - z_ref).max() <= STREAM_ATOL, (tag, np.abs(z - z_ref).max())
        assert np.isfinite(z).all() and abs(z.mean()) < 5.0 / np.sqrt(z.size) and abs(z.std() - 1.0) < 5.0 / np.sqrt(2 * z.size), tag
        # X columns: copied row for row
        X_rep = s.X.repeat_interleave(K, dim=0)
        assert torch.equal(s.smp_X.t[:, :Dx].contiguous().view(torch.int32), X_rep.contiguous().view(torch.int32)), tag
        # latent columns and the regulariser from the exported draws, in float64
        rep = lambda a: np.repeat(a[:rows], K, axis=0)
        sample, _, _, kl = ec.lv_tail(rep(ref), rep(inp["F"]), z, case.sampled_kl)
        _check("C", "%s sample_X[:, Dx:]" % tag, _np(s.smp_X.t)[:, Dx:], sample[:, Dx:], ec.bound(e["sample"], sample[:, Dx:]))
        # (the kernel sums the Lw per-dimension terms in float32: ``kl_sum`` is the recorded error of that sum)
        _check("C", "%s sample_kl" % tag, _np(s.smp_kl.t), kl.sum(1), ec.bound(e["kl_sum"], kl.sum(1)))


def test_site_c_two_encoders_in_one_launch(gpu_device):
    for p in ec.PAIRS:
        (a, ra), (b, rb) = p["first"], p["second"]
        sa, sb = _SiteC(ec.BY_ID[a], gpu_device, ra), _SiteC(ec.BY_ID[b], gpu_device, rb)
        rc, msg = _precompute(gpu_device, [sa, sb])
        assert rc == 0, msg
        _check_c_out(sa, "%s first %s rows=%d" % (p["id"], a, ra))
        _check_c_out(sb, "%s second %s rows=%d" % (p["id"], b, rb))
        # and the other way round: the second encoder's block offset follows a single, short block
        sa, sb = _SiteC(ec.BY_ID[a], gpu_device, ra), _SiteC(ec.BY_ID[b], gpu_device, rb)
        rc, msg = _precompute(gpu_device, [sb, sa])
        assert rc == 0, msg
        _check_c_out(sb, "%s first %s rows=%d" % (p["id"], b, rb))
        _check_c_out(sa, "%s second %s rows=%d" % (p["id"], a, ra))


# ---- site D ---------------------------------------------------------------------------------------------------------------------------
def _run_d(case, dev, rows):
    """iwvi_encoder_backward_act -> (dW list, db list (None where the bias is missing)).
    The contract for a missing bias: the caller has no parameter there, so it hands over no destination (``db == NULL`` with
    ``enc_b == NULL``, ``db[l] == NULL`` with ``enc_b[l] == NULL``), and the call then writes no db for that layer: the reduction skips a
    null destination, and every buffer that WAS handed over keeps its guards.  (A destination handed over all the same would receive the
    column sums of that layer's delta, the gradient with respect to the zero that stands in for the bias; no caller of the library does.)"""
    from dgps_with_iwvi_amd import _abi
    inp, _ = _inputs(case)
    enc = _encoder(case, dev)
    Wp, bp, dims, n, keep = enc.abi_args()
    XY, d_out = _dev(inp["XY"][:rows], dev), _dev(inp["d_out"][:rows], dev)
    dW = [_Guarded(tuple(w.shape), dev) for w in enc.Ws]
    db = None if enc.bs is None else [None if b is None else _Guarded(tuple(b.shape), dev) for b in enc.bs]
    dWp = _abi.ptr_array([g.t for g in dW])
    dbp = None if db is None else _abi.ptr_array([None if g is None else g.t for g in db])
    ws = torch.empty(_abi.lib().iwvi_encoder_backward_ws_bytes(rows, dims, n), dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().iwvi_encoder_backward_act(_abi.ptr(XY), rows, Wp, bp, dims, n, enc.act, _abi.ptr(d_out), dWp, dbp,
                                                    ws.data_ptr(), _abi.stream_ptr()))
    torch.cuda.synchronize()
    guards = dW + [g for g in (db or []) if g is not None]
    assert all(g.pads_intact() for g in guards)
    return [_np(g.t) for g in dW], [None] * n if db is None else [None if g is None else _np(g.t) for g in db]


@_ALL
def test_site_d_adjoint(gpu_device, case):
    inp, _ = _inputs(case)
    rel = 8.0 * ec.ERR32[case.id]["grad"] + 1e-6                 # ``bound`` relative to each tensor's maximum
    for rows in ec.A_ROWS:
        rW, rb = ec.mlp_grads(inp["XY"][:rows], inp["Ws"], inp["bs"], case.dims, case.act, inp["d_out"][:rows])
        gW, gb = _run_d(case, gpu_device, rows)
        for l, (g, r) in enumerate(zip(gW + gb, rW + rb)):
            name = "%s rows=%d %s%d" % (case.id, rows, "dW" if l < len(gW) else "db", l % len(gW))
            assert (g is None) == (r is None), name              # a missing bias: no db buffer was handed over, none is compared
            if r is not None:
                m = np.abs(r).max()
                _check("D", name, g, r, rel * (m if m > 0 else 1.0))


# ---- A, B and C run the same MLP in float32 ---------------------------------------------------------------------------------------------
@_ALL
def test_sites_agree_with_each_other(gpu_device, case):
    _, ref = _inputs(case)
    e, Lw, D = ec.ERR32[case.id], ec.latent_dim(case), ec.layer_width(case)
    rows = ec.A_ROWS[-1]
    _, mean_a, var_a, _ = _run_a(case, gpu_device, rows, 1)
    _, mean_b, var_b, _ = _run_b(case, gpu_device, 1)
    mu_tol, var_tol = 2.0 * ec.bound(e["out"], ref[:, :Lw]), 2.0 * ec.bound(e["var"], np.logaddexp(0.0, ref[:, Lw:] - 3.0) ** 2)
    pts = slice(0, ec.B_POINTS * ec.B_SAMPLES, ec.B_SAMPLES)     # site B's first sample of each data point
    _check("ABC", "%s mu A vs B" % case.id, mean_a[:ec.B_POINTS, D:], mean_b[pts, D:], mu_tol)
    _check("ABC", "%s var A vs B" % case.id, var_a[:ec.B_POINTS, D:], var_b[pts, D:], var_tol)
    if ec.expect(case.id, "C") != "evaluate":                    # (beyond site C's LDS: A against B is all there is)
        return
    s = _SiteC(case, gpu_device, ec.C_ROWS[0])
    rc, msg = _precompute(gpu_device, [s])
    assert rc == 0, msg
    out_c = _np(s.out.t)
    _check("ABC", "%s mu A vs C" % case.id, mean_a[:, D:], out_c[:rows, :Lw], mu_tol)
    _check("ABC", "%s mu B vs C" % case.id, mean_b[pts, D:], out_c[:ec.B_POINTS, :Lw], mu_tol)


# ---- beyond site C's LDS ----------------------------------------------------------------------------------------------------------------
def _hip_last_errors():
    """hipGetLastError() of every HIP runtime mapped into this process (it also clears the state it reports)."""
    paths = set()
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                paths.add(line.split()[-1])
    assert paths
    out = []
    for p in sorted(paths):
        fn = ctypes.CDLL(p).hipGetLastError
        fn.restype = ctypes.c_int
        out.append(int(fn()))
    return out


@_OVER_C
def test_beyond_site_c_is_refused_before_any_launch_and_nothing_sticks(gpu_device, case):
    from dgps_with_iwvi_amd import _abi
    need = ec.LDS[case.id][0]
    assert need > ec.LDS_LIMIT
    torch.cuda.synchronize()
    _hip_last_errors()
    for tail in (None, dict(K=2, sampled_kl=1, want_z=True)):
        s = _SiteC(case, gpu_device, ec.C_ROWS[2], tail=tail, words=_words(gpu_device))
        rc, msg = _precompute(gpu_device, [s])
        print("C %s: status %d, %r" % (case.id, rc, msg))
        assert rc == _abi.ERR_UNSUPPORTED and str(need) in msg and "LDS" in msg, (rc, msg)
        assert s.enc.precompute_lds_bytes() == need and not s.enc.fits_precompute()       # the Python side's copy of the formula names the same bytes
        assert all(b.untouched() for b in s.bufs)
        assert not any(_hip_last_errors())
    # a valid call right after it
    ok = _SiteC(ec.BY_ID["base20"], gpu_device, ec.C_ROWS[2])
    rc, msg = _precompute(gpu_device, [ok])
    assert rc == 0, msg
    _check_c_out(ok, "base20 after the refusal of %s" % case.id)
    # the layer kernel takes it (sites A and B above evaluate it): the plan the table recorded is the plan the driver makes
    a_bytes, b_bytes = ec.AB_PLAN[case.id]
    assert ec.lv_plan(case, ec.A_ROWS[-1], 1, ec.A_ROWS[-1])[1][2] == a_bytes
    assert ec.lv_plan(case, ec.B_POINTS * ec.B_SAMPLES, ec.B_SAMPLES, ec.B_POINTS)[1][2] == b_bytes


def _model_spec(hidden, seed):
    """synthetic's LV + GP stack with the recognition network's hidden layers swapped."""
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=2, M=32, B=12, K=5, Dx=6, R=3, Dy=1, with_lv=True, latent_dim=2, mixing="dense", seed=seed)
    lv = spec["layers"][0]
    assert lv["type"] == "lv"
    rng = np.random.default_rng(seed)
    dims = [lv["dims"][0], *hidden, lv["dims"][-1]]
    lv["dims"] = dims
    lv["enc_W"] = [np.asarray(rng.standard_normal((a, b)) * (2.0 / (a + b)) ** 0.5, np.float32) for a, b in zip(dims[:-1], dims[1:])]
    lv["enc_b"] = [np.asarray(rng.standard_normal(b) * 0.1, np.float32) for b in dims[1:]]
    return spec


@pytest.mark.parametrize("hidden,fits", [((64, 64), True), ((64, 64, 64), False)], ids=["64x64", "64x64x64"])
def test_model_with_a_wide_recognition_network(gpu_device, hidden, fits):
    """A model whose encoder is at (and beyond) what the precompute launch holds still evaluates its bound and its gradients: the encoder
    beyond it goes through the layer kernel.  Tolerances: the suite's stated ones (ELBO 1e-4, beside gradients 2e-4, gradients 5e-3 of each
    tensor's maximum)."""
    from dgps_with_iwvi_amd import backward, synthetic
    from oracle.from_spec import build_oracle, oracle_noise
    from oracle.grad_oracle import iw_elbo_and_gradients
    spec = _model_spec(hidden, seed=61)
    zs = synthetic.make_noise(spec, seed=62)
    model = synthetic.build_model(spec, gpu_device)
    enc = model.layers[0].encoder
    assert enc.fits_precompute() == fits and (enc.precompute_lds_bytes() <= ec.LDS_LIMIT) == fits
    zd = [_dev(z, gpu_device) for z in zs]
    elbo = float(model.compute_log_likelihood(zd))
    ref = build_oracle(spec).build_likelihood(oracle_noise(spec, zs))
    print("model %s: elbo %.9g oracle %.9g rel %.2e" % (hidden, elbo, ref, abs(elbo - ref) / abs(ref)))
    assert np.isfinite(elbo) and abs(elbo - ref) <= 1e-4 * abs(ref), (elbo, ref)
    val, gref = iw_elbo_and_gradients(spec, zs)
    e2, grads = backward.iw_elbo_and_gradients(model, zd)
    torch.cuda.synchronize()
    assert abs(float(e2) - val) <= 2e-4 * abs(val), (float(e2), val)
    assert sorted(grads) == sorted(gref)
    for k, v in grads.items():
        r = np.asarray(gref[k], np.float64)
        g = v.detach().double().cpu().numpy().reshape(r.shape)
        err, scale = np.abs(g - r).max(), max(np.abs(r).max(), 1e-12)
        assert err <= 5e-3 * scale, "%s: max err %.3e vs scale %.3e" % (k, err, scale)
    if fits:
        model.lv_in_precompute = True
        assert model.lv_in_precompute
    else:
        with pytest.raises(ValueError) as ei:                    # refused when it is switched on, with the byte count
            model.lv_in_precompute = True
        assert str(enc.precompute_lds_bytes()) in str(ei.value) and not model.lv_in_precompute


def test_error_ratios_report(gpu_device):
    """Not a check of its own: the largest error / bound ratio each site reached in this run (every ratio was asserted <= 1 above)."""
    for site in sorted(RATIOS):
        print("largest error / bound at site %-3s: %.3f (%s)" % ((site,) + RATIOS[site]))
    assert all(r <= 1.0 for r, _ in RATIOS.values())
