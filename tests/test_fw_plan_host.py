"""The fused forward's host plan (csrc/dgp_forward.hip, ``fw_plan``) against recorded answers, through ``iwvi_debug_forward_plan``.

The entry runs every check and decision of the forward driver -- descriptor translation, stage-2 schedule, LDS fit, packed arrival,
``choose_variant`` -- and returns before the first HIP call, so this runs on a GPU-less host and never launches.  The pointers handed in
are made-up addresses: the plan reads only whether they are null.  ``tests/golden/fw_plan.npz`` holds what the library answered before
the driver was gathered into one plan (recorded by ``scripts/record_fw_plan.py`` from the real entries on a host without a device, where
they plan, set the variant word and then fail at ``hipFuncSetAttribute`` with the LDS bytes in the error text; the launch grid is
``ceil(T / (16 * ns))`` of the recorded ``ns``).  Equality is exact: status, error text of a refusal, variant word, grid, LDS bytes.

The grid (``grid()``, 3 892 cases of which 139 are refusals) is a union of sweeps on both sides of every condition in the plan: M with odd /
even block counts, nbk <= 8 / > 8 / >= 16 and M % 16 != 0; T for every ``ns``, whole and ragged chunks, more than 511 workgroups; stack depth;
input width on both sides of 10; R / P up to the point where the LDS fit drops the solve stream, Z~, then ``ns``; both kernels; the three
layer flags; latent-variable layers without encoder, with ``enc_out`` and with an in-kernel encoder; injected, drawn and zero noise; no
ELBO descriptor, the IW bound with K in 1..40, ``mode_vi``, strided samples, the adjoint heads, ``lw_init``, ``x_per_sample``, more than
64 global KL entries, per-layer outputs; both predictive tails with S that caps ``ns`` to odd values; the three development options.
It reaches all 59 ``k_dgp_forward`` instantiations (59 distinct (tail, word) pairs; 29 distinct words); none is unreachable.

The copy-list cases: a latent-variable layer with an in-kernel encoder of 8 maps puts 16 entries on the prologue's copy list (48 hold).
Two such layers and a GP layer (34 entries) plan as recorded; three (50) and four (66) are refused, where they used to be written past
the list's end."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from dgps_with_iwvi_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fw_plan.npz")

F = 0x10000                    # a made-up, 16-byte aligned, non-null address: never dereferenced
COLS = ("tail", "M", "T", "S", "L", "Dx", "R", "P", "kern", "flags", "lv", "noise", "elbo", "K", "outs", "opt", "bad")
BASE = dict(tail=0, M=128, T=16400, S=0, L=2, Dx=8, R=5, P=8, kern=0, flags=0, lv=0, noise=0, elbo=1, K=8, outs=0, opt=0, bad=0)
# lv: 0 none, 1 leading LV layer with enc_out, 2 with an in-kernel encoder, 3 without encoder (prior mode)
# noise: 0 drawn in the kernel, 1 injected, 2 zero_noise            outs: 1 = the last layer writes its sample (a per-layer output)
# elbo: 0 out_logw without a descriptor, 1 IW bound, 2 mode_vi, 3 strided samples, 4 adjoint heads, 5 lw_init, 6 x_per_sample,
#       7 three global KL arrays of 32 entries (> 64), 8 neither out_logw nor Y (a plain forward)
# tail 1 / 2 (density / samples): T is the number of points N, S the samples per point; noise 1 there = z_y given (samples)
OPTS = (None, ("IWVI_FW_NO_LEAN", 1), ("IWVI_FW_SLOW_TAIL", 1), ("IWVI_FW_MAX_NS", 2))
MS = (16, 32, 48, 112, 120, 128, 144, 240, 256, 272, 512)
TS = (16, 80, 96, 4096, 16400, 16416, 81920)


def _c(**kw):
    d = dict(BASE)
    d.update(kw)
    return tuple(d[k] for k in COLS)


def grid():
    """[n, len(COLS)] int64, one row per case."""
    P = itertools.product
    rows = []
    rows += [_c(M=M, T=T, L=L, flags=f) for M, T, L, f in P(MS, TS, (1, 2, 4), (0, 1, 2))]                      # shape x depth x arithmetic
    rows += [_c(M=M, T=T, kern=1, flags=f, L=L) for M, T, f, L in P((128, 272), TS, (0, 1, 2), (1, 2))]          # Matern52
    rows += [_c(M=M, T=T, flags=f, K=4) for M, T, f in P((112, 128, 144, 256), (4100, 8200, 12300, 16000), (0, 1, 2))]   # ns = 2, 3, 4
    rows += [_c(M=M, T=T, L=L, Dx=Dx, R=R, P=Pp) for M, T, L, Dx, R in P((128, 256, 512), (80, 4096, 81920), (1, 2), (8, 10, 11, 30), (1, 5, 17, 32))
             for Pp in (R, 16, 17, 32)]                                                                        # widths: the LDS fit, SHP's D <= 10 / P <= 16
    rows += [_c(M=M, T=T, L=L, lv=lv, noise=nz) for M, T, L, lv, nz in P((32, 128, 256), (80, 4096, 16400, 81920), (1, 2), (1, 2, 3), (0, 1, 2))]
    rows += [_c(M=M, T=T, noise=nz, flags=f) for M, T, nz, f in P((128, 256), (80, 16400), (1, 2), (0, 1))]
    rows += [_c(M=M, T=T, elbo=e, K=K, outs=o) for M, T, e, K, o in P((128, 256), (160, 16000, 32000, 81920), (1, 2, 3, 4, 5, 6, 7), (1, 5, 8, 20, 32, 40), (0, 1))]
    rows += [_c(M=M, T=T, elbo=e, K=1, outs=1) for M, T, e in P((128, 256), (160, 16400, 81920), (0, 8))]
    rows += [_c(M=M, T=T, K=K, flags=f, opt=o, elbo=e) for M, T, K, f, o, e in P((128, 256), (160, 16000, 81920), (8, 20), (0, 1), (1, 2, 3), (1, 4))]
    rows += [_c(tail=t, M=M, T=N, S=S, L=L, flags=f, noise=nz, P=Pp, R=Pp) for t, M, (N, S), L, f, nz, Pp in
             P((1, 2), MS, ((10, 8), (100, 50), (1000, 13), (1000, 100)), (1, 2), (0, 1, 2), (0, 1), (1,)) if t == 2 or nz == 0]
    rows += [_c(tail=t, M=M, T=1000, S=100, L=2, lv=3, opt=o) for t, M, o in P((1, 2), (128, 256), (0, 3))]
    rows += [_c(bad=b) for b in range(1, len(BAD_BOUND) + 1)]
    rows += [_c(tail=t, T=100, S=50, P=1, R=1, bad=b) for t in (1, 2) for b in range(101, 101 + len(BAD_PREDICT))]
    return np.array(rows, dtype=np.int64)


class Call:
    """The argument list of ``iwvi_dgp_forward`` for one case, with whatever host arrays the descriptors point to kept alive."""

    def __init__(self, case):
        c = dict(zip(COLS, (int(v) for v in case)))
        self.c, self.keep = c, []
        pred = c["tail"] != 0
        n_lv = 1 if c["lv"] else 0
        self.descs = (_abi.LayerDesc * _abi.MAX_STACK)()
        self.n_layers = n_lv + c["L"]
        self.Dx, self.Dy, self.XYdim = c["Dx"], c["P"], c["Dx"] + c["P"]
        self.XY = F if c["lv"] == 2 else None
        D = c["Dx"]
        for i in range(self.n_layers):
            d = self.descs[i]
            if c["noise"] == 1 and not pred:
                d.noise = F
            d.zero_noise = 1 if c["noise"] == 2 else 0
            if i < n_lv:
                d.type, d.latent_dim = _abi.LAYER_LV, 1
                if c["lv"] == 1:
                    d.enc_out = F
                elif c["lv"] == 2:
                    self.encoder(d, (self.XYdim, 20, 2))
                D += 1
                continue
            d.type, d.state, d.M, d.D, d.R, d.P = _abi.LAYER_GP, 0x100000 * (i + 1), c["M"], D, c["R"], c["P"]
            d.kern_type, d.mf_type, d.variance, d.mf_A = c["kern"], _abi.MF_LINEAR, 1.0, F
            d.mf_b = F if i % 2 == 0 else None
            d.W = F if c["P"] != c["R"] else None
            D = c["P"]
        self.descs[self.n_layers - 1].flags = c["flags"]
        if c["outs"]:
            self.descs[self.n_layers - 1].sample = F
        K = c["K"]
        self.X, self.Y, self.out_logw, self.rng, self.lik_var, self.elbo = F, F, F, F, 0.1, None
        if pred:
            self.T, self.row_div, self.row_mod = c["T"] * c["S"], c["S"], c["T"]
            self.z_y = F if c["noise"] == 1 else None
        else:
            self.T, self.row_div, self.row_mod = c["T"], K, max(c["T"] // K, 1)
            if c["elbo"] == 8:
                self.Y = self.out_logw = None
                self.Dy = 0
            elif c["elbo"]:
                e = self.elbo = _abi.ElboDesc()
                e.B, e.K, e.stride_b, e.stride_k, e.scale, e.mode_vi = c["T"] // K, K, K, 1, 1.0, 1 if c["elbo"] == 2 else 0
                e.out_elbo, e.ws, e.out_logp = F, F, F
                self.kl = (ctypes.c_void_p * 3)(F, F, F)
                self.kl_n = (ctypes.c_int32 * 3)(32, 32, 32)
                e.kl_global, e.n_glob = self.kl, 1
                if c["elbo"] == 3:
                    e.stride_b, e.stride_k = 1, e.B
                if c["elbo"] == 4:
                    e.adj_w = e.adj_dmean = e.adj_dvar = e.adj_sums = F
                if c["elbo"] == 5:
                    e.lw_init = F
                if c["elbo"] == 6:
                    e.x_per_sample = 1
                if c["elbo"] == 7:
                    e.kl_global_counts, e.n_glob = self.kl_n, 3
        if 0 < c["bad"] <= 100:
            BAD_BOUND[c["bad"] - 1](self)
        elif c["bad"] > 100:
            BAD_PREDICT[c["bad"] - 101](self)

    def encoder(self, d, dims, bias=True):
        n = len(dims) - 1
        W, b, dd = (ctypes.c_void_p * n)(*[F] * n), (ctypes.c_void_p * n)(*[F] * n), (ctypes.c_int32 * (n + 1))(*dims)
        self.keep += [W, b, dd]
        d.enc_W, d.enc_b, d.enc_dims, d.n_enc, d.enc_act = W, b if bias else None, dd, n, _abi.ACT_TANH

    def forward_args(self):
        """iwvi_dgp_forward's (and, with a tail selector and an output array appended, iwvi_debug_forward_plan's)."""
        return (self.descs, self.n_layers, self.X, self.Dx, self.XY, self.XYdim, self.Y, self.Dy, self.T, self.row_div, self.row_mod,
                self.lik_var, 1, self.rng, self.out_logw, ctypes.byref(self.elbo) if self.elbo is not None else None, None)

    def plan_args(self):
        """The same call for ``iwvi_debug_forward_plan``: the predictive tails pass z_y in XY's place and their output in out_logw's."""
        a = list(self.forward_args())
        if self.c["tail"]:
            a[4] = self.z_y
        return tuple(a) + (self.c["tail"],)


def _set(**kw):
    return lambda s: [setattr(s, k, v) for k, v in kw.items()]


def _layer(i, **kw):
    return lambda s: [setattr(s.descs[i], k, v) for k, v in kw.items()]


def _elbo(**kw):
    return lambda s: [setattr(s.elbo, k, v) for k, v in kw.items()]


def _enc(**kw):
    def f(s):
        s.descs[2] = s.descs[1]                                  # an LV layer in front of the two GP layers
        s.descs[1] = s.descs[0]
        d = s.descs[0]
        ctypes.memset(ctypes.byref(d), 0, ctypes.sizeof(d))
        d.type, d.latent_dim = _abi.LAYER_LV, 1
        s.descs[1].D, s.n_layers, s.XY = s.Dx + 1, 3, F
        dims = list(kw.get("dims", (s.XYdim, 20, 2)))
        s.encoder(d, dims)
        for k, v in kw.items():
            if k == "null_w":
                d.enc_W[v] = None
            elif k != "dims":
                setattr(d, k, v) if k != "XY" else setattr(s, "XY", v)
    return f


# one refusal of each kind of the bound's entry, in the driver's order of checks (BASE with one thing wrong)
BAD_BOUND = (
    _set(n_layers=0), _set(n_layers=9), _set(X=None), _set(Dx=33), _set(row_div=0), _set(T=0x7fffffff), _set(Y=None), _set(lik_var=0.0),
    _layer(0, D=9), _layer(1, state=None), _layer(0, M=513), _layer(0, R=33), _layer(1, W=None, R=4), _layer(0, mf_type=_abi.MF_IDENTITY, P=7, W=F),
    _layer(0, mf_A=None), _layer(0, mf_type=3), _layer(1, kern_type=7), _layer(0, type=2), _layer(1, P=9, W=F), _set(rng=None),
    _enc(latent_dim=0), _enc(XY=None), _enc(n_enc=9), _enc(dims=(5, 20, 2)), _enc(dims=(16, 20, 3)), _enc(dims=(16, 65, 2)), _enc(null_w=1), _enc(enc_act=9),
    _set(out_logw=None), _elbo(B=0), _elbo(n_glob=17), _elbo(stride_b=9), _elbo(stride_k=-1), _elbo(kl_global=None), _elbo(n_glob=3, kl_global_counts=(ctypes.c_int32 * 3)(1, 33, 1)),
    _elbo(adj_w=F), _elbo(adj_w=F, adj_dmean=F, adj_dvar=F, adj_sums=F, mode_vi=1), _elbo(adj_w=F, adj_dmean=F, adj_dvar=F, adj_sums=F, K_total=16),
    lambda s: (_set(T=81920, row_div=32, row_mod=2560)(s), _elbo(B=2560, K=32, stride_b=32, adj_w=F, adj_dmean=F, adj_dvar=F, adj_sums=F)(s)),
)
BAD_PREDICT = (_set(row_div=0), _set(row_mod=-1), _set(row_mod=0x7fffffff), _set(out_logw=None), _set(Dy=33), _set(lik_var=0.0),
               _set(rng=None), _layer(0, type=_abi.LAYER_LV, enc_out=F))


def copy_list_call(n_lv):
    """n_lv latent-variable layers with an in-kernel encoder of 8 maps (3 -> 2 -> ... -> 2) each, then one GP layer (M = 32, R = P = 1, no
    mixing matrix, zero mean function), T = 160: 16 copy-list entries per LV layer, 2 for the GP layer."""
    s = Call(_c(M=32, T=160, L=1, Dx=1, R=1, P=1, elbo=0, K=1))
    g = s.descs[0]
    g.mf_type, g.mf_A, g.mf_b, g.D = _abi.MF_ZERO, None, None, 1 + n_lv
    s.descs[n_lv] = g
    for i in range(n_lv):
        d = s.descs[i]
        ctypes.memset(ctypes.byref(d), 0, ctypes.sizeof(d))
        d.type, d.latent_dim = _abi.LAYER_LV, 1
        s.encoder(d, [3] + [2] * 8)
    s.n_layers, s.XY, s.XYdim = n_lv + 1, F, 3
    return s


def plan(lib, call):
    """(status, variant word, grid, LDS bytes, error text of a refusal) of ``iwvi_debug_forward_plan``."""
    out = (ctypes.c_int64 * 3)()
    rc = lib.iwvi_debug_forward_plan(*call.plan_args(), out)
    return rc, out[0], out[1], out[2], lib.iwvi_last_error().decode() if rc else ""


def each_option(cases):
    """(option or None, indices of its cases); the caller sets and restores the option."""
    for k, opt in enumerate(OPTS):
        idx = np.flatnonzero(cases[:, COLS.index("opt")] == k)
        if idx.size:
            yield opt, idx


def expected_rows():
    """(tail, word) of the 59 k_dgp_forward instantiations."""
    general = {(0, ns | s << 8 | b << 9) for ns in (1, 2, 3, 4, 5) for s in (0, 1) for b in (0, 1)} | {(0, ns | 0x1200) for ns in (1, 2, 3, 4, 5)}
    lean = {(0, 5 | s << 8 | m) for s in (0, 1) for m in (1 << 10, 1 << 11)}
    tails = {(t, ns | s << 8 | b << 9) for t in (1, 2) for ns in (1, 3, 5) for s in (0, 1) for b in (0, 1)} | {(t, ns | 0x1200) for t in (1, 2) for ns in (1, 3, 5)}
    return general | lean | tails


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi.lib()


def test_plan_matches_the_recorded_answers(lib):
    gold = np.load(GOLDEN)
    cases = grid()
    assert cases.shape == gold["cases"].shape and np.array_equal(cases, gold["cases"])
    got = np.zeros((len(cases), 4), dtype=np.int64)
    texts = {}
    for opt, idx in each_option(cases):
        try:
            if opt:
                _abi.set_debug_option(*opt)
            for i in idx:
                r = plan(lib, Call(cases[i]))
                got[i] = r[:4]
                if r[0]:
                    texts[int(i)] = r[4]
        finally:
            if opt:
                _abi.set_debug_option(opt[0], 0)
    want = np.stack([gold["status"], gold["word"], gold["grid"], gold["lds"]], axis=1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "first differing cases %s: got %s, recorded %s" % (cases[bad[:3]].tolist(), got[bad[:3]].tolist(), want[bad[:3]].tolist())
    recorded = dict(zip(gold["err_case"].tolist(), gold["err_text"].tolist()))
    assert texts == recorded
    assert len(recorded) == 139 and sorted(set(gold["status"].tolist())) == [_abi.ERR_UNSUPPORTED, _abi.ERR_ARG, 0]
    ok = gold["status"] == 0
    reached = set(zip(cases[ok, 0].tolist(), gold["word"][ok].tolist()))
    assert reached == expected_rows() and len(reached) == 59


def test_copy_list_is_bounded(lib):
    gold = np.load(GOLDEN)
    assert list(plan(lib, copy_list_call(2))[:4]) == gold["copy2"].tolist() and gold["copy2"][0] == 0      # 34 entries: plans as before
    for n_lv, entries in ((3, 50), (4, 66)):
        rc, _, _, _, text = plan(lib, copy_list_call(n_lv))
        assert rc == _abi.ERR_UNSUPPORTED and "%d entries" % entries in text and "FW_MAX_COPY = 48" in text, (n_lv, rc, text)
