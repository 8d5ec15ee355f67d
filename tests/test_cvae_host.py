"""The CVAE baseline without a GPU: the restatement of tests/cvae_restatement.py against torch.distributions, the C-ABI's declarations,
struct layouts and argument refusals (made before any HIP call, so a GPU-less host can provoke them), the model factory on the CPU, and the
tolerance guard: for every input set the GPU tests use, the float32 restatement sits within ONE TENTH of the tolerance the GPU test applies,
so that tolerance is ten times the arithmetic's own noise."""
import ctypes
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvae_restatement as cr   # noqa: E402

ENTRY_POINTS = ("iwvi_cvae_ws_bytes", "iwvi_cvae_elbo", "iwvi_cvae_elbo_and_grad", "iwvi_cvae_predict_samples")


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------
def test_kl_and_log_density_agree_with_torch_distributions():
    g = torch.Generator().manual_seed(0)
    mu, raw = torch.randn(40, 3, dtype=torch.float64, generator=g), 3.0 * torch.randn(40, 3, dtype=torch.float64, generator=g)
    sigma = torch.exp(0.5 * raw)
    ref = torch.distributions.kl_divergence(torch.distributions.Normal(mu, sigma), torch.distributions.Normal(torch.zeros_like(mu), 1.0))
    torch.testing.assert_close(cr.kl_to_standard_normal(mu, sigma * sigma, raw), ref, rtol=1e-12, atol=1e-12)
    y, m = torch.randn(40, 3, dtype=torch.float64, generator=g), torch.randn(40, 3, dtype=torch.float64, generator=g)
    var = torch.tensor(0.05, dtype=torch.float64)
    torch.testing.assert_close(cr.gaussian_log_density(y, m, var), torch.distributions.Normal(m, var.sqrt()).log_prob(y), rtol=1e-12, atol=1e-12)


def test_clipped_entries_have_zero_gradient():
    raw = torch.tensor([-40.0, cr.CLIP_LO - 1e-9, -3.0, 0.0, 20.0, cr.CLIP_HI + 1e-9, 60.0], dtype=torch.float64, requires_grad=True)
    c = cr.clip_raw(raw)
    assert c.detach().tolist() == [cr.CLIP_LO, cr.CLIP_LO, -3.0, 0.0, 20.0, cr.CLIP_HI, cr.CLIP_HI]
    torch.exp(0.5 * c).sum().backward()
    assert raw.grad[[0, 1, 5, 6]].abs().max() == 0.0 and (raw.grad[[2, 3, 4]] > 0).all()


def test_the_clip_case_clips_in_both_directions():
    ref = cr.value_and_grads(cr.make_case(*cr.CLIP_CASE, clip=True))
    assert (ref["raw"] < cr.CLIP_LO).sum() >= 2 and (ref["raw"] > cr.CLIP_HI).sum() >= 1
    assert ((ref["raw"] >= cr.CLIP_LO) & (ref["raw"] <= cr.CLIP_HI)).sum() >= 2
    assert all(np.isfinite(v).all() for k in ("dWs", "dbs", "dWs_dec", "dbs_dec") for v in ref[k]) and math.isfinite(ref["elbo"])


# ---- the tolerance guard ---------------------------------------------------------------------------------------------------------------
def _guard(case, what):
    r64, r32 = cr.value_and_grads(case, torch.float64), cr.value_and_grads(case, torch.float32)
    scale = abs(r64["logp"]) + abs(r64["kl"])
    for k in ("elbo", "logp", "kl"):
        err = abs(r32[k] - r64[k]) / scale
        print("%s %s: float32 restatement off by %.3g of |log p| + |KL| (a tenth of the GPU tolerance: %.1g)" % (what, k, err, 0.1 * cr.BOUND_RTOL))
        assert err <= 0.1 * cr.BOUND_RTOL, (what, k, err)
    for k in ("dWs", "dbs", "dWs_dec", "dbs_dec"):
        for i, (a, b) in enumerate(zip(r32[k], r64[k])):
            err = cr.max_norm_err(a, b)
            assert err <= 0.1 * cr.GRAD_RTOL, (what, k, i, err)
    err = abs(r32["dvariance"] - r64["dvariance"]) / abs(r64["dvariance"])
    assert err <= 0.1 * cr.GRAD_RTOL, (what, "dvariance", err)


@pytest.mark.parametrize("shape", cr.KERNEL_CASES, ids=lambda s: "%s-%d-%d-%d-B%d" % ("_".join(map(str, s[0])) or "lin", *s[1:]))
def test_tolerance_guard_for_the_kernel_cases(shape):
    _guard(cr.make_case(*shape), str(shape))


def test_tolerance_guard_for_the_clip_case():
    _guard(cr.make_case(*cr.CLIP_CASE, clip=True), "clip")


@pytest.mark.parametrize("net", cr.SAMPLER_NETS, ids=lambda s: "_".join(map(str, s[0])) or "lin")
def test_tolerance_guard_for_the_sampler_cases(net):
    for N, S in cr.SAMPLER_SHAPES:
        case, Xs, z, zy = cr.sampler_inputs(*net, N, S)
        for y_noise in (True, False):
            a, b = cr.samples(case, Xs, z, zy, torch.float32, y_noise=y_noise), cr.samples(case, Xs, z, zy, torch.float64, y_noise=y_noise)
            assert a.shape == (N, S, net[2])
            assert cr.max_norm_err(a, b) <= 0.1 * cr.SAMPLE_RTOL, (net, N, S, cr.max_norm_err(a, b))


# ---- declarations ----------------------------------------------------------------------------------------------------------------------
def test_header_prototypes_exports_and_version():
    from dgps_with_iwvi_amd import _abi
    header = open(os.path.join(ROOT, "include", "iwvi_hip.h")).read()
    lib = _abi.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _abi.PROTOTYPES
        assert getattr(lib, name) is not None
    assert lib.iwvi_version() == 19 == _abi.ABI_VERSION
    defs = dict(re.findall(r"#define\s+(IWVI_CVAE_[A-Z_]+)\s+(\d+)", header))
    assert (int(defs["IWVI_CVAE_MAX_MAPS"]), int(defs["IWVI_CVAE_MAX_WIDTH"]), int(defs["IWVI_CVAE_MAX_L"]), int(defs["IWVI_CVAE_MAX_DY"])) == \
        (_abi.CVAE_MAX_MAPS, _abi.CVAE_MAX_WIDTH, _abi.CVAE_MAX_L, _abi.CVAE_MAX_DY) == (4, 128, 8, 8)
    assert int(defs["IWVI_CVAE_NO_Y_NOISE"]) == _abi.CVAE_NO_Y_NOISE


def test_ctypes_structs_match_the_header_layout(tmp_path):
    from dgps_with_iwvi_amd import _abi
    structs = [("iwvi_cvae_desc", _abi.CvaeDesc), ("iwvi_cvae_grads", _abi.CvaeGrads)]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "iwvi_hip.h"', "int main(void) {"]
    for cname, cls in structs:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {}
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        s, f, v = ln.split()
        got[(s, f)] = int(v)
    for cname, cls in structs:
        assert ctypes.sizeof(cls) == got[(cname, "sizeof")]
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == got[(cname, fname)], (cname, fname)


# ---- refusals (nothing below dereferences a pointer: every call is refused first) ------------------------------------------------------
FAKE = 0x1000


class _Desc:
    def __init__(self, hidden=(7,), Dx=5, Dy=1, L=1, **over):
        from dgps_with_iwvi_amd import _abi
        enc, dec = cr.widths(hidden, Dx, Dy, L)
        enc, dec = over.pop("enc_dims", enc), over.pop("dec_dims", dec)
        n = over.pop("n_maps", len(enc) - 1)
        self.keep = [(ctypes.c_void_p * 8)(*([FAKE] * 8)) for _ in range(4)] + [(ctypes.c_int32 * 8)(*(list(enc) + [0] * (8 - len(enc)))),
                                                                               (ctypes.c_int32 * 8)(*(list(dec) + [0] * (8 - len(dec))))]
        d = self.d = _abi.CvaeDesc()
        d.enc_W, d.enc_b, d.dec_W, d.dec_b = (ctypes.cast(k, ctypes.POINTER(ctypes.c_void_p)) for k in self.keep[:4])
        d.enc_dims, d.dec_dims = (ctypes.cast(k, ctypes.POINTER(ctypes.c_int32)) for k in self.keep[4:])
        d.n_maps, d.Dx, d.Dy, d.L, d.act, d.variance = n, Dx, Dy, L, 0, 0.05
        for k, v in over.items():
            if k == "null_weight":
                self.keep[v[0]][v[1]] = None
            elif k == "null_field":
                setattr(d, v, None)
            else:
                setattr(d, k, v)


def _grads(_abi, **over):
    keep = [(ctypes.c_void_p * 8)(*([FAKE] * 8)) for _ in range(4)]
    g = _abi.CvaeGrads()
    g.enc_dW, g.enc_db, g.dec_dW, g.dec_db = (ctypes.cast(k, ctypes.POINTER(ctypes.c_void_p)) for k in keep)
    g.dvariance = FAKE
    for k, v in over.items():
        setattr(g, k, v)
    return g, keep


BAD_DESCS = [
    (dict(n_maps=0), "linear maps"), (dict(n_maps=5), "linear maps"),
    (dict(enc_dims=[6, 129, 2], dec_dims=[6, 129, 1]), "width"), (dict(enc_dims=[6, 0, 2], dec_dims=[6, 0, 1]), "width"),
    (dict(L=0), "L ="), (dict(L=9, enc_dims=[6, 7, 18], dec_dims=[14, 7, 1]), "L ="),
    (dict(Dy=0), "Dy ="), (dict(Dy=9, enc_dims=[14, 7, 2], dec_dims=[6, 7, 9]), "Dy ="),
    (dict(enc_dims=[5, 7, 2]), "enc_dims[0]"), (dict(dec_dims=[5, 7, 1]), "dec_dims[0]"),
    (dict(enc_dims=[6, 7, 3]), "enc_dims[last]"), (dict(dec_dims=[6, 7, 2]), "dec_dims[last]"),
    (dict(dec_dims=[6, 8, 1]), "hidden width"),
    (dict(act=7), "activation"), (dict(null_field="enc_W"), "null pointer"), (dict(null_field="dec_dims"), "null pointer"),
    (dict(null_weight=(2, 1)), "null weight"),
]


def _train_call(lib, name, d, X=FAKE, Y=FAKE, B=4, eps=FAKE, rng=None, out=FAKE, grads=None, ws=FAKE):
    args = [ctypes.byref(d) if d is not None else None, X, Y, B, eps, 0, rng, None, out]
    if name == "iwvi_cvae_elbo_and_grad":
        args.append(ctypes.byref(grads) if grads is not None else None)
    rc = getattr(lib, name)(*args, ws, None)
    return rc, lib.iwvi_last_error().decode()


@pytest.mark.parametrize("name", ["iwvi_cvae_elbo", "iwvi_cvae_elbo_and_grad"])
def test_training_entries_refuse_bad_arguments(name):
    from dgps_with_iwvi_amd import _abi
    lib = _abi.lib()
    g, gkeep = _grads(_abi)
    for over, word in BAD_DESCS:
        hidden = (7, 7) if over.get("null_weight") else (7,)
        rc, msg = _train_call(lib, name, _Desc(hidden=hidden, **over).d, grads=g)
        assert rc == _abi.ERR_ARG and name in msg and word in msg, (over, rc, msg)
    ok = _Desc()
    for kw, word in [(dict(X=None), "null"), (dict(Y=None), "null"), (dict(out=None), "null"), (dict(B=0), "B ="), (dict(B=-3), "B ="),
                     (dict(ws=None), "workspace"), (dict(eps=None, rng=None), "rng_state")]:
        rc, msg = _train_call(lib, name, ok.d, grads=g, **kw)
        assert rc == _abi.ERR_ARG and name in msg and word in msg, (kw, rc, msg)
    rc, msg = _train_call(lib, name, None, grads=g)
    assert rc == _abi.ERR_ARG and name in msg
    if name == "iwvi_cvae_elbo_and_grad":
        for bad in (None, _grads(_abi, dvariance=None)[0], _grads(_abi, dec_db=None)[0]):
            rc, msg = _train_call(lib, name, ok.d, grads=bad)
            assert rc == _abi.ERR_ARG and name in msg and "grads" in msg, (rc, msg)


def test_predict_samples_refuses_bad_arguments():
    from dgps_with_iwvi_amd import _abi
    lib, name = _abi.lib(), "iwvi_cvae_predict_samples"

    def call(d, X=FAKE, N=3, S=5, z=FAKE, zy=FAKE, flags=0, rng=None, out=FAKE):
        rc = lib.iwvi_cvae_predict_samples(ctypes.byref(d), X, N, S, z, zy, flags, 0, rng, out, None)
        return rc, lib.iwvi_last_error().decode()
    for over, word in BAD_DESCS:
        hidden = (7, 7) if over.get("null_weight") else (7,)
        rc, msg = call(_Desc(hidden=hidden, **over).d)
        assert rc == _abi.ERR_ARG and name in msg and word in msg, (over, rc, msg)
    ok = _Desc()
    for kw, word in [(dict(X=None), "null"), (dict(out=None), "null"), (dict(N=0), "N ="), (dict(S=0), "N ="), (dict(S=-1), "N ="),
                     (dict(N=1 << 20, S=1 << 11), "2^31"), (dict(z=None), "rng_state"), (dict(zy=None), "rng_state"), (dict(flags=2), "flags")]:
        rc, msg = call(ok.d, **kw)
        assert rc == _abi.ERR_ARG and name in msg and word in msg, (kw, rc, msg)
    # the no-y-noise flag needs no z_y and, with z injected, no counter: it passes validation (and would launch) -- not called here


def test_ws_bytes():
    from dgps_with_iwvi_amd import _abi
    lib = _abi.lib()
    d = _Desc(hidden=(100, 100), Dx=8).d
    sizes = [lib.iwvi_cvae_ws_bytes(ctypes.byref(d), B) for B in (0, 1, 2, 7, 8, 9, 64, 65, 512, 1000, 100000)]
    assert sizes[0] == 0 and sizes[1] > 0
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    per_row = 4 * sum(i + o for dims in cr.widths((100, 100), 8, 1, 1) for i, o in zip(dims[:-1], dims[1:]))
    assert sizes[-1] >= 100000 * per_row                              # every map's input rows and deltas fit
    assert lib.iwvi_cvae_ws_bytes(ctypes.byref(d), -1) == 0
    assert lib.iwvi_cvae_ws_bytes(ctypes.byref(_Desc(n_maps=0).d), 8) == 0


# ---- the model factory on the CPU ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("configuration,hidden", [("", []), ("50", [50]), ("100_100", [100, 100]), ("50_x_50", [50, 50])])
def test_build_cvae_model_on_the_cpu(configuration, hidden):
    from dgps_with_iwvi_amd.build_models import build_cvae_model
    from dgps_with_iwvi_amd.cvae import CVAE
    rng = np.random.RandomState(3)
    X, Y = rng.randn(200, 8), rng.randn(200, 1)
    ARGS = types.SimpleNamespace(mode="CVAE", configuration=configuration, minibatch_size=37, lr=5e-3)
    np.random.seed(11)                                                # the initial weights come from the host generator, as in the reference
    m = build_cvae_model(ARGS, X, Y, device="cpu")
    assert isinstance(m, CVAE) and m.name == "CVAE" and m.latent_dim == 1 and m.batch_size == 37
    assert m.X.shape == (37, 8) and m.Y.shape == (37, 1) and m.X.dtype == torch.float32
    assert [tuple(w.shape) for w in m.Ws] == list(zip(([9] + hidden), (hidden + [2])))
    assert [tuple(w.shape) for w in m.Ws_dec] == list(zip(([9] + hidden), (hidden + [1])))
    for Ws, bs in ((m.Ws, m.bs), (m.Ws_dec, m.bs_dec)):
        for w, b in zip(Ws, bs):
            assert w.dtype == torch.float32 and b.shape == (w.shape[1],) and (b == 0).all()
            n, sd = w.numel(), (2.0 / sum(w.shape)) ** 0.5
            if n >= 50:                                               # the standard error of a sample standard deviation: sd / sqrt(2 (n - 1))
                assert abs(float(w.double().std()) - sd) <= 5.0 * sd / (2.0 * (n - 1)) ** 0.5, (tuple(w.shape), float(w.std()), sd)
    assert m.variance == 0.05 and float(m.variance_dev) == np.float32(0.05)
    assert m.global_step == 0 and callable(m.train_op) and callable(m.init_op)


def test_build_model_points_to_the_cvae_builder():
    from dgps_with_iwvi_amd.build_models import build_model
    ARGS = types.SimpleNamespace(mode="CVAE", configuration="50", minibatch_size=16)
    with pytest.raises(NotImplementedError, match="build_cvae_model"):
        build_model(ARGS, np.zeros((4, 2)), np.zeros((4, 1)))


def test_minibatches_follow_dgp_vi():
    """The iterator is the one of models.DGP_VI: RandomState(0), shuffled epochs, the same buffers on every step."""
    from dgps_with_iwvi_amd.cvae import CVAE
    rng = np.random.RandomState(0)
    X, Y = rng.randn(10, 2).astype(np.float32), rng.randn(10, 1).astype(np.float32)
    m = CVAE(X, Y, 1, [], batch_size=4, device="cpu")
    perm_rng = np.random.RandomState(0)
    perm, pos = perm_rng.permutation(10), 0
    ptr = None
    for step in range(6):
        if step:
            m.next_minibatch()
        if pos + 4 > 10:
            perm, pos = perm_rng.permutation(10), 0
        np.testing.assert_array_equal(m.X.numpy(), X[perm[pos:pos + 4]])
        np.testing.assert_array_equal(m.Y.numpy(), Y[perm[pos:pos + 4]])
        pos += 4
        assert ptr in (None, m.X.data_ptr())
        ptr = m.X.data_ptr()
