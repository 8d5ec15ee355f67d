"""``iwvi_psis_summary`` at the C-ABI without a GPU: the prototype and the descriptor's layout, and every refusal, which returns
IWVI_ERR_ARG with its text before any HIP call."""
import ctypes
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


P = 16                                                           # a non-null address that is never dereferenced


def _desc(_abi, mode="terms", **kw):
    """A descriptor every check accepts (pointers are the address 16), then ``kw`` on top."""
    d = _abi.PsisDesc()
    if mode == "terms":
        d.terms, d.n_terms = P, 1
    else:
        d.fmean, d.fvar, d.Y, d.Dy, d.lik_variance = P, P, P, 2, 0.5
    d.N, d.S, d.stride_n, d.stride_s = 4, 100, 100, 1
    d.out_raw = P
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_the_prototype_and_the_header_agree():
    from dgps_with_iwvi_amd import _abi
    assert "iwvi_psis_summary" in _abi.PROTOTYPES and _abi.ABI_VERSION == 19
    text = open(os.path.join(ROOT, "include", "iwvi_hip.h")).read()
    assert "int iwvi_psis_summary(const iwvi_psis_desc* desc, void* stream);" in text and "#define IWVI_ABI_VERSION 19" in text
    assert "psis.hip" in open(os.path.join(ROOT, "dgps_with_iwvi_amd", "csrc", "Makefile")).read()


def test_the_descriptor_mirrors_the_header_layout(tmp_path):
    from dgps_with_iwvi_amd import _abi
    cls = _abi.PsisDesc
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "iwvi_hip.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(iwvi_psis_desc));']
    lines += ['  printf("%s %%zu\\n", offsetof(iwvi_psis_desc, %s));' % (f, f) for f, _ in cls._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert ctypes.sizeof(cls) == int(got["sizeof"])
    for f, _ in cls._fields_:
        assert getattr(cls, f).offset == int(got[f]), f


def test_every_refusal_returns_before_any_launch():
    _abi, lib = _lib()
    E = _abi.ERR_ARG
    call = lambda d: lib.iwvi_psis_summary(None if d is None else ctypes.byref(d), None)
    null1 = (ctypes.c_void_p * 1)()                              # a host array holding one NULL pointer
    ok1 = (ctypes.c_void_p * 1)(P)
    dims0, dims1 = (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(1)
    nan = float("nan")
    cases = [
        (None, b"null descriptor"),
        (_desc(_abi, N=-1), b"N=-1 out of range"),
        (_desc(_abi, S=0), b"S=0 out of range"),
        (_desc(_abi, S=16385), b"S=16385 out of range"),
        (_desc(_abi, stride_n=-1), b"must not be negative"),
        (_desc(_abi, stride_s=-100), b"must not be negative"),
        (_desc(_abi, terms=None), b"neither terms nor moments"),
        (_desc(_abi, fmean=P, fvar=P), b"both terms and moments"),
        (_desc(_abi, n_terms=0), b"n_terms=0 outside"),
        (_desc(_abi, n_terms=33), b"n_terms=33 outside"),
        (_desc(_abi, "moments", Dy=0), b"Dy=0 outside"),
        (_desc(_abi, "moments", Dy=33), b"Dy=33 outside"),
        (_desc(_abi, "moments", fvar=None), b"moments need fmean and fvar"),
        (_desc(_abi, n_kl=-1), b"n_kl=-1 outside"),
        (_desc(_abi, n_kl=5), b"n_kl=5 outside"),
        (_desc(_abi, n_kl=1, kl_local=null1, kl_dims=dims1), b"null kl_local pointer 0"),
        (_desc(_abi, n_kl=1, kl_dims=dims1), b"null kl_local pointer 0"),
        (_desc(_abi, n_kl=1, kl_local=ok1, kl_dims=dims0), b"kl_dims[0] must be at least 1"),
        (_desc(_abi, "moments", Y=None), b"moments without Y"),
        (_desc(_abi, "moments", lik_variance=0.0), b"must be positive"),
        (_desc(_abi, "moments", lik_variance=-1.0), b"must be positive"),
        (_desc(_abi, "moments", lik_variance=nan), b"must be positive"),
        (_desc(_abi, out_raw=None), b"no output at all"),
        (_desc(_abi, "moments", out_raw=None), b"no output at all"),
    ]
    for d, text in cases:
        assert call(d) == E, text
        assert text in lib.iwvi_last_error(), (text, lib.iwvi_last_error())
    # every single output alone is an output
    for f in ("out_logw", "out_raw", "out_ess", "out_khat", "out_psis"):
        assert call(_desc(_abi, **dict({"N": 0, "out_raw": None}, **{f: P}))) == 0


def test_no_points_is_ok_and_launches_nothing():
    _abi, lib = _lib()
    for mode in ("terms", "moments"):
        assert lib.iwvi_psis_summary(ctypes.byref(_desc(_abi, mode, N=0)), None) == 0
    # ... but the arguments are still checked
    assert lib.iwvi_psis_summary(ctypes.byref(_desc(_abi, N=0, S=0)), None) == _abi.ERR_ARG


def test_the_python_surface_refuses_on_the_host():
    import torch
    from dgps_with_iwvi_amd import evaluation, psis
    assert psis.MAX_S == 16384
    with pytest.raises(ValueError, match="16384"):
        psis.summarise(1, 16385, 16385, 1, terms=torch.zeros(1, 16385))
    with pytest.raises(ValueError, match=r"\[N, S\]"):
        evaluation.psis_summary(torch.zeros(5))
    with pytest.raises(TypeError):
        evaluation.psis_summary(torch.zeros(2, 5, dtype=torch.float64))
    from dgps_with_iwvi_amd._abi import IwviError
    with pytest.raises(IwviError, match="no CPU fallback"):
        evaluation.psis_summary(torch.zeros(2, 5))


def test_kernel_resources_lists_the_kernel_without_scratch():
    from dgps_with_iwvi_amd import kernel_resources as kr
    assert "k_psis_summary" in kr.NO_SCRATCH
    if not os.path.exists(kr.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf here")
    rows = [r for r in kr.kernel_table() if r["demangled"] == "k_psis_summary"]
    assert len(rows) == 1 and rows[0]["private_segment_fixed_size"] == 0 and rows[0]["vgpr_spill_count"] == 0, rows


def test_the_model_refuses_before_any_launch():
    """S above the sort's capacity, and more latent-variable layers than the weight takes regularisers: both named, both on the host."""
    import numpy as np
    import torch
    from dgps_with_iwvi_amd import build_models
    from dgps_with_iwvi_amd.likelihoods import Gaussian
    from dgps_with_iwvi_amd.models import DGP_IWVI
    rng = np.random.RandomState(0)
    X, Y = rng.randn(20, 2).astype(np.float32), rng.randn(20, 1).astype(np.float32)
    cpu = torch.device("cpu")
    np.random.seed(1)
    one = DGP_IWVI(X, Y, build_models.build_layers("L1", X, 8, rng=np.random.RandomState(2)), Gaussian(0.1), num_samples=3).to(cpu)
    with pytest.raises(ValueError, match="1..16384"):
        one.importance_log_density(X[:4], Y[:4], 16385)
    with pytest.raises(ValueError, match="proposal"):
        one.importance_log_density(X[:4], Y[:4], 10, proposal="q")
    with pytest.raises(ValueError, match="kind"):
        one.importance_log_density(X[:4], Y[:4], 10, kind="density")
    five = DGP_IWVI(X, Y, build_models.build_layers("L1_L1_L1_L1_L1", X, 8, rng=np.random.RandomState(2)), Gaussian(0.1), num_samples=3).to(cpu)
    with pytest.raises(ValueError, match="5 latent-variable layers.*at most 4.*IWVI_MAX_KL"):
        five.importance_log_density(X[:4], Y[:4], 10)
    key = one._mb_key()
    with pytest.raises(ValueError, match="Y must be"):
        one.importance_log_density(X[:4], Y[:3], 10)
    assert one._mb_key() == key
