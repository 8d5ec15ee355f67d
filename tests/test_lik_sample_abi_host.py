"""iwvi_lik_sample_y without a device: the header declares it, the library exports it, _abi.PROTOTYPES binds it, and a null or invalid
descriptor is refused before anything touches a GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


def test_header_declares_the_entry_as_an_additive_extension():
    text = open(os.path.join(ROOT, "include", "iwvi_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+iwvi_lik_sample_y\s*\(([^)]*)\)", code)
    assert m, "include/iwvi_hip.h does not declare iwvi_lik_sample_y"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 12 and args[0].startswith("const iwvi_lik_desc*") and "serial_dev" in args[8] and args[-1].startswith("void*")
    assert re.search(r"#define\s+IWVI_ABI_VERSION\s+19\b", code)


def test_library_exports_it_and_the_prototype_binds_it():
    _abi, lib = _lib()
    assert "iwvi_lik_sample_y" in _abi.PROTOTYPES
    res, args = _abi.PROTOTYPES["iwvi_lik_sample_y"]
    assert res is _abi.c_int and len(args) == 12
    fn = lib.iwvi_lik_sample_y
    assert fn.restype is _abi.c_int and list(fn.argtypes) == list(args)


def test_a_null_or_invalid_descriptor_is_refused_without_a_device():
    _abi, lib = _lib()
    assert lib.iwvi_lik_sample_y(None, None, None, 4, 1, None, 0, 0, None, None, None, None) == _abi.ERR_ARG
    assert b"iwvi_lik_sample_y" in lib.iwvi_last_error() and b"descriptor" in lib.iwvi_last_error()
    d = _abi.LikDesc()
    d.type = 7
    assert lib.iwvi_lik_sample_y(d, None, None, 4, 1, None, 0, 0, None, None, None, None) == _abi.ERR_ARG
    d.type, d.param[0] = _abi.LIK_GAUSSIAN, 1.0
    assert lib.iwvi_lik_sample_y(d, None, None, 4, 1, None, 0, 0, None, None, None, None) == _abi.ERR_ARG      # null out_y
    assert b"out_y" in lib.iwvi_last_error()
    assert lib.iwvi_lik_sample_y(d, None, None, -1, 1, None, 0, 0, None, None, None, None) == _abi.ERR_ARG


def test_every_likelihood_has_sample_y():
    from dgps_with_iwvi_amd import likelihoods as L
    for cls in (L.Gaussian, L.Bernoulli, L.StudentT, L.MultiClass, L.Poisson, L.Exponential, L.Gamma, L.Beta, L.Ordinal):
        assert callable(getattr(cls, "sample_y", None)), cls.__name__
