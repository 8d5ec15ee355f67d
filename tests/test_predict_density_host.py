"""The Monte Carlo predictive density's C-ABI surface on a GPU-less host: exported, prototyped completely, refused arguments answered
before any HIP call, and the predictive variants of the fused forward built without scratch memory."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("iwvi_dgp_predict_density", "iwvi_dgp_predict_density_ws_bytes", "iwvi_gaussian_log_density")


def _header():
    text = open(os.path.join(ROOT, "include", "iwvi_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


def test_header_version_is_19_and_matches_the_binding():
    from dgps_with_iwvi_amd import _abi
    ver = int(re.search(r"#define IWVI_ABI_VERSION (\d+)", _header()).group(1))
    assert ver == _abi.ABI_VERSION == 19


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_exported_and_its_argtypes_are_complete(name):
    _abi, lib = _lib()
    assert hasattr(lib, name)
    decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, _header())
    assert decl, name
    nargs = len([a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"])
    assert len(_abi.PROTOTYPES[name][1]) == nargs
    assert lib.iwvi_version() == _abi.ABI_VERSION


def test_refused_arguments_return_before_any_launch():
    import ctypes
    _abi, lib = _lib()
    d = (_abi.LayerDesc * 1)()
    assert lib.iwvi_dgp_predict_density_ws_bytes(0, 5) == 0
    assert lib.iwvi_dgp_predict_density_ws_bytes(1000, 2000) == (1000 + 1000 * 2000 // 16) * 8
    buf = ctypes.c_void_p(16)                            # never dereferenced: every call below is refused on its sizes
    assert lib.iwvi_dgp_predict_density(d, 1, buf, 8, buf, 1, 10, 0, 0.1, None, 0, buf, buf, buf, None) == _abi.ERR_ARG
    assert b"S=0" in lib.iwvi_last_error()
    assert lib.iwvi_dgp_predict_density(d, 1, buf, 8, None, 1, 10, 4, 0.1, None, 0, buf, buf, buf, None) == _abi.ERR_ARG
    assert lib.iwvi_dgp_predict_density(d, 1, buf, 8, buf, 1, 10, 4, 0.1, None, 0, buf, buf, None, None) == _abi.ERR_ARG
    assert lib.iwvi_dgp_predict_density(d, 1, buf, 8, buf, 1, 1 << 20, 1 << 12, 0.1, None, 0, buf, buf, buf, None) == _abi.ERR_ARG
    assert lib.iwvi_dgp_predict_density(d, 1, buf, 8, buf, 1, 0, 4, 0.1, None, 0, buf, buf, buf, None) == 0      # nothing to do
    assert lib.iwvi_gaussian_log_density(buf, None, buf, 0.0, None, 4, 1, 1, 4, buf, None) == _abi.ERR_ARG
    assert lib.iwvi_gaussian_log_density(None, None, buf, 0.1, None, 4, 1, 1, 4, buf, None) == _abi.ERR_ARG


def test_predictive_variants_are_built_without_scratch():
    from dgps_with_iwvi_amd import kernel_resources as kr
    if not os.path.exists(kr.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf here")
    rows = {r["demangled"]: r for r in kr.kernel_table()}
    pred = [d for d in rows if d.startswith("k_dgp_forward<") and d.split(",")[3] == "3"]
    # sub-tiles 1 / 3 / 5 x (split-f16 or fp32 stage 2) x (M <= 128 or larger), and the float64 stage-1 route
    assert len(pred) == 15, sorted(pred)
    for ns in (1, 3, 5):
        for s16 in ("true", "false"):
            for big in ("true", "false"):
                assert "k_dgp_forward<%d,%s,%s,3,false>" % (ns, s16, big) in rows
        assert "k_dgp_forward<%d,false,true,3,true>" % ns in rows
    for d in pred + ["k_pred_lse_merge", "k_gauss_log_density"]:
        assert rows[d]["private_segment_fixed_size"] == 0, d
        assert rows[d]["vgpr_count"] <= 256, d
