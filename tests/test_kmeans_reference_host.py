"""The device k-means on a GPU-less host: the float64 restatement (tests/kmeans_reference.py) against ``scipy.cluster.vq.kmeans2`` bit
for bit, the start SciPy's ``minit="points"`` takes from NumPy's global stream, and the surface of ``iwvi_kmeans`` (declared, exported,
prototyped; the ABI number stays 19; bad arguments refused before any HIP call; the kernels in the scratch guard)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
from scipy.cluster.vq import kmeans2

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import kmeans_reference as R   # noqa: E402


@pytest.mark.parametrize("N,M,D,seed", R.CASES + R.LARGE_CASES)
def test_restatement_equals_scipy_bit_for_bit(N, M, D, seed):
    X, C0 = R.case_inputs(N, M, D, seed)
    C, labels, counts, inertia, gap = R.kmeans_reference(X, C0, R.ITERS)
    sc, sl = kmeans2(X.astype(np.float64), C0.astype(np.float64), iter=R.ITERS, minit="matrix")
    print("N=%d M=%d D=%d: max |centroid diff| %.1e, labels differing %d, min_gap %.2e" % (N, M, D, np.abs(C - sc).max(), int((labels != sl).sum()), gap))
    assert np.array_equal(C, sc) and np.array_equal(labels, sl)
    assert np.array_equal(counts, np.bincount(sl, minlength=M)) and counts.sum() == N and inertia >= 0.0
    assert gap > 1e-10                                           # what tests/test_gpu_kmeans.py asks before it compares labels


@pytest.mark.parametrize("N,M,D,seed", [c for c in R.CASES if c[0] <= 4099])
def test_the_points_start_is_scipys_own_draw(N, M, D, seed):
    X, C0 = R.case_inputs(N, M, D, seed)                          # np.random.seed(seed); choice
    after_ours = np.random.randint(1 << 30)
    np.random.seed(seed)
    sc, sl = kmeans2(X.astype(np.float64), M, iter=R.ITERS, minit="points")
    assert np.random.randint(1 << 30) == after_ours               # both consume the same amount of the global stream
    C, labels = R.kmeans_reference(X, C0, R.ITERS)[:2]
    assert np.array_equal(C, sc) and np.array_equal(labels, sl)


def test_restatement_rules_for_ties_and_empty_clusters():
    X = np.array([[0.0, 0.0], [0.0, 0.0], [4.0, 0.0], [4.0, 0.0], [4.0, 0.0]], dtype=np.float32)
    C0 = np.array([[1.0, 0.0], [1.0, 0.0], [9.0, 9.0]], dtype=np.float32)
    C, labels, counts, inertia, gap = R.kmeans_reference(X, C0, 1)
    assert labels.tolist() == [0, 0, 0, 0, 0] and counts.tolist() == [5, 0, 0] and gap == 0.0
    assert np.array_equal(C, [[2.4, 0.0], [1.0, 0.0], [9.0, 9.0]]) and inertia == 2 * 1.0 + 3 * 9.0
    assert R.kmeans_reference(X, C0[:1], 3)[4] == np.inf          # M = 1: nothing to tie with


# ---- the entry point's surface ---------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "iwvi_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_entry_points_are_declared_prototyped_and_refuse_without_a_gpu():
    from dgps_with_iwvi_amd import _abi
    for name, nargs in (("iwvi_kmeans", 13), ("iwvi_kmeans_ws_bytes", 3)):
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, _header())
        assert decl, "%s is not declared in include/iwvi_hip.h" % name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == nargs == len(_abi.PROTOTYPES[name][1])
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    lib = _abi.lib()
    assert lib.iwvi_version() == _abi.ABI_VERSION == 19          # additive: the number did not move
    ws = lib.iwvi_kmeans_ws_bytes
    assert ws(0, 128, 8) == 0 and ws(100, 0, 8) == 0 and ws(100, 513, 8) == 0 and ws(100, 8, 0) == 0 and ws(100, 8, 33) == 0 and ws(1 << 31, 8, 8) == 0
    assert ws(4099, 128, 8) > 128 * 8 * 8 and ws(5, 8, 2) > 0     # (M > N is allowed)
    assert ws((1 << 31) - 1, 512, 32) == ws(1 << 20, 512, 32)     # the workspace stops growing with N: a fixed number of partials
    buf = ctypes.c_void_p(256)                                    # never dereferenced: every call below is refused on its arguments

    def refused(text, X=buf, N=100, D=8, Z=buf, M=16, iters=10, out=buf, w=buf):
        assert lib.iwvi_kmeans(X, N, D, Z, M, iters, out, None, None, None, None, w, None) == _abi.ERR_ARG == -1
        msg = lib.iwvi_last_error()
        assert b"iwvi_kmeans" in msg and text in msg, msg

    refused(b"null X", X=None)
    refused(b"null Z_init", Z=None)
    refused(b"null out_Z", out=None)
    refused(b"null ws", w=None)
    refused(b"N=0", N=0)
    refused(b"N=-5", N=-5)
    refused(b"N=2147483648", N=1 << 31)
    refused(b"D=0", D=0)
    refused(b"D=33", D=33)
    refused(b"M=0", M=0)
    refused(b"M=513", M=513)
    refused(b"iters=0", iters=0)
    refused(b"iters=-1", iters=-1)


def test_kernels_are_listed_and_built_without_scratch():
    from dgps_with_iwvi_amd import kernel_resources as kr
    assert {"k_km_init", "k_km_step", "k_km_update"} <= set(kr.NO_SCRATCH)
    if not os.path.exists(kr.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    rows = [r for r in kr.check() if r["demangled"].startswith("k_km_")]
    # init; the step at the D ceilings 8 / 16 / 32, the first two with one and with two points per lane; three updates
    assert len(rows) == 9, sorted(r["demangled"] for r in rows)
    assert all(r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 for r in rows)


def test_python_side_refuses_before_the_library_is_touched():
    import torch
    from dgps_with_iwvi_amd import build_models, kmeans
    X = np.zeros((20, 3), dtype=np.float32)
    for kw in (dict(k=4, minit="++"), dict(k=4, minit="random"), dict(k=4, iter=0), dict(k=21), dict(k=0),
               dict(k=np.zeros((4, 2), dtype=np.float32), minit="matrix"), dict(k=np.zeros(4, dtype=np.float32), minit="matrix")):
        with pytest.raises(ValueError):
            kmeans.kmeans2(X, **kw)
    with pytest.raises(ValueError):
        kmeans.kmeans2(np.zeros(20, dtype=np.float32), 4)
    with pytest.raises(ValueError):
        kmeans.kmeans2(np.zeros((20, 33), dtype=np.float32), 4)
    if not torch.cuda.is_available():
        with pytest.raises(Exception) as e:
            kmeans.kmeans2(X, 4)                                  # a CPU device: no fallback
        assert "no CPU fallback" in str(e.value)
    with pytest.raises(ValueError, match="kmeans"):
        build_models.build_layers("G2", np.zeros((20, 3)), 4, kmeans="gpu")


def test_build_layers_on_the_host_is_the_direct_scipy_call():
    """``kmeans="host"``, the default: bit for bit what the function computed before it had the keyword."""
    from dgps_with_iwvi_amd import build_models
    X = np.random.RandomState(11).randn(600, 4).astype(np.float32).astype(np.float64)
    np.random.seed(11)
    Z = kmeans2(X, 32, minit="points")[0]
    for kw in ({}, {"kmeans": "host"}):
        np.random.seed(11)
        layers = build_models.build_layers("G3", X, 32, **kw)
        for layer in layers:                                      # the deeper layer shares the columns
            assert np.array_equal(layer._Z().detach().cpu().numpy()[:, :4], Z.astype(layer._Z().detach().cpu().numpy().dtype))
