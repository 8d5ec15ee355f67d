"""The two sizing entries of the layer adjoint (``iwvi_gp_layer_backward_needs_u`` / ``_ws_bytes``) against recorded answers.

They are pure host arithmetic over the adjoint's chain plan (csrc/backward.hip, ``chain_plan`` / ``bwd_layout``), so they run on
a GPU-less host.  ``tests/golden/bw_sizing.npz`` holds the answers of the library before the plan was gathered into one function,
over a grid on both sides of every switch in that arithmetic: M a multiple of 16 or not; M <= 128, 129-256, > 256; odd and even
numbers of 16-row blocks; T % 16; more than 1024 per-workgroup shares.  16 184 cases, ``needs_u`` == 1 for 4 815 of them.
Equality is exact: a moved route threshold or workspace offset shows here before any GPU run."""
import itertools
import os

import numpy as np
import pytest

from dgps_with_iwvi_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bw_sizing.npz")

MS = (16, 32, 48, 64, 96, 120, 128, 144, 176, 192, 240, 256, 272, 288, 320, 496, 512)
TS = (16, 48, 64, 80, 1024, 2048, 4096, 4112, 5120, 8192, 16384, 16400, 20480, 32768, 81920, 204800, 819200)
DS = (1, 8, 9, 16, 17, 20, 32)
RS = (1, 5, 17, 32)


def grid():
    """[n, 5] int64 rows (T, M, D, R, P); P in (R, 32) for every R."""
    return np.array([(T, M, D, R, P) for M, T, D, R in itertools.product(MS, TS, DS, RS) for P in (R, 32)], dtype=np.int64)


def evaluate(lib, cases):
    needs_u = np.array([lib.iwvi_gp_layer_backward_needs_u(int(T), int(M), int(D), int(R), int(P)) for T, M, D, R, P in cases], dtype=np.int8)
    ws_bytes = np.array([lib.iwvi_gp_layer_backward_ws_bytes(int(T), int(M), int(D), int(R)) for T, M, D, R, _ in cases], dtype=np.int64)
    return needs_u, ws_bytes


def test_sizing_entries_match_the_recorded_answers():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    gold = np.load(GOLDEN)
    cases = grid()
    assert cases.shape == (16184, 5) and np.array_equal(cases, gold["cases"])
    assert int(gold["needs_u"].sum()) == 4815                      # both answers well represented
    needs_u, ws_bytes = evaluate(_abi.lib(), cases)
    bad = np.flatnonzero((needs_u != gold["needs_u"]) | (ws_bytes != gold["ws_bytes"]))
    assert bad.size == 0, "first differing (T, M, D, R, P): %s" % (cases[bad[:5]].tolist(),)
