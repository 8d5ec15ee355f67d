"""The table of tests/forward_variant_cases.py is complete and every row of it plans to its word -- on the CPU, through
``iwvi_debug_forward_plan`` (which returns before the first HIP call; the pointers are made-up addresses, as in tests/test_fw_plan_host.py).

Complete: the (tail, word) pairs of the table are exactly the OK pairs recorded in tests/golden/fw_plan.npz, whose grid reaches every
``k_dgp_forward`` instantiation of ``fw_variants[]`` (test_fw_plan_host.py asserts that).  Whoever adds an instantiation and re-records
the plan golden fails here until the GPU table has a row for it.

The descriptors mirror what ``DGP_VI._fused_forward`` hands over for a ``synthetic.make_spec(L=2, ...)`` stack: an inner layer with mixing
matrix and Linear mean function (D = Dx, R, P = Dx), a plain final layer with the Zero mean function (D = Dx, R = P = Dy), injected noise
on both, the bound's descriptor with per-layer outputs, or the predictive / sampling call of N points x S samples."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import forward_variant_cases as fv   # noqa: E402
from test_fw_plan_host import COLS, F, GOLDEN, Call, _c, plan   # noqa: E402

from dgps_with_iwvi_amd import _abi   # noqa: E402


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi.lib()


def row_call(r, outs=True):
    """The forward call of a runnable row, as the device model makes it."""
    s = fv.STACKS[r.stack]
    if r.tail == fv.TAIL_BOUND:
        B, K = r.shape
        call = Call(_c(tail=0, M=s["M"], T=B * K, L=fv.L, Dx=fv.DX, R=s["R"], P=fv.DX, noise=1, elbo=1, K=K))
        e = call.elbo
        call.kl_n = (ctypes.c_int32 * 2)(s["R"], fv.DY)           # the per-latent-GP KL shares of the two GP layers
        e.kl_global_counts, e.n_glob, e.scale = call.kl_n, 2, fv.SPEC_B / B
    else:
        N, S = r.shape
        call = Call(_c(tail=r.tail, M=s["M"], T=N, S=S, L=fv.L, Dx=fv.DX, R=s["R"], P=fv.DX, noise=1, elbo=0))
    inner, final = call.descs[0], call.descs[1]
    inner.W, inner.mf_type, inner.mf_A, inner.mf_b = F, _abi.MF_LINEAR, F, F
    final.D, final.R, final.P, final.W = fv.DX, fv.DY, fv.DY, None
    final.mf_type, final.mf_A, final.mf_b = _abi.MF_ZERO, None, None
    call.Dy = fv.DY
    for d in (inner, final):
        d.noise = F
        if outs and r.tail == fv.TAIL_BOUND:
            d.sample = d.mean = d.var = F
    inner.flags = _abi.LAYER_F64_STAGE1 if s["f64"] else 0
    final.flags = 0
    return call


def test_table_pairs_are_the_recorded_instantiations():
    gold = np.load(GOLDEN)
    ok = gold["status"] == 0
    recorded = set(zip(gold["cases"][ok, COLS.index("tail")].tolist(), gold["word"][ok].tolist()))
    table = {(r.tail, r.word) for r in fv.ROWS}
    assert table == recorded, "rows without an instantiation %s; instantiations without a row %s" % (
        sorted((t, hex(w)) for t, w in table - recorded), sorted((t, hex(w)) for t, w in recorded - table))
    # every pair has a row that is run or names the test that covers it, and nothing else skips the GPU
    for pair in recorded:
        mine = [r for r in fv.ROWS if (r.tail, r.word) == pair]
        assert any(r.run for r in mine) or all(r.covered_by and r.covered_by.startswith("tests/test_gpu_lean_variant.py::") for r in mine), pair
    not_run = {(r.tail, r.word) for r in fv.ROWS if not r.run}
    assert not_run == {(fv.TAIL_BOUND, 5 | m | s) for m in (fv.LEAN, fv.SHP) for s in (0, fv.S16)}
    assert len({(r.tail, r.word) for r in fv.RUNNABLE}) == len(recorded) - len(not_run)
    assert len(set(map(fv.row_id, fv.RUNNABLE))) == len(fv.RUNNABLE)


def test_covering_tests_exist():
    for r in fv.ROWS:
        if not r.run:
            path, name = r.covered_by.split("::")
            with open(os.path.join(os.path.dirname(HERE), path)) as f:
                assert "def %s(" % name in f.read(), r.covered_by


def test_the_ragged_totals_are_what_the_table_says():
    """ns by T alone, points straddling workgroups, a partial last chunk of the stated size."""
    assert [B * fv.BOUND_K for B in fv.BOUND_B.values()] == [77, 4102, 8197, 12292, 16387]
    assert [fv.PREDICT_N * S for S in fv.PREDICT_S.values()] == [91, 8203, 16393]
    last = {}
    for r in fv.RUNNABLE:
        T, chunk = fv.total_rows(r), 16 * r.ns
        want = min(-(-T // 4096), 5)
        assert r.ns == (want if r.tail == fv.TAIL_BOUND or want % 2 else want - 1)
        assert chunk % r.shape[1] and T % chunk                    # K (S) divides no chunk; the last chunk is partial
        last[(r.tail != fv.TAIL_BOUND, r.ns)] = T % chunk
        if r.tail != fv.TAIL_BOUND or r.ns == 1:                   # few points: none of them is an inducing point (make_spec: Z = X[:M])
            assert fv.data_rows(r.shape[0]).start >= max(s["M"] for s in fv.STACKS.values())
    assert fv.data_rows(fv.SPEC_B) == slice(0, fv.SPEC_B)
    assert last == {(False, 1): 13, (False, 2): 6, (False, 3): 37, (False, 4): 4, (False, 5): 67, (True, 1): 11, (True, 3): 43, (True, 5): 73}


@pytest.mark.parametrize("r", fv.RUNNABLE, ids=fv.row_id)
def test_row_plans_to_its_word(lib, r):
    T = fv.total_rows(r)
    for outs in (True, False):                                    # (the bound tail runs with and without per-layer outputs)
        rc, word, grid, lds, text = plan(lib, row_call(r, outs))
        assert rc == 0, text
        assert word == r.word, "%s planned %#x" % (fv.row_id(r), word)
        assert grid == -(-T // (16 * r.ns)) and 0 < lds <= 160 * 1024
    # the flags the table states are what the word says
    s = fv.STACKS[r.stack]
    nbk = -(-s["M"] // 16)
    assert bool(r.word & fv.S16) == (nbk % 2 == 0 and not s["f64"]) and bool(r.word & fv.BIG) == (nbk > 8 or s["f64"])
    assert bool(r.word & fv.F64) == s["f64"] and not r.word & (fv.LEAN | fv.SHP) and r.word & 0xff == r.ns


@pytest.mark.parametrize("stack", list(fv.STACKS))
def test_stack_is_as_well_conditioned_as_the_stacks_the_tolerances_are_stated_for(stack):
    """max / min of diag(Lm) of every GP layer, in float64 from the spec alone (what ``DGP_VI.autotune_f64`` measures on the device)."""
    from dgps_with_iwvi_amd import synthetic
    from oracle import iwvi_oracle as O
    spec = synthetic.make_spec(**fv.spec_kwargs(stack))
    for l in spec["layers"]:
        assert l["Z"].shape[1] == fv.DX > 3                       # (settings.f64_auto_max_dim: no layer drifts to the float64 route)
        d = np.diag(np.linalg.cholesky(O.Kuu(l["Z"], O.RBF(fv.DX, variance=l["var"], lengthscales=l["ls"]))))
        assert d.max() / d.min() <= fv.MAX_DIAG_RATIO, (stack, d.max() / d.min())
