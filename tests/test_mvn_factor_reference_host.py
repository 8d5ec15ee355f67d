"""CPU pins of tests/mvn_factor_reference.py: the float64 run is np.linalg.cholesky on well-conditioned blocks, the documented exact
factors (dead pivot in the middle, clamp then dead, non-positive diagonal, rank one), what the clamp and the dead-pivot rule are for, and
the residual bound on the float32 run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvn_factor_reference as mf   # noqa: E402

EXACT = [
    ([[4, 2, -2], [2, 1, -1], [-2, -1, 10]], [[2, 0, 0], [1, 0, 0], [-1, 0, 3]]),      # dead pivot in the middle, a live one after it
    ([[1, 2], [2, 1]], [[1, 0], [1, 0]]),                                              # clamp, then dead
    ([[-1, .5], [.5, 4]], [[0, 0], [0, 2]]),                                           # non-positive diagonal entry
    # a POSITIVE pivot below 1e-6 C_jj (2^-21 = 4.8e-7): dead by the rule, where `d > 0` would put 2^-11 / 2^-10.5 = 0.71 into L_21
    ([[1, 1, 1], [1, 1 + 2.0 ** -21, 1 + 2.0 ** -11], [1, 1 + 2.0 ** -11, 2]], [[1, 0, 0], [1, 0, 0], [1, 0, 1]]),
    (2.25 * np.ones((5, 5)), 1.5 * np.outer(np.ones(5), np.eye(5)[0])),                # rank one: 1.5 e_1 1^T (first column)
]


def _well_conditioned(N, seed=0):
    G = np.random.default_rng(seed).standard_normal((N, N + 5))
    return G @ G.T / N + 0.1 * np.eye(N)


@pytest.mark.parametrize("N", [1, 2, 17, 64, 193])
def test_float64_run_is_cholesky_on_well_conditioned_blocks(N):
    C = _well_conditioned(N, N)
    L, live = mf.factor(C, return_live=True)
    assert live.all() and np.all(np.triu(L, 1) == 0)
    np.testing.assert_allclose(L, np.linalg.cholesky(C), rtol=1e-12, atol=1e-13)
    Lj = mf.factor(C, jitter=1e-3)
    np.testing.assert_allclose(Lj, np.linalg.cholesky(C + 1e-3 * np.eye(N)), rtol=1e-12, atol=1e-13)
    Cu = C + np.triu(np.full((N, N), 7.0), 1)                                 # only the lower triangle is read
    assert np.array_equal(mf.factor(Cu), L)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("C,Lref", EXACT)
def test_exact_factors(C, Lref, dtype):
    L = mf.factor(np.array(C, dtype=np.float64), dtype=dtype)
    assert L.dtype == np.dtype(dtype)
    assert np.array_equal(L, np.array(Lref, dtype=dtype))


def test_rank_one_at_the_lds_switch_sizes_and_with_jitter():
    for N in (192, 193):
        L = mf.factor(2.25 * np.ones((N, N)), dtype=np.float32)
        assert np.all(L[:, 0] == 1.5) and np.all(L[:, 1:] == 0)
    C = 2.25 * np.ones((8, 8))
    for dtype in (np.float64, np.float32):
        L, live = mf.factor(C, jitter=1e-2, dtype=dtype, return_live=True)
        assert live.all()                                                      # the jitter makes every pivot live
        L = L.astype(np.float64)
        np.testing.assert_allclose(L @ L.T, C + 1e-2 * np.eye(8), rtol=0, atol=1e-14 if dtype == np.float64 else 2e-6)


def test_what_the_clamp_and_the_dead_pivot_rule_are_for():
    # a block that is indefinite "by rounding": rank one plus a perturbation that leaves the second pivot at +3e-7 (live without the rule)
    C = np.array([[1.0, 1.0, 1.0], [1.0, 1.0 + 3e-7, 1.0 + 2e-4], [1.0, 1.0 + 2e-4, 1.0]])
    L = mf.factor(C)
    assert np.all(L[:, 1] == 0) and np.abs(L).max() <= 1.0 + 1e-12
    no_rule = mf.factor(C, dead_rule=False, clamp=False)
    assert no_rule[2, 1] > 0.3                                                 # 2e-4 / sqrt(3e-7): noise amplified 1800 x
    clamped_only = mf.factor(C, dead_rule=False)
    assert np.abs(clamped_only).max() <= 1.0 + 1e-12                           # the clamp alone bounds it by sqrt(C_ii)
    no_clamp = mf.factor(np.array([[1.0, 2.0], [2.0, 1.0]]), clamp=False)
    assert no_clamp[1, 0] == 2.0


@pytest.mark.parametrize("N", [2, 65, 193])
def test_float32_run_meets_the_residual_bound(N):
    C = _well_conditioned(N, 100 + N).astype(np.float32)
    L = mf.factor(C, dtype=np.float32).astype(np.float64)
    res = np.abs(np.tril(L @ L.T - C.astype(np.float64)))
    assert np.all(res <= mf.residual_bound(L, N))
    L64 = np.linalg.cholesky(C.astype(np.float64))
    assert np.abs(L - L64).max() <= np.linalg.cond(C.astype(np.float64)) * mf.gamma(N + 2) * np.abs(L64).max()


def test_gamma():
    assert mf.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6) and mf.gamma(194) == pytest.approx(194 * 2.0 ** -24, rel=2e-5)
