"""The float64 restatement of ``iwvi_psis_summary`` (tests/psis_reference.py) pinned by PROPERTIES, not by the kernel: the GPU tests
compare the kernel with it, so it has to be right on its own."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import psis_reference as R   # noqa: E402


@pytest.mark.parametrize("k", [0.3, 0.7])
def test_khat_recovers_the_shape_of_pareto_weights(k):
    """l = k Exp(1): the weights exp(l) are Pareto with shape k.  Mean khat over 50 seeded replicates at S = 16384 within 0.05 of k."""
    got = []
    for rep in range(50):
        rng = np.random.default_rng([7, rep, int(k * 10)])
        got.append(R.psis_point(k * rng.exponential(1.0, 16384))[2])
    got = np.array(got)
    print("k = %.1f: mean khat %.4f, sd %.4f" % (k, got.mean(), got.std()))
    assert np.isfinite(got).all()
    assert abs(got.mean() - k) < 0.05, (k, got.mean(), got.std())


def test_a_constant_shifts_the_estimates_and_leaves_the_diagnostics():
    rng = np.random.default_rng(3)
    for S in (21, 64, 257, 2049, 5000):
        l = rng.standard_normal(S) * 1.5
        for c in (-1000.0, -7.25, 0.5, 12.0):                    # (the rounding of l + c moves a log-weight by 1e-13 at most)
            a, b = R.psis_point(l), R.psis_point(l + c)
            assert abs(b[0] - a[0] - c) < 1e-9 and abs(b[3] - a[3] - c) < 1e-9
            assert abs(b[2] - a[2]) < 1e-9 and abs(b[1] - a[1]) < 1e-9 * a[1]


@pytest.mark.parametrize("S", [1, 4, 20, 21, 500])
def test_all_equal_weights(S):
    raw, ess, khat, psis = R.psis_point(np.full(S, -3.25))
    assert khat == np.inf and psis == raw and abs(raw + 3.25) < 1e-12 and abs(ess - S) < 1e-9 * S


@pytest.mark.parametrize("S", [1, 4, 20])
def test_short_samples_have_no_fit(S):
    l = np.random.default_rng(S).standard_normal(S)
    raw, ess, khat, psis = R.psis_point(l)
    assert khat == np.inf and psis == raw
    assert abs(raw - (np.log(np.exp(l).sum()) - math.log(S))) < 1e-12


def test_21_distinct_weights_have_a_finite_khat():
    l = np.random.default_rng(21).standard_normal(21)
    raw, ess, khat, psis = R.psis_point(l)
    assert np.isfinite(khat) and np.isfinite(psis) and 1.0 <= ess <= 21.0


def test_tail_length_switches_formula_at_225():
    assert [R.tail_len(S) for S in (224, 225, 226)] == [45, 45, 46]          # ceil(44.8), 45 = 45, ceil(3 sqrt 226 = 45.1)
    assert 0.2 * 224 < 3 * math.sqrt(224) and 0.2 * 225 == 3 * math.sqrt(225) == 45.0 and 0.2 * 226 > 3 * math.sqrt(226)
    assert R.tail_len(224) == math.ceil(0.2 * 224) and R.tail_len(226) == math.ceil(3 * math.sqrt(226))
    assert R.tail_len(10000) == 300 < math.ceil(0.2 * 10000) and R.tail_len(100) == 20 < math.ceil(3 * math.sqrt(100))
    assert [R.tail_len(S) for S in (1, 4, 20, 21, 16384)] == [1, 1, 4, 5, 384]
    # the switch is visible in the result: at S = 226 the 46 largest distinct weights are the tail, at 225 the 45 largest
    for S, M in ((225, 45), (226, 46)):
        l = np.linspace(-3.0, 0.0, S)
        x = np.sort(l - l.max())
        assert (x > x[S - M - 1]).sum() == M


def test_ties_at_the_cutoff_shorten_the_tail():
    S = 100                                                      # M = 20: cutoff = x[79]
    l = np.linspace(-5.0, 0.0, S)
    a = R.psis_point(l)
    t = l.copy()
    t[80:90] = t[79]                                             # ten entries tied WITH the cutoff: not strictly above it
    x = np.sort(t - t.max())
    assert (x > x[S - 21]).sum() == 10
    b = R.psis_point(t)
    assert np.isfinite(a[2]) and np.isfinite(b[2]) and a[2] != b[2]
    u = l.copy()
    u[80:96] = u[79]                                             # sixteen tied: four left, no fit
    c = R.psis_point(u)
    assert c[2] == np.inf and c[3] == c[0]


def test_minus_infinity_is_a_zero_weight():
    rng = np.random.default_rng(5)
    l = 2.0 * rng.standard_normal(400)
    pad = np.concatenate([l, np.full(100, -np.inf)])
    a, b = R.psis_point(l), R.psis_point(pad)
    assert abs(b[1] - a[1]) < 1e-9 * a[1]                          # the ess does not see zero weights
    assert abs(b[0] - (a[0] + math.log(400) - math.log(500))) < 1e-12
    assert np.isfinite(b[2]) and np.isfinite(b[3])
    raw, ess, khat, psis = R.psis_point(np.full(50, -np.inf))
    assert raw == -np.inf and psis == -np.inf and ess == 0.0 and khat == np.inf


def test_a_nan_gives_nan_in_all_four():
    l = np.random.default_rng(6).standard_normal(64)
    l[17] = np.nan
    assert all(np.isnan(v) for v in R.psis_point(l))
    s = R.summary(np.stack([l, np.zeros(64)]))
    assert np.isnan(s["raw"][0]) and s["raw"][1] == 0.0 and s["khat"][1] == np.inf


def test_smoothing_caps_the_tail_at_the_largest_weight_and_keeps_the_body():
    rng = np.random.default_rng(8)
    l = 3.0 * rng.standard_normal(2000)
    raw, ess, khat, psis = R.psis_point(l)
    assert np.isfinite(khat) and psis <= l.max() + 1e-12
    body = np.sort(l)[:2000 - R.tail_len(2000)]
    assert psis >= np.log(np.exp(body - l.max()).sum()) + l.max() - math.log(2000) - 1e-12


def test_log_weight_assembly_of_both_modes():
    rng = np.random.default_rng(9)
    N, S, Dy = 3, 7, 2
    fm, fv, Y = rng.standard_normal((N, S, Dy)), rng.uniform(0.1, 1.0, (N, S, Dy)), rng.standard_normal((N, Dy))
    kls = [rng.standard_normal((N, S, 2)), rng.standard_normal((N, S, 1))]
    s = 0.37
    from scipy import stats
    pred = stats.norm.logpdf(Y[:, None], fm, np.sqrt(fv + s)).sum(-1) - kls[0].sum(-1) - kls[1].sum(-1)
    vexp = (stats.norm.logpdf(Y[:, None], fm, math.sqrt(s)) - 0.5 * fv / s).sum(-1) - kls[0].sum(-1) - kls[1].sum(-1)
    l0, big0, n0 = R.logw_moments(fm, fv, Y, s, 0, kls)
    l1, big1, n1 = R.logw_moments(fm, fv, Y, s, 1, kls)
    np.testing.assert_allclose(l0, pred, rtol=0, atol=1e-12)
    np.testing.assert_allclose(l1, vexp, rtol=0, atol=1e-12)
    assert n0 == n1 == 8 * Dy + 3 and (big0 >= np.abs(l0) - 1e-12).all()
    terms = rng.standard_normal((N, S, 3))
    lt, bigt, nt = R.logw_terms(terms, kls)
    np.testing.assert_allclose(lt, terms.sum(-1) - kls[0].sum(-1) - kls[1].sum(-1), rtol=0, atol=1e-12)
    assert nt == 6 and (bigt >= np.abs(lt) - 1e-12).all()
