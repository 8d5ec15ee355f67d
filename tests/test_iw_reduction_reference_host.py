"""Pins tests/iw_reduction_reference.py (no GPU): log-mean-exp and softmax against SciPy on every input family, the shard merge
against the unsharded reduction, the heads against float64 autograd of the bound, and the float32 restatement of the device recurrence
against the float64 reference within the rounding the GPU tests allow the kernels."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy.special import logsumexp, softmax

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iw_reduction_reference as R   # noqa: E402

SHAPES = [(3, K) for K in R.ALL_K] + [(65, 5), (257, 65)]


@pytest.mark.parametrize("name", R.FAMILIES)
def test_families_are_float32_valued_and_the_reference_is_finite_on_them(name):
    for B, K in SHAPES:
        L = R.family(name, B, K, seed=1)
        assert L.shape == (B, K) and np.array_equal(L, R.f32(L))
        lp, (m, s) = R.logp(L), R.partials(L)
        w = R.heads(L, np.zeros((B, K, 1)), np.zeros((B, K, 1)), np.zeros((B, 1)), 0.5, 7.0)[0]
        for a in (lp, m, s, w, R.logp(L, mode_vi=True), R.tol_reduce(L), R.tol_vi(L)):
            assert np.all(np.isfinite(a)), (name, B, K)
        np.testing.assert_allclose(lp, logsumexp(L, axis=1) - math.log(K), rtol=1e-14, atol=1e-13)
        np.testing.assert_allclose(w, 7.0 * softmax(L, axis=1), rtol=1e-12, atol=0)
        np.testing.assert_allclose(w.sum(1), 7.0, rtol=1e-13)
        np.testing.assert_allclose(R.logp(L, K_total=K + 9), logsumexp(L, axis=1) - math.log(K + 9), rtol=1e-14, atol=1e-13)
        if name == "wide":                                       # the result is the maximum, up to float32 spacing; one live weight
            assert np.all(np.abs(lp + math.log(K) - L.max(1)) <= R.spacing32(L.max(1)))
            assert np.all((w.astype(np.float32) != 0).sum(1) == 1) and np.all(w.max(1).astype(np.float32) == np.float32(7.0))
        if name == "dominant" and K > 1:
            assert np.all(np.sort(L, 1)[:, -1] - np.sort(L, 1)[:, -2] > 35.0)
            assert {int(p) for p in L.argmax(1)} <= set(R.dominant_positions(K))
            if B >= 5:
                assert {int(p) for p in L.argmax(1)} == set(R.dominant_positions(K))
        if name == "rising":
            assert np.all(np.diff(L, axis=1) > 2.9)
        if name == "ties_two" and K > 1:
            assert np.all((L == L.max(1, keepdims=True)).sum(1) == 2)
        if name == "ties_all":
            assert np.all(L == L[:, :1]) and np.allclose(lp, L[:, 0], rtol=1e-14)


def test_dropping_or_doubling_a_sample_moves_logp_far_beyond_the_tolerance():
    """The near-equal family's point: at K = 130 one sample less or more moves logp by about 1 / (2 K) (a sample that lies low by
    two standard deviations: a little less) -- hundreds of times the tolerance."""
    L = R.family("near_equal", 65, 130, seed=2)
    lp = R.logp(L)
    dropped = np.log(np.exp(L[:, :-1] - L.max(1, keepdims=True)).sum(1)) + L.max(1) - math.log(130)
    doubled = np.log(np.exp(np.concatenate([L, L[:, :1]], 1) - L.max(1, keepdims=True)).sum(1)) + L.max(1) - math.log(130)
    assert np.all(R.tol_reduce(L) < 1e-5)
    assert np.all(np.abs(dropped - lp) > 1.0 / (4 * 130)) and np.all(np.abs(doubled - lp) > 1.0 / (4 * 130))
    assert np.all(np.abs(dropped - lp) > 100 * R.tol_reduce(L)) and np.all(np.abs(doubled - lp) > 100 * R.tol_reduce(L))


@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_merge_of_uneven_shards_is_the_unsharded_reduction(G):
    rng = np.random.default_rng(G)
    B, sizes = 9, [1] + [int(s) for s in rng.integers(2, 9, G - 1)]
    shards = [R.family("near_equal", B, K, seed=10 + i) for i, K in enumerate(sizes)]
    if G > 1:
        shards[1] = shards[1] - 200.0                             # one shard's maximum 200 nats below another's
    L = np.concatenate(shards, 1)
    ms = np.stack([np.stack(R.partials(s), -1) for s in shards])
    np.testing.assert_allclose(R.merge(ms, L.shape[1]), logsumexp(L, axis=1) - math.log(L.shape[1]), rtol=1e-14, atol=1e-13)


def test_bound_is_the_scaled_sum_minus_the_global_terms():
    lp = R.logp(R.family("near_equal", 257, 17, seed=3))
    kls = R.global_kls(3, R.MAX_R, seed=4)
    assert R.bound(lp, 2.5, kls) == pytest.approx(2.5 * lp.sum() - sum(k.sum() for k in kls), rel=1e-14)
    assert R.bound(lp, 2.5) == pytest.approx(2.5 * lp.sum(), rel=1e-14)


@pytest.mark.parametrize("mode_vi", [False, True], ids=["iw", "vi"])
@pytest.mark.parametrize("Dy,n_kl,width", [(1, 0, 1), (3, 1, 3), (1, R.MAX_KL, 1)])
def test_heads_are_the_float64_autograd_gradient_of_the_bound(mode_vi, Dy, n_kl, width):
    rng = np.random.default_rng(5)
    B, K, s, scale = 7, 9, 0.37, 3.25
    fm, fv, Y = rng.standard_normal((B, K, Dy)), rng.uniform(0.01, 0.5, (B, K, Dy)), rng.standard_normal((B, Dy))
    kls = [rng.uniform(0, 2, (B, K, width)) for _ in range(n_kl)]
    glob = R.global_kls(2, 3, seed=6)
    L, big, n_add = R.gaussian_logw(fm, fv, Y, s, kls)
    assert n_add == 3 * Dy + n_kl * width and np.all(big >= np.abs(L))
    tm, tv, ts = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (fm, fv, s))
    tL = (-0.5 * math.log(2 * math.pi) - 0.5 * torch.log(ts) - 0.5 * ((torch.tensor(Y)[:, None, :] - tm) ** 2 + tv) / ts).sum(2)
    for k in kls:
        tL = tL - torch.tensor(k).sum(2)
    np.testing.assert_allclose(L, tL.detach().numpy(), rtol=1e-13, atol=1e-13)
    tL.retain_grad()
    tlp = tL.mean(1) if mode_vi else torch.logsumexp(tL, 1) - math.log(K)
    val = scale * tlp.sum() - sum(float(g.sum()) for g in glob)
    val.backward()
    lp = R.logp(L, mode_vi=mode_vi)
    assert R.bound(lp, scale, glob) == pytest.approx(float(val), rel=1e-13)
    w, dm, dv, dl = R.heads(L, fm, fv, Y, s, scale, mode_vi=mode_vi)
    np.testing.assert_allclose(w, tL.grad.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(dm, tm.grad.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(dv, tv.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert dl == pytest.approx(float(ts.grad), rel=1e-12)


def test_sharded_heads_use_the_global_normaliser():
    L = R.family("near_equal", 5, 12, seed=7)
    lse = logsumexp(L, axis=1)
    w = R.heads(L[:, :5], np.zeros((5, 5, 1)), np.zeros((5, 5, 1)), np.zeros((5, 1)), 1.0, 2.0, lse_global=lse)[0]
    np.testing.assert_allclose(w, 2.0 * softmax(L, axis=1)[:, :5], rtol=1e-12)


def test_regulariser_split_and_global_arrays():
    L = R.family("dominant", 4, 9, seed=8)
    for n, width in ((1, 1), (R.MAX_KL, 3)):
        kls = R.split_regularisers(-L, n, width, seed=9)
        assert len(kls) == n and all(k.shape == (4, 9, width) and np.array_equal(k, R.f32(k)) for k in kls)
        got, big, n_add = R.gaussian_logw(np.zeros((4, 9, 1)), np.zeros((4, 9, 1)), np.zeros((4, 1)), 1.0 / (2 * math.pi), kls)
        assert n_add == 3 + n * width
        np.testing.assert_allclose(got, L, atol=(n * width + 1) * 2.0 ** -24 * 64)
    assert [len(g) for g in R.global_kls(R.MAX_GLOB, R.MAX_R)] == [R.MAX_R] * R.MAX_GLOB


@pytest.mark.parametrize("name", R.FAMILIES)
def test_float32_restatement_of_the_recurrence_stays_within_the_stated_tolerance(name):
    """The device recurrence in NumPy float32 (correctly rounded exp / log) against the float64 reference: within a QUARTER of the 2e-6 term
    plus the spacing term -- the kernels get the factor of 4 for the hardware's exp and log."""
    worst = 0.0
    for B, K in SHAPES:
        L = R.family(name, B, K, seed=11)
        m, s, lp = R.restate_f32(L)
        ref = R.logp(L)
        err = np.abs(lp.astype(np.float64) - ref)
        tol = R.tol_reduce(L) - 2e-6 + 0.5e-6
        worst = max(worst, float((err - (R.tol_reduce(L) - 2e-6)).max()))
        assert np.all(err <= tol), (name, B, K, float(err.max()), float(tol.min()))
        assert np.array_equal(m.astype(np.float64), L.max(1))
    print("%s: worst excess over the spacing term %.3e (allowed 5e-7)" % (name, worst))
