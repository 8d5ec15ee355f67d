"""``iwvi_mvn_sample`` called directly: the factor the device forms is READ (S = N copies of a block, z[s] = e_s, zero mean: the output is
column s of L, exactly) and compared with the rule restated in tests/mvn_factor_reference.py and with float64 Cholesky -- on both sides of
the LDS / scratch switch (N = 192 needs 149 KB of dynamic LDS, N = 193 the caller's scratch), with jitter, on blocks whose factor is exact
in float32 (dead pivots, the clamp, a non-positive diagonal) and on blocks that are rank-deficient by rounding."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvn_factor_reference as mf   # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _call(dev, mean, cov, z, jitter=0.0, with_ws=True):
    """mean [S, N, R], cov [S, R, N, N], z [S, R, N] float32 arrays -> sample [S, N, R] float64 (the output starts as NaN)."""
    from dgps_with_iwvi_amd import _abi
    S, N, R = mean.shape
    md, cd, zd = (torch.as_tensor(np.array(a, dtype=np.float32, order="C"), device=dev) for a in (mean, cov, z))
    out = torch.full((S, N, R), NAN, dtype=torch.float32, device=dev)
    nws = _abi.lib().iwvi_mvn_sample_ws_bytes(S, N, R)
    assert nws == (0 if N <= mf.MVN_LDS_N else 4 * S * R * (N * N + 2 * N))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if (nws and with_ws) else None
    _abi.check(_abi.lib().iwvi_mvn_sample(_abi.ptr(md), _abi.ptr(cd), _abi.ptr(zd), _abi.ptr(out), S, N, R, float(jitter),
                                          _abi.ptr(ws), _abi.stream_ptr()))
    torch.cuda.synchronize()
    return out.double().cpu().numpy()


def _device_factor(dev, blocks, jitter=0.0):
    """blocks [R, N, N] -> the device's L [R, N, N] (float64 holding float32 values): sample[s, n, r] = L_r[n, s] for z[s, r] = e_s."""
    blocks = np.asarray(blocks, dtype=np.float32)
    R, N, _ = blocks.shape
    cov = np.broadcast_to(blocks[None], (N, R, N, N))
    z = np.broadcast_to(np.eye(N, dtype=np.float32)[:, None, :], (N, R, N))
    out = _call(dev, np.zeros((N, N, R), np.float32), cov, z, jitter)
    assert not np.isnan(out).any()
    return out.transpose(2, 1, 0)


def _well_conditioned(N, R, seed):
    G = np.random.default_rng(seed).standard_normal((R, N, N + 5))
    return (G @ G.transpose(0, 2, 1) / N + 0.1 * np.eye(N)).astype(np.float32)


def _check_against_cholesky(L, C64, N):
    """L: the device's factor of the block C64 (float64 holding what the kernel factorised)."""
    assert np.all(np.triu(L, 1) == 0)
    res = np.abs(np.tril(L @ L.T - C64))
    bound = mf.residual_bound(L, N)
    assert np.all(res <= bound), (N, float((res / bound).max()))
    L64 = np.linalg.cholesky(C64)
    tol = np.linalg.cond(C64) * mf.gamma(N + 2) * np.abs(L64).max()
    assert np.abs(L - L64).max() <= tol, (N, np.abs(L - L64).max(), tol)
    return float((res / bound).max()), float(np.abs(L - L64).max() / tol)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 192, 193])
def test_factor_of_well_conditioned_blocks(gpu_device, N):
    """G G^T / N + 0.1 I, two different blocks: residual within 2 gamma_{N+2} |L||L|^T entry-wise (Higham's float32 Cholesky bound, doubled
    for rsqrt and the fma order), L within cond(C) gamma_{N+2} max|L| of the float64 factor, lower triangular.  Then the same factor
    through a call with a non-zero mean and dense z.  Observed on an MI355X: residual / bound <= 0.22 (N = 1; <= 0.05 from N = 63 on), |L - L64| / tol <= 0.22 (N = 1; <= 0.002 from N = 63 on)."""
    C = _well_conditioned(N, 2, N)
    L = _device_factor(gpu_device, C)
    for r in range(2):
        print("N=%d block %d: residual/bound %.3g, |L - L64|/tol %.3g" % ((N, r) + _check_against_cholesky(L[r], C[r].astype(np.float64), N)))
    rng = np.random.default_rng(N + 1)
    mean, z = rng.standard_normal((2, N, 2)).astype(np.float32), rng.standard_normal((2, 2, N)).astype(np.float32)
    got = _call(gpu_device, mean, np.broadcast_to(C[None], (2, 2, N, N)), z)
    ref = mean + np.einsum("rik,srk->sir", L, z.astype(np.float64))
    mag = np.einsum("rik,srk->sir", np.abs(L), np.abs(z).astype(np.float64))
    assert np.all(np.abs(got - ref) <= mf.gamma(N + 1) * mag + np.spacing(np.abs(ref).astype(np.float32)))     # a float32 dot, one add


SMALL_EXACT = [
    ([[4, 2, -2], [2, 1, -1], [-2, -1, 10]], [[2, 0, 0], [1, 0, 0], [-1, 0, 3]]),      # dead pivot in the middle, a live one after it
    ([[1, 2], [2, 1]], [[1, 0], [1, 0]]),                                              # clamp, then dead
    ([[-1, .5], [.5, 4]], [[0, 0], [0, 2]]),                                           # non-positive diagonal entry
    # a POSITIVE pivot below 1e-6 C_jj (2^-21 = 4.8e-7): dead by the rule, where `d > 0` would put 2^-11 / 2^-10.5 = 0.71 into L_21
    ([[1, 1, 1], [1, 1 + 2.0 ** -21, 1 + 2.0 ** -11], [1, 1 + 2.0 ** -11, 2]], [[1, 0, 0], [1, 0, 0], [1, 0, 1]]),
]


def _assert_exact_structure(L, Lref):
    Lref = np.asarray(Lref, dtype=np.float64)
    assert np.all(L[Lref == 0] == 0)                                                   # dead columns and the upper triangle: exactly 0
    assert np.all(np.abs(L - Lref) <= 4 * np.spacing(np.abs(Lref).astype(np.float32)))  # live entries: every operation is exact, 4 ulp for rsqrt


@pytest.mark.parametrize("C,Lref", SMALL_EXACT)
def test_exact_factors(gpu_device, C, Lref):
    assert np.array_equal(mf.factor(np.array(C, dtype=np.float64), dtype=np.float32), np.array(Lref, dtype=np.float32))
    _assert_exact_structure(_device_factor(gpu_device, np.array([C], dtype=np.float32))[0], Lref)


@pytest.mark.parametrize("N", [5, 192, 193])
def test_rank_one_block_is_one_column(gpu_device, N):
    """2.25 11^T -> 1.5 e_1 1^T: pivots 2.25, 0, 0, ...; in LDS (192: the largest launch) and in scratch (193)."""
    L = _device_factor(gpu_device, 2.25 * np.ones((1, N, N), np.float32))[0]
    _assert_exact_structure(L, 1.5 * np.outer(np.ones(N), np.eye(N)[0]))


def test_jitter(gpu_device):
    """jitter != 0: the rank-one block becomes full rank (against the restated rule), a well-conditioned block is chol(C + jitter I);
    both within the residual bound applied to C + jitter I as the kernel forms it (a float32 sum on the diagonal)."""
    for C, jitter in ((2.25 * np.ones((8, 8), np.float32), 1e-2), (_well_conditioned(33, 1, 5)[0], 1e-3)):
        N = C.shape[0]
        L = _device_factor(gpu_device, C[None], jitter)[0]
        Cj = C.copy()
        Cj[np.arange(N), np.arange(N)] += np.float32(jitter)
        Cj = Cj.astype(np.float64)
        print("jitter %g N=%d: residual/bound %.3g, |L - L64|/tol %.3g" % ((jitter, N) + _check_against_cholesky(L, Cj, N)))
        Lr, live = mf.factor(C.astype(np.float64), jitter=float(np.float32(jitter)), return_live=True)
        assert live.all()
        assert np.abs(L - Lr).max() <= np.linalg.cond(Cj) * mf.gamma(N + 2) * np.abs(Lr).max()


@pytest.mark.parametrize("N,rank", [(40, 1), (40, 3), (65, 3)])
def test_rank_deficient_by_rounding(gpu_device, N, rank):
    """fl32(1.5 G G^T), unit-norm rows of G [N, rank]: the trailing pivots are float32 rounding noise of either sign.  Asserted: |L_ij| <=
    sqrt(C_ii) to an ulp, and max |L L^T - C| <= 4 x the larger of the float64 and float32 CPU restatements' own residuals (4: another
    summation order, rsqrt).  NOT asserted: L entry by entry, or which pivots are dead -- a noise pivot near 1e-6 of its diagonal entry can fall on
    either side of the rule in one arithmetic and not in another (the larger N, the larger the noise relative to 1e-6), which is harmless
    to L L^T.  On these inputs, and on the same recipe at (192, 3), both CPU restatements keep exactly `rank` pivots live.
    Residuals / max|C| (device, float64 restatement, float32 restatement) on an MI355X:
      (40, 1): 7.3e-8, 1.5e-16, 1.2e-7;  (40, 3): 3.3e-7, 1.1e-7, 2.7e-7;  (65, 3): 1.3e-6, 2.2e-7, 7.0e-7."""
    G = np.random.default_rng(N * 10 + rank).standard_normal((N, rank))
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    C = np.tril(1.5 * G @ G.T)
    C = (C + np.tril(C, -1).T).astype(np.float32)
    C64 = C.astype(np.float64)
    L = _device_factor(gpu_device, C[None])[0]

    def res(F):
        F = np.asarray(F, dtype=np.float64)
        return float(np.abs(F @ F.T - C64).max())
    r_dev, r64, r32 = res(L), res(mf.factor(C64)), res(mf.factor(C, dtype=np.float32))
    print("rank-deficient N=%d rank=%d: residual / max|C| device %.3g, float64 restatement %.3g, float32 restatement %.3g"
          % (N, rank, r_dev / C64.max(), r64 / C64.max(), r32 / C64.max()))
    bound = np.sqrt(np.maximum(np.diagonal(C), 0)).astype(np.float32)
    assert np.all(np.abs(L) <= (bound + np.spacing(bound)).astype(np.float64)[:, None])
    assert np.all(np.triu(L, 1) == 0)
    assert r_dev <= 4 * max(r64, r32)


@pytest.mark.parametrize("N", [5, 193])
def test_layout_of_blocks_means_and_draws(gpu_device, N):
    """S = 3, R = 2, every block, mean and z different: the [S, N, R] / [S, R, N, N] / [S, R, N] indexing and, at N = 193, each
    block's own slice of the scratch -- against per-block float64 Cholesky."""
    S, R = 3, 2
    rng = np.random.default_rng(N)
    C = _well_conditioned(N, S * R, 7 * N).reshape(S, R, N, N)
    mean = (3 * rng.standard_normal((S, N, R))).astype(np.float32)
    z = rng.standard_normal((S, R, N)).astype(np.float32)
    got = _call(gpu_device, mean, C, z)
    assert not np.isnan(got).any()
    for s in range(S):
        for r in range(R):
            C64 = C[s, r].astype(np.float64)
            L64 = np.linalg.cholesky(C64)
            ref = mean[s, :, r] + L64 @ z[s, r]
            az = np.abs(z[s, r]).astype(np.float64)
            # the factor's own error (cond gamma max|L|, as above) on every term, a float32 dot product, one rounded add
            tol = (np.linalg.cond(C64) * mf.gamma(N + 2) * np.abs(L64).max() * az.sum() + mf.gamma(N + 1) * (np.abs(L64) @ az)
                   + np.spacing(np.abs(ref).astype(np.float32)))
            assert np.all(np.abs(got[s, :, r] - ref) <= tol), (s, r, float((np.abs(got[s, :, r] - ref) / tol).max()))


def test_arguments(gpu_device):
    from dgps_with_iwvi_amd import _abi
    lib = _abi.lib()
    assert lib.iwvi_mvn_sample_ws_bytes(3, 192, 2) == 0 and lib.iwvi_mvn_sample_ws_bytes(7, 1, 32) == 0
    assert lib.iwvi_mvn_sample_ws_bytes(3, 193, 2) == 4 * 3 * 2 * (193 * 193 + 2 * 193)
    N = 193
    C = torch.eye(N, device=gpu_device).reshape(1, 1, N, N).contiguous()
    m, z = torch.zeros(1, N, 1, device=gpu_device), torch.ones(1, 1, N, device=gpu_device)
    out = torch.full((1, N, 1), NAN, device=gpu_device)
    rc = lib.iwvi_mvn_sample(_abi.ptr(m), _abi.ptr(C), _abi.ptr(z), _abi.ptr(out), 1, N, 1, 0.0, None, _abi.stream_ptr())
    assert rc == _abi.ERR_ARG and b"scratch" in lib.iwvi_last_error()                  # N > 192 without ws
    assert lib.iwvi_mvn_sample(_abi.ptr(m), _abi.ptr(C), _abi.ptr(z), _abi.ptr(out), 0, N, 1, 0.0, None, _abi.stream_ptr()) == 0   # S = 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                                # neither call wrote anything
