"""NumPy restatement of the rounding-tolerant PSD factorisation inside ``iwvi_mvn_sample`` (k_mvn_sample, csrc/gp_layer.hip).  TEST
INFRASTRUCTURE ONLY: tests/test_mvn_factor_reference_host.py pins this module on the CPU, tests/test_gpu_mvn_sample.py compares the kernel
with it.

The rule, for one block C [N, N] (its lower triangle is read) and a jitter added to the diagonal:
  bound_i = sqrt(max(C_ii + jitter, 0));
  right-looking, column j at a time, on the running lower triangle A (A = tril(C) + jitter I to begin with):
    d = A_jj;  pivot j is LIVE iff d > 1e-6 bound_j^2;
    live:  L_ij = clamp(A_ij / sqrt(d), -bound_i, bound_i) for i > j (the kernel multiplies by rsqrt(d)),  L_jj = min(d / sqrt(d), bound_j);
    dead:  the whole column j of L is 0;
    A_ik -= L_ij L_kj for j < k <= i.
Every operation is rounded to ``dtype`` (float32: the kernel's arithmetic, except that it fuses the update's multiply-add and uses the
hardware rsqrt; float64: the same rule without float32 rounding).  On a well-conditioned block this is the Cholesky factor.
"""
import numpy as np

PIVOT_RTOL = 1e-6          # k_mvn_sample: `d > 1e-6f * bound[j] * bound[j]`
MVN_LDS_N = 192            # csrc/gp_layer.hip: blocks up to this size are factorised in LDS, larger ones in the caller's scratch


def factor(C, jitter=0.0, dtype=np.float64, clamp=True, dead_rule=True, return_live=False):
    """C [N, N] -> L [N, N] of `dtype` (strict upper triangle 0).  ``clamp`` / ``dead_rule`` = False switch a part of the rule off (to
    show what it is for)."""
    dt = np.dtype(dtype).type
    N = C.shape[0]
    A = np.tril(np.asarray(C).astype(dt))
    A[np.arange(N), np.arange(N)] += dt(jitter)
    bound = np.sqrt(np.maximum(np.diagonal(A).copy(), dt(0)))
    live = np.zeros(N, bool)
    for j in range(N):
        d = A[j, j]
        live[j] = bool(d > dt(PIVOT_RTOL) * bound[j] * bound[j]) if dead_rule else bool(d > 0)
        if live[j]:
            inv = dt(1) / np.sqrt(d)
            col = A[j + 1:, j] * inv
            A[j + 1:, j] = np.clip(col, -bound[j + 1:], bound[j + 1:]) if clamp else col
            A[j, j] = min(d * inv, bound[j]) if clamp else d * inv
        else:
            A[j:, j] = dt(0)
        c = A[j + 1:, j]
        A[j + 1:, j + 1:] -= np.tril(np.outer(c, c))
    assert A.dtype == np.dtype(dtype)
    return (A, live) if return_live else A


def gamma(n, u=2.0 ** -24):
    """Higham's gamma_n = n u / (1 - n u)."""
    return n * u / (1.0 - n * u)


def residual_bound(L, N):
    """Entry-wise bound on |L L^T - C| for a float32 Cholesky factor L of an N x N block: Higham (Accuracy and Stability of Numerical
    Algorithms, Thm 10.3) gives gamma_{N+1} (|L| |L|^T)_ij for the textbook algorithm; 2 gamma_{N+2} leaves room for the hardware rsqrt
    (1 ulp) in place of a division by a correctly rounded square root and for the order of the fused updates."""
    aL = np.abs(np.asarray(L, dtype=np.float64))
    return 2.0 * gamma(N + 2) * (aL @ aL.T)
