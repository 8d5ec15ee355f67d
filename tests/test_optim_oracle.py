"""Known-answer pins of the optimiser oracle (oracle/optim_oracle.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import optim_oracle as oo   # noqa: E402


def test_natgrad_with_unit_step_solves_a_conjugate_problem_in_one_step():
    """loss(m, S) = KL[N(m, S) || N(m*, S*)]: the natural gradient with gamma = 1 lands on (m*, S*) from any start
    (the defining property of a natural-gradient step in an exponential family)."""
    rng = np.random.default_rng(0)
    n = 6
    A = rng.standard_normal((n, n)); S_star = A @ A.T + n * np.eye(n); m_star = rng.standard_normal(n)
    L0 = np.tril(rng.standard_normal((n, n))) * 0.3 + np.eye(n); m0 = rng.standard_normal(n)
    P = np.linalg.inv(S_star)
    # gradients of the KL w.r.t. m and L (S = L L^T): dKL/dm = P (m - m*), dKL/dS = 1/2 (P - S^-1) -> dKL/dL = 2 dKL/dS L
    S0 = L0 @ L0.T
    g_m = P @ (m0 - m_star)
    g_L = np.tril(2.0 * (0.5 * (P - np.linalg.inv(S0))) @ L0)
    mu, Ls = oo.natgrad_step(m0[:, None], L0[None], g_m[:, None], g_L[None], 1.0)
    np.testing.assert_allclose(mu[:, 0], m_star, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(Ls[0] @ Ls[0].T, S_star, rtol=1e-9, atol=1e-10)


def test_natgrad_small_step_is_a_descent_direction_and_keeps_S_positive_definite():
    rng = np.random.default_rng(1)
    n = 5
    A = rng.standard_normal((n, n)); S_star = A @ A.T + n * np.eye(n); m_star = rng.standard_normal(n)
    P = np.linalg.inv(S_star)
    kl = lambda m, L: 0.5 * (np.trace(P @ L @ L.T) + (m - m_star) @ P @ (m - m_star) - n
                             + np.log(np.linalg.det(S_star)) - 2 * np.log(np.diag(L)).sum())
    L0 = np.eye(n); m0 = np.zeros(n)
    g_m = P @ (m0 - m_star)
    g_L = np.tril((P - np.linalg.inv(L0 @ L0.T)) @ L0)
    mu, Ls = oo.natgrad_step(m0[:, None], L0[None], g_m[:, None], g_L[None], 0.1)
    assert kl(mu[:, 0], Ls[0]) < kl(m0, L0)
    assert np.all(np.diag(Ls[0]) > 0)


def test_adam_first_step_moves_by_lr_against_the_gradient_sign_and_respects_positivity():
    p = [np.array([1.0, -2.0, 3.0]), np.array([0.5, 2.0])]
    opt = oo.Adam(p, [False, True], lr=0.01)
    new = opt.step([np.array([0.3, -0.2, 10.0]), np.array([5.0, -5.0])])
    np.testing.assert_allclose(new[0], p[0] - 0.01 * np.sign([0.3, -0.2, 10.0]), rtol=0, atol=1e-7)   # |step 1| = lr
    x0 = oo.to_unconstrained(p[1], True)
    np.testing.assert_allclose(oo.to_constrained(x0, True), p[1], rtol=1e-12)
    np.testing.assert_allclose(new[1], oo.to_constrained(x0 - 0.01 * np.sign([5.0, -5.0]), True), rtol=1e-6)
    assert np.all(new[1] > 0)


def test_staircase_decay():
    assert oo.staircase_decay(0.1, 999, 0.5) == 0.1 and oo.staircase_decay(0.1, 1000, 0.5) == 0.05
    assert oo.staircase_decay(0.1, 2500, 0.5) == 0.025


def conjugate_gaussian_case(M, R, seed=0):
    """A Gaussian model that is linear in the whitened u: y_r = A u_r + noise of variance 0.01, N = 4 M points, prior u_r ~ N(0, I).
    -> float32 (q_mu [M, R], q_sqrt [R, M, M]) = (0, I), the float32 roundings of the LOSS gradients there (loss = -ELBO; computed in
    float64), and the closed-form optimum (m*, chol(S*)) in float64: S* = (I + A^T A / s)^-1, m*_r = S* A^T y_r / s.
    Also used by tests/test_gpu_training.py::test_natgrad_unit_step_solves_the_conjugate_problem."""
    rng = np.random.default_rng([seed, M, R])
    N, s = 4 * M, 0.01
    A = rng.standard_normal((N, M)) / np.sqrt(N)
    Y = A @ rng.standard_normal((M, R)) + np.sqrt(s) * rng.standard_normal((N, R))
    q_mu, q_sqrt = np.zeros((M, R), dtype=np.float32), np.tile(np.eye(M, dtype=np.float32), (R, 1, 1))
    # -E_q log p(y | u) + KL[q || N(0, I)] at (m, L): d/dm = -A^T (y - A m) / s + m;  d/dS = A^T A / (2 s) + (I - S^-1) / 2;  d/dL = tril(2 dS L)
    g_mu = (-(A.T @ Y) / s).astype(np.float32)
    g_sqrt = np.tile(np.tril(A.T @ A / s).astype(np.float32), (R, 1, 1))
    S_star = np.linalg.inv(np.eye(M) + A.T @ A / s)
    return q_mu, q_sqrt, g_mu, g_sqrt, S_star @ (A.T @ Y) / s, np.tile(np.linalg.cholesky(S_star), (R, 1, 1))


def within_natgrad_tolerance(got, ref):
    """The natural-gradient step's tolerance (tests/test_gpu_training.py: rtol = 2e-5) with atol = 2e-6 x the largest |ref| of the array."""
    return bool(np.all(np.abs(np.asarray(got, dtype=np.float64) - ref) <= 2e-5 * np.abs(ref) + 2e-6 * np.abs(ref).max()))


def test_oracle_on_float32_gradients_lands_on_the_conjugate_optimum():
    """gamma = 1 from (0, I) on the float32-rounded gradients of the linear-Gaussian model: the oracle is within the device test's
    tolerance of the closed form, so comparing the device with the oracle there tests the known answer."""
    for M, R in ((40, 2), (128, 5), (200, 1)):
        q_mu, q_sqrt, g_mu, g_sqrt, m_star, L_star = conjugate_gaussian_case(M, R)
        mu, Ls = oo.natgrad_step(q_mu, q_sqrt, g_mu, g_sqrt, 1.0)
        assert within_natgrad_tolerance(mu, m_star) and within_natgrad_tolerance(Ls, L_star), (M, R)
        assert 0.02 < np.abs(np.diagonal(L_star, axis1=1, axis2=2)).max() < 0.5      # far from the q_sqrt = I it started at
