"""NumPy float64 restatement of the proper scoring rules of dgps_with_iwvi_amd.evaluation, BY THE DEFINITIONS: the CRPS and the energy score
by the double sum over all pairs of samples (not the sorted-sum identity the kernel uses, not an upper triangle), the counts by comparison,
the quantiles by ``np.quantile``, the pinball loss from those.  Every function returns the terms the tolerances are stated in (A and
G / S^2, or B / S^2) beside the scores.  Samples are taken as given (float32 values widened to float64)."""
import math

import numpy as np


def crps(samples, y):
    """samples [S, N], y [N] -> dict(crps, crps_fair, A, G_over_S2) [N] each: A = mean_s |x_s - y|, G = 1/2 sum_s sum_t |x_s - x_t|."""
    x = np.asarray(samples, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    S, N = x.shape
    A = np.abs(x - y[None, :]).mean(0)
    G = np.empty(N)
    for n in range(N):                                                   # S^2 terms per point, in row blocks (S = 16384: 2 GiB at once)
        col, tot = x[:, n], 0.0
        for lo in range(0, S, 1024):
            tot += np.abs(col[lo:lo + 1024, None] - col[None, :]).sum()
        G[n] = 0.5 * tot
    return {"crps": A - G / S ** 2, "crps_fair": A - G / (S * (S - 1.0)), "A": A, "G_over_S2": G / S ** 2}


def counts(samples, y):
    """-> (below, equal) [N] int64: #{s: x_s < y}, #{s: x_s == y}, on the values as given."""
    x = np.asarray(samples)
    y = np.asarray(y).reshape(-1)
    return (x < y[None, :]).sum(0).astype(np.int64), (x == y[None, :]).sum(0).astype(np.int64)


def quantiles(samples, probs):
    """-> [N, n_probs] float64, NumPy's default (linear) rule."""
    return np.quantile(np.asarray(samples, dtype=np.float64), np.asarray(probs, dtype=np.float64), axis=0).T


def pinball(samples, y, probs):
    """-> (loss [N, n_probs], |y - Q| [N, n_probs]): max(tau (y - Q), (tau - 1) (y - Q))."""
    Q = quantiles(samples, probs)
    tau = np.asarray(probs, dtype=np.float64)[None, :]
    d = np.asarray(y, dtype=np.float64).reshape(-1, 1) - Q
    return np.maximum(tau * d, (tau - 1.0) * d), np.abs(d)


def energy(samples, Y):
    """samples [S, N, D], Y [N, D] -> dict(energy, energy_fair, A, B_over_S2) [N] each: A = mean_s |x_s - y|, B = sum_{s<t} |x_s - x_t|
    = half the sum over ALL ordered pairs, Euclidean norms."""
    x = np.asarray(samples, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    S, N, D = x.shape
    A = np.sqrt(((x - Y[None]) ** 2).sum(-1)).mean(0)
    B = np.empty(N)
    for n in range(N):
        p, tot = x[:, n, :], 0.0
        for lo in range(0, S, 512):
            tot += np.sqrt(((p[lo:lo + 512, None, :] - p[None, :, :]) ** 2).sum(-1)).sum()
        B[n] = 0.5 * tot
    return {"energy": A - B / S ** 2, "energy_fair": A - B / (S * (S - 1.0)), "A": A, "B_over_S2": B / S ** 2}


def crps_normal(y, mu=0.0, sigma=1.0):
    """The closed form for N(mu, sigma^2): sigma [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)], z = (y - mu) / sigma."""
    z = (y - mu) / sigma
    Phi = 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
    phi = math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return sigma * (z * (2.0 * Phi - 1.0) + 2.0 * phi - 1.0 / math.sqrt(math.pi))


def pit_midrank(below, equal, S):
    return (np.asarray(below, np.float64) + 0.5 * np.asarray(equal, np.float64) + 0.5) / (S + 1.0)


def calibration_error(pit):
    """sup_u |ECDF(u) - u| over u in [0, 1] by the definition's two one-sided gaps at every jump."""
    p = np.sort(np.asarray(pit, dtype=np.float64).reshape(-1))
    n = p.size
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max((i / n - p).max(), (p - (i - 1.0) / n).max()))


def pit_hist(pit, bins):
    p = np.asarray(pit, dtype=np.float64).reshape(-1)
    return np.bincount(np.clip(np.floor(p * bins).astype(np.int64), 0, bins - 1), minlength=bins)
