"""Float64 NumPy statement of what ``iwvi_psis_summary`` (csrc/psis.hip) computes per point from its S draws: the log-weight in both
input modes, the log-mean weight, Kish's effective sample size, and Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao,
Gabry: "Pareto smoothed importance sampling") with the generalized-Pareto fit of Zhang & Stephens (2009) under the PSIS prior.
TEST INFRASTRUCTURE ONLY: tests/test_psis_reference_host.py pins it by properties; tests/test_gpu_psis.py and
tests/test_gpu_importance_model.py compare the kernel with it on the same float32 inputs.

Per point, on its log-weights l [S]:
    x       = sort(l - max l)
    M       = ceil(min(0.2 S, 3 sqrt(S)));  cutoff = max(x[S - M - 1], log(2^-126));  tail = the entries STRICTLY above cutoff
    n <= 4  (S < 21, all-equal weights, ...): khat = +inf, psis = raw
    else    e = exp(tail) - exp(cutoff) (ascending);  (k, sigma) = the fit;  khat = (n k + 5) / (n + 10);
            tail_i <- min(log(sigma expm1(-khat log1p(-p_i)) / khat + exp(cutoff)), 0), p_i = (i - 0.5) / n;  not finite khat / sigma: unsmoothed
A -inf log-weight is a zero weight; all -inf: raw = psis = -inf, ess = 0, khat = +inf; a NaN (or a +inf, which has no weight to be
relative to) anywhere in the point's inputs: NaN in all four."""
import math

import numpy as np

LOG_TINY = math.log(2.0 ** -126)
EPS = 2.0 ** -52
MAX_S = 16384                                                    # csrc/sample_sort.h: SS_MAX_S
# the GPU tests' bounds on khat (absolute), psis (a multiple of the bound on raw) and ess (relative): tests/test_gpu_psis.py says where they
# come from; gpu_psis_bound caps the psis bound at the bound on raw + 1e-5
GPU_KHAT_TOL, GPU_PSIS_MULT, GPU_ESS_RTOL = 4 * 1.15e-7, 4 * 0.607, 4 * 1.24e-7


def gpu_psis_bound(tol_raw):
    return np.minimum(GPU_PSIS_MULT * np.asarray(tol_raw), np.asarray(tol_raw) + 1e-5)


def tail_len(S):
    """M = ceil(min(0.2 S, 3 sqrt(S)))."""
    return int(math.ceil(min(0.2 * S, 3.0 * math.sqrt(S))))


def gpd_fit(e):
    """Zhang & Stephens' estimator with the PSIS prior on ascending exceedances e [n] -> (khat, sigma)."""
    e = np.asarray(e, dtype=np.float64)
    n = e.size
    m = 30 + int(math.floor(math.sqrt(n)))
    j = np.arange(1, m + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        b = (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * e[int(math.floor(n / 4.0 + 0.5)) - 1]) + 1.0 / e[n - 1]
        k = np.log1p(-b[:, None] * e[None, :]).mean(1)
        L = n * (np.log(-b / k) - k - 1.0)
        w = np.exp(L - L.max())
        w = w / w.sum()
        w = np.where(w < 10.0 * EPS, 0.0, w)
        w = w / w.sum()
        bp = float((w * b).sum())
        kp = float(np.log1p(-bp * e).mean())
        sigma = -kp / bp
        khat = (n * kp + 5.0) / (n + 10.0)
    return khat, sigma


def psis_point(l):
    """l [S] float64 -> (raw, ess, khat, psis)."""
    l = np.asarray(l, dtype=np.float64)
    S = l.size
    nan = float("nan")
    if np.isnan(l).any() or (l == np.inf).any():
        return nan, nan, nan, nan
    mx = float(l.max())
    if mx == -np.inf:
        return -np.inf, 0.0, np.inf, -np.inf
    x = np.sort(l - mx)
    w = np.exp(x)
    s1 = float(w.sum())
    raw = mx + math.log(s1) - math.log(S)
    ess = min(max(s1 * s1 / float((w * w).sum()), 1.0), float(S))
    M = tail_len(S)
    if S - M - 1 < 0:
        return raw, ess, np.inf, raw
    cutoff = max(float(x[S - M - 1]), LOG_TINY)
    tail = x[x > cutoff]
    n = tail.size
    if n <= 4:
        return raw, ess, np.inf, raw
    ec = math.exp(cutoff)
    khat, sigma = gpd_fit(np.exp(tail) - ec)
    if not (math.isfinite(khat) and math.isfinite(sigma)):
        return raw, ess, khat, raw
    p = (np.arange(1, n + 1, dtype=np.float64) - 0.5) / n
    with np.errstate(all="ignore"):
        q = -sigma * np.log1p(-p) if abs(khat) < EPS else sigma * np.expm1(-khat * np.log1p(-p)) / khat
        sm = np.minimum(np.log(q + ec), 0.0)
    lw = x.copy()
    lw[S - n:] = sm
    psis = mx + math.log(float(np.exp(lw).sum())) - math.log(S)
    return raw, ess, khat, psis


def summary(logw):
    """logw [N, S] -> dict of float64 [N]: raw, ess, khat, psis."""
    logw = np.asarray(logw, dtype=np.float64)
    out = np.array([psis_point(r) for r in logw], dtype=np.float64).reshape(-1, 4)
    return {"raw": out[:, 0], "ess": out[:, 1], "khat": out[:, 2], "psis": out[:, 3]}


# ---- the log-weight of a draw, both input modes: value, the largest |term or partial sum| in the device's order, additions -----------
def logw_terms(terms, kls=()):
    """terms [N, S, n_terms], kls: [N, S, width] each -> (l, big, n_add): l = sum_j terms - sum of the regularisers."""
    terms = np.asarray(terms, dtype=np.float64)
    acc, big, n_add = np.zeros(terms.shape[:2]), np.zeros(terms.shape[:2]), 0
    with np.errstate(invalid="ignore"):
        for j in range(terms.shape[-1]):
            acc = acc + terms[..., j]
            big = np.maximum.reduce([big, np.abs(terms[..., j]), np.abs(acc)])
            n_add += 1
        for kl in kls:
            kl = np.asarray(kl, dtype=np.float64)
            for c in range(kl.shape[-1]):
                acc = acc - kl[..., c]
                big = np.maximum.reduce([big, np.abs(kl[..., c]), np.abs(acc)])
                n_add += 1
    return acc, big, n_add


def logw_moments(fmean, fvar, Y, lik_var, var_exp, kls=()):
    """fmean, fvar [N, S, Dy], Y [N, Dy].  var_exp = 0: sum_d log N(y; m, v + s); 1: sum_d [log N(y; m, s) - v / (2 s)]; minus the
    regularisers.  n_add counts 8 float32 roundings per output, each of at most one spacing of the largest magnitude met: y - m (whose
    relative error the square doubles: two), the square, v + s, the logarithm, the product inside it, the quotient, the difference of the
    two halves and the accumulation."""
    fmean, fvar, Y = (np.asarray(a, dtype=np.float64) for a in (fmean, fvar, Y))
    N, S, Dy = fmean.shape
    acc, big = np.zeros((N, S)), np.zeros((N, S))
    for d in range(Dy):
        e = Y[:, None, d] - fmean[..., d]
        if var_exp:
            c, q = -0.5 * math.log(2 * math.pi * lik_var), 0.5 * (e * e + fvar[..., d]) / lik_var
        else:
            v = fvar[..., d] + lik_var
            c, q = -0.5 * np.log(2 * math.pi * v), 0.5 * e * e / v
        acc = acc + (c - q)
        big = np.maximum.reduce([big, np.abs(q), np.abs(c - q), np.abs(acc), np.abs(c) * np.ones_like(q)])
    n_add = 8 * Dy
    for kl in kls:
        kl = np.asarray(kl, dtype=np.float64)
        for c in range(kl.shape[-1]):
            acc = acc - kl[..., c]
            big = np.maximum.reduce([big, np.abs(kl[..., c]), np.abs(acc)])
            n_add += 1
    return acc, big, n_add


# ---- input families of the GPU test (float32 values as float64) ---------------------------------------------------------------------
FAMILIES = ("ln0.5", "ln2", "ln4", "ln0.5_off", "ln2_off", "ln4_off", "quantised", "equal", "dominant_first", "dominant_last",
            "quarter_ninf", "all_ninf", "one_nan")


def family(name, N, S, seed=0):
    rng = np.random.default_rng([seed, N, S, FAMILIES.index(name)])
    z = rng.standard_normal((N, S))
    if name.startswith("ln"):
        L = float(name[2:].split("_")[0]) * z + (-1000.0 if name.endswith("_off") else 0.0)   # (at -1000 the float32 spacing, 6e-5, makes ties)
    elif name == "quantised":
        L = np.round(2.0 * z * 4.0) / 4.0
    elif name == "equal":
        L = np.repeat(rng.uniform(-5, 5, (N, 1)), S, 1)
    elif name in ("dominant_first", "dominant_last"):
        L = z - 40.0
        L[:, 0 if name == "dominant_first" else S - 1] = 0.5
    elif name == "quarter_ninf":
        L = 2.0 * z
        L[:, rng.permutation(S)[:max(S // 4, 1)]] = -np.inf
    elif name == "all_ninf":
        L = np.full((N, S), -np.inf)
    elif name == "one_nan":
        L = 2.0 * z
        L[np.arange(N), rng.integers(0, S, N)] = np.nan
        if N > 1:
            L[1] = 2.0 * z[1]                                    # (a clean point beside the NaN ones: it must not be affected)
    else:
        raise ValueError(name)
    return np.asarray(L, dtype=np.float32).astype(np.float64)
