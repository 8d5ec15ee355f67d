"""Host reference for ``iwvi_lik_sample_y`` (NumPy / SciPy, float64): the conditional CDFs and PMFs of every likelihood from the
definitions in include/iwvi_hip.h, the statistics the GPU test asserts, the inputs it uses, and NumPy samplers of the same distributions --
correct ones and deliberately perturbed ones (tests/test_lik_sample_reference_host.py: every statistic passes on the former and fires on
the latter, which pins the bounds without a GPU).

BOUNDS (derived, not tuned; some seventy statistics give a false-alarm probability of about 1e-7 in total):
  KS        D <= 3.3 / sqrt(n)              false alarm 2 exp(-2 3.3^2) = 7e-10
  z         |z| <= 6                        false alarm 2e-9
  chi^2     <= chi2.isf(1e-9, dof)
"""
import numpy as np
from scipy import special, stats

N_STAT = 1 << 20
KS_C = 3.3
Z_MAX = 6.0
CHI2_P = 1e-9
JIT = 1e-3
PTRS_MIN = 10.0                 # csrc/likelihood_sample.hip: inversion below, PTRS from here on
POIS_NORMAL = float(1 << 24)    # ... and the rounded normal from here on
BINSIZE = 1.5
ORD_EDGES = np.array([-1.0, 0.0, 0.7, 2.0])
ORD_SIGMA = 0.8
# continuous cases of the GPU test: name -> (type, parameters)
CONTINUOUS = {"gaussian": ("gaussian", dict(variance=0.3)), "student_t": ("student_t", dict(scale=0.7, df=4.0)),
              "exponential": ("exponential", {}), "gamma_2.5": ("gamma", dict(shape=2.5)), "gamma_0.5": ("gamma", dict(shape=0.5)),
              "beta_6": ("beta", dict(scale=6.0)), "beta_2": ("beta", dict(scale=2.0))}
BETA_RANGE = {"beta_6": 1.0, "beta_2": 0.5}          # fmean in [-r, r], fvar = NULL: alpha, beta >= 0.6
POISSON_RATES = [0.3, 4.0, 50.0, 1000.0, 1e5, 0.99 * PTRS_MIN, 1.01 * PTRS_MIN, 0.99 * POIS_NORMAL, 1.01 * POIS_NORMAL]


def ks_bound(n):
    return KS_C / np.sqrt(n)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def moments(n, seed, lo=-3.0, hi=3.0):
    """mu in [lo, hi], v log-uniform in [1e-4, 4], both ends present, float32."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(lo, hi, n)
    v = np.exp(rng.uniform(np.log(1e-4), np.log(4.0), n))
    mu[:2] = lo, hi
    v[:2] = 1e-4, 4.0
    return mu.astype(np.float32), v.astype(np.float32)


def beta_moments(n, seed, r):
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-r, r, n)
    mu[:2] = -r, r
    return mu.astype(np.float32)


# ---- definitions ---------------------------------------------------------------------------------------------------------------------
def ip(f, jit=JIT):
    return special.ndtr(f) * (1.0 - 2.0 * jit) + jit


def cdf(kind, y, f, **p):
    """F(y | f), float64, for the continuous types."""
    y, f = np.asarray(y, np.float64), np.asarray(f, np.float64)
    if kind == "gaussian":
        return special.ndtr((y - f) / np.sqrt(p["variance"]))
    if kind == "student_t":
        return stats.t.cdf((y - f) / p["scale"], p["df"])
    if kind == "exponential":
        return -np.expm1(-y * np.exp(-f))
    if kind == "gamma":
        return special.gammainc(p["shape"], y * np.exp(-f))
    if kind == "beta":
        m = ip(f)
        return special.betainc(m * p["scale"], p["scale"] - m * p["scale"], y)
    raise ValueError(kind)


def ordinal_probs(f, edges=ORD_EDGES, sigma=ORD_SIGMA):
    """[n, bins]: P_j(f) / sum_k P_k(f).  The jitter's factor 1 - 2e-3 is common to every P_j and cancels."""
    f = np.asarray(f, np.float64).reshape(-1, 1)
    c = special.ndtr((np.asarray(edges)[None, :] - f) / sigma)
    c = np.concatenate([np.zeros_like(f), c, np.ones_like(f)], 1)
    return np.diff(c, axis=1)


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
def ks_D(u):
    """Kolmogorov-Smirnov distance of ``u`` from the uniform distribution on [0, 1]."""
    u = np.sort(np.asarray(u, np.float64).ravel())
    n = u.size
    i = np.arange(1, n + 1)
    return float(max(np.max(i / n - u), np.max(u - (i - 1) / n)))


def binned_z(resid, var, key, nbins=8):
    """Sort by ``key`` into ``nbins`` equal bins -> per bin sum(resid) / sqrt(sum(var))."""
    order = np.argsort(np.asarray(key).ravel(), kind="stable")
    r, v = np.asarray(resid, np.float64).ravel()[order], np.asarray(var, np.float64).ravel()[order]
    return np.array([r[c].sum() / np.sqrt(v[c].sum()) for c in np.array_split(np.arange(r.size), nbins)])


def bernoulli_z(y, f):
    p = ip(np.asarray(f, np.float64))
    return binned_z(np.asarray(y, np.float64) - p, p * (1.0 - p), p)


def poisson_z(y, lam, nbins=8):
    """Per bin of rate: the mean z sum(y - lam) / sqrt(sum lam) and the dispersion z (sum (y - lam)^2 / lam - n) / sqrt(sum(2 + 1 / lam))."""
    y, lam = np.asarray(y, np.float64).ravel(), np.asarray(lam, np.float64).ravel()
    order = np.argsort(lam, kind="stable")
    y, lam = y[order], lam[order]
    zm, zd = [], []
    for c in np.array_split(np.arange(y.size), nbins):
        zm.append((y[c] - lam[c]).sum() / np.sqrt(lam[c].sum()))
        zd.append((((y[c] - lam[c]) ** 2 / lam[c]).sum() - c.size) / np.sqrt((2.0 + 1.0 / lam[c]).sum()))
    return np.array(zm), np.array(zd)


def bernoulli_fixed_z(y, fm):
    """All moments at one ``fm`` (fvar = NULL): z of the count of ones.  At fm = -6 / +6 the jitter IS the probability of the rare label
    (1049 of 2^20 expected, about 0 without it): the case with power for the jitter, which the bins over wide moments lack."""
    y = np.asarray(y, np.float64).ravel()
    p = float(ip(fm))
    return float((y.sum() - y.size * p) / np.sqrt(y.size * p * (1.0 - p)))


def beta_dispersion_z(y, f, scale):
    """Pooled z of sum((y - m)^2 - Var) with m = ip(f), Var = m (1 - m) / (scale + 1), against the Beta's own fourth moment: the scale
    moves the PIT by little (KS D = 0.0029 for x 1.02 at scale 6) but the variance by scale / (scale + 1) of its error."""
    y, m = np.asarray(y, np.float64).ravel(), ip(np.asarray(f, np.float64).ravel())
    a, b = m * scale, scale - m * scale
    var = m * (1.0 - m) / (scale + 1.0)
    mu4 = (stats.beta.stats(a, b, moments="k") + 3.0) * var ** 2
    return float(((y - m) ** 2 - var).sum() / np.sqrt((mu4 - var ** 2).sum()))


def ordinal_f(n, seed):
    """f uniform over the edges and a margin, for fvar = NULL: the case in which sigma is seen (float32)."""
    f = np.random.default_rng(seed).uniform(-2.5, 3.5, n)
    f[:2] = -2.5, 3.5
    return f.astype(np.float32)


def ordinal_sigma_z(y, f, edges=ORD_EDGES, sigma=ORD_SIGMA):
    """Pooled z of sum w (y - E[y | f]) with w = d E[y | f] / d log sigma (a 1 % difference quotient): the direction in which an error
    of sigma moves the labels.  Per-bin counts pooled over wide moments barely move with sigma (|z| = 2.6 for x 1.02); this gives about 8."""
    j = np.arange(len(edges) + 1)
    P = ordinal_probs(f, edges, sigma)
    Ey = (P * j).sum(1)
    Vy = (P * j * j).sum(1) - Ey ** 2
    w = ((ordinal_probs(f, edges, 1.01 * sigma) * j).sum(1) - Ey) / 0.01
    return float((w * (np.asarray(y, np.float64).ravel() - Ey)).sum() / np.sqrt((w * w * Vy).sum()))


def ordinal_z(y, f, edges=ORD_EDGES, sigma=ORD_SIGMA):
    P = ordinal_probs(f, edges, sigma)
    y = np.asarray(y).ravel()
    return np.array([((y == j) - P[:, j]).sum() / np.sqrt((P[:, j] * (1.0 - P[:, j])).sum()) for j in range(P.shape[1])])


def _pool(obs, exp, least=5.0):
    """Pool neighbouring cells from the left until each holds an expected count of ``least``; the remainder joins the last cell."""
    o, e, out_o, out_e = 0.0, 0.0, [], []
    for a, b in zip(obs, exp):
        o += a
        e += b
        if e >= least:
            out_o.append(o)
            out_e.append(e)
            o = e = 0.0
    if out_e:
        out_o[-1] += o
        out_e[-1] += e
    return np.array(out_o), np.array(out_e)


def poisson_chi2(y, lam):
    """chi^2 goodness of fit of ``y`` against Poisson(lam) -> (chi2, dof, limit).  Cells are the integers, pooled to an expected count of
    at least 5, the tails folded into the end cells.  From 2^24 on a float32 target holds only EVEN integers: round-to-nearest sends the
    half-open unit intervals around an odd integer to its even neighbours, so the cells are the even integers with
    pmf(2k) + (pmf(2k - 1) + pmf(2k + 1)) / 2 (the pmf is smooth at that rate: the split is exact to 1 / lam)."""
    y = np.asarray(y, np.float64).ravel()
    n = y.size
    sd = np.sqrt(lam)
    lo, hi = int(max(0.0, np.floor(lam - 8.0 * sd - 10.0))), int(np.ceil(lam + 8.0 * sd + 10.0))
    step = 2 if lam >= POIS_NORMAL else 1
    if step == 2:
        lo -= lo % 2
        hi += hi % 2
    k = np.arange(lo, hi + 1)
    pmf = stats.poisson.pmf(k, lam)
    if step == 2:
        cells = pmf[0::2].copy()
        odd = pmf[1::2]
        cells[:-1] += 0.5 * odd
        cells[1:] += 0.5 * odd
        pmf = cells
    idx = np.clip(np.rint((y - lo) / step), 0, pmf.size - 1).astype(np.int64)
    obs = np.bincount(idx, minlength=pmf.size).astype(np.float64)
    exp = pmf * n
    exp[0] += n * stats.poisson.cdf(lo - 1, lam)             # the tails (8 standard deviations out) fold into the end cells
    exp[-1] += n * stats.poisson.sf(hi, lam)
    o, e = _pool(obs, exp)
    chi2 = float(((o - e) ** 2 / e).sum())
    dof = o.size - 1
    return chi2, dof, float(stats.chi2.isf(CHI2_P, dof))


def chi2_counts(obs, probs):
    obs = np.asarray(obs, np.float64)
    e = obs.sum() * np.asarray(probs, np.float64)
    return float(((obs - e) ** 2 / e).sum()), obs.size - 1, float(stats.chi2.isf(CHI2_P, obs.size - 1))


def hit_z(hits, n, eps):
    return (hits - n * (1.0 - eps)) / np.sqrt(n * eps * (1.0 - eps))


# ---- NumPy samplers (correct, or perturbed) -------------------------------------------------------------------------------------------
def sample(kind, f, rng, shape_mult=1.0, link_mult=1.0, jit=JIT, normal_t=False, **p):
    """y ~ p(y | f).  Perturbations: ``shape_mult`` scales the shape / scale parameter, ``link_mult`` the link's argument, ``jit`` replaces
    the probit jitter, ``normal_t`` replaces the Student-t by the normal of its variance."""
    f = np.asarray(f, np.float64) * link_mult
    n = f.shape
    if kind == "gaussian":
        return f + np.sqrt(p["variance"] * shape_mult) * rng.standard_normal(n)
    if kind == "bernoulli":
        return (rng.uniform(size=n) < ip(f, jit)).astype(np.float64)
    if kind == "student_t":
        s, df = p["scale"] * shape_mult, p["df"]
        if normal_t:
            return f + s * np.sqrt(df / (df - 2.0)) * rng.standard_normal(n)
        return f + s * rng.standard_normal(n) / np.sqrt(rng.gamma(0.5 * df, size=n) / (0.5 * df))
    if kind == "poisson":
        return rng.poisson(p["binsize"] * np.exp(f)).astype(np.float64)
    if kind == "exponential":
        return -np.exp(f) * shape_mult * np.log(1.0 - rng.uniform(size=n))
    if kind == "gamma":
        return np.exp(f) * rng.gamma(p["shape"] * shape_mult, size=n)
    if kind == "beta":
        m = ip(f, jit)
        s = p["scale"] * shape_mult
        ga, gb = rng.gamma(m * s), rng.gamma(s - m * s)
        return ga / (ga + gb)
    if kind == "ordinal":
        P = ordinal_probs(f, p.get("edges", ORD_EDGES), p.get("sigma", ORD_SIGMA) * shape_mult)
        return (rng.uniform(size=n)[:, None] > np.cumsum(P, 1)[:, :-1]).sum(1).astype(np.float64)
    raise ValueError(kind)


def draw_f(mu, v, rng):
    return np.asarray(mu, np.float64) + np.sqrt(np.asarray(v, np.float64)) * rng.standard_normal(np.shape(mu))
