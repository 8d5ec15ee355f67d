"""Float64 statement of the importance-weight reductions (models.py:134-150 of the reference: the per-sample log-weight, its
log-mean-exp over the K samples, the softmax weights and the scaled sum over the points), on explicit arrays.  TEST INFRASTRUCTURE ONLY:
tests/test_iw_reduction_reference_host.py pins it against SciPy and float64 autograd; tests/test_gpu_iw_reduction.py and
tests/test_gpu_fused_tail_reduction.py compare every HIP form of the reduction with it.

Arrays are NumPy float64 throughout; ``L`` is [B, K] (point, sample) whatever layout the device reads.  Besides the reference this module
holds the input families of those tests (seeded, rounded to float32 first), the tolerances they share, and a float32 restatement of the
device recurrence (``restate_f32``: SEG lanes, running maximum, rescale) against which a rounding constant may be measured."""
import math

import numpy as np

MAX_KL, MAX_R, MAX_GLOB, MAX_GLOB_BWD = 4, 32, 16, 8           # include/iwvi_hip.h: IWVI_MAX_KL, IWVI_MAX_R; csrc/lv_elbo.hip: MAX_GLOB; IWVI_MAX_LAYERS
ALL_K = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 100, 128, 130)
ALL_B = (1, 3, 63, 64, 65, 257)
FAMILIES = ("near_equal", "dominant", "rising", "wide", "ties_all", "ties_two")


def f32(a):
    """Round to float32, return float64."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def spacing32(x):
    """Distance from |x| to the next float32 above it."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def seg_of(K):
    """Lanes per data point of k_elbo / k_lik_elbo (the host dispatch of csrc/lv_elbo.hip)."""
    return 4 if K <= 4 else 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def partials(L):
    """(m [B], s [B]) = (max_k L, sum_k exp(L - m))."""
    L = np.asarray(L, dtype=np.float64)
    m = L.max(1)
    return m, np.exp(L - m[:, None]).sum(1)


def logp(L, K_total=None, mode_vi=False):
    """logsumexp_k L - log K_total [B]; VI: the mean over k."""
    L = np.asarray(L, dtype=np.float64)
    if mode_vi:
        return L.mean(1)
    m, s = partials(L)
    return m + np.log(s) - math.log(K_total or L.shape[1])


def merge(ms, K_total):
    """[G, B, 2] partials of G shards -> logp [B]."""
    ms = np.asarray(ms, dtype=np.float64)
    m = ms[..., 0].max(0)
    s = (ms[..., 1] * np.exp(ms[..., 0] - m)).sum(0)
    return m + np.log(s) - math.log(K_total)


def bound(lp, scale, kls=()):
    """scale * sum_b logp - sum of the global KL arrays (math.fsum: the exact float64 sum, rounded once)."""
    return scale * math.fsum(np.asarray(lp, dtype=np.float64).tolist()) - math.fsum(v for a in kls for v in np.asarray(a, dtype=np.float64).reshape(-1).tolist())


def heads(L, fmean, fvar, Y, lik_var, scale, mode_vi=False, lse_global=None):
    """w [B, K] = scale softmax_k L (VI: scale / K; ``lse_global`` [B]: scale exp(L - lse_global), a K-shard against the job's
    normaliser), d_mean = w e / s, d_var = -w / (2 s) [B, K, Dy] with e = Y - fmean, and sum_bkd w d/ds of the Gaussian expectation."""
    L, fmean, fvar, Y = (np.asarray(a, dtype=np.float64) for a in (L, fmean, fvar, Y))
    B, K = L.shape
    if mode_vi:
        w = np.full((B, K), scale / K)
    elif lse_global is not None:
        w = scale * np.exp(L - np.asarray(lse_global, dtype=np.float64)[:, None])
    else:
        m, s = partials(L)
        w = scale * np.exp(L - m[:, None]) / s[:, None]
    e = Y[:, None, :] - fmean
    d_mean = w[..., None] * e / lik_var
    d_var = -0.5 * w[..., None] / lik_var * np.ones_like(e)
    d_lik = (w[..., None] * (-0.5 / lik_var + 0.5 * (e * e + fvar) / lik_var ** 2)).sum()
    return w, d_mean, d_var, d_lik


def gaussian_logw(fmean, fvar, Y, lik_var, kls=()):
    """L [B, K] = sum_d [-log(2 pi s) / 2 - ((y - f)^2 + v) / (2 s)] - sum of the local regularisers (models.py:134-142);
    fmean, fvar [B, K, Dy], Y [B, Dy], kls: [B, K, width] each.  Also returns the largest |term or running partial sum| per sample
    [B, K] in the order the device adds them up, and the number of float32 additions per sample (3 per output: the two inside the term and
    the accumulation; 1 per regulariser entry)."""
    fmean, fvar, Y = (np.asarray(a, dtype=np.float64) for a in (fmean, fvar, Y))
    B, K, Dy = fmean.shape
    c0 = -0.5 * math.log(2 * math.pi) - 0.5 * math.log(lik_var)
    acc, big = np.zeros((B, K)), np.zeros((B, K))
    for d in range(Dy):
        q = ((Y[:, None, d] - fmean[..., d]) ** 2 + fvar[..., d]) * (0.5 / lik_var)
        acc = acc + (c0 - q)
        big = np.maximum.reduce([big, np.abs(q), np.abs(c0 - q), np.abs(acc)])
    n_add = 3 * Dy
    for kl in kls:
        kl = np.asarray(kl, dtype=np.float64)
        for j in range(kl.shape[-1]):
            acc = acc - kl[..., j]
            big = np.maximum.reduce([big, np.abs(kl[..., j]), np.abs(acc)])
            n_add += 1
    return acc, big, n_add


# ---- tolerances -----------------------------------------------------------------------------------------------------------------------
def tol_reduce(L, K_total=None):
    """On logp computed from float32 log-weights that are the inputs themselves: 4 spacing32(max(|m|, log K_total)) + 2e-6 [B] -- three
    float32 operations (m + log s, - log K, the rounding of log K) of at most half a spacing each, and the relative error of the sum of
    exponentials (K terms of 1-ulp hardware exponentials, added in float32) through the logarithm."""
    L = np.asarray(L, dtype=np.float64)
    return 4 * spacing32(np.maximum(np.abs(L.max(1)), math.log(K_total or L.shape[1]))) + 2e-6


def tol_vi(L):
    """On the float32 mean over k: the K - 1 additions round to at most half a spacing of sum_k |L| each and the error of the sum is
    divided by K with it, so (K - 1) / K half spacings, plus one spacing of the result for the division."""
    L = np.asarray(L, dtype=np.float64)
    return 0.5 * spacing32(np.abs(L).sum(1)) + spacing32(L.mean(1))


def tol_logw(big, n_add):
    """On a per-sample log-weight summed in float32 (and so on logp): (additions per sample + 4) spacing32(largest |partial sum|);
    ``big`` [B, K] from gaussian_logw -> [B] (the worst sample of the point)."""
    return (n_add + 4) * spacing32(np.asarray(big).max(1))


def tol_w(w_ref, scale, tol_L):
    """|dw| <= scale (w_ref / scale (exp(tol_L) - 1 + 4e-6) + 1e-30): relative on live weights, nothing added on underflowed ones."""
    return scale * (np.asarray(w_ref) / scale * (np.expm1(np.asarray(tol_L))[:, None] + 4e-6) + 1e-30)


def bound_tol(lp_dev, scale):
    """The bound is float64 arithmetic on the float32 logp the device published: B 2^-52 relative to scale sum |logp| (+ the same on
    the global KL total, which the caller adds)."""
    lp = np.abs(np.asarray(lp_dev, dtype=np.float64))
    return lp.size * 2.0 ** -52 * abs(scale) * max(lp.sum(), 1e-300)


# ---- float32 restatement of the device recurrence ------------------------------------------------------------------------------------
def restate_f32(L, SEG=None):
    """k_elbo's recurrence in NumPy float32: passes of SEG samples, the pass maximum, nm = max(m, cm), a pairwise (shuffle-tree) sum of
    exp(L - nm), ssum = ssum exp(m - nm) + cs.  -> (m, ssum, logp) float32 [B].  For measuring the rounding of the recurrence itself."""
    L = np.asarray(L, dtype=np.float32)
    B, K = L.shape
    SEG = SEG or seg_of(K)
    m = np.full(B, -np.inf, dtype=np.float32)
    ssum = np.zeros(B, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, K, SEG):
            blk = np.full((B, SEG), -np.inf, dtype=np.float32)
            n = min(SEG, K - k0)
            blk[:, :n] = L[:, k0:k0 + n]
            nm = np.maximum(m, blk.max(1))
            e = np.exp((blk - nm[:, None]).astype(np.float32)).astype(np.float32)
            w = SEG
            while w > 1:                                          # the xor-shuffle tree
                w //= 2
                e = (e[:, :w] + e[:, w:2 * w]).astype(np.float32)
            resc = np.where(np.isinf(m), np.float32(0), ssum * np.exp((m - nm).astype(np.float32)).astype(np.float32)).astype(np.float32)
            ssum = (resc + e[:, 0]).astype(np.float32)
            m = nm
    lp = ((m + np.log(ssum).astype(np.float32)).astype(np.float32) - np.float32(math.log(K))).astype(np.float32)
    return m, ssum, lp


# ---- input families -------------------------------------------------------------------------------------------------------------------
def dominant_positions(K):
    """k = 0, SEG - 1, SEG, K - 1 and 64 where they exist."""
    SEG = seg_of(K)
    return sorted({p for p in (0, SEG - 1, SEG, K - 1, 64) if 0 <= p < K})


def family(name, B, K, seed=0, c_max=10.0):
    """[B, K] float64 array of float32 values.  Row b takes the b-th variant of the family (dominant position, tie positions) in turn."""
    rng = np.random.default_rng([seed, B, K, FAMILIES.index(name)])
    c = rng.uniform(-c_max, c_max, (B, 1))
    pos = dominant_positions(K)
    if name == "near_equal":
        L = c + 0.3 * rng.standard_normal((B, K))
    elif name == "dominant":                                     # one sample 40 nats above the rest (the rest near c - 40: |L| <= c_max + 41)
        L = c - 40.0 + 0.3 * rng.standard_normal((B, K))
        for b in range(B):
            L[b, pos[b % len(pos)]] = c[b, 0]
    elif name == "rising":
        L = c + 3.0 * np.arange(K)[None, :]
    elif name == "wide":                                         # the maximum near -1e4, everything else at least 200 below, down to -2e4
        L = np.empty((B, K))
        for b in range(B):
            rest = np.linspace(-2.0e4, -1.02e4, max(K - 1, 1))[:K - 1] + rng.uniform(-20, 20, K - 1)
            row = np.concatenate([[-1.0e4 + rng.uniform(-50, 50)], rng.permutation(rest)])
            p = pos[b % len(pos)]
            row[[0, p]] = row[[p, 0]]
            L[b] = row
    elif name == "ties_all":
        L = np.repeat(c, K, 1)
    elif name == "ties_two":                                     # two exactly equal maxima 5 nats up, in turn at the ends and across a SEG boundary
        L = c + 0.3 * rng.standard_normal((B, K))
        if K > 1:
            pairs = [(0, K - 1)] + ([(seg_of(K) - 1, seg_of(K))] if K > seg_of(K) else []) + ([(63, 64)] if K > 64 else [])
            for b in range(B):
                i, j = pairs[b % len(pairs)]
                L[b, i] = L[b, j] = np.float32(c[b, 0] + 5.0)
    else:
        raise ValueError(name)
    return f32(L)


def shape_cases():
    """All K against one B (65: two workgroups of k_elbo, a last pass with one live point), all B against two K (5: the first SEG boundary;
    65: the second trip of the k0 loop)."""
    return [(65, K) for K in ALL_K] + [(B, K) for B in ALL_B if B != 65 for K in (5, 65)]


def global_kls(n, count, seed=0):
    """n float64 arrays of ``count`` entries each."""
    rng = np.random.default_rng([seed, n, count])
    return [rng.uniform(0.0, 3.0, count) for _ in range(n)]


def split_regularisers(target, n, width, seed=0):
    """n float32-valued arrays [B, K, width] whose sum over arrays and entries is close to ``target`` [B, K] (what the device subtracts;
    the reference reads the same rounded entries, so nothing needs to be exact)."""
    rng = np.random.default_rng([seed, n, width])
    target = np.asarray(target, dtype=np.float64)
    parts = rng.uniform(-1.0, 1.0, (n * width,) + target.shape)
    parts[-1] = target - parts[:-1].sum(0)
    parts = f32(parts)
    return [np.ascontiguousarray(np.moveaxis(parts[i * width:(i + 1) * width], 0, -1)) for i in range(n)]
