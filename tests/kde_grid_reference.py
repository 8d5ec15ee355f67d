"""NumPy float64 restatement of ``iwvi_kde_density_grid`` (csrc/kde_grid.hip) and the input generators its tests share.
tests/test_kde_grid_host.py pins the restatement against ``sklearn.neighbors.KernelDensity``; tests/test_gpu_kde_grid.py compares the
kernel with it on the same float32 values.

  log p^_n(l) = logsumexp_s(-((l - x_ns) / h_n)^2 / 2) - log(S h_n) - log sqrt(2 pi)

with the log-sum-exp taken relative to its largest term, h_n = 1.06 std_n S^(-1/5) (population standard deviation) or a fixed value.
Silverman with all samples of a point equal: a point mass (+inf at that value, -inf elsewhere, bandwidth 0).  A NaN sample: NaN in the
point's row, mean, standard deviation and bandwidth.  A NaN level: NaN in that entry."""
import numpy as np

LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def kde_log_density_grid(samples, levels, bandwidth=None):
    """samples [S, N], levels [G] or [N, G] (any float type; widened to float64) -> (logdens [N, G], mean_std [N, 2], bandwidth [N]),
    all float64."""
    x = np.asarray(samples, dtype=np.float64)
    S, N = x.shape
    lev = np.asarray(levels, dtype=np.float64)
    lev = np.broadcast_to(lev, (N, lev.shape[-1])) if lev.ndim == 1 else lev
    G = lev.shape[1]
    out = np.empty((N, G))
    ms = np.empty((N, 2))
    bw = np.empty(N)
    for n in range(N):
        col = x[:, n]
        if np.isnan(col).any():
            out[n], ms[n], bw[n] = np.nan, np.nan, np.nan
            continue
        mean, sd = col.mean(), col.std()                          # population standard deviation
        h = 1.06 * sd * float(S) ** -0.2 if bandwidth is None else float(bandwidth)
        ms[n], bw[n] = (mean, sd), h
        if h == 0.0:                                              # all samples equal under Silverman: a point mass
            out[n] = np.where(lev[n] == col[0], np.inf, -np.inf)
            out[n][np.isnan(lev[n])] = np.nan
            continue
        with np.errstate(invalid="ignore"):
            e = -0.5 * ((lev[n][:, None] - col[None, :]) / h) ** 2   # [G, S]
            m = e.max(axis=1)
            out[n] = m + np.log(np.exp(e - m[:, None]).sum(axis=1)) - np.log(S * h) - LOG_SQRT_2PI
    return out, ms, bw


def naive_log_density(samples, level, h):
    """log(sum(exp(...))) without the shift: what underflows to -inf in the far tails."""
    x = np.asarray(samples, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return float(np.log(np.exp(-0.5 * ((level - x) / h) ** 2).sum()) - np.log(x.size * h) - LOG_SQRT_2PI)


# ---- inputs: float32 values, shared by the host and the GPU tests ----------------------------------------------------------------------
def draws(rng, n, kind):
    """n float32 draws: 'normal'; 'bimodal' (two separated modes of unequal weight and width); 'offset' (50 + 1e-3 z: the mean is
    5e4 standard deviations from zero, what a one-pass variance would cancel on)."""
    z = rng.standard_normal(n)
    if kind == "bimodal":
        z = np.where(rng.random(n) < 0.4, z * 0.3 - 2.0, z * 0.5 + 1.5)
    elif kind == "offset":
        z = 50.0 + 1e-3 * z
    elif kind != "normal":
        raise KeyError(kind)
    return z.astype(np.float32)


def kind_for(S):
    """The distribution the issue's cases pair with a sample count."""
    return "normal" if S <= 3 else "offset" if S == 4099 else "bimodal"


def sample_matrix(S, N, seed=0):
    """[S, N] float32: column n drawn as ``kind_for(S)`` (every third column the 'offset' kind once N > 2), shifted and scaled per column."""
    rng = np.random.default_rng(1000 * S + N + seed)
    cols = []
    for n in range(N):
        kind = "offset" if (N > 2 and n % 3 == 2) else kind_for(S)
        c = draws(rng, S, kind).astype(np.float64)
        if kind != "offset":
            c = c * rng.uniform(0.2, 2.0) + rng.standard_normal() * 3.0
        cols.append(c.astype(np.float32))
    return np.stack(cols, axis=1)


def tail_levels(col, n_core=37):
    """float32 levels for one column of float32 samples: ``n_core`` across +-4 standard deviations, then mean - 80 std, mean + 300 std
    and a level equal to a sample (the last three entries, in that order)."""
    c = np.asarray(col, dtype=np.float64)
    mean, sd = c.mean(), c.std()
    core = mean + sd * np.linspace(-4.0, 4.0, n_core)
    return np.concatenate([core, [mean - 80.0 * sd, mean + 300.0 * sd, c[len(c) // 2]]]).astype(np.float32)


def level_matrix(samples, G):
    """[N, G] float32 per-point levels: for G >= 4 the last three are the two far tails and a level equal to a sample, the rest spans
    +-4 standard deviations; below that, levels inside the bulk."""
    x = np.asarray(samples)
    out = np.empty((x.shape[1], G), dtype=np.float32)
    for n in range(x.shape[1]):
        if G >= 4:
            out[n] = tail_levels(x[:, n], G - 3)
        else:
            c = x[:, n].astype(np.float64)
            out[n] = (c.mean() + c.std() * np.linspace(-1.5, 2.5, G + 2)[1:-1]).astype(np.float32)
    return out
