"""The statistics of tests/test_gpu_lik_sample.py on NumPy samplers, at the same inputs and sizes (no GPU): each statistic passes on the
correct sampler and FIRES on a perturbed one -- shape or scale x 1.02, the link's argument x 1.05, the Student-t replaced by the normal
of its variance, the probit jitter dropped.  This pins the bounds of tests/lik_sample_reference.py: wide enough for a correct sampler at
n = 2^20, narrow enough to see a 2 % error.  Where a pooled statistic has no power against one of these, a statistic that has stands
beside it and the GPU test asserts both: the Bernoulli at fixed fmean = -6 / +6 (the jitter), the Beta's dispersion z (its scale), the
Ordinal's sigma-directed z.  What NO statistic here sees is the jitter inside the BETA's link: on fmean in [-1, 1] it moves m = ip(f)
by at most 7e-4 (printed below; moments wide enough to show it put alpha near 1e-3, where float32 targets round to 0 and 1)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lik_sample_reference as R   # noqa: E402

N = R.N_STAT


def _inputs(name, rng):
    if name in R.BETA_RANGE:
        return R.beta_moments(N, 21, R.BETA_RANGE[name]).astype(np.float64)
    return R.draw_f(*R.moments(N, 21), rng)


# name -> perturbations that the KS statistic must see
PERTURBED = {"gaussian": [dict(shape_mult=1.02 ** 2), dict(link_mult=1.05)],          # (the scale is the standard deviation)
             "student_t": [dict(shape_mult=1.02), dict(normal_t=True)],
             "exponential": [dict(shape_mult=1.02)],
             "gamma_2.5": [dict(shape_mult=1.02)],
             "gamma_0.5": [dict(shape_mult=1.02)],
             # (the Beta's KS sees the scale only at scale 2; test_beta_dispersion_and_mean_z below sees scale and link at both)
             "beta_6": [],
             "beta_2": [dict(shape_mult=1.02)]}


@pytest.mark.parametrize("name", sorted(R.CONTINUOUS))
def test_ks_passes_and_fires(name):
    kind, par = R.CONTINUOUS[name]
    rng = np.random.default_rng(100)
    f = _inputs(name, rng)
    D = R.ks_D(R.cdf(kind, R.sample(kind, f, rng, **par), f, **par))
    print("%s: KS D = %.5f (bound %.5f)" % (name, D, R.ks_bound(N)))
    assert D <= R.ks_bound(N)
    for pert in PERTURBED[name]:
        Dp = R.ks_D(R.cdf(kind, R.sample(kind, f, rng, **dict(par, **pert)), f, **par))
        print("%s perturbed %s: KS D = %.5f" % (name, pert, Dp))
        assert Dp > R.ks_bound(N)


def test_bernoulli_z_passes_and_fires():
    rng = np.random.default_rng(101)
    f = R.draw_f(*R.moments(N, 31), rng)
    z = R.bernoulli_z(R.sample("bernoulli", f, rng), f)
    print("bernoulli: z =", np.round(z, 2))
    assert np.abs(z).max() <= R.Z_MAX
    zp = R.bernoulli_z(R.sample("bernoulli", f, rng, link_mult=1.05), f)
    print("bernoulli link x 1.05: z =", np.round(zp, 2))
    assert np.abs(zp).max() > R.Z_MAX
    # the jitter: the bins over wide moments give |z| = 5.7 without it; at fixed fmean = -6 / +6 it is the rare label's whole probability
    print("bernoulli jitter dropped, binned: z =", np.round(R.bernoulli_z(R.sample("bernoulli", f, rng, jit=0.0), f), 2))
    for fm in (-6.0, 6.0):
        ff = np.full(N, fm)
        z0, z1 = (R.bernoulli_fixed_z(R.sample("bernoulli", ff, rng, jit=j), fm) for j in (R.JIT, 0.0))
        print("bernoulli at fmean %g: z = %.2f; jitter dropped %.2f" % (fm, z0, z1))
        assert abs(z0) <= R.Z_MAX < abs(z1)


@pytest.mark.parametrize("name", ["beta_6", "beta_2"])
def test_beta_dispersion_and_mean_z(name):
    kind, par = R.CONTINUOUS[name]
    f = _inputs(name, None)
    rng = np.random.default_rng(106)
    mean_z = lambda y: R.binned_z(y - R.ip(f), R.ip(f) * (1.0 - R.ip(f)) / (par["scale"] + 1.0), f)
    y = R.sample(kind, f, rng, **par)
    zd, zm = R.beta_dispersion_z(y, f, par["scale"]), mean_z(y)
    print("%s: dispersion z = %.2f, mean z per bin of f =" % (name, zd), np.round(zm, 2))
    assert abs(zd) <= R.Z_MAX and np.abs(zm).max() <= R.Z_MAX
    zs = R.beta_dispersion_z(R.sample(kind, f, rng, **dict(par, shape_mult=1.02)), f, par["scale"])
    zl = mean_z(R.sample(kind, f, rng, **dict(par, link_mult=1.05)))
    yj = R.sample(kind, f, rng, **dict(par, jit=0.0))
    print("%s: scale x 1.02 dispersion z = %.2f; link x 1.05 mean z =" % (name, zs), np.round(zl, 2),
          "; jitter dropped (NOT seen): %.2f," % R.beta_dispersion_z(yj, f, par["scale"]), np.round(mean_z(yj), 2))
    assert abs(zs) > R.Z_MAX and np.abs(zl).max() > R.Z_MAX


def test_poisson_statistics_pass_and_fire():
    rng = np.random.default_rng(102)
    f = rng.uniform(-2.0, 4.0, N)
    lam = R.BINSIZE * np.exp(f)
    zm, zd = R.poisson_z(R.sample("poisson", f, rng, binsize=R.BINSIZE), lam)
    print("poisson: mean z =", np.round(zm, 2), " dispersion z =", np.round(zd, 2))
    assert np.abs(zm).max() <= R.Z_MAX and np.abs(zd).max() <= R.Z_MAX
    zm, _ = R.poisson_z(R.sample("poisson", f, rng, binsize=1.02 * R.BINSIZE), lam)
    assert np.abs(zm).max() > R.Z_MAX
    _, zd = R.poisson_z(np.rint(lam + np.sqrt(1.05 * lam) * rng.standard_normal(N)), lam)     # over-dispersed
    assert np.abs(zd).max() > R.Z_MAX


@pytest.mark.parametrize("rate", [0.3, 50.0, 1e5, 1.01 * R.POIS_NORMAL], ids=lambda r: "%g" % r)
def test_poisson_chi2_passes_and_fires(rate):
    rng = np.random.default_rng(103)
    if rate >= R.POIS_NORMAL:                                # what a float32 target holds there: even integers
        y = (rate + np.sqrt(rate) * rng.standard_normal(N)).astype(np.float32).astype(np.float64)
        bad = (1.001 * rate + np.sqrt(rate) * rng.standard_normal(N)).astype(np.float32).astype(np.float64)
    else:
        y, bad = rng.poisson(rate, N), rng.poisson(1.02 * rate, N)
    chi2, dof, lim = R.poisson_chi2(y, rate)
    chi2b, _, _ = R.poisson_chi2(bad, rate)
    print("poisson rate %g: chi2 = %.1f on %d dof (limit %.1f); perturbed %.1f" % (rate, chi2, dof, lim, chi2b))
    assert chi2 <= lim < chi2b


def test_ordinal_z_passes_and_fires():
    rng = np.random.default_rng(104)
    f = R.draw_f(*R.moments(N, 51), rng)
    z = R.ordinal_z(R.sample("ordinal", f, rng), f)
    print("ordinal: z =", np.round(z, 2))
    assert np.abs(z).max() <= R.Z_MAX
    zp = R.ordinal_z(R.sample("ordinal", f, rng, link_mult=1.05), f)
    print("ordinal link x 1.05: z =", np.round(zp, 2))
    assert np.abs(zp).max() > R.Z_MAX
    # sigma: pooled over moments this wide the bin counts barely move (x 1.02: |z| = 2.6); the sigma-directed z on fvar = NULL sees it
    print("ordinal sigma x 1.02, per bin: z =", np.round(R.ordinal_z(R.sample("ordinal", f, rng, shape_mult=1.02), f), 2))
    f0 = R.ordinal_f(N, 52).astype(np.float64)
    z0, z1, z2 = (R.ordinal_sigma_z(R.sample("ordinal", f0, rng, shape_mult=m), f0) for m in (1.0, 1.02, 1.0 / 1.02))
    print("ordinal sigma-directed z = %.2f; sigma x 1.02: %.2f; / 1.02: %.2f" % (z0, z1, z2))
    assert abs(z0) <= R.Z_MAX and abs(z1) > R.Z_MAX and abs(z2) > R.Z_MAX


def test_multiclass_statistics():
    rng = np.random.default_rng(105)
    n, eps, C = N, 0.05, 4
    hit = rng.uniform(size=n) >= eps
    assert abs(R.hit_z(hit.sum(), n, eps)) <= R.Z_MAX
    assert abs(R.hit_z((rng.uniform(size=n) >= 1.05 * eps).sum(), n, eps)) > R.Z_MAX
    off = rng.integers(1, C, (~hit).sum())
    chi2, dof, lim = R.chi2_counts(np.bincount(off, minlength=C)[1:], np.full(C - 1, 1.0 / (C - 1)))
    assert dof == C - 2 and chi2 <= lim
    skew = np.where(rng.uniform(size=off.size) < 0.1, 1, off)
    assert R.chi2_counts(np.bincount(skew, minlength=C)[1:], np.full(C - 1, 1.0 / (C - 1)))[0] > lim
