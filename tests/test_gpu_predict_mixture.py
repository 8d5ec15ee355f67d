"""iwvi_lik_predict_mixture, DGP_VI.predict_mixture and evaluation.evaluate_mixture on the GPU against the float64 restatement
(tests/mixture_restatement.py, pinned by tests/test_predict_mixture_host.py).

TOLERANCES (derived; every figure is printed before it is asserted).  With tau_d, tau_m, tau_v the ELEMENTWISE bounds of a type -- the
formula the existing test of that likelihood asserts its elementwise callables with, evaluated on the moments of THIS test:
  Bernoulli, Student-t   4 x the DESIGN.md section 6 record, absolute (tests/test_gpu_likelihoods.py: 1.503e-6, 1.291e-6), all three;
  MultiClass             4 x its records, absolute (tests/test_gpu_multiclass.py: density 1.321e-5, mean 1.433e-6, var 1.422e-6);
  Poisson / Exponential / Gamma   8 x 2^-24 x S, S = explink_restatement.density_scale / mean_var_scales (tests/test_gpu_explink.py);
  Gaussian               density 1e-5 |d| (tests/test_gpu_predict_density.py:91); its moments are mu and one rounded sum v + variance:
                         2^-24 |E| and 2^-24 (V + E^2) per draw, doubled for the rounding of the float32 result;
the mixture's bounds follow:
  log_density  sum_d max_s tau_d  +  RED x 2^-24 x (1 + |want|).  A log-sum-exp of values each within tau is within tau; the second term is
               the reduction's own: the rounding of the float32 result (2^-24 |want|) and the float32 exp of the shifted terms, an absolute
               error of a few 2^-24 in the logarithm.  That constant cannot be derived: RED_MEASURED is the worst multiple of
               2^-24 (1 + |want|) a plain float32 NumPy evaluation of the same reduction (mixture_restatement.lse_float32) reaches on the
               per-draw values of the shapes below, for every segment width; RED = 3 x that for the device's intrinsics;
  mean         max_s tau_m  (a mean of values each within tau_m, summed in float64);
  var          max_s tau_v + 4 max_s |E_s| max_s tau_m  (d/dE of mean(V + E^2) - mean(E)^2 is bounded by 2|E| + 2|mean|).
Through the stack the reference's moments come from predict_f_multisample (one launch per layer) while predict_mixture reads the layer
launch's: the two agree as tests/test_gpu_predict_density.py:140 asserts of the Gaussian's two routes, 2e-5 max(1, |value|), which is added."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import explink_restatement as XR   # noqa: E402
import mixture_restatement as MX   # noqa: E402
import multiclass_restatement as MR   # noqa: E402

pytestmark = pytest.mark.gpu

U = MX.U
RED_MEASURED = 0.932      # python tests/test_gpu_predict_mixture.py (no GPU needed) prints it
RED = 3.0 * RED_MEASURED
ROUTES = 2e-5
REC_QUAD = {"bernoulli": 1.503e-6, "student_t": 1.291e-6}
REC_MC = {"predict_density": 1.321e-5, "predict_mean": 1.433e-6, "predict_var": 1.422e-6}
SHAPES = [(1, 1, 1), (5, 3, 1), (7, 20, 3), (67, 5, 1), (3, 70, 2), (9, 257, 1)]
KINDS = {"gaussian": dict(variance=0.3), "bernoulli": {}, "student_t": dict(scale=0.7, df=4.0),
         "poisson": dict(binsize=1.5), "exponential": {}, "gamma": dict(shape=2.5)}


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)), device=dev)


def _n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _liks(kind, **kw):
    from dgps_with_iwvi_amd import likelihoods as L
    cls = {"gaussian": L.Gaussian, "bernoulli": L.Bernoulli, "student_t": L.StudentT, "poisson": L.Poisson,
           "exponential": L.Exponential, "gamma": L.Gamma}
    if kind == "multiclass":
        return L.MultiClass(kw["num_classes"]), MX.make(kind, **kw)
    return cls[kind](**kw), MX.make(kind, **kw)


def _targets(kind, rng, N, Dy):
    if kind == "bernoulli":
        return (rng.uniform(size=(N, Dy)) > 0.5).astype(np.float32)
    if kind == "poisson":
        return rng.integers(0, 8, (N, Dy)).astype(np.float32)
    if kind == "exponential":
        y = rng.uniform(0.0, 9.0, (N, Dy)).astype(np.float32)
        y[0, 0] = 0.0
        return y
    if kind == "gamma":
        return rng.uniform(0.05, 9.0, (N, Dy)).astype(np.float32)
    if kind == "multiclass":
        return (np.arange(N) % Dy).astype(np.float32)[:, None]
    return rng.uniform(-2.5, 2.5, (N, Dy)).astype(np.float32)


def _moments(rng, N, S, Dy):
    """[S, N, Dy] float32 on the existing tests' ranges: mu in [-3, 3], v in [1e-4, 4] log-uniform, both ends present."""
    mu = rng.uniform(-3.0, 3.0, (S, N, Dy)).astype(np.float32)
    v = np.exp(rng.uniform(np.log(1e-4), np.log(4.0), (S, N, Dy))).astype(np.float32)
    v.reshape(-1)[0], v.reshape(-1)[-1] = 1e-4, 4.0
    return mu, v


def elementwise_bounds(kind, ref, m64, v64, Y):
    """(tau_d [S, N, Dy or 1], tau_m, tau_v [S, N, Dy]) of the module docstring, float64."""
    one = np.ones_like(m64)
    if kind in REC_QUAD:
        return 4 * REC_QUAD[kind] * one, 4 * REC_QUAD[kind] * one, 4 * REC_QUAD[kind] * one
    if kind == "multiclass":
        return 4 * REC_MC["predict_density"] * one[..., :1], 4 * REC_MC["predict_mean"] * one, 4 * REC_MC["predict_var"] * one
    Ys = np.broadcast_to(np.asarray(Y, np.float64), m64.shape).copy()
    if kind == "gaussian":
        E, V = (a.numpy() for a in ref.predict_mean_and_var(m64, v64))
        return 1e-5 * np.abs(ref.predict_density(m64, v64, Ys).numpy()), 2 * U * np.abs(E), 2 * U * (V + E ** 2)
    sm, sv = XR.mean_var_scales(ref, m64, v64)
    return 8 * U * XR.density_scale(ref, m64, v64, Ys).numpy(), 8 * U * sm.numpy(), 8 * U * sv.numpy()


def mixture_bounds(kind, ref, m64, v64, Y, want):
    td, tm, tv = elementwise_bounds(kind, ref, m64, v64, Y)
    out = {"mean": tm.max(0), "var": tv.max(0) + 4 * np.abs(want["E"]).max(0) * tm.max(0)}
    if "log_density" in want:
        out["log_density"] = td.max(0).sum(-1) + RED * U * (1 + np.abs(want["log_density"]))
    return out


def call(dev, desc, fm, fv, Y, N, S, Dy, sample_major=False, logp=True, moments=True):
    """The bare entry point on [S, N, Dy] host moments laid out point-major (rows n S + s) or sample-major (rows s N + n)."""
    from dgps_with_iwvi_amd import _abi
    lay = (lambda a: a) if sample_major else (lambda a: np.transpose(a, (1, 0, 2)))
    fm_d, fv_d = _t(lay(fm), dev), _t(lay(fv), dev)
    y_d = _t(Y, dev) if logp else None
    out = {}
    if logp:
        out["log_density"] = torch.full((N,), float("nan"), device=dev)
    if moments:
        out["mean"], out["var"] = (torch.full((N, Dy), float("nan"), device=dev) for _ in range(2))
    sn, ss = (1, N) if sample_major else (S, 1)
    _abi.check(_abi.lib().iwvi_lik_predict_mixture(desc, _abi.ptr(fm_d), _abi.ptr(fv_d), _abi.ptr(y_d), N, S, Dy, sn, ss,
                                                   _abi.ptr(out.get("log_density")), _abi.ptr(out.get("mean")), _abi.ptr(out.get("var")),
                                                   _abi.stream_ptr()))
    return out


def _assert_within(tag, got, want, tol):
    worst = 0.0
    for k in tol:
        g, w = _n64(got[k]), want[k]
        assert g.shape == w.shape and np.isfinite(g).all(), (tag, k, g.shape, w.shape)
        ratio = float((np.abs(g - w) / tol[k]).max())
        print("%s %-12s max err %.3e, worst err / tol %.3f" % (tag, k, float(np.abs(g - w).max()), ratio))
        worst = max(worst, ratio)
    assert worst <= 1.0, (tag, worst)


# ---- 1: the entry point on explicit moments, every type ----------------------------------------------------------------------------
_CASES = [(k, None) for k in KINDS] + [("multiclass", C) for C in (2, 4, 32)]


@pytest.mark.parametrize("kind,C", _CASES, ids=["%s%s" % (k, "" if C is None else C) for k, C in _CASES])
def test_entry_point_matches_the_restatement(gpu_device, kind, C):
    lik, ref = _liks(kind, **(KINDS[kind] if C is None else dict(num_classes=C)))
    for N, S, Dy in SHAPES:
        if C is not None:
            Dy = C                                                   # (one column of moments per class: the shapes give (N, S))
        rng = np.random.default_rng([N, S, Dy])
        mu, v = _moments(rng, N, S, Dy)
        Y = _targets(kind, rng, N, Dy)
        m64, v64 = mu.astype(np.float64), v.astype(np.float64)
        want = MX.mixture(ref, m64, v64, Y.astype(np.float64))
        tol = mixture_bounds(kind, ref, m64, v64, Y, want)
        for sample_major in (False, True):
            got = call(gpu_device, lik.lik_desc(), mu, v, Y, N, S, Dy, sample_major)
            _assert_within("%s N=%d S=%d Dy=%d %s" % (kind, N, S, Dy, "sample-major" if sample_major else "point-major"), got, want, tol)


# ---- 2: optional outputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,C", [("student_t", None), ("gamma", None), ("multiclass", 4)])
def test_optional_outputs_are_bit_identical(gpu_device, kind, C):
    lik, _ = _liks(kind, **(KINDS[kind] if C is None else dict(num_classes=C)))
    N, S, Dy = 37, 21, C or 3
    rng = np.random.default_rng(2)
    mu, v = _moments(rng, N, S, Dy)
    Y = _targets(kind, rng, N, Dy)
    all3 = call(gpu_device, lik.lik_desc(), mu, v, Y, N, S, Dy)
    only_lp = call(gpu_device, lik.lik_desc(), mu, v, Y, N, S, Dy, moments=False)
    only_mv = call(gpu_device, lik.lik_desc(), mu, v, Y, N, S, Dy, logp=False)
    assert set(only_lp) == {"log_density"} and set(only_mv) == {"mean", "var"}
    assert torch.equal(all3["log_density"], only_lp["log_density"])
    assert torch.equal(all3["mean"], only_mv["mean"]) and torch.equal(all3["var"], only_mv["var"])
    assert all(bool(torch.isfinite(t).all()) for t in all3.values())


# ---- 3: the grid stride ------------------------------------------------------------------------------------------------------------
def test_grid_stride_covers_every_point(gpu_device):
    """Bernoulli, S = 2 (4 lanes per point, 64 points per workgroup -- the most), N = 1024 x 64 + 3: the first three points of a second
    sweep of the grid.  Reference: the float64 reduction of the device's OWN elementwise outputs, so what is left is the reduction's term
    and the rounding of the float32 results -- plus one float32 ulp of a draw's value, because the same device function is inlined into
    two kernels and the compiler may contract it differently."""
    from dgps_with_iwvi_amd import likelihoods
    lik = likelihoods.Bernoulli()
    S, N = 2, 1024 * 64 + 3
    rng = np.random.default_rng(3)
    mu, v = _moments(rng, N, S, 1)
    Y = _targets("bernoulli", rng, N, 1)
    got = call(gpu_device, lik.lik_desc(), mu, v, Y, N, S, 1)
    m, vv, yy = _t(mu, gpu_device), _t(v, gpu_device), _t(np.broadcast_to(Y, (S, N, 1)), gpu_device)
    d = _n64(lik.predict_density(m, vv, yy))
    E, V = (_n64(a) for a in lik.predict_mean_and_var(m, vv))
    want = {"log_density": MX.lse_mean(d.sum(-1)), "mean": E.mean(0), "var": (V + E ** 2).mean(0) - E.mean(0) ** 2}
    tol = {"log_density": RED * U * (1 + np.abs(want["log_density"])) + 2 * U * np.abs(d).max(0).sum(-1),
           "mean": U * np.abs(want["mean"]) + 2 * U * np.abs(E).max(0),
           "var": U * np.abs(want["var"]) + 2 * U * (V + E ** 2).max(0) + 4 * np.abs(E).max(0) * 2 * U * np.abs(E).max(0)}
    _assert_within("grid stride", got, want, tol)


# ---- 4: the max-shift --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gaussian", "student_t"])
def test_log_sum_exp_is_shifted_by_the_maximum(gpu_device, kind):
    """N = 4, S = 33 (one full chunk of 32 and a ragged one): every draw's log density is below -1e4, so exp of the unshifted value
    underflows (float32 and float64 alike), and one draw per point -- in another chunk position for every point -- beats the rest by more
    than 100.  These values are far off the grids of the elementwise records, so the elementwise bound is the relative one: 1e-5 |d| for
    the Gaussian (its existing formula is relative); for the Student-t 8 x 2^-24 |d| -- its log density is a sum of three float32
    logarithms (logf, log1pf: <= 2 ulp each) times constants, d itself is its dominant term, and 8 is the project's constant for such a
    chain (tests/test_gpu_explink.py: C8)."""
    N, S = 4, 33
    rng = np.random.default_rng(4)
    big = [0, 31, 32, 17]                                            # the position of the largest draw, per point
    if kind == "gaussian":
        lik, ref = _liks("gaussian", variance=0.005)
        mu = rng.uniform(20.3, 21.0, (S, N, 1)).astype(np.float32)   # y = 0, s = 0.01: d = -50 mu^2 - ... <= -20600
        for n, s in enumerate(big):
            mu[s, n, 0] = 19.7                                       # -19400: ahead by ~1200
        v = np.full((S, N, 1), 0.005, dtype=np.float32)
        rel = 1e-5
    else:
        lik, ref = _liks("student_t", scale=1.0, df=400.0)
        mu = -rng.uniform(2e15, 4e15, (S, N, 1)).astype(np.float32)  # y = 0: d ~ -200.5 log(mu^2 / 400) <= -1.28e4
        for n, s in enumerate(big):
            mu[s, n, 0] = -1e15                                      # ahead by 401 log 2 = 278 at the least
        v = np.full((S, N, 1), 1e-4, dtype=np.float32)
        rel = 8 * U
    Y = np.zeros((N, 1), dtype=np.float32)
    m64, v64 = mu.astype(np.float64), v.astype(np.float64)
    d = MX.draw_log_density(ref, m64, v64, Y)
    srt = np.sort(d, 0)
    assert d.max() < -1e4 and (srt[-1] - srt[-2]).min() > 100 and np.all(np.exp(d) == 0.0)
    assert [int(i) for i in d.argmax(0)] == big
    want = {"log_density": MX.lse_mean(d)}
    got = call(gpu_device, lik.lik_desc(), mu, v, Y, N, S, 1, moments=False)
    assert bool(torch.isfinite(got["log_density"]).all())
    tol = {"log_density": rel * np.abs(d).max(0) + RED * U * (1 + np.abs(want["log_density"]))}
    _assert_within("max-shift " + kind, got, want, tol)


def test_multiclass_minimum_density_comes_out_exactly(gpu_device):
    """A density of exactly -inf cannot occur (epsilon > 0).  Where every draw puts the label LAST by a wide margin, every cdf factor sits on
    its jitter 1e-4, p = sum_i w_i (1e-4)^(C-1) and the density is log(p (1 - eps - eps_1) + eps_1), log(eps / (C - 1)) to the documented
    clips, for every draw: the log-sum-exp of S equal values must return that value EXACTLY (exp(0) = 1, S / S), i.e. the device's own
    elementwise predict_density of one such draw, bit for bit, and the float64 value within the elementwise bound."""
    C, N, S = 3, 4, 33
    lik, ref = _liks("multiclass", num_classes=C)
    rng = np.random.default_rng(5)
    Y = (np.arange(N) % C).astype(np.float32)[:, None]
    mu = rng.uniform(35.0, 45.0, (S, N, C)).astype(np.float32)
    for n in range(N):
        mu[:, n, int(Y[n, 0])] *= -1.0
    v = np.full((S, N, C), 0.01, dtype=np.float32)
    got = call(gpu_device, lik.lik_desc(), mu, v, Y, N, S, C, moments=False)["log_density"]
    one = lik.predict_density(_t(mu[0], gpu_device), _t(v[0], gpu_device), _t(Y, gpu_device))[:, 0]
    assert torch.equal(got, one), (got, one)
    eps, eps1 = 1e-3, 1e-3 / (C - 1)
    want = math.log((1e-4) ** (C - 1) * (1 - eps - eps1) + eps1)
    print("multiclass minimum: got %r, float64 %.9f, log(eps / (C - 1)) %.9f" % (got.tolist(), want, math.log(eps1)))
    assert float(np.abs(_n64(got) - want).max()) <= 4 * REC_MC["predict_density"] and abs(want - math.log(eps1)) < 1e-4


# ---- 5: through the stack ----------------------------------------------------------------------------------------------------------
def _stack(kind, lv, dev):
    from dgps_with_iwvi_amd import synthetic
    if kind == "multiclass":
        spec = MR.make_spec(3, L=2, M=16, B=10, K=3, lv=lv, seed=9)
        lik, ref = _liks(kind, num_classes=3)
    else:
        spec = synthetic.make_spec(L=2, M=16, B=10, K=3, with_lv=lv, Dy=2, seed=9, distinct_y=True)
        if kind == "bernoulli":
            spec["Y"] = (spec["Y"] > 0).astype(np.float64)
        elif kind == "poisson":
            spec["Y"] = XR.targets(spec, "poisson")
        lik, ref = _liks(kind, **KINDS[kind])
    return spec, lik, ref, synthetic.build_model(spec, dev, likelihood=lik)


def _zs(spec, S, N, dev, seed=3):
    rng = np.random.default_rng(seed)
    return [_t(rng.standard_normal((S, N, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1])), dev) for l in spec["layers"]]


@pytest.mark.parametrize("lv", [True, False], ids=["lv", "nolv"])
@pytest.mark.parametrize("kind", ["bernoulli", "multiclass", "poisson", "student_t"])
def test_predict_mixture_through_the_stack(gpu_device, kind, lv):
    N, S = 9, 6
    spec, lik, ref, model = _stack(kind, lv, gpu_device)
    X, Y = spec["X"][:N], spec["Y"][:N]
    zs = _zs(spec, S, N, gpu_device)
    got = model.predict_mixture(X, S, Y=Y, zs=zs)
    Dout = 3 if kind == "multiclass" else 2
    assert tuple(got["mean"].shape) == tuple(got["var"].shape) == (N, Dout) and tuple(got["log_density"].shape) == (N,)
    assert set(model.predict_mixture(X, S, zs=zs)) == {"mean", "var"}
    m, v = model.predict_f_multisample(X, S, zs=zs)
    m64, v64 = _n64(m), _n64(v)
    want = MX.mixture(ref, m64, v64, Y)
    tol = {k: t + ROUTES * np.maximum(1.0, np.abs(want[k])) for k, t in mixture_bounds(kind, ref, m64, v64, Y, want).items()}
    _assert_within("%s lv=%s vs restatement" % (kind, lv), got, want, tol)
    # points are independent: batches change nothing
    bat = model.predict_mixture(X, S, Y=Y, zs=zs, batch_size=4)
    assert all(torch.equal(got[k], bat[k]) for k in got)
    # predict_log_density IS this route now ...
    pld = model.predict_log_density(X, Y, S, zs=zs)
    assert torch.equal(pld, got["log_density"])
    # ... and agrees with the layer-by-layer route it replaces: both sides carry the elementwise bound
    old = model._predict_log_density_layerwise(X, Y, S, zs=zs)
    err = np.abs(_n64(pld) - _n64(old))
    lim = 2 * tol["log_density"]
    print("%s lv=%s one-launch vs layer-wise: max err %.3e, worst err / tol %.3f" % (kind, lv, err.max(), (err / lim).max()))
    assert (err <= lim).all()
    # drawn noise: the counter advances, so two calls differ, and both are finite
    a, b = model.predict_mixture(X, S, Y=Y), model.predict_mixture(X, S, Y=Y)
    assert all(bool(torch.isfinite(t).all()) for t in list(a.values()) + list(b.values()))
    assert not torch.equal(a["log_density"], b["log_density"])


# ---- 6: the Gaussian cross-check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lv", [True, False], ids=["lv", "nolv"])
def test_gaussian_mixture_matches_the_one_launch_route(gpu_device, lv):
    from dgps_with_iwvi_amd import synthetic
    N, S = 9, 6
    spec = synthetic.make_spec(L=2, M=16, B=10, K=3, with_lv=lv, Dy=2, seed=9, distinct_y=True)
    model = synthetic.build_model(spec, gpu_device)
    X, Y = spec["X"][:N], spec["Y"][:N]
    zs = _zs(spec, S, N, gpu_device)
    got = model.predict_mixture(X, S, Y=Y, zs=zs)
    one = _n64(model.predict_log_density(X, Y, S, zs=zs))           # iwvi_dgp_predict_density: the fused Gaussian tail
    err = np.abs(_n64(got["log_density"]) - one).max()
    print("gaussian lv=%s: |mixture - one-launch| %.3e" % (lv, err))
    assert err <= 2e-5 * max(1.0, np.abs(one).max())                # tests/test_gpu_predict_density.py:140, between its two routes
    m, v = model.predict_f_multisample(X, S, zs=zs)
    want = MX.mixture(MX.make("gaussian", variance=spec["lik_var"]), _n64(m), _n64(v), Y)
    np.testing.assert_allclose(_n64(got["mean"]), want["mean"], rtol=ROUTES, atol=ROUTES)
    np.testing.assert_allclose(_n64(got["var"]), want["var"], rtol=ROUTES, atol=ROUTES)


# ---- 7: validation -----------------------------------------------------------------------------------------------------------------
def test_validation(gpu_device):
    from dgps_with_iwvi_amd import _abi, likelihoods, synthetic
    N, S = 9, 6
    spec, lik, ref, model = _stack("multiclass", True, gpu_device)
    X, Y = spec["X"][:N], spec["Y"][:N]
    with pytest.raises(ValueError, match="Y must be"):
        model.predict_mixture(X, S, Y=Y[:-1])
    with pytest.raises(ValueError, match="Y must be"):
        model.predict_mixture(X, S, Y=np.eye(3)[Y[:, 0].astype(int)])            # one-hot labels
    with pytest.raises(ValueError, match="targets must be integers"):
        model.predict_mixture(X, S, Y=Y + 0.5)
    with pytest.raises(ValueError, match="S must be"):
        model.predict_mixture(X, 0, Y=Y)
    with pytest.raises(ValueError, match="X must be"):
        model.predict_mixture(X[:, :-1], S, Y=Y)
    with pytest.raises(ValueError, match="zs"):
        model.predict_mixture(X, S, Y=Y, zs=_zs(spec, S + 1, N, gpu_device))
    with pytest.raises(NotImplementedError, match="predict_mixture"):
        model.predict_y_samples_fused(X, S)
    spec2 = synthetic.make_spec(L=2, M=16, B=10, K=3, with_lv=False, Dy=2, seed=9, distinct_y=True)
    with pytest.raises(ValueError, match="Y must be"):
        synthetic.build_model(spec2, gpu_device, likelihood=likelihoods.StudentT(0.7, 4.0)).predict_mixture(spec2["X"][:N], S, Y=spec2["Y"][:N, :1])
    st2 = synthetic.build_model(spec2, gpu_device, likelihood=likelihoods.StudentT(scale=0.7, df=2.0))
    with pytest.raises(ValueError, match="df > 2"):
        st2.predict_mixture(spec2["X"][:N], S, Y=spec2["Y"][:N])
    assert bool(torch.isfinite(st2.predict_log_density(spec2["X"][:N], spec2["Y"][:N], S)).all())   # the density alone needs no variance
    # the bare entry point: df = 2 is refused for the moments and accepted with out_logp alone
    rng = np.random.default_rng(7)
    mu, v = _moments(rng, 5, 3, 1)
    Yt = _targets("student_t", rng, 5, 1)
    d2 = likelihoods.StudentT(scale=0.7, df=2.0).lik_desc()
    with pytest.raises(_abi.IwviError, match="df > 2") as ei:
        call(gpu_device, d2, mu, v, Yt, 5, 3, 1)
    assert ei.value.rc == _abi.ERR_ARG
    got = call(gpu_device, d2, mu, v, Yt, 5, 3, 1, moments=False)
    want = MX.mixture(MX.make("student_t", scale=0.7, df=2.0 + 1e-9), mu.astype(np.float64), v.astype(np.float64), Yt)["log_density"]
    np.testing.assert_allclose(_n64(got["log_density"]), want, rtol=0, atol=4 * REC_QUAD["student_t"] + RED * U * (1 + np.abs(want).max()))


# ---- 8: evaluate_mixture -----------------------------------------------------------------------------------------------------------
def _reset_noise(model, seed):
    from dgps_with_iwvi_amd import settings
    settings.set_seed(seed)
    model._words().zero_()


def test_evaluate_mixture_classifiers(gpu_device):
    from dgps_with_iwvi_amd import evaluation, likelihoods, synthetic
    import lik_restatement as R
    for name, (spec, _), lik in (("multiclass", MR.three_class_problem(), likelihoods.MultiClass(3)),
                                 ("bernoulli", R.two_class_problem(), likelihoods.Bernoulli())):
        model = synthetic.build_model(spec, gpu_device, likelihood=lik)
        Xt, Yt = spec["X"][:40], spec["Y"][:40]
        _reset_noise(model, 21)
        res = evaluation.evaluate_mixture(model, Xt, Yt, num_predict_samples=50, predict_batch_size=16, return_predictions=True)
        assert set(res) == {"test_loglik_mc", "test_accuracy", "mean", "var"} | (set() if name == "multiclass" else {"test_rmse"})
        mean = res["mean"]
        if name == "multiclass":
            assert mean.shape == (40, 3)
            acc = float((np.argmax(mean, 1) == Yt[:, 0]).mean())                 # (NumPy's argmax: the first maximum)
        else:
            assert mean.shape == (40, 1)
            acc = float(((mean > 0.5) == (Yt == 1)).mean())
            assert abs(res["test_rmse"] - math.sqrt(((mean.astype(np.float64) - Yt) ** 2).mean())) <= 1e-6
        assert round(res["test_accuracy"] * 40) == round(acc * 40) and abs(res["test_accuracy"] - acc) <= 1e-12 and 0.0 <= acc <= 1.0
        _reset_noise(model, 21)
        lp = model.predict_mixture(Xt, 50, Y=Yt, batch_size=16)["log_density"]
        assert res["test_loglik_mc"] == float(lp.double().mean()) and math.isfinite(res["test_loglik_mc"])
        print("%s: %r" % (name, {k: v for k, v in res.items() if k not in ("mean", "var")}))


def test_evaluate_mixture_counts(gpu_device):
    from dgps_with_iwvi_amd import evaluation, likelihoods, synthetic
    spec = synthetic.make_spec(L=2, M=16, B=40, K=3, with_lv=True, Dy=2, seed=9, distinct_y=True)
    spec["Y"] = XR.targets(spec, "poisson")
    model = synthetic.build_model(spec, gpu_device, likelihood=likelihoods.Poisson(binsize=1.5))
    res = evaluation.evaluate_mixture(model, spec["X"][:40], spec["Y"][:40], num_predict_samples=50)
    assert set(res) == {"test_loglik_mc", "test_rmse"} and all(math.isfinite(v) for v in res.values()) and res["test_rmse"] > 0
    with pytest.raises(ValueError):
        evaluation.evaluate_mixture(model, spec["X"][:40], spec["Y"][:39])


# ---- 9: graph replay ---------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_the_eager_call(gpu_device):
    """One predict_mixture batch -- precompute, the layer launch, iwvi_lik_predict_mixture: a single chain of kernels on one stream --
    captured and replayed: bit-identical to the eager call on the same noise."""
    N, S = 9, 6
    spec, lik, ref, model = _stack("poisson", True, gpu_device)
    X, Y = _t(spec["X"][:N], gpu_device), _t(spec["Y"][:N], gpu_device)
    zs = _zs(spec, S, N, gpu_device)
    eager = model.predict_mixture(X, S, Y=Y, zs=zs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.predict_mixture(X, S, Y=Y, zs=zs)                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = model.predict_mixture(X, S, Y=Y, zs=zs)
    for t in cap.values():
        t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(cap[k], eager[k]) for k in eager)


def measure_red():
    """RED_MEASURED: the worst multiple of 2^-24 (1 + |want|) reached by the float32 NumPy reduction on the float32-rounded per-draw values
    of test 1's cases, over every segment width the launcher picks from."""
    worst = 0.0
    for kind, C in _CASES:
        ref = MX.make(kind, **(KINDS[kind] if C is None else dict(num_classes=C)))
        for N, S, Dy in SHAPES:
            if C is not None:
                Dy = C
            rng = np.random.default_rng([N, S, Dy])
            mu, v = _moments(rng, N, S, Dy)
            Y = _targets(kind, rng, N, Dy)
            lp32 = MX.draw_log_density(ref, mu.astype(np.float64), v.astype(np.float64), Y.astype(np.float64)).astype(np.float32)
            want = MX.lse_mean(lp32.astype(np.float64))
            for seg in (4, 8, 16, 32, 64):
                got = MX.lse_float32(lp32, seg).astype(np.float64)
                worst = max(worst, float((np.abs(got - want) / (U * (1 + np.abs(want)))).max()))
    return worst


if __name__ == "__main__":
    print("RED_MEASURED = %.3f" % measure_red())
