"""iwvi_lik_sample_y, the likelihoods' sample_y, DGP_VI.predict_y_draws and evaluation.evaluate_draws on the GPU.

The draws are checked as DISTRIBUTIONS, conditional on the f the launch exports: the PIT F(y | f) of the continuous types by
Kolmogorov-Smirnov, binned z statistics for the Bernoulli, the Poisson and the Ordinal, chi^2 goodness of fit for the Poisson at fixed
rates and for the MultiClass's misses.  Definitions, statistics and bounds: tests/lik_sample_reference.py (pinned on NumPy samplers,
correct and perturbed, by tests/test_lik_sample_reference_host.py).  n = 2^20 per statistic, fixed seeds: a run is deterministic.
Bounds: KS D <= 3.3 / sqrt(n); |z| <= 6; chi^2 <= chi2.isf(1e-9, dof) -- below 1e-7 of false alarm over the whole file.
Every statistic is printed before it is asserted."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import lik_sample_reference as R   # noqa: E402

pytestmark = pytest.mark.gpu
N = R.N_STAT
ROUTES = 2e-5                  # tests/test_gpu_predict_mixture.py: between the two moment routes


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)), device=dev)


def _n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _lik(kind, **p):
    from dgps_with_iwvi_amd import likelihoods as L
    if kind == "multiclass":
        return L.MultiClass(p["num_classes"], invlink=L.RobustMax(p["num_classes"], p.get("epsilon", 1e-3)))
    if kind == "ordinal":
        return L.Ordinal(p.get("edges", R.ORD_EDGES))
    return {"gaussian": L.Gaussian, "bernoulli": L.Bernoulli, "student_t": L.StudentT, "poisson": L.Poisson,
            "exponential": L.Exponential, "gamma": L.Gamma, "beta": L.Beta}[kind](**p)


def _draw(lik, mu, v, dev, serial=1, seed=0, z_f=None):
    """(y, f) as float64 arrays from ONE launch on float32 moments (v None: f = mu); a vector of moments is one column, [n, 1]."""
    col = lambda a: None if a is None else _t(np.asarray(a).reshape(-1, 1) if np.ndim(a) == 1 else a, dev)
    y, f = lik.sample_y(col(mu), col(v), z_f=col(z_f), return_f=True, seed=seed, serial=serial)
    y, f = _n64(y), _n64(f)
    return (y[:, 0], f[:, 0]) if np.ndim(mu) == 1 else (y, f)


def _raw(desc, fm, fv, T, Dy, out_y, z_f=None, seed=0, serial=0, serial_dev=None, out_f=None):
    from dgps_with_iwvi_amd import _abi
    p = lambda t: None if t is None else (t if isinstance(t, ctypes.c_void_p) else _abi.ptr(t))
    return _abi.lib().iwvi_lik_sample_y(desc, p(fm), p(fv), T, Dy, p(z_f), seed, serial, p(serial_dev), p(out_y), p(out_f), _abi.stream_ptr())


# ---- 1: f is what it says ---------------------------------------------------------------------------------------------------------------
def test_exported_f_is_the_stated_formula(gpu_device):
    """out_f against fmean + sqrt(fvar) z_f evaluated in float32 operations (a correctly rounded square root, then the product and the
    sum rounded once): within 2 ulp of the float32 result, elementwise; with fvar = NULL out_f == fmean bit for bit."""
    mu, v = R.moments(N, 11)
    z = np.random.default_rng(12).standard_normal(N).astype(np.float32)
    lik = _lik("gaussian", variance=0.3)
    _, f = _draw(lik, mu, v, gpu_device, z_f=z)
    want = (np.sqrt(v).astype(np.float64) * z.astype(np.float64) + mu.astype(np.float64)).astype(np.float32)
    ulps = np.abs(f - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print("out_f vs the float32 formula: max %.3g ulp, %d of %d differ" % (ulps.max(), int((ulps > 0).sum()), N))
    assert ulps.max() <= 2.0
    assert mu.min() == -3.0 and mu.max() == 3.0 and v.min() == np.float32(1e-4) and v.max() == 4.0
    y0, f0 = lik.sample_y(_t(mu, gpu_device)[:, None], None, return_f=True, serial=3)
    assert torch.equal(f0, _t(mu, gpu_device)[:, None])
    assert not torch.equal(y0, f0)


# ---- 2: continuous types, conditional on the exported f -------------------------------------------------------------------------------
def _continuous_inputs(name):
    if name in R.BETA_RANGE:
        return R.beta_moments(N, 21, R.BETA_RANGE[name]), None
    return R.moments(N, 21)


@pytest.mark.parametrize("name", sorted(R.CONTINUOUS))
def test_continuous_pit_passes_ks(gpu_device, name):
    kind, par = R.CONTINUOUS[name]
    mu, v = _continuous_inputs(name)
    lik = _lik(kind, **par)
    for serial in (1, 2):                                    # serial + 1: other draws, the same statistic
        y, f = _draw(lik, mu, v, gpu_device, serial=serial)
        D = R.ks_D(R.cdf(kind, y, f, **par))
        print("%s serial %d: KS D = %.5f (bound %.5f)" % (name, serial, D, R.ks_bound(N)))
        assert np.isfinite(y).all()
        assert D <= R.ks_bound(N)
        if serial == 1:
            y1 = y
    assert (y != y1).mean() > 0.99


@pytest.mark.parametrize("name", ["gaussian", "student_t", "gamma_2.5", "beta_6"])
def test_trained_scalar_is_read_from_the_device(gpu_device, name):
    """param0_dev holds the true value, param[0] another one: the draws follow the device's."""
    kind, par = R.CONTINUOUS[name]
    key = {"gaussian": "variance", "student_t": "scale", "gamma": "shape", "beta": "scale"}[kind]
    lik = _lik(kind, **dict(par, **{key: 3.0 * par[key]}))
    lik.bind_device_variance(_t([par[key]], gpu_device))
    d = lik.lik_desc()
    assert d.param[0] == np.float32(3.0 * par[key]) and d.param0_dev
    mu, v = _continuous_inputs(name)
    y, f = _draw(lik, mu, v, gpu_device, serial=5)
    D = R.ks_D(R.cdf(kind, y, f, **par))
    print("%s from param0_dev: KS D = %.5f (bound %.5f)" % (name, D, R.ks_bound(N)))
    assert D <= R.ks_bound(N)


# ---- 3: Bernoulli ----------------------------------------------------------------------------------------------------------------------
def test_bernoulli_binned_z(gpu_device):
    mu, v = R.moments(N, 31)
    for serial in (1, 2):
        y, f = _draw(_lik("bernoulli"), mu, v, gpu_device, serial=serial)
        z = R.bernoulli_z(y, f)
        print("bernoulli serial %d: z per bin of p =" % serial, np.round(z, 2))
        assert set(np.unique(y)) <= {0.0, 1.0}
        assert np.abs(z).max() <= R.Z_MAX


def test_bernoulli_jitter_at_fixed_moments(gpu_device):
    """fmean = -6 / +6, fvar = NULL: the jitter is the rare label's whole probability (1049 of 2^20 expected, about 0 without it; the
    host test's z is 32 with the jitter dropped) -- the bins over wide moments cannot tell."""
    for fm in (-6.0, 6.0):
        y, f = _draw(_lik("bernoulli"), np.full(N, fm, np.float32), None, gpu_device, serial=3)
        z = R.bernoulli_fixed_z(y, fm)
        print("bernoulli at fmean %g: %d ones of %d, z = %.2f" % (fm, int(y.sum()), N, z))
        assert (f == fm).all() and abs(z) <= R.Z_MAX


@pytest.mark.parametrize("name", ["beta_6", "beta_2"])
def test_beta_dispersion_and_mean_z(gpu_device, name):
    """The statistics that see the Beta's scale (x 1.02: |z| = 12) and its link (x 1.05: |z| = 10-30), which the pooled PIT does not."""
    kind, par = R.CONTINUOUS[name]
    mu, _ = _continuous_inputs(name)
    y, f = _draw(_lik(kind, **par), mu, None, gpu_device, serial=4)
    m = R.ip(f)
    zd, zm = R.beta_dispersion_z(y, f, par["scale"]), R.binned_z(y - m, m * (1.0 - m) / (par["scale"] + 1.0), f)
    print("%s: dispersion z = %.2f, mean z per bin of f =" % (name, zd), np.round(zm, 2))
    assert abs(zd) <= R.Z_MAX and np.abs(zm).max() <= R.Z_MAX


# ---- 4: Poisson ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", R.POISSON_RATES, ids=lambda r: "%g" % r)
def test_poisson_fixed_rate_chi2(gpu_device, rate):
    f32 = np.float32(np.log(rate / R.BINSIZE))
    y, f = _draw(_lik("poisson", binsize=R.BINSIZE), np.full(N, f32), None, gpu_device, serial=7)
    lam = float(np.float32(R.BINSIZE) * np.exp(f32))        # the rate the float32 moment stands for
    assert (f == f32).all()
    chi2, dof, lim = R.poisson_chi2(y, lam)
    print("poisson rate %.9g: chi2 = %.1f on %d dof (limit %.1f); mean %.6g" % (lam, chi2, dof, lim, y.mean()))
    assert (y >= 0).all() and (y == np.floor(y)).all()
    assert chi2 <= lim


def test_poisson_varying_rate_mean_and_dispersion(gpu_device):
    rng = np.random.default_rng(41)
    mu = rng.uniform(-2.0, 4.0, N).astype(np.float32)
    mu[:2] = -2.0, 4.0
    for serial in (1, 2):
        y, f = _draw(_lik("poisson", binsize=R.BINSIZE), mu, None, gpu_device, serial=serial)
        zm, zd = R.poisson_z(y, R.BINSIZE * np.exp(f))
        print("poisson serial %d: mean z =" % serial, np.round(zm, 2), " dispersion z =", np.round(zd, 2))
        assert (y >= 0).all() and (y == np.floor(y)).all()
        assert np.abs(zm).max() <= R.Z_MAX and np.abs(zd).max() <= R.Z_MAX


def test_poisson_caps_hold_where_nothing_is_accepted(gpu_device):
    """A rate that overflows gives +inf, a NaN moment NaN, and the launch returns: the loops are capped (no sampler accepts here)."""
    mu = np.array([100.0, np.nan, 0.0, 100.0, np.nan], dtype=np.float32)
    y, _ = _draw(_lik("poisson", binsize=R.BINSIZE), mu, None, gpu_device)
    print("poisson at fmean", mu, "->", y)
    assert np.isposinf(y[[0, 3]]).all() and np.isnan(y[[1, 4]]).all() and np.isfinite(y[2])
    for kind, par in [("gamma", dict(shape=0.5)), ("beta", dict(scale=2.0)), ("student_t", dict(scale=1.0, df=3.0)), ("bernoulli", {}),
                      ("gaussian", dict(variance=1.0)), ("exponential", {}), ("ordinal", {})]:
        yk, _ = _draw(_lik(kind, **par), mu, np.ones(5, np.float32), gpu_device)
        assert np.isnan(yk[[1, 4]]).all() and np.isfinite(yk[2]), (kind, yk)


# ---- 5: Ordinal --------------------------------------------------------------------------------------------------------------------------
def test_ordinal_bin_z(gpu_device):
    lik = _lik("ordinal")
    lik._buffer()[:1].fill_(R.ORD_SIGMA)                     # the device's sigma; the host copy (param[0]) stays 1.0
    assert lik.lik_desc().param[0] == 1.0
    mu, v = R.moments(N, 51)
    for serial in (1, 2):
        y, f = _draw(lik, mu, v, gpu_device, serial=serial)
        z = R.ordinal_z(y, f)
        print("ordinal serial %d: z per bin =" % serial, np.round(z, 2), " counts", np.bincount(y.astype(int).ravel(), minlength=5))
        assert set(np.unique(y)) <= {0.0, 1.0, 2.0, 3.0, 4.0}
        assert np.abs(z).max() <= R.Z_MAX


def test_ordinal_sigma_directed_z(gpu_device):
    """fvar = NULL, f uniform over the edges: the z along d E[y | f] / d sigma (sigma x 1.02 gives |z| = 8-9 on the host)."""
    lik = _lik("ordinal")
    lik._buffer()[:1].fill_(R.ORD_SIGMA)
    f32 = R.ordinal_f(N, 52)
    y, f = _draw(lik, f32, None, gpu_device, serial=6)
    z = R.ordinal_sigma_z(y, f)
    print("ordinal sigma-directed z = %.2f" % z)
    assert (f == f32).all() and abs(z) <= R.Z_MAX


# ---- 6: MultiClass ---------------------------------------------------------------------------------------------------------------------
def _first_argmax(f):
    return np.argmax(f, axis=1)                              # (NumPy's argmax is the first maximum)


@pytest.mark.parametrize("eps", [0.05, 1e-3])
def test_multiclass_hits_and_misses(gpu_device, eps):
    C, n = 4, N
    mu, v = R.moments(n * C, 61)
    mu, v = mu.reshape(n, C), v.reshape(n, C)
    mu[: n // 4, 1] = mu[: n // 4, 2]                          # ties, constructed: with fvar = 0 there ...
    v[: n // 4, 1:3] = 0.0
    y, f = _draw(_lik("multiclass", num_classes=C, epsilon=eps), mu, v, gpu_device, serial=2)
    assert y.shape == (n, 1) and f.shape == (n, C)
    y = y[:, 0]
    assert set(np.unique(y)) <= set(range(C))
    am = _first_argmax(f)
    tie = (f[:, 1] == f[:, 2]) & (am == 1)
    assert tie.sum() > n // 32                               # ... rows whose maximum is attained twice: the hit is the first
    for name, rows in (("all rows", np.ones(n, bool)), ("tied rows", tie)):
        hit = y[rows] == am[rows]
        zh = R.hit_z(hit.sum(), rows.sum(), eps)
        off = ((y[rows] - am[rows]) % C)[~hit].astype(int)
        chi2, dof, lim = R.chi2_counts(np.bincount(off, minlength=C)[1:], np.full(C - 1, 1.0 / (C - 1)))
        print("multiclass eps %g, %s (%d): hit z = %.2f; miss offsets chi2 = %.2f on %d dof (limit %.1f)" % (eps, name, rows.sum(), zh, chi2, dof, lim))
        assert abs(zh) <= R.Z_MAX and chi2 <= lim


# ---- 7: the grid stride, the tails, determinism and freshness ---------------------------------------------------------------------------
@pytest.mark.parametrize("Dy", [1, 3])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 257 * 4096 + 3])
def test_every_element_is_written_and_nothing_else(gpu_device, T, Dy):
    from dgps_with_iwvi_amd import _abi
    lik = _lik("gamma", shape=0.5)
    g = torch.Generator(device="cpu").manual_seed(T + Dy)
    fm = torch.rand(T, Dy, generator=g).to(gpu_device)
    fv = torch.rand(T, Dy, generator=g).to(gpu_device)
    bufs = [torch.full((T * Dy + 8,), -7.0, device=gpu_device) for _ in range(2)]
    _abi.check(_raw(lik.lik_desc(), fm, fv, T, Dy, bufs[0], serial=4, out_f=bufs[1]))
    for b in bufs:
        assert (b[T * Dy:] == -7.0).all()
    assert (bufs[0][:T * Dy] > 0).all() and (bufs[1][:T * Dy] != -7.0).all()
    again = torch.full((T * Dy,), -7.0, device=gpu_device)
    _abi.check(_raw(lik.lik_desc(), fm, fv, T, Dy, again, serial=4))
    assert torch.equal(again, bufs[0][:T * Dy])              # same (seed, serial): the same bits
    _abi.check(_raw(lik.lik_desc(), fm, fv, T, Dy, again, serial=4, seed=1))
    assert not torch.equal(again, bufs[0][:T * Dy])


def test_empty_launch(gpu_device):
    from dgps_with_iwvi_amd import _abi
    out = torch.full((4,), -7.0, device=gpu_device)
    assert _raw(_lik("bernoulli").lik_desc(), None, None, 0, 1, out) == 0
    assert (out == -7.0).all()
    y = _lik("bernoulli").sample_y(torch.empty(0, 2, device=gpu_device), torch.empty(0, 2, device=gpu_device))
    assert tuple(y.shape) == (0, 2)


def test_serial_word_advances_and_a_replayed_graph_draws_fresh_values(gpu_device):
    from dgps_with_iwvi_amd import _abi
    lik = _lik("poisson", binsize=R.BINSIZE)
    T = 5000                                                   # 20 workgroups: the ticket is taken by more than one
    fm = torch.full((T, 1), 1.0, device=gpu_device)
    word = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    outs = [torch.empty(T, device=gpu_device) for _ in range(2)]
    for o in outs:
        _abi.check(_raw(lik.lik_desc(), fm, None, T, 1, o, serial_dev=word))
    assert int(word.item()) == 2 and not torch.equal(outs[0], outs[1])
    host = torch.empty(T, device=gpu_device)
    _abi.check(_raw(lik.lik_desc(), fm, None, T, 1, host, serial=1))
    assert torch.equal(host, outs[1])                          # the device's serial 1 is the host's serial 1
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    out = torch.empty(T, device=gpu_device)
    with torch.cuda.stream(side):
        _abi.check(_raw(lik.lik_desc(), fm, None, T, 1, out, serial_dev=word))      # (warm-up outside the capture)
        with torch.cuda.graph(graph, stream=side):
            _abi.check(_raw(lik.lik_desc(), fm, None, T, 1, out, serial_dev=word))
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seen.append(out.clone())
    print("serial word after 2 launches, a warm-up and 2 replays:", int(word.item()), " means", [float(s.mean()) for s in seen])
    assert int(word.item()) == 5 and not torch.equal(seen[0], seen[1])
    for s in seen:
        assert abs(float(s.double().mean()) - R.BINSIZE * np.e) <= R.Z_MAX * np.sqrt(R.BINSIZE * np.e / T)


# ---- 8: validation -----------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_device):
    from dgps_with_iwvi_amd import _abi, likelihoods as L
    lib = _abi.lib()
    fm = torch.zeros(4, 3, device=gpu_device)
    out = torch.full((12,), -7.0, device=gpu_device)
    good = _lik("gaussian", variance=1.0).lik_desc()

    def refused(rc, word):
        msg = lib.iwvi_last_error().decode()
        print("refused:", msg)
        assert rc == _abi.ERR_ARG and "iwvi_lik_sample_y" in msg and word in msg, (rc, msg)

    refused(_raw(None, fm, fm, 4, 3, out), "descriptor")
    bad = _abi.LikDesc()
    bad.type = 7
    refused(_raw(bad, fm, fm, 4, 3, out), "unknown")
    bad.type, bad.param[0] = _abi.LIK_GAMMA, -1.0
    refused(_raw(bad, fm, fm, 4, 3, out), "shape")
    bad.type, bad.param[0], bad.param[1] = _abi.LIK_ORDINAL, 1.0, 3.0
    refused(_raw(bad, fm, fm, 4, 3, out), "param0_dev")
    refused(_raw(good, fm, fm, -1, 3, out), "T")
    refused(_raw(good, fm, fm, 4, 0, out), "Dy")
    refused(_raw(good, fm, fm, 4, _abi.MAX_P + 1, out), "Dy")
    refused(_raw(_lik("multiclass", num_classes=4).lik_desc(), fm, fm, 4, 3, out), "MultiClass")
    refused(_raw(good, fm, fm, 4, 3, None), "out_y")
    assert (out == -7.0).all()
    with pytest.raises(_abi.IwviError):
        L.Poisson().sample_y(torch.zeros(3, 1), torch.ones(3, 1))


# ---- 9: through the stack -------------------------------------------------------------------------------------------------------------
def _stack(kind, lv, dev, Dy=2):
    """The specs of tests/test_gpu_predict_mixture.py: L = 2, M = 16, with and without a latent-variable layer, multiclass C = 3."""
    from dgps_with_iwvi_amd import synthetic
    import multiclass_restatement as MR
    if kind == "multiclass":
        spec = MR.make_spec(3, L=2, M=16, B=10, K=3, lv=lv, seed=9)
        lik = _lik(kind, num_classes=3)
    else:
        spec = synthetic.make_spec(L=2, M=16, B=10, K=3, with_lv=lv, Dy=Dy, seed=9, distinct_y=True)
        par = {"bernoulli": {}, "poisson": dict(binsize=1.5), "student_t": dict(scale=0.7, df=4.0)}[kind]
        if kind == "bernoulli":
            spec["Y"] = (spec["Y"] > 0).astype(np.float64)
        elif kind == "poisson":
            spec["Y"] = np.floor(np.abs(spec["Y"]) * 3.0)
        lik = _lik(kind, **par)
    return spec, synthetic.build_model(spec, dev, likelihood=lik)


def _zs(spec, S, n, dev, seed=3):
    rng = np.random.default_rng(seed)
    return [_t(rng.standard_normal((S, n, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1])), dev) for l in spec["layers"]]


@pytest.mark.parametrize("lv", [True, False], ids=["lv", "nolv"])
@pytest.mark.parametrize("kind", ["bernoulli", "multiclass", "poisson", "student_t"])
def test_predict_y_draws_through_the_stack(gpu_device, kind, lv):
    """The exported f is the layer-by-layer route's m + sqrt(v) z_f, and the draws' mean per point and output lies within 6 standard errors
    of predict_mixture's mean (the standard error from its law-of-total-variance figure over S).  Every batch has a serial of its own BY
    DESIGN (the element index restarts with the launch), so ``batch_size=4`` does not give the bits of one batch: the distributional
    check is asserted on the batched result instead, and the same call with the same serial is asserted to give the same bits."""
    n, S = 9, 4096
    spec, model = _stack(kind, lv, gpu_device)
    X = spec["X"][:n]
    zs = _zs(spec, S, n, gpu_device)
    Dy = 3 if kind == "multiclass" else 2
    z_f = _t(np.random.default_rng(5).standard_normal((S, n, Dy)), gpu_device)
    y, f = model.predict_y_draws(X, S, zs=zs, z_f=z_f, return_f=True, serial=1)
    assert tuple(y.shape) == (S, n, 1 if kind == "multiclass" else 2) and tuple(f.shape) == (S, n, Dy)
    assert y.stride(1) > y.stride(0)                         # a transposed view of [N, S, Dt]: a point's draws are contiguous
    m, v = model.predict_f_multisample(X, S, zs=zs)
    want = _n64(m) + np.sqrt(_n64(v)) * _n64(z_f)
    err = np.abs(_n64(f) - want) / np.maximum(1.0, np.abs(want))
    print("%s lv=%s: out_f vs predict_f_multisample: max scaled error %.3g (bound %.1g)" % (kind, lv, err.max(), ROUTES))
    assert err.max() <= ROUTES
    pm = model.predict_mixture(X, S, zs=zs)
    pmean, pvar = _n64(pm["mean"]), _n64(pm["var"])
    again = model.predict_y_draws(X, S, zs=zs, z_f=z_f, serial=1)
    assert torch.equal(again, y)
    fresh = model.predict_y_draws(X, S, zs=zs)                # z_f drawn, the serial from the model's device word
    batched = model.predict_y_draws(X, S, zs=zs, batch_size=4, serial=1)
    assert not torch.equal(fresh, y)
    for name, draws in (("one batch", y), ("z_f drawn", fresh), ("batch_size=4", batched)):
        d = _n64(draws)
        if kind == "multiclass":
            freq = np.stack([(d[:, :, 0] == c).mean(0) for c in range(3)], 1)
            z = (freq - pmean) / np.sqrt(pmean * (1.0 - pmean) / S)
            assert set(np.unique(d)) <= {0.0, 1.0, 2.0}
        else:
            z = (d.mean(0) - pmean) / np.sqrt(pvar / S)
        print("%s lv=%s, %s: max |z| of the draws' mean against predict_mixture = %.2f" % (kind, lv, name, np.abs(z).max()))
        assert np.abs(z).max() <= R.Z_MAX
    if kind == "poisson":
        assert (_n64(y) >= 0).all() and (_n64(y) == np.floor(_n64(y))).all()
    with pytest.raises(NotImplementedError, match="predict_y_draws"):
        model.predict_y_samples_fused(X, 4)


@pytest.mark.parametrize("kind", ["poisson", "student_t"])
def test_evaluate_draws_is_self_consistent(gpu_device, kind):
    """Y drawn from predict_y_draws itself (another serial): the coverage of the central 90 % interval lies within 6 binomial standard
    errors of 0.9 -- for the Poisson of what a discrete interval can achieve: the share of a point's own draws inside its (closed)
    interval, averaged over the points, computed on the host from the same draws."""
    from dgps_with_iwvi_amd import evaluation
    spec, model = _stack(kind, True, gpu_device, Dy=1)
    Xt = np.tile(spec["X"], (200, 1))
    n, S = Xt.shape[0], 2000
    Y = model.predict_y_draws(Xt, 1)[0]                        # [n, 1]
    word = model._words()
    word[3] = 100
    res = evaluation.evaluate_draws(model, Xt, Y, num_predict_samples=S, predict_batch_size=1000, interval=0.9)
    print(kind, res)
    keys = {"test_coverage", "test_interval_width", "test_rmse"} | ({"test_loglik"} if kind == "student_t" else set())
    assert set(res) == keys and all(np.isfinite(v) for v in res.values())
    target = 0.9
    if kind == "poisson":
        word[3] = 100                                          # the same serials: the same draws
        share = []
        for lo in range(0, n, 1000):
            d = model.predict_y_draws(Xt[lo:lo + 1000], S)[:, :, 0]
            q = evaluation.sample_stats(d, shapiro=False, quantiles=[0.05, 0.95])["quantiles"]      # the interval evaluate_draws used
            share.append(((d >= q[:, 0]) & (d <= q[:, 1])).double().mean(0))
        target = float(torch.cat(share).mean().item())
        assert target >= 0.9
    se = np.sqrt(target * (1.0 - target) / n)
    print("%s: coverage %.4f against %.4f (standard error %.4f)" % (kind, res["test_coverage"], target, se))
    assert abs(res["test_coverage"] - target) <= 6.0 * se
    assert res["test_interval_width"] > 0
