"""Host-side checks of the Beta / Ordinal likelihoods (probit link): the pinning of the float64 restatement (tests/bounded_restatement.py)
the GPU tests compare the kernels with, the derivation of the GPU tests' constant, the Python surface that needs no GPU, and the C-ABI's
refusals, which return before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bounded_restatement as X   # noqa: E402

JIT = X.JIT


# ---- the float64 restatement is itself pinned ----------------------------------------------------------------------------------
def test_restatement_logp_matches_scipy():
    from scipy import stats
    f = np.linspace(-4.0, 4.0, 81)
    m = stats.norm.cdf(f) * (1 - 2 * JIT) + JIT
    for kind, kw, ys in X.ELEMENTWISE_CASES:
        lik = X.make(kind, **kw)
        for y in ys:
            got = lik.logp(f, np.full_like(f, y)).numpy()
            if kind == "beta":
                s = kw["scale"]
                want = stats.beta.logpdf(min(max(y, 1e-6), 1 - 1e-6), m * s, s - m * s)
            else:
                e, sig = np.concatenate([[-np.inf], kw["bin_edges"], [np.inf]]), kw["sigma"]
                ip = lambda x: stats.norm.cdf(x) * (1 - 2 * JIT) + JIT
                want = np.log(ip(e[int(y) + 1] / sig - f / sig) - ip(e[int(y)] / sig - f / sig) + 1e-6)
            np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11, err_msg="%s %r y=%g" % (kind, kw, y))


def test_ordinal_bins_sum_to_what_the_jitter_leaves_and_the_moments_are_theirs():
    lik = X.Ordinal(X.ELEMENTWISE_EDGES, sigma=1.3)
    f = np.linspace(-6.0, 6.0, 49)
    P = lik.bin_probs(f).numpy()
    np.testing.assert_allclose(P.sum(-1), 0.998, rtol=0, atol=1e-14)
    for y in range(4):
        np.testing.assert_allclose(lik.prob(f, np.full_like(f, y)).numpy(), P[:, y], rtol=0, atol=1e-15)
    j = np.arange(4.0)
    np.testing.assert_allclose(lik.conditional_mean(f).numpy(), (P * j).sum(-1), rtol=1e-14)
    np.testing.assert_allclose(lik.conditional_variance(f).numpy(), (P * j ** 2).sum(-1) - (P * j).sum(-1) ** 2, rtol=1e-12, atol=1e-14)
    b = X.Beta(scale=2.0)
    mm = b.conditional_mean(f).numpy()
    np.testing.assert_allclose(b.conditional_variance(f).numpy(), (mm - mm ** 2) / 3.0, rtol=1e-14)


def test_the_rule_is_exact_for_polynomials_in_both_forms():
    """Nodes and weights: E f^k under N(mu, v) for k <= 8, and the log-space form on g = log(1 + f^2 + f^4), to float64."""
    mu, v = np.array([0.3, -1.0, 1.2]), np.array([0.05, 0.5, 1.0])
    m2, m4 = mu ** 2 + v, mu ** 4 + 6 * mu ** 2 * v + 3 * v ** 2
    np.testing.assert_allclose(X.quad(lambda f: f ** 2, mu, v).numpy(), m2, rtol=1e-13)
    np.testing.assert_allclose(X.quad(lambda f: f ** 4, mu, v).numpy(), m4, rtol=1e-13)
    np.testing.assert_allclose(X.quad(lambda f: (f - X._t(mu)[..., None]) ** 8, mu, v).numpy(), 105 * v ** 4, rtol=1e-12)
    np.testing.assert_allclose(X.quad(lambda f: torch.log(1 + f ** 2 + f ** 4), mu, v, logspace=True).numpy(), np.log(1 + m2 + m4), rtol=1e-13)


def _rule(n, g, mu, v, logspace=False):
    x, w = np.polynomial.hermite.hermgauss(n)
    vals = np.array([g(mu + np.sqrt(2.0 * v) * xi) for xi in x])
    if logspace:
        return float(np.log((np.exp(vals - vals.max()) * w).sum() / np.sqrt(np.pi)) + vals.max())
    return float((vals * w).sum() / np.sqrt(np.pi))


@pytest.mark.parametrize("kind,kw,ys", X.ELEMENTWISE_CASES[1::2], ids=["beta-2", "ordinal-1.3"])
def test_quadrature_matches_adaptive_integration_at_a_few_moments(kind, kw, ys):
    """The 20-point rule against scipy.integrate.quad of the same integrands under N(mu, v): variational_expectations, the predictive
    density and the predictive mean / variance.  The rule is not exact for these integrands (a Beta density at y = 1e-3 is far from a
    polynomial in f: 3e-3 off at v = 1, in GPflow as here), so each comparison is allowed the rule's own convergence estimate -- twice its
    distance to the 48-point rule -- plus 1e-9 of 1 + |value|; the restatement's ``quad`` must BE the 20-point rule to 1e-12."""
    from scipy import integrate, stats
    lik = X.make(kind, **kw)
    for mu, v in ((0.3, 0.05), (-1.0, 0.5), (1.2, 1.0)):
        sd = np.sqrt(v)
        E = lambda g: integrate.quad(lambda f: stats.norm.pdf(f, mu, sd) * g(f), mu - 10 * sd, mu + 10 * sd, epsabs=1e-13, epsrel=1e-12, limit=200)[0]
        at = lambda g: (lambda f: float(g(np.array([f]))[0]))

        def check(what, got, g, want, logspace=False):
            r20, r48 = _rule(20, g, mu, v, logspace), _rule(48, g, mu, v, logspace)
            assert abs(got - r20) <= 1e-12 * (1.0 + abs(r20)), (what, got, r20)
            tol = 2.0 * abs(r20 - r48) + 1e-9 * (1.0 + abs(want))
            assert abs(got - want) <= tol, (kind, what, mu, v, got, want, tol)
        pm, pv = lik.predict_mean_and_var(np.array([mu]), np.array([v]))
        em, e2 = E(at(lik.conditional_mean)), E(at(lik.second_moment))
        check("mean", float(pm), at(lik.conditional_mean), em)
        check("second moment", float(pv) + float(pm) ** 2, at(lik.second_moment), e2)
        for y in ys[1:3]:
            g = at(lambda f: lik.logp(f, np.full_like(f, y)))
            check("var_exp y=%g" % y, float(lik.variational_expectations(np.array([mu]), np.array([v]), np.array([y]))), g, E(g))
            check("density y=%g" % y, float(lik.predict_density(np.array([mu]), np.array([v]), np.array([y]))), g, np.log(E(lambda f: np.exp(g(f)))), True)


def test_heads_of_the_restatement_match_central_differences():
    MU, V = X.moment_grid()
    MU, V = MU[::37], V[::37]
    for kind, kw, ys in X.ELEMENTWISE_CASES[1::2]:
        lik = X.make(kind, **kw)
        Y = np.full_like(MU, ys[2])
        dmu, dv, dpar, *_ = X.heads(lik, MU, V, Y)
        h = 1e-4                                                 # (the Ordinal's float64 difference of two cdfs carries 1e-11: no smaller step)
        ve = lambda m, v: lik.variational_expectations(m, v, Y).numpy()
        np.testing.assert_allclose(dmu.numpy(), (ve(MU + h, V) - ve(MU - h, V)) / (2 * h), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(dv.numpy(), (ve(MU, V * (1 + 2e-2)) - ve(MU, V * (1 - 2e-2))) / (4e-2 * V), rtol=1e-3, atol=5e-5)
        p0 = getattr(lik, lik.par_name)
        setattr(lik, lik.par_name, p0 + h)
        up = ve(MU, V)
        setattr(lik, lik.par_name, p0 - h)
        dn = ve(MU, V)
        setattr(lik, lik.par_name, p0)
        np.testing.assert_allclose(dpar.numpy(), (up - dn) / (2 * h), rtol=1e-5, atol=1e-6)


def test_the_bound_of_the_gpu_tests_is_three_times_plain_float32():
    """C_BOUND is derived: the kernels' formulas in float32 NumPy over the GPU tests' own cases, times 3, rounded up."""
    worst = X.measure_float32()
    print("float32 NumPy, multiples of 2^-24 S: " + "  ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    top = max(worst.values())
    assert 3.0 * top <= X.C_BOUND <= 3.0 * top + 1.0, (top, X.C_BOUND)


def test_naive_float32_difference_loses_the_far_bins():
    """What the erfc form is for: at 8 sigma from a bin the plain float32 Phi(l) - Phi(r) puts log(P + 1e-6) off by 1e-2, the one-sided
    form stays at float32 resolution."""
    from scipy import special
    lik = X.Ordinal(X.ELEMENTWISE_EDGES, sigma=1.0)
    f = np.linspace(-8.0, 8.0, 321).astype(np.float32)
    y = np.full_like(f, 1.0)
    ref = lik.logp(f.astype(np.float64), y.astype(np.float64)).numpy()
    good = X.Float32(lik).logp(f, y)
    Phi = lambda x: (np.float32(0.5) * special.erfc(-x * np.float32(1 / np.sqrt(2)))).astype(np.float32)
    naive = np.log(np.float32(1 - 2 * JIT) * (Phi(np.float32(0.0) - f) - Phi(np.float32(-1.0) - f)) + np.float32(1e-6))
    assert np.abs(naive - ref).max() > 5e-3 and np.abs(good - ref).max() < 5e-6, (np.abs(naive - ref).max(), np.abs(good - ref).max())


def test_targets_cover_the_clip_and_every_bin():
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=2, M=32, B=12, K=4, with_lv=True, seed=3)
    yb = X.targets(spec, "beta")
    assert yb[0, 0] == 0.0 and yb[1, 0] == 1.0 and (yb >= 0).all() and (yb <= 1).all()
    yo = X.targets(spec, "ordinal")
    assert sorted(set(yo.reshape(-1).tolist())) == [0.0, 1.0, 2.0, 3.0]


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_classes_descriptors_and_refusals():
    import dgps_with_iwvi.likelihoods as alias
    from dgps_with_iwvi_amd import _abi, likelihoods
    from dgps_with_iwvi_amd.models import DGP_VI
    assert alias.Beta is likelihoods.Beta and alias.Ordinal is likelihoods.Ordinal
    b = likelihoods.Beta(scale=0.5)
    d = b.lik_desc()
    assert (d.type, d.param[0], d.param0_dev) == (8, 0.5, None) and b.trained_scalar() == ("lik_scale", 0.5) and b.grad_name == "lik_scale"
    b.scale = 3.0
    assert b.scale == 3.0 and b.lik_desc().param[0] == 3.0 and likelihoods.Beta().scale == 1.0
    assert likelihoods.Beta(invlink=likelihoods.inv_probit).scale == 1.0 and likelihoods.Beta(invlink="inv_probit").scale == 1.0
    with pytest.raises(AttributeError):
        b.variance
    with pytest.raises(NotImplementedError, match="logit"):
        likelihoods.Beta(invlink="logit")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            likelihoods.Beta(scale=bad)
    o = likelihoods.Ordinal([-1.0, 0.0, 1.5])
    assert o.sigma == 1.0 and o.num_bins == 4 and o.grad_name == "lik_sigma" and o.trained_scalar() == ("lik_sigma", 1.0)
    assert o.bin_edges.tolist() == [-1.0, 0.0, 1.5] and not o.bin_edges.flags.writeable
    o.sigma = 0.7
    buf = o._buffer()
    assert buf.dtype == torch.float32 and buf.tolist() == pytest.approx([0.7, -1.0, 0.0, 1.5])
    d = o.lik_desc()
    assert (d.type, d.param[1], d.param0_dev) == (9, 3.0, buf.data_ptr()) and d.param[0] == pytest.approx(0.7)
    view = o.trained_scalar_view()
    assert view.data_ptr() == buf.data_ptr() and view.numel() == 1
    o.bind_device_variance(view)                                 # the trainer's call: its own view is accepted ...
    with pytest.raises(ValueError, match="own device buffer"):
        o.bind_device_variance(torch.ones(1))                    # ... a foreign tensor is not
    view.fill_(0.9)
    assert o.sigma == pytest.approx(0.7)                         # nobody said the device copy moved
    o.mark_device_variance_changed()
    assert o.sigma == pytest.approx(0.9) and o.host_value() == o.sigma
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            o.sigma = bad
    for bad in ([], list(range(32)), [0.0, 0.0], [1.0, 0.5], [0.0, float("inf")], [float("nan")], [0.0, 1e-50]):      # (1e-50 is 0 in float32)
        with pytest.raises(ValueError, match="bin edges"):
            likelihoods.Ordinal(bad)
    assert likelihoods.Ordinal(list(range(31))).num_bins == _abi.MAX_P == 32
    assert not likelihoods.is_gaussian(b) and not likelihoods.is_gaussian(o)
    # targets
    b.check_targets(np.array([[0.0], [0.3], [1.0]]))
    o.check_targets(torch.tensor([[0.0], [3.0]]))
    for bad in (-0.1, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"in \[0, 1\]"):
            b.check_targets(np.array([[0.5], [bad]]))
    for bad in (-1.0, 4.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"integers in \[0, 3\]"):
            o.check_targets(np.array([[1.0], [bad]]))
    with pytest.raises(ValueError, match=r"in \[0, 1\]"):        # the models check at construction, before anything touches a device
        DGP_VI(np.zeros((3, 2)), np.array([[0.5], [1.5], [0.2]]), [], likelihoods.Beta())
    with pytest.raises(ValueError, match="integers"):
        DGP_VI(np.zeros((3, 2)), np.array([[1.0], [0.5], [2.0]]), [], likelihoods.Ordinal([0.0, 1.0]))
    # model.to(device) moves the Ordinal's buffer with the data
    moved = []

    class Spy(likelihoods.Ordinal):
        def to(self, device):
            moved.append(device)
            return super().to(device)
    spy = Spy([0.0, 1.0])
    spy._buffer()
    DGP_VI(np.zeros((3, 2)), np.array([[1.0], [0.0], [2.0]]), [], spy).to(torch.device("cpu"))
    assert moved == [torch.device("cpu")] and spy._buffer().device.type == "cpu" and spy._buffer().tolist() == [1.0, 0.0, 1.0]
    if not torch.cuda.is_available():
        with pytest.raises(_abi.IwviError, match="no CPU fallback"):  # the arithmetic exists as HIP kernels only
            b.logp(torch.zeros(3, 1), torch.full((3, 1), 0.5))


def test_checkpoint_round_trip_of_the_likelihood():
    from dgps_with_iwvi_amd import build_models, likelihoods
    o = likelihoods.Ordinal([-1.0, 0.0, 1.5])
    o.sigma = 0.75
    for lik, kind, params, fresh in ((likelihoods.Beta(scale=0.75), "Beta", [0.75], likelihoods.Beta()),
                                     (o, "Ordinal", [0.75, -1.0, 0.0, 1.5], likelihoods.Ordinal([0.0, 1.0, 2.0]))):
        st = build_models.likelihood_state(lik)
        assert sorted(st) == ["likelihood.params", "likelihood.type"] and str(st["likelihood.type"]) == kind
        assert st["likelihood.params"].dtype == np.float64 and st["likelihood.params"].tolist() == params
        build_models.load_likelihood_state(fresh, st)
        assert build_models.likelihood_state(fresh)["likelihood.params"].tolist() == params
        for other in (likelihoods.Gaussian(0.3), likelihoods.StudentT(), likelihoods.Bernoulli(), likelihoods.Gamma(),
                      likelihoods.Ordinal([0.0]) if kind == "Beta" else likelihoods.Beta()):
            with pytest.raises(ValueError, match="checkpoint holds a %s" % kind):
                build_models.load_likelihood_state(other, st)
    # the restored edges are written into an existing device buffer in place
    live = likelihoods.Ordinal([0.0, 1.0, 2.0])
    ptr = live._buffer().data_ptr()
    build_models.load_likelihood_state(live, build_models.likelihood_state(o))
    assert live._buffer().data_ptr() == ptr and live._buffer().tolist() == pytest.approx([0.75, -1.0, 0.0, 1.5])
    with pytest.raises(ValueError, match="3 bin edges, the model one with 2"):
        build_models.load_likelihood_state(likelihoods.Ordinal([0.0, 1.0]), build_models.likelihood_state(o))

    class MyBeta(likelihoods.Beta):                              # a subclass keeps its parent's checkpoint type
        pass
    mine = MyBeta()
    build_models.load_likelihood_state(mine, build_models.likelihood_state(MyBeta(scale=4.0)))
    assert mine.scale == 4.0


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


def _desc(_abi, type_, p0=1.0, p1=0.0, dev=None):
    d = _abi.LikDesc()
    d.type, d.param[0], d.param[1], d.param0_dev = type_, p0, p1, dev
    return d


def test_header_names_the_two_types_and_nothing_moved():
    from dgps_with_iwvi_amd import _abi
    text = open(os.path.join(os.path.dirname(HERE), "include", "iwvi_hip.h")).read()
    for name, value in (("IWVI_LIK_BETA", 8), ("IWVI_LIK_ORDINAL", 9)):
        assert "%s = %d" % (name, value) in text, name
    assert (_abi.LIK_BETA, _abi.LIK_ORDINAL) == (8, 9)
    assert "IWVI_LIK_GAMMA = 6" in text and "#define IWVI_ABI_VERSION 19" in text and "7: unassigned" in text
    assert " = 7" not in text[text.index("enum { IWVI_LIK_GAUSSIAN"):text.index("typedef struct iwvi_lik_desc")]      # value 7 stays unassigned
    # the descriptor's layout: type, param[2], lgc, param0_dev -- 24 bytes on a 64-bit host, the pointer at 16
    assert [f[0] for f in _abi.LikDesc._fields_] == ["type", "param", "lgc", "param0_dev"]
    assert ctypes.sizeof(_abi.LikDesc) == 24 and _abi.LikDesc.param0_dev.offset == 16 and _abi.LikDesc.lgc.offset == 12
    struct = text[text.index("typedef struct iwvi_lik_desc {"):text.index("} iwvi_lik_desc;")]
    assert [ln.strip() for ln in struct.splitlines()[1:]] == ["int32_t type;", "float param[2];", "float lgc;", "const float* param0_dev;"]


def test_refused_arguments_return_before_any_launch():
    _abi, lib = _lib()
    assert lib.iwvi_version() == _abi.ABI_VERSION == 19
    p = ctypes.c_void_p(16)                                      # never dereferenced: every call below is refused on its arguments
    E = _abi.ERR_ARG
    elem = lambda fn, d, out=p: fn(d, p, p, p, 4, 1, 1, 4, out, None)
    pmv = lambda d, om=p, ov=p: lib.iwvi_lik_predict_mean_and_var(d, p, p, 4, om, ov, None)
    red = lambda d, logp=p, elbo=p, ticket=p: lib.iwvi_lik_elbo_reduce(d, p, p, p, 4, 2, 1, 2, 1, None, None, 0, None, None, 0, 1.0, 2, 0,
                                                                       None, logp, elbo, ticket, None)
    bwd = lambda d, sums=p, ws=p: lib.iwvi_lik_elbo_backward(d, p, p, p, 1, None, None, 0, 4, 2, 1.0, 0, p, p, p, None, None, 0, None, 2,
                                                             sums, ws, None)
    mix = lambda d: lib.iwvi_lik_predict_mixture(d, p, p, p, 4, 3, 1, 3, 1, p, p, p, None)
    every = (lambda d: elem(lib.iwvi_lik_var_exp, d), lambda d: elem(lib.iwvi_lik_predict_density, d), pmv, red, bwd, mix)
    B, O, dev = _abi.LIK_BETA, _abi.LIK_ORDINAL, 16
    for bad, text in ((_desc(_abi, B, p0=0.0), b"Beta scale"), (_desc(_abi, B, p0=-2.0), b"Beta scale"), (_desc(_abi, B, p0=float("nan")), b"Beta scale"),
                      (_desc(_abi, O, p1=0.0, dev=dev), b"bin edges"), (_desc(_abi, O, p1=32.0, dev=dev), b"bin edges"),
                      (_desc(_abi, O, p1=2.5, dev=dev), b"bin edges"), (_desc(_abi, O, p1=float("nan"), dev=dev), b"bin edges"),
                      (_desc(_abi, O, p1=3.0), b"Ordinal needs param0_dev"),
                      (_desc(_abi, O, p0=0.0, p1=3.0, dev=dev), b"Ordinal sigma"), (_desc(_abi, O, p0=-1.0, p1=3.0, dev=dev), b"Ordinal sigma"),
                      (_desc(_abi, O, p0=float("nan"), p1=31.0, dev=dev), b"Ordinal sigma"),
                      (_desc(_abi, 7), b"unknown likelihood type 7"), (_desc(_abi, 10), b"unknown likelihood type 10")):
        for call in every:
            assert call(bad) == E
            assert text in lib.iwvi_last_error(), (text, lib.iwvi_last_error())
    for good in (_desc(_abi, B, p0=1.5), _desc(_abi, B, p0=1.5, dev=dev), _desc(_abi, O, p0=1.0, p1=31.0, dev=dev), _desc(_abi, O, p0=1.0, p1=1.0, dev=dev)):
        for fn in (lib.iwvi_lik_var_exp, lib.iwvi_lik_predict_density):
            assert elem(fn, good, out=None) == E                 # NULL outputs
            assert fn(good, p, p, p, 4, 0, 1, 4, p, None) == E   # Dy = 0
            assert fn(good, p, p, None, 4, 1, 1, 4, p, None) == E   # no targets
        assert lib.iwvi_lik_var_exp(good, p, None, p, 4, 1, 1, 4, p, None) == E      # the expectation needs the variance (logp does not)
        assert pmv(good, om=None) == E and pmv(good, ov=None) == E
        assert red(good, logp=None, elbo=None) == E              # nothing asked for
        assert red(good, logp=None) == E and red(good, ticket=None) == E             # out_elbo needs out_logp and a ticket
        assert bwd(good, sums=None) == E and bwd(good, ws=None) == E
        assert lib.iwvi_lik_predict_mixture(good, p, p, None, 4, 3, 1, 3, 1, p, p, p, None) == E     # out_logp without Y
        assert lib.iwvi_lik_var_exp(good, p, p, p, 0, 1, 1, 1, p, None) == 0          # T = 0: nothing to do, nothing launched
        assert lib.iwvi_lik_predict_mixture(good, p, p, p, 0, 3, 1, 3, 1, p, p, p, None) == 0


def test_kernel_resources_lists_the_new_kernels_without_scratch():
    from dgps_with_iwvi_amd import kernel_resources as kr
    if not os.path.exists(kr.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf here")
    rows = kr.check()
    for base, n in (("k_bo_elbo", 10), ("k_bo_elbo_bwd", 2), ("k_bo_elem", 6), ("k_bo_mix", 10)):    # two types x (5 SEG | 1 | 3 MODE | 5 SEG)
        mine = [r for r in rows if r["demangled"].split("<")[0] == base]
        assert len(mine) == n, (base, [r["demangled"] for r in mine])
        assert {r["demangled"].split("<")[1].split(",")[0].rstrip(">") for r in mine} == {"8", "9"}
        for r in mine:
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
        # the budget: a multiple of 8, at most 128 (four waves per SIMD), that every instantiation fits and none leaves 8 to spare
        most = max(r["vgpr_count"] for r in mine)
        assert base in kr.NO_SCRATCH and kr.MAX_VGPRS[base] % 8 == 0 and most <= kr.MAX_VGPRS[base] <= 128
        assert kr.MAX_VGPRS[base] - most < 8, (base, most, kr.MAX_VGPRS[base])
