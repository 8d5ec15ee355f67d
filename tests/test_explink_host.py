"""Host-side checks of the Poisson / Exponential / Gamma likelihoods (exp link): the pinning of the float64 restatement
(tests/explink_restatement.py) the GPU tests compare the kernels with, the Python surface that needs no GPU, and the C-ABI's refusals,
which return before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import explink_restatement as X   # noqa: E402

CASES = [("poisson", dict(binsize=1.0), (0.0, 1.0, 3.0, 40.0)), ("poisson", dict(binsize=2.5), (0.0, 7.0)),
         ("exponential", {}, (0.0, 0.05, 1.3, 9.0)),
         ("gamma", dict(shape=2.5), (0.05, 1.3, 9.0)), ("gamma", dict(shape=50.0), (0.5, 30.0)), ("gamma", dict(shape=0.6), (0.5, 3.0))]


# ---- the float64 restatement is itself pinned ----------------------------------------------------------------------------------
def test_restatement_logp_matches_scipy():
    from scipy import stats
    f = np.linspace(-4.0, 4.0, 81)
    lam = np.exp(f)
    for kind, kw, ys in CASES:
        lik = X.make(kind, **kw)
        for y in ys:
            got = lik.logp(f, np.full_like(f, y)).numpy()
            if kind == "poisson":
                want = stats.poisson.logpmf(y, kw["binsize"] * lam)
            elif kind == "exponential":
                want = stats.expon.logpdf(y, scale=lam)
            else:
                want = stats.gamma.logpdf(y, kw["shape"], scale=lam)
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, err_msg="%s %r y=%g" % (kind, kw, y))
            # the one-shape form the closed forms and the error scales are written in is the same function
            np.testing.assert_allclose(X._ExpLink.logp(lik, f, np.full_like(f, y)).numpy(), want, rtol=1e-12, atol=1e-12)


def test_closed_form_expectation_is_the_quadrature_of_logp():
    """GPflow's two branches agree: on the grid (mu in [-3, 3], v in [1e-4, 4]) the 20-point rule reproduces E[exp f], so the closed form
    equals the rule over logp to 1e-10 of the sum of the terms' magnitudes."""
    MU, V = X.moment_grid()
    worst = 0.0
    for kind, kw, ys in CASES:
        lik = X.make(kind, **kw)
        for y in ys:
            Y = np.full_like(MU, y)
            closed = lik.variational_expectations(MU, V, Y).numpy()
            rule = X.quad(lambda f: lik.logp(f, X._t(Y)[..., None]), MU, V).numpy()
            scale = X.var_exp_scale(lik, MU, V, Y).numpy()
            rel = float((np.abs(closed - rule) / scale).max())
            worst = max(worst, rel)
            assert rel <= 1e-10, (kind, kw, y, rel)
    print("closed form vs 20-point rule: worst %.3e of the terms' magnitudes" % worst)


def test_digamma_recurrence_and_series_reach_float64():
    """The device evaluates psi(a) by the recurrence up to a >= 6 and the asymptotic series through x^-10: the same arithmetic here against
    scipy.special.digamma."""
    from scipy import special

    def psi(x):
        r = 0.0
        for _ in range(6):
            if not x < 6.0:
                break
            r -= 1.0 / x
            x += 1.0
        i = 1.0 / x
        i2 = i * i
        return r + np.log(x) - 0.5 * i - i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132)))))

    for a in (1e-3, 0.05, 0.6, 1.0, 2.5, 5.999, 6.0, 50.0, 1e4):
        assert abs(psi(a) - special.digamma(a)) <= 2e-11 * max(1.0, abs(special.digamma(a))), a


# ---- the Python surface without a device ----------------------------------------------------------------------------------------
def test_python_surface_without_a_device():
    import dgps_with_iwvi.likelihoods as alias
    from dgps_with_iwvi_amd import _abi, likelihoods
    from dgps_with_iwvi_amd.models import DGP_VI
    assert (_abi.LIK_POISSON, _abi.LIK_EXPONENTIAL, _abi.LIK_GAMMA) == (4, 5, 6)
    for name in ("Poisson", "Exponential", "Gamma"):
        cls = getattr(likelihoods, name)
        assert getattr(alias, name) is cls
        for meth in ("logp", "variational_expectations", "predict_mean_and_var", "predict_density", "lik_desc", "check_targets"):
            assert callable(getattr(cls, meth)), (cls, meth)
        with pytest.raises(NotImplementedError, match="exp link"):
            cls(invlink="log")
        with pytest.raises(NotImplementedError, match="square"):
            cls(invlink=np.square)
        cls(invlink=likelihoods.exp), cls(invlink=np.exp), cls(invlink=torch.exp), cls(invlink="exp")
    # descriptors
    p = likelihoods.Poisson(binsize=2.5)
    d = p.lik_desc()
    assert (d.type, d.param[0], d.param0_dev) == (4, 2.5, None) and p.grad_name is None and p.trained_scalar() is None and p.binsize == 2.5
    assert likelihoods.Poisson().lik_desc().param[0] == 1.0
    e = likelihoods.Exponential()
    assert (e.lik_desc().type, e.lik_desc().param0_dev, e.grad_name, e.trained_scalar()) == (5, None, None, None)
    g = likelihoods.Gamma(shape=0.5)
    d = g.lik_desc()
    assert (d.type, d.param[0], d.param0_dev) == (6, 0.5, None) and g.trained_scalar() == ("lik_shape", 0.5) and g.grad_name == "lik_shape"
    g.shape = 3.0
    assert g.shape == 3.0 and g.lik_desc().param[0] == 3.0 and likelihoods.Gamma().shape == 1.0
    with pytest.raises(AttributeError):
        g.variance
    assert not likelihoods.is_gaussian(p) and not likelihoods.is_gaussian(e) and not likelihoods.is_gaussian(g)
    # constructor refusals
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="binsize"):
            likelihoods.Poisson(binsize=bad)
        with pytest.raises(ValueError, match="shape"):
            likelihoods.Gamma(shape=bad)
    # targets
    p.check_targets(np.array([[0.0], [3.0], [40.0]]))
    e.check_targets(torch.tensor([[0.0], [0.05]]))
    g.check_targets(np.array([[0.05], [9.0]]))
    for bad in (-1.0, 2.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="integers >= 0"):
            p.check_targets(np.array([[1.0], [bad]]))
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match=">= 0"):
            e.check_targets(np.array([[1.0], [bad]]))
    for bad in (0.0, -2.0, float("inf")):
        with pytest.raises(ValueError, match="> 0"):
            g.check_targets(np.array([[1.0], [bad]]))
    with pytest.raises(ValueError, match="> 0"):                # the models check at construction, before anything touches a device
        DGP_VI(np.zeros((3, 2)), np.array([[1.0], [0.0], [2.0]]), [], likelihoods.Gamma())
    with pytest.raises(ValueError, match="integers >= 0"):
        DGP_VI(np.zeros((3, 2)), np.array([[1.0], [0.5], [2.0]]), [], likelihoods.Poisson())
    with pytest.raises(_abi.IwviError, match="no CPU fallback"):  # the arithmetic exists as HIP kernels only
        g.logp(torch.zeros(3, 1), torch.ones(3, 1))


def test_checkpoint_keys_of_the_likelihood():
    from dgps_with_iwvi_amd import build_models, likelihoods
    for lik, kind, params, fresh in ((likelihoods.Poisson(binsize=2.5), "Poisson", [2.5], likelihoods.Poisson()),
                                     (likelihoods.Exponential(), "Exponential", [], likelihoods.Exponential()),
                                     (likelihoods.Gamma(shape=0.75), "Gamma", [0.75], likelihoods.Gamma())):
        st = build_models.likelihood_state(lik)
        assert sorted(st) == ["likelihood.params", "likelihood.type"] and str(st["likelihood.type"]) == kind
        assert st["likelihood.params"].dtype == np.float64 and st["likelihood.params"].tolist() == params
        build_models.load_likelihood_state(fresh, st)
        assert build_models.likelihood_state(fresh)["likelihood.params"].tolist() == params
        for other in (likelihoods.Gaussian(0.3), likelihoods.StudentT(), likelihoods.Bernoulli(),
                      *(o for o in (likelihoods.Poisson(), likelihoods.Exponential(), likelihoods.Gamma()) if type(o) is not type(lik))):
            with pytest.raises(ValueError, match="checkpoint holds a %s" % kind):
                build_models.load_likelihood_state(other, st)
    with pytest.raises(ValueError, match="checkpoint holds"):
        build_models.load_likelihood_state(likelihoods.Gamma(), build_models.likelihood_state(likelihoods.StudentT()))

    class MyGamma(likelihoods.Gamma):                            # a subclass keeps its parent's checkpoint type
        pass
    mine = MyGamma()
    build_models.load_likelihood_state(mine, build_models.likelihood_state(MyGamma(shape=4.0)))
    assert mine.shape == 4.0


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


def _desc(_abi, type_, p0=1.0, p1=0.0):
    d = _abi.LikDesc()
    d.type, d.param[0], d.param[1] = type_, p0, p1
    return d


def test_header_names_the_three_types():
    text = open(os.path.join(os.path.dirname(HERE), "include", "iwvi_hip.h")).read()
    for name, value in (("IWVI_LIK_POISSON", 4), ("IWVI_LIK_EXPONENTIAL", 5), ("IWVI_LIK_GAMMA", 6)):
        assert "%s = %d" % (name, value) in text, name
    assert "IWVI_LIK_MULTICLASS = 3" in text and "#define IWVI_ABI_VERSION 19" in text     # additive: nothing moved


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
    every = (lambda d: elem(lib.iwvi_lik_var_exp, d), lambda d: elem(lib.iwvi_lik_predict_density, d), pmv, red, bwd)
    for bad, text in ((_desc(_abi, _abi.LIK_POISSON, p0=0.0), b"binsize"), (_desc(_abi, _abi.LIK_POISSON, p0=-2.0), b"binsize"),
                      (_desc(_abi, _abi.LIK_POISSON, p0=float("nan")), b"binsize"),
                      (_desc(_abi, _abi.LIK_GAMMA, p0=-1.0), b"shape"), (_desc(_abi, _abi.LIK_GAMMA, p0=0.0), b"shape"),
                      (_desc(_abi, 7), b"unknown likelihood type 7"), (_desc(_abi, 100), b"unknown likelihood type"),
                      (_desc(_abi, -1), b"unknown likelihood type")):
        for call in every:
            assert call(bad) == E
            assert text in lib.iwvi_last_error(), (text, lib.iwvi_last_error())
    for type_ in (_abi.LIK_POISSON, _abi.LIK_EXPONENTIAL, _abi.LIK_GAMMA):
        good = _desc(_abi, type_, p0=1.5)
        for fn in (lib.iwvi_lik_var_exp, lib.iwvi_lik_predict_density):
            assert elem(fn, good, out=None) == E                 # NULL outputs
            assert fn(good, p, p, p, 4, 0, 1, 4, p, None) == E   # Dy = 0
            assert fn(good, p, p, None, 4, 1, 1, 4, p, None) == E   # no targets
        assert lib.iwvi_lik_var_exp(good, p, None, p, 4, 1, 1, 4, p, None) == E      # the expectation needs the variance (logp does not)
        assert pmv(good, om=None) == E and pmv(good, ov=None) == E
        assert red(good, logp=None, elbo=None) == E              # nothing asked for
        assert red(good, logp=None) == E and red(good, ticket=None) == E             # out_elbo needs out_logp and a ticket
        assert bwd(good, sums=None) == E and bwd(good, ws=None) == E
        assert lib.iwvi_lik_var_exp(good, p, p, p, 0, 1, 1, 1, p, None) == 0          # T = 0: nothing to do, nothing launched
    # the Exponential has no parameter to refuse
    assert lib.iwvi_lik_var_exp(_desc(_abi, _abi.LIK_EXPONENTIAL, p0=-3.0), p, p, p, 0, 1, 1, 1, p, None) == 0


def test_kernel_resources_lists_the_new_kernels_without_scratch():
    from dgps_with_iwvi_amd import kernel_resources as kr
    if not os.path.exists(kr.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf here")
    rows = kr.check()
    for base, n in (("k_xl_elbo", 5), ("k_xl_elbo_bwd", 1), ("k_xl_elem", 3)):
        mine = [r for r in rows if r["demangled"].split("<")[0] == base]
        assert len(mine) == n, (base, [r["demangled"] for r in mine])
        for r in mine:
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
        # the budget: a multiple of 8, at most 128 (four waves per SIMD), that every instantiation fits
        most = max(r["vgpr_count"] for r in mine)
        assert most <= kr.MAX_VGPRS[base] <= 128 and kr.MAX_VGPRS[base] % 8 == 0, (base, most, kr.MAX_VGPRS[base])
