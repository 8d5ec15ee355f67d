"""Host-side checks of the Bernoulli / Student-t likelihoods: the C-ABI additions (exported, prototyped, refusing bad arguments without a
device), the Python surface that needs no GPU, and the pinning of the float64 restatement (tests/lik_restatement.py) the GPU tests
compare the kernels with."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import lik_restatement as R   # noqa: E402

NEW = ("iwvi_lik_elbo_reduce", "iwvi_lik_elbo_backward", "iwvi_lik_var_exp", "iwvi_lik_predict_density", "iwvi_lik_predict_mean_and_var")


def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


def _header():
    return open(os.path.join(os.path.dirname(HERE), "include", "iwvi_hip.h")).read()


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_exported_and_prototyped_completely(name):
    _abi, lib = _lib()
    assert hasattr(lib, name)
    decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, _header())
    assert decl, name
    nargs = len([a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"])
    assert len(_abi.PROTOTYPES[name][1]) == nargs
    assert lib.iwvi_version() == _abi.ABI_VERSION == 19          # additive: the number did not move
    assert "#define IWVI_ABI_VERSION 19" in _header()


def test_descriptor_layout_matches_the_header():
    _abi, _ = _lib()
    d = _abi.LikDesc
    assert [f[0] for f in d._fields_] == ["type", "param", "lgc", "param0_dev"]
    assert (d.type.offset, d.param.offset, d.lgc.offset, d.param0_dev.offset, ctypes.sizeof(d)) == (0, 4, 12, 16, 24)
    assert (_abi.LIK_GAUSSIAN, _abi.LIK_BERNOULLI_PROBIT, _abi.LIK_STUDENT_T) == (0, 1, 2)


def _desc(_abi, type_, p0=1.0, p1=3.0):
    d = _abi.LikDesc()
    d.type, d.param[0], d.param[1] = type_, p0, p1
    return d


def test_refused_arguments_return_before_any_launch():
    _abi, lib = _lib()
    p = ctypes.c_void_p(16)                                      # never dereferenced: every call below is refused on its arguments
    E = _abi.ERR_ARG
    elem = lambda fn, d, out=p: fn(d, p, p, p, 4, 1, 1, 4, out, None)
    pmv = lambda d, om=p, ov=p: lib.iwvi_lik_predict_mean_and_var(d, p, p, 4, om, ov, None)
    red = lambda d, logp=p, elbo=p, ticket=p: lib.iwvi_lik_elbo_reduce(d, p, p, p, 4, 2, 1, 2, 1, None, None, 0, None, None, 0, 1.0, 2, 0,
                                                                       None, logp, elbo, ticket, None)
    bwd = lambda d, sums=p, ws=p: lib.iwvi_lik_elbo_backward(d, p, p, p, 1, None, None, 0, 4, 2, 1.0, 0, p, p, p, None, None, 0, None, 2,
                                                             sums, ws, None)
    for bad in (_desc(_abi, 3), _desc(_abi, -1), _desc(_abi, _abi.LIK_STUDENT_T, p0=0.0), _desc(_abi, _abi.LIK_STUDENT_T, p0=-1.0),
                _desc(_abi, _abi.LIK_STUDENT_T, p1=0.0), _desc(_abi, _abi.LIK_GAUSSIAN, p0=0.0)):
        assert elem(lib.iwvi_lik_var_exp, bad) == E
        assert elem(lib.iwvi_lik_predict_density, bad) == E
        assert pmv(bad) == E
        assert red(bad) == E
        assert bwd(bad) == E
    assert b"unknown likelihood type" in (elem(lib.iwvi_lik_var_exp, _desc(_abi, 3)), lib.iwvi_last_error())[1]
    good = _desc(_abi, _abi.LIK_STUDENT_T)
    assert pmv(_desc(_abi, _abi.LIK_STUDENT_T, p1=2.0)) == E     # the variance of a Student-t needs df > 2 ...
    assert b"df > 2" in lib.iwvi_last_error()
    assert pmv(_desc(_abi, _abi.LIK_STUDENT_T, p1=1.5)) == E
    for fn in (lib.iwvi_lik_var_exp, lib.iwvi_lik_predict_density):
        assert elem(fn, good, out=None) == E                     # NULL outputs
        assert fn(None, p, p, p, 4, 1, 1, 4, p, None) == E       # NULL descriptor
        assert fn(good, p, p, p, 4, 0, 1, 4, p, None) == E       # Dy = 0
    assert lib.iwvi_lik_var_exp(good, p, None, p, 4, 1, 1, 4, p, None) == E      # the expectation needs the variance (logp does not)
    assert pmv(good, om=None) == E and pmv(good, ov=None) == E
    assert red(good, logp=None, elbo=None) == E                  # nothing asked for
    assert red(good, logp=None) == E and red(good, ticket=None) == E             # out_elbo needs out_logp and a ticket
    assert bwd(good, sums=None) == E and bwd(good, ws=None) == E
    bern = _desc(_abi, _abi.LIK_BERNOULLI_PROBIT, p0=0.0, p1=0.0)                # no parameter to validate
    assert lib.iwvi_lik_var_exp(bern, p, p, p, 0, 1, 1, 1, p, None) == 0          # T = 0: nothing to do, nothing launched


def test_python_surface_without_a_device():
    import dgps_with_iwvi.likelihoods as alias
    from dgps_with_iwvi_amd import _abi, likelihoods
    assert alias.Bernoulli is likelihoods.Bernoulli and alias.StudentT is likelihoods.StudentT and alias.Gaussian is likelihoods.Gaussian
    for cls in (likelihoods.Bernoulli, likelihoods.StudentT, likelihoods.Gaussian):
        for meth in ("logp", "variational_expectations", "predict_mean_and_var", "predict_density", "lik_desc"):
            assert callable(getattr(cls, meth)), (cls, meth)
    with pytest.raises(NotImplementedError, match="logit"):
        likelihoods.Bernoulli(invlink="logit")
    likelihoods.Bernoulli(invlink=likelihoods.inv_probit)
    assert likelihoods.Bernoulli().lik_desc().type == _abi.LIK_BERNOULLI_PROBIT and likelihoods.Bernoulli().trained_scalar() is None
    t = likelihoods.StudentT(scale=0.5, df=4.0)
    d = t.lik_desc()
    assert (d.type, d.param[0], d.param[1], d.param0_dev) == (_abi.LIK_STUDENT_T, 0.5, 4.0, None)
    from math import lgamma
    assert abs(d.lgc - (lgamma(2.5) - lgamma(2.0))) < 1e-7
    assert t.trained_scalar() == ("lik_scale", 0.5) and (t.scale, t.df) == (0.5, 4.0)
    with pytest.raises(AttributeError):
        t.variance
    with pytest.raises(ValueError):
        likelihoods.StudentT(scale=0.0)
    with pytest.raises(ValueError, match="df > 2"):
        likelihoods.StudentT(df=2.0).predict_mean_and_var(torch.zeros(1), torch.ones(1))
    likelihoods.Bernoulli().check_targets(np.array([[0.0], [1.0], [1.0]]))
    for bad in ([[0.0], [0.999]], [[-1.0], [1.0]], [[2.0]], [[float("nan")]]):
        with pytest.raises(ValueError, match="0 or 1"):
            likelihoods.Bernoulli().check_targets(np.array(bad))
    from dgps_with_iwvi_amd.models import DGP_VI
    with pytest.raises(ValueError, match="0 or 1"):            # the models check at construction, before anything touches a device
        DGP_VI(np.zeros((3, 2)), np.array([[0.0], [1.0], [-1.0]]), [], likelihoods.Bernoulli())

    class MyStudentT(likelihoods.StudentT):                      # a subclass keeps its parent's checkpoint type
        pass
    from dgps_with_iwvi_amd import build_models
    st = build_models.likelihood_state(MyStudentT(0.5, 4.0))
    mine = MyStudentT()
    build_models.load_likelihood_state(mine, st)
    assert (mine.scale, mine.df) == (0.5, 4.0)
    g = likelihoods.Gaussian(0.25)
    assert (g.lik_desc().type, g.lik_desc().param[0], g.variance, g.trained_scalar()) == (_abi.LIK_GAUSSIAN, 0.25, 0.25, ("lik_var", 0.25))
    assert likelihoods.is_gaussian(g) and not likelihoods.is_gaussian(t)
    with pytest.raises(_abi.IwviError, match="no CPU fallback"):  # the arithmetic exists as HIP kernels only
        t.logp(torch.zeros(3, 1), torch.zeros(3, 1))


def test_checkpoint_keys_of_the_likelihood():
    from dgps_with_iwvi_amd import build_models, likelihoods
    t = likelihoods.StudentT(scale=0.5, df=4.0)
    st = build_models.likelihood_state(t)
    assert sorted(st) == ["likelihood.params", "likelihood.type"] and str(st["likelihood.type"]) == "StudentT"
    t2 = likelihoods.StudentT()
    build_models.load_likelihood_state(t2, st)
    assert (t2.scale, t2.df) == (0.5, 4.0)
    assert str(build_models.likelihood_state(likelihoods.Bernoulli())["likelihood.type"]) == "Bernoulli"
    build_models.load_likelihood_state(likelihoods.Bernoulli(), build_models.likelihood_state(likelihoods.Bernoulli()))
    g = likelihoods.Gaussian(0.3)
    assert list(build_models.likelihood_state(g)) == ["likelihood.variance"]     # a Gaussian is stored as ever
    g2 = likelihoods.Gaussian(1.0)
    build_models.load_likelihood_state(g2, {"likelihood.variance": np.float64(0.3)})   # ... and a file from before still loads
    assert g2.variance == 0.3
    with pytest.raises(ValueError, match="checkpoint holds"):
        build_models.load_likelihood_state(g2, st)


# ---- the float64 restatement is itself pinned ----------------------------------------------------------------------------------
def test_restatement_logp_matches_scipy():
    from scipy import stats
    f = np.linspace(-6.0, 6.0, 97)
    for y in (-2.5, 0.4, 3.0):
        for scale, df in ((1.0, 3.0), (0.7, 4.0), (2.0, 2.5)):
            got = R.StudentT(scale, df).logp(f, np.full_like(f, y)).numpy()
            np.testing.assert_allclose(got, stats.t(df, loc=f, scale=scale).logpdf(y), rtol=1e-12, atol=0)
    p = R.inv_probit(f).numpy()
    np.testing.assert_allclose(p, stats.norm.cdf(f) * (1 - 2e-3) + 1e-3, rtol=1e-12, atol=0)
    for y in (0.0, 1.0):
        got = R.Bernoulli().logp(f, np.full_like(f, y)).numpy()
        np.testing.assert_allclose(got, stats.bernoulli.logpmf(int(y), p), rtol=1e-12, atol=0)


def _gap(lik, ys):
    from scipy import integrate
    MU, V = R.moment_grid()
    worst = 0.0
    for y in ys:
        ve = lik.variational_expectations(MU, V, np.full_like(MU, y)).numpy()
        yt = torch.tensor(y, dtype=torch.float64)
        for i, (m, v) in enumerate(zip(MU, V)):
            sd = np.sqrt(v)
            f = lambda x: float(lik.logp(torch.tensor(x, dtype=torch.float64), yt)) * np.exp(-0.5 * ((x - m) / sd) ** 2) / (sd * np.sqrt(2 * np.pi))
            ref, _ = integrate.quad(f, m - 12 * sd, m + 12 * sd, epsabs=1e-13, epsrel=1e-13, limit=200, points=[m])
            worst = max(worst, abs(ve[i] - ref))
    return worst


def test_restatement_var_exp_against_the_integral():
    """The 20-point rule against scipy.integrate.quad of the same integrand on mu in [-3, 3] x v in [1e-4, 4] (25 x 24 points).  The gap is
    a property of the rule (GPflow's default, which defines the result), not of any code here.  MEASURED maximum absolute gap:
    Bernoulli (y in {0, 1}) 1.0115e-2 -- at v = 4, where the jittered probit's log flattens at log 1e-3 inside the nodes' span --,
    Student-t (scale 1, df 3; y in {-1.5, 0.3, 2.5}) 6.964e-4.  Asserted at twice the measured values."""
    gb = _gap(R.Bernoulli(), (0.0, 1.0))
    gt = _gap(R.StudentT(1.0, 3.0), (-1.5, 0.3, 2.5))
    print("rule vs integral: Bernoulli %.4e, Student-t %.4e" % (gb, gt))
    assert gb <= 2 * 1.0115e-2, gb
    assert gt <= 2 * 6.964e-4, gt
    assert gb > 1e-6 and gt > 1e-6                               # (a rule that matched the integral exactly would not be the 20-point rule)


def test_restatement_bound_reduces_to_the_oracle_for_a_quadratic():
    """The 20-point rule integrates the Gaussian log-density (a quadratic) exactly: with a Gaussian 'likelihood' in its place the
    restatement's bound is the oracle's own -- the moment recording and the swap of the expectation are right."""
    import math
    from dgps_with_iwvi_amd import synthetic
    from oracle.ref_torch_cpu import CpuDGP

    class G:
        def variational_expectations(self, Fmu, Fvar, Y):
            return R.quad(lambda f: -0.5 * math.log(2 * math.pi * 0.01) - 0.5 * (Y[..., None] - f) ** 2 / 0.01, Fmu, Fvar)

    spec = synthetic.make_spec(L=2, M=16, B=6, K=3, with_lv=True, seed=5)
    zs = synthetic.make_noise(spec, seed=6)
    for mode_vi in (False, True):
        ref = float(CpuDGP(spec).elbo_tensor(zs, mode_vi=mode_vi))
        got = float(R.LikDGP(spec, G()).elbo_tensor(zs, mode_vi=mode_vi))
        assert abs(got - ref) <= 1e-10 * abs(ref), (mode_vi, got, ref)
