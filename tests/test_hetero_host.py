"""The heteroskedastic Gaussian likelihood without a GPU: the float64 restatement (tests/hetero_restatement.py) against brute-force Monte
Carlo, central differences and a fine quadrature; the clip; the float32 restatement of the kernels' formulas within a third of the GPU
tests' constants; the class surface, the checkpoint round trip, ``target_dim`` / ``output_dim``; and the refusals of the built library."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import hetero_restatement as H   # noqa: E402

LIK = H.HeteroskedasticGaussian()


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------------
def test_variational_expectation_and_density_against_monte_carlo():
    """E logp and log E p over 4e6 joint draws of (f, g), two target columns with different moments: within 5 standard errors."""
    rng = np.random.default_rng(5)
    Fmu, Fvar, Y = np.array([[0.4, -1.0, -0.8, 0.3]]), np.array([[0.3, 0.05, 0.5, 0.2]]), np.array([[1.0, -1.4]])
    n = 4_000_000
    F = Fmu + np.sqrt(Fvar) * rng.standard_normal((n, 4))
    lp = LIK.logp(F, Y).numpy()
    ve = LIK.variational_expectations(Fmu, Fvar, Y).numpy()[0]
    se = lp.std(0) / math.sqrt(n)
    assert np.all(np.abs(lp.mean(0) - ve) <= 5 * se), (lp.mean(0), ve, se)
    # the predictive density: f integrated out in closed form, g by Monte Carlo
    g = F[:, 2:]
    s = Fvar[:, :2] + np.exp(g)
    p = np.exp(-0.5 * (Y - Fmu[:, :2]) ** 2 / s) / np.sqrt(2 * np.pi * s)
    want, got = np.log(p.mean(0)), LIK.predict_density(Fmu, Fvar, Y).numpy()[0]
    se = p.std(0) / math.sqrt(n) / p.mean(0)
    assert np.all(np.abs(got - want) <= 5 * se + 1e-6), (got, want, se)
    # the predictive moments: the law of total variance on the same draws
    m, v = (a.numpy()[0] for a in LIK.predict_mean_and_var(Fmu, Fvar))
    assert np.array_equal(m, Fmu[0, :2])
    ev = np.exp(g)
    assert np.all(np.abs(ev.mean(0) + Fvar[0, :2] - v) <= 5 * ev.std(0) / math.sqrt(n))


def test_heads_against_central_differences():
    Fmu, Fvar, Y = (a[:400] for a in H.cases(3))
    dm, dv = (a.numpy() for a in LIK.heads(Fmu, Fvar, Y))
    E = lambda m, v: LIK.variational_expectations(m, v, Y).numpy()
    h = 1e-6
    for j in range(6):
        step = np.zeros(6)
        step[j] = h
        d = j % 3
        fd_m = (E(Fmu + step, Fvar) - E(Fmu - step, Fvar))[:, d] / (2 * h)
        fd_v = (E(Fmu, Fvar + step) - E(Fmu, Fvar - step))[:, d] / (2 * h)
        np.testing.assert_allclose(dm[:, j], fd_m, rtol=1e-6, atol=1e-6 * (1 + np.abs(dm[:, j]).max()))
        np.testing.assert_allclose(dv[:, j], fd_v, rtol=1e-6, atol=1e-6 * (1 + np.abs(dv[:, j]).max()))
    # ... and autograd through the clamp gives the same, at and beyond the clip too
    Fmu, Fvar, Y = H.cases(2)
    mu, var = (torch.tensor(a, requires_grad=True) for a in (Fmu, Fvar))
    gm, gv = torch.autograd.grad(LIK.variational_expectations(mu, var, Y).sum(), (mu, var))
    dm, dv = LIK.heads(Fmu, Fvar, Y)
    np.testing.assert_allclose(gm.numpy(), dm.numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(gv.numpy(), dv.numpy(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_the_clip_in_value_and_heads(sign):
    """a = -m_g + v_g/2 at +-60, just inside and just outside: the value uses exp(+-60) from the clip on, the m_g / v_g heads through r
    vanish beyond it (dE/dm_g = -1/2, dE/dv_g = 0) and pass at the end itself; the m_f / v_f heads keep the clipped r."""
    y, mf, vf = 0.9, 0.2, 0.3
    q = (y - mf) ** 2 + vf
    for a, active in ((60.0, False), (59.99, False), (60.01, True), (75.0, True)):
        Fmu, Fvar = np.array([[mf, -sign * a]]), np.array([[vf, 0.0]])
        r = math.exp(sign * min(a, 60.0))
        ve = float(LIK.variational_expectations(Fmu, Fvar, [[y]]))
        assert ve == pytest.approx(-H.HL2P + 0.5 * sign * a - 0.5 * q * r, rel=1e-14)
        dm, dv = (t.numpy()[0] for t in LIK.heads(Fmu, Fvar, [[y]]))
        assert dm[0] == pytest.approx((y - mf) * r, rel=1e-14) and dv[0] == pytest.approx(-0.5 * r, rel=1e-14)
        if active:
            assert dm[1] == -0.5 and dv[1] == 0.0
        else:
            assert dm[1] == pytest.approx(-0.5 + 0.5 * q * r, rel=1e-14) and dv[1] == pytest.approx(-0.25 * q * r, rel=1e-14)
    # float32 cannot overflow: the largest value any exponent can take
    assert np.isfinite(np.float32(math.exp(60.0)) * np.float32(1e12))
    # logp, predict_mean_and_var and sample_y clip their exponents too
    assert float(LIK.logp([[0.0, -sign * 100.0]], [[1.0]])) == pytest.approx(-H.HL2P + 50.0 * sign - 0.5 * math.exp(sign * 60.0), rel=1e-14)
    assert float(LIK.predict_mean_and_var([[0.0, sign * 100.0]], [[0.0, 0.0]])[1]) == pytest.approx(math.exp(sign * 60.0), rel=1e-14)
    assert float(LIK.sample_y([[0.0, sign * 200.0]], [[0.0, 0.0]], [[0.0, 0.0]], [[1.0]])[0]) == pytest.approx(math.exp(sign * 60.0), rel=1e-14)


def test_the_twenty_point_rule_is_adequate_on_the_tests_inputs():
    """The density rows of ``cases``: the 20-point rule within 1e-2 nats of the 200-point rule (6.8e-3 at v_g = 3.99, the largest variance of
    the rows); the rows left out of the density checks are the ones it cannot reach.  With v_g -> 0 the density is the Gaussian's."""
    worst, where = H.rule_error()
    print("20-point against 200-point rule: worst %.3e nats at (m_f, v_f, m_g, v_g, y) = %s" % (worst, tuple(float(x) for x in where)))
    assert worst <= 1e-2
    Fmu, Fvar, Y = H.cases(1)
    far = (LIK.predict_density(Fmu, Fvar, Y, 20) - LIK.predict_density(Fmu, Fvar, Y, 200)).abs().numpy()[-H.N_BEYOND_RULE:]
    assert far.min() > 100.0
    s = 0.4 + math.exp(-0.7)
    want = -0.5 * math.log(2 * math.pi * s) - 0.5 * 0.8 ** 2 / s
    assert float(LIK.predict_density([[0.3, -0.7]], [[0.4, 0.0]], [[1.1]])) == pytest.approx(want, abs=1e-7)   # (the floor 1e-8 moves it by < 1e-8)


def test_the_float32_restatement_stays_within_a_third_of_the_gpu_constants():
    """What the GPU tests allow -- 8 x 2^-24 S for the closed forms (tests/test_gpu_explink.py's constant), 16 x 2^-24 S for the log-space
    quadrature (tests/test_gpu_bounded.py's) -- is three times what a plain float32 evaluation of the kernels' formulas reaches on the very
    same inputs: measured 2.11 / 2.18 / 2.25 / 2.55 / 2.15 (var_exp, logp, predictive variance, d_mean, d_var) and 1.50 (density)."""
    worst = H.measure_float32()
    print("float32 restatement, worst multiples of 2^-24 S: " + "  ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    for name, w in worst.items():
        assert 3.0 * w <= (H.C_QUAD if name == "predict_density" else H.C_CLOSED), (name, w)


def test_mixture_of_one_draw_is_the_elementwise_result():
    Fmu, Fvar, Y = (a[:50] for a in H.cases(2))
    out = H.mixture(LIK, Fmu[None], Fvar[None], Y)
    m, v = LIK.predict_mean_and_var(Fmu, Fvar)
    np.testing.assert_allclose(out["mean"], m.numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(out["var"], v.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out["log_density"], LIK.predict_density(Fmu, Fvar, Y).sum(-1).numpy(), rtol=1e-13)


# ---- the class surface -----------------------------------------------------------------------------------------------------------------------
def test_class_surface_alias_and_descriptor():
    from dgps_with_iwvi_amd import _abi, likelihoods
    import dgps_with_iwvi.likelihoods as alias
    assert alias.HeteroskedasticGaussian is likelihoods.HeteroskedasticGaussian
    lik = likelihoods.HeteroskedasticGaussian()
    d = lik.lik_desc()
    assert (d.type, d.param[0], d.param[1], d.param0_dev) == (11, 0.0, 0.0, None) and _abi.LIK_HETERO_GAUSSIAN == 11
    assert lik.grad_name is None and lik.trained_scalar() is None and lik.outputs_per_target == 2
    assert not likelihoods.is_gaussian(lik) and hasattr(lik, "sample_y")
    for bad in (1, 3, 0, -2, None, _abi.MAX_P + 2):
        with pytest.raises(ValueError, match="even"):
            lik.check_output_dim(bad)
    for good in (2, 4, _abi.MAX_P):
        lik.check_output_dim(good)
    lik.check_targets(np.array([[-3.5], [0.0], [1e6]]))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            lik.check_targets(np.array([[0.0], [bad]]))


def test_target_and_output_widths_for_every_likelihood():
    from dgps_with_iwvi_amd import likelihoods as L
    het = L.HeteroskedasticGaussian()
    assert L.target_dim(het, 2) == 1 and L.target_dim(het, 6) == 3 and L.output_dim(het, 1) == 2 and L.output_dim(het, 3) == 6
    assert L.predictive_dim(het, 6) == 3
    mc = L.MultiClass(5)
    assert L.target_dim(mc, 5) == 1 and L.output_dim(mc, 1) == 5 and L.predictive_dim(mc, 5) == 5
    for other in (L.Gaussian(0.1), L.Bernoulli(), L.StudentT(), L.Poisson(), L.Exponential(), L.Gamma(), L.Beta(), L.Ordinal([0.0, 1.0]), None):
        for w in (1, 3):
            assert L.target_dim(other, w) == w and L.output_dim(other, w) == w and L.predictive_dim(other, w) == w
    assert L.target_dim(het, None) is None


def test_models_refuse_a_wrong_final_layer_or_targets_on_the_host():
    from dgps_with_iwvi_amd import likelihoods, synthetic
    dev = torch.device("cpu")
    spec = synthetic.make_spec(L=1, M=8, B=6, K=2, Dx=2, Dy=3)
    with pytest.raises(ValueError, match="even"):
        synthetic.build_model(dict(spec, Y=spec["Y"][:, :1]), dev, likelihood=likelihoods.HeteroskedasticGaussian())
    hs = synthetic.make_hetero_spec(L=1, M=8, B=6, K=2, Dx=2)
    assert hs["Y"].shape == (8, 1) and hs["layers"][-1]["q_mu"].shape[1] == 2
    bad = hs["Y"].copy()
    bad[2, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        synthetic.build_model(dict(hs, Y=bad), dev, likelihood=likelihoods.HeteroskedasticGaussian())
    lv = synthetic.make_hetero_spec(L=2, M=8, B=6, K=2, Dx=3, with_lv=True)
    assert lv["layers"][0]["dims"][0] == 4 and lv["layers"][0]["enc_W"][0].shape[0] == 4
    sd = synthetic.hetero_noise_sd(np.array([[-5.0, 0.0], [0.0, 9.0], [5.0, 0.0]]))
    assert sd[0] < sd[1] < sd[2] and abs(sd[1] - 0.35) < 1e-12


def test_checkpoint_round_trip_and_its_refusals():
    from dgps_with_iwvi_amd import build_models, likelihoods
    lik = likelihoods.HeteroskedasticGaussian()
    st = build_models.likelihood_state(lik)
    assert str(st["likelihood.type"]) == "HeteroskedasticGaussian" and st["likelihood.params"].size == 0
    build_models.load_likelihood_state(likelihoods.HeteroskedasticGaussian(), st)
    with pytest.raises(ValueError, match="HeteroskedasticGaussian"):
        build_models.load_likelihood_state(likelihoods.Gaussian(0.1), st)
    with pytest.raises(ValueError, match="HeteroskedasticGaussian"):
        build_models.load_likelihood_state(lik, build_models.likelihood_state(likelihoods.Gaussian(0.1)))
    with pytest.raises(ValueError, match="HeteroskedasticGaussian"):
        build_models.load_likelihood_state(lik, build_models.likelihood_state(likelihoods.Exponential()))


# ---- the C-ABI on a host without a GPU ---------------------------------------------------------------------------------------------------------
def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


def _desc(_abi, type_, p0=0.0, p1=0.0):
    d = _abi.LikDesc()
    d.type, d.param[0], d.param[1] = type_, p0, p1
    return d


def test_header_names_type_11_and_nothing_moved():
    text = open(os.path.join(os.path.dirname(HERE), "include", "iwvi_hip.h")).read()
    assert "IWVI_LIK_HETERO_GAUSSIAN = 11" in text and "#define IWVI_ABI_VERSION 19" in text
    enum = text[text.index("enum { IWVI_LIK_GAUSSIAN"):text.index("typedef struct iwvi_lik_desc")]
    assert " = 7" not in enum and " = 10" not in enum and "IWVI_LIK_ORDINAL = 9" in enum


def test_type_11_is_accepted_where_7_and_10_are_refused_and_its_arguments_are_checked():
    _abi, lib = _lib()
    assert lib.iwvi_version() == _abi.ABI_VERSION == 19
    p = ctypes.c_void_p(16)                                      # never dereferenced: every call below is refused on its arguments or has nothing to do
    E = _abi.ERR_ARG
    elem = lambda fn, d, Dy=2, out=p, Y=p, T=4: fn(d, p, p, Y, T, Dy, 1, 4, out, None)
    pmv = lambda d, n=8, om=p, ov=p: lib.iwvi_lik_predict_mean_and_var(d, p, p, n, om, ov, None)
    red = lambda d, Dy=2, logp=p, elbo=p, ticket=p: lib.iwvi_lik_elbo_reduce(d, p, p, p, 4, 2, Dy, 2, 1, None, None, 0, None, None, 0, 1.0, 2, 0,
                                                                             None, logp, elbo, ticket, None)
    bwd = lambda d, Dy=2, sums=p, ws=p: lib.iwvi_lik_elbo_backward(d, p, p, p, Dy, None, None, 0, 4, 2, 1.0, 0, p, p, p, None, None, 0, None, 2,
                                                                   sums, ws, None)
    mix = lambda d, Dy=2, N=4, Y=p, lp=p, m=p, v=p: lib.iwvi_lik_predict_mixture(d, p, p, Y, N, 3, Dy, 3, 1, lp, m, v, None)
    smp = lambda d, Dy=2, T=4, out=p: lib.iwvi_lik_sample_y(d, p, p, T, Dy, None, 1, 2, None, out, None, None)
    for t in (7, 10, 12):
        for call in (lambda d: elem(lib.iwvi_lik_var_exp, d), lambda d: elem(lib.iwvi_lik_predict_density, d), pmv, red, bwd, mix, smp):
            assert call(_desc(_abi, t)) == E
            assert b"unknown likelihood type %d" % t in lib.iwvi_last_error()
    # param[] is ignored: whatever it holds, the descriptor is taken (T = 0 / N = 0: accepted, nothing to do, nothing launched)
    for d in (_desc(_abi, 11), _desc(_abi, 11, p0=-3.0, p1=float("nan"))):
        assert elem(lib.iwvi_lik_var_exp, d, T=0) == 0 and elem(lib.iwvi_lik_predict_density, d, T=0) == 0
        assert mix(d, N=0) == 0 and smp(d, T=0) == 0
    assert pmv(_desc(_abi, 11, p1=4.0), n=0) == 0
    d = _desc(_abi, 11)
    limit = b"2..%d" % _abi.MAX_P
    for Dy in (1, 3, 0, -2, _abi.MAX_P + 1, _abi.MAX_P + 2):   # odd, non-positive, beyond the limit -- with the limit in the text
        for call in (lambda: elem(lib.iwvi_lik_var_exp, d, Dy), lambda: elem(lib.iwvi_lik_predict_density, d, Dy), lambda: red(d, Dy),
                     lambda: bwd(d, Dy), lambda: mix(d, Dy), lambda: smp(d, Dy)):
            assert call() == E
            assert b"heteroskedastic" in lib.iwvi_last_error() and limit in lib.iwvi_last_error(), (Dy, lib.iwvi_last_error())
    # predict_mean_and_var has no Dy argument: the row width travels in param[1], n must be a multiple of it
    for w in (0.0, 3.0, 2.5, float(_abi.MAX_P + 2)):
        assert pmv(_desc(_abi, 11, p1=w)) == E and limit in lib.iwvi_last_error()
    assert pmv(_desc(_abi, 11, p1=6.0), n=8) == E and b"T x 6" in lib.iwvi_last_error()
    good = _desc(_abi, 11, p1=2.0)
    for fn in (lib.iwvi_lik_var_exp, lib.iwvi_lik_predict_density):
        assert elem(fn, good, out=None) == E                     # NULL outputs
        assert elem(fn, good, Y=None) == E                       # no targets
    assert lib.iwvi_lik_var_exp(good, p, None, p, 4, 2, 1, 4, p, None) == E          # the expectation needs the variance (logp does not)
    assert pmv(good, om=None) == E and pmv(good, ov=None) == E
    assert red(good, logp=None, elbo=None) == E                  # nothing asked for
    assert red(good, logp=None) == E and red(good, ticket=None) == E
    assert bwd(good, sums=None) == E and bwd(good, ws=None) == E
    assert mix(good, Y=None) == E and mix(good, lp=None, m=None, v=None, Y=None) == E and mix(good, m=None) == E
    assert smp(good, out=None) == E


def test_kernel_resources_lists_the_new_kernels_without_scratch():
    from dgps_with_iwvi_amd import kernel_resources as kr
    if not os.path.exists(kr.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf here")
    rows = kr.check()
    for base, n in (("k_hg_elbo", 5), ("k_hg_elbo_bwd", 1), ("k_hg_elem", 3), ("k_hg_mix", 5)):
        mine = [r for r in rows if r["demangled"].split("<")[0] == base]
        assert len(mine) == n, (base, [r["demangled"] for r in mine])
        for r in mine:
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
        most = max(r["vgpr_count"] for r in mine)
        assert base in kr.NO_SCRATCH and kr.MAX_VGPRS[base] % 8 == 0 and most <= kr.MAX_VGPRS[base] <= 128
        assert kr.MAX_VGPRS[base] - most < 8, (base, most, kr.MAX_VGPRS[base])
    assert any(r["demangled"] == "k_lik_sample<11>" for r in rows)
