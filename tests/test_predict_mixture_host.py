"""iwvi_lik_predict_mixture on a GPU-less host: the symbol, its refusals (before any launch, with null device pointers), the float64
restatement tests/mixture_restatement.py pinned against a brute-force evaluation, and the register budget of the new kernels."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import mixture_restatement as MX   # noqa: E402


def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


def _desc(_abi, type_, p0=0.0, p1=0.0):
    d = _abi.LikDesc()
    d.type, d.param[0], d.param[1] = type_, p0, p1
    return d


def test_header_declares_the_symbol_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "iwvi_hip.h")).read()
    assert re.search(r"\bint\s+iwvi_lik_predict_mixture\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert re.search(r"#define\s+IWVI_ABI_VERSION\s+19\b", text)
    _abi, lib = _lib()
    assert hasattr(lib, "iwvi_lik_predict_mixture") and "iwvi_lik_predict_mixture" in _abi.PROTOTYPES
    assert lib.iwvi_version() == 19 == _abi.ABI_VERSION


def test_bad_arguments_are_refused_before_any_launch():
    """Every refusal of the header's list: IWVI_ERR_ARG and a text, with null (or never dereferenced) device pointers, on a GPU-less host."""
    _abi, lib = _lib()
    f = lib.iwvi_lik_predict_mixture
    P = ctypes.c_void_p(64)                                      # "given": refused before anything could read it
    bern = _desc(_abi, _abi.LIK_BERNOULLI_PROBIT)
    mc4 = _desc(_abi, _abi.LIK_MULTICLASS, 1e-3, 4.0)

    def refused(*args):
        assert f(*args) == _abi.ERR_ARG, args
        text = lib.iwvi_last_error()
        assert b"iwvi_lik_predict_mixture" in text, text
        return text

    # (lik, fmean, fvar, Y, N, S, Dy, stride_n, stride_s, out_logp, out_mean, out_var, stream)
    assert b"null likelihood" in refused(None, P, P, P, 4, 3, 1, 3, 1, P, P, P, None)
    refused(ctypes.byref(bern), P, P, P, -1, 3, 1, 3, 1, P, P, P, None)                       # N < 0
    refused(ctypes.byref(bern), P, P, P, 4, 0, 1, 3, 1, P, P, P, None)                        # S < 1
    refused(ctypes.byref(bern), P, P, P, 4, 3, 0, 3, 1, P, P, P, None)                        # Dy < 1
    refused(ctypes.byref(bern), P, P, P, 4, 3, _abi.MAX_P + 1, 3, 1, P, P, P, None)           # Dy > IWVI_MAX_P
    assert b"MultiClass" in refused(ctypes.byref(mc4), P, P, P, 4, 3, 3, 3, 1, P, P, P, None)   # Dy != C
    refused(ctypes.byref(bern), P, P, None, 4, 3, 1, 3, 1, P, P, P, None)                     # out_logp without Y
    refused(ctypes.byref(bern), P, P, P, 4, 3, 1, 3, 1, None, P, P, None)                     # Y without out_logp
    assert b"no output" in refused(ctypes.byref(bern), P, P, None, 4, 3, 1, 3, 1, None, None, None, None)
    refused(ctypes.byref(bern), P, P, None, 4, 3, 1, 3, 1, None, P, None, None)               # out_mean without out_var
    refused(ctypes.byref(bern), P, P, None, 4, 3, 1, 3, 1, None, None, P, None)
    refused(ctypes.byref(_desc(_abi, 17)), P, P, P, 4, 3, 1, 3, 1, P, P, P, None)             # unknown type
    # a Student-t with df <= 2 is refused when the moments are asked for -- and only then: with out_logp alone the call gets past the
    # descriptor (here to the next refusal, S < 1, so that nothing is launched)
    st2 = _desc(_abi, _abi.LIK_STUDENT_T, 1.0, 2.0)
    assert b"df > 2" in refused(ctypes.byref(st2), P, P, P, 4, 3, 1, 3, 1, P, P, P, None)
    assert b"S = 0" in refused(ctypes.byref(st2), P, P, P, 4, 0, 1, 3, 1, P, None, None, None)
    # N = 0: nothing to do, nothing launched, every type
    for d in (bern, mc4, _desc(_abi, _abi.LIK_GAUSSIAN, 0.3), _desc(_abi, _abi.LIK_POISSON, 1.0)):
        assert f(ctypes.byref(d), None, None, None, 0, 3, 4 if d is mc4 else 1, 3, 1, None, None, None, None) == _abi.ERR_ARG   # still: no output
        assert f(ctypes.byref(d), None, None, P, 0, 3, 4 if d is mc4 else 1, 3, 1, P, P, P, None) == 0


def test_restatement_matches_a_brute_force_quadrature_mixture():
    """Student-t (a quadrature type): SciPy's logsumexp over the draws of a log density that is itself a logsumexp over an explicit
    20-point hermgauss rule, and the moments by explicit sums over the same rule -- nothing of lik_restatement.quad is used."""
    from scipy.special import gammaln, logsumexp
    rng = np.random.default_rng(5)
    S, N, Dy, s, nu = 7, 5, 2, 0.7, 4.0
    m, v = rng.uniform(-3, 3, (S, N, Dy)), np.exp(rng.uniform(np.log(1e-4), np.log(4.0), (S, N, Dy)))
    Y = rng.uniform(-2, 2, (N, Dy))
    x, w = np.polynomial.hermite.hermgauss(20)
    w = w / math.sqrt(math.pi)
    f = m[..., None] + np.sqrt(2.0 * v)[..., None] * x                                       # [S, N, Dy, 20]
    logp = (gammaln(0.5 * (nu + 1)) - gammaln(0.5 * nu) - 0.5 * math.log(nu * math.pi) - math.log(s)
            - 0.5 * (nu + 1) * np.log1p(((Y[None, :, :, None] - f) / s) ** 2 / nu))
    dens = logsumexp(logp + np.log(w), axis=-1)                                               # [S, N, Dy]
    want_lp = logsumexp(dens.sum(-1), axis=0) - math.log(S)
    E = (f * w).sum(-1)
    V = ((s * s * nu / (nu - 2.0) + f ** 2) * w).sum(-1) - E ** 2
    want_mean = E.mean(0)
    want_var = (V + E ** 2).mean(0) - want_mean ** 2
    got = MX.mixture(MX.make("student_t", scale=s, df=nu), m, v, Y)
    np.testing.assert_allclose(got["log_density"], want_lp, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["mean"], want_mean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["var"], want_var, rtol=1e-10, atol=1e-12)


def test_restatement_matches_the_closed_form_bernoulli():
    from scipy.special import logsumexp
    from scipy.stats import norm
    rng = np.random.default_rng(6)
    S, N, Dy = 9, 6, 3
    m, v = rng.uniform(-3, 3, (S, N, Dy)), np.exp(rng.uniform(np.log(1e-4), np.log(4.0), (S, N, Dy)))
    Y = (rng.uniform(size=(N, Dy)) > 0.5).astype(np.float64)
    p = norm.cdf(m / np.sqrt(1.0 + v)) * (1 - 2e-3) + 1e-3                                    # [S, N, Dy]
    dens = np.where(Y[None] == 1, np.log(p), np.log1p(-p))
    got = MX.mixture(MX.make("bernoulli"), m, v, Y)
    np.testing.assert_allclose(got["log_density"], logsumexp(dens.sum(-1), axis=0) - math.log(S), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["mean"], p.mean(0), rtol=1e-12)
    # law of total variance for a Bernoulli mixture: the mixture of Bernoullis is a Bernoulli with the mean probability
    np.testing.assert_allclose(got["var"], p.mean(0) * (1 - p.mean(0)), rtol=1e-10, atol=1e-14)


def test_restatement_edge_cases_and_the_float32_reduction():
    lp = np.array([[-np.inf, -3.0], [-np.inf, -1.0], [-np.inf, -np.inf]])
    got = MX.lse_mean(lp)
    assert got[0] == -np.inf and abs(got[1] - (math.log(math.exp(-3) + math.exp(-1)) - math.log(3))) < 1e-14
    rng = np.random.default_rng(7)
    lp32 = rng.uniform(-40, 0, (70, 11)).astype(np.float32)
    lp32[:, 0] = -np.inf
    for seg in (4, 64):
        g32 = MX.lse_float32(lp32, seg)
        assert g32[0] == -np.inf
        np.testing.assert_allclose(g32[1:], MX.lse_mean(lp32.astype(np.float64))[1:], rtol=0, atol=1e-5)
    # the Gaussian written out, and the multi-class mixture mean is a distribution over the classes
    g = MX.mixture(MX.make("gaussian", variance=0.3), np.zeros((2, 1, 1)), np.ones((2, 1, 1)), np.array([[0.5]]))
    assert abs(g["log_density"][0] - (-0.5 * math.log(2 * math.pi * 1.3) - 0.125 / 1.3)) < 1e-14 and abs(g["var"][0, 0] - 1.3) < 1e-14
    mc = MX.mixture(MX.make("multiclass", num_classes=4), rng.uniform(-3, 3, (5, 3, 4)), rng.uniform(0.1, 2, (5, 3, 4)), np.array([[0.0], [3.0], [1.0]]))
    assert mc["mean"].shape == (3, 4) and np.all(np.abs(mc["mean"].sum(1) - 1.0) < 5e-3)      # (up to the rule and the cdf jitter)
    np.testing.assert_allclose(mc["var"], mc["mean"] - mc["mean"] ** 2, rtol=1e-12, atol=1e-14)


def test_kernel_resources_cover_the_new_kernels():
    from dgps_with_iwvi_amd import kernel_resources as kr
    if not os.path.exists(kr.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("no llvm-readelf here")
    rows = kr.check()
    for k, cap in (("k_lik_mix", 128), ("k_mc_mix", 128), ("k_xl_mix", 96)):
        assert k in kr.NO_SCRATCH and kr.MAX_VGPRS[k] == cap
        mine = [r for r in rows if r["demangled"].startswith(k + "<")]
        assert sorted(r["demangled"] for r in mine) == sorted("%s<%d>" % (k, s) for s in (4, 8, 16, 32, 64)), mine
        assert all(r["private_segment_fixed_size"] == 0 and r["vgpr_count"] <= cap for r in mine)
    # the guard fires on one of them
    worse = [dict(r) for r in rows]
    for r in worse:
        if r["demangled"] == "k_mc_mix<64>":
            r["private_segment_fixed_size"] = 128
    with pytest.raises(AssertionError, match="k_mc_mix<64>"):
        kr.check(worse)
