"""The device-side evaluation's surface on a GPU-less host: ``iwvi_dgp_predict_samples`` and ``iwvi_sample_stats`` are declared, exported and
prototyped completely (an additive extension: the ABI number stays 19), refuse bad arguments before any HIP call, and the host half of the
Shapiro-Wilk statistic -- Royston's coefficients, ``evaluation.shapiro_coefficients`` -- reproduces ``scipy.stats.shapiro``."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("iwvi_dgp_predict_samples", "iwvi_sample_stats")
SIZES = (3, 4, 5, 6, 11, 12, 64, 255, 256, 2000, 2001, 5000, 16384)


def _header():
    text = open(os.path.join(ROOT, "include", "iwvi_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_exported_and_prototyped_completely(name):
    _abi, lib = _lib()
    assert hasattr(lib, name)
    decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, _header())
    assert decl, name
    nargs = len([a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"])
    assert len(_abi.PROTOTYPES[name][1]) == nargs
    assert lib.iwvi_version() == _abi.ABI_VERSION == 19          # additive: the number did not move


def test_sample_stats_refuses_bad_arguments_before_any_launch():
    _abi, lib = _lib()
    buf = ctypes.c_void_p(16)                                    # never dereferenced: every call below is refused on its arguments
    call = lambda samples, S, probs, n_probs, y=buf: lib.iwvi_sample_stats(samples, 1, S, y, 4, S, buf, probs, n_probs,
                                                                            buf, buf, buf, buf, buf, None)
    assert call(buf, 1, None, 0) == _abi.ERR_ARG
    assert b"S=1" in lib.iwvi_last_error()
    assert call(buf, 16385, None, 0) == _abi.ERR_ARG
    assert b"S=16385" in lib.iwvi_last_error()
    assert call(None, 100, None, 0) == _abi.ERR_ARG
    assert b"null samples" in lib.iwvi_last_error()
    assert call(buf, 100, None, 3) == _abi.ERR_ARG
    assert b"n_probs=3" in lib.iwvi_last_error()
    assert call(buf, 100, None, 0, y=None) == _abi.ERR_ARG       # out_logp / out_sqerr without y
    assert lib.iwvi_sample_stats(buf, 1, 100, buf, 4, 100, None, None, 0, buf, buf, buf, buf, None, None) == _abi.ERR_ARG   # out_W without coefficients
    assert lib.iwvi_sample_stats(buf, 0, 100, buf, 4, 100, buf, None, 0, buf, buf, buf, buf, None, None) == _abi.ERR_ARG   # a zero stride
    assert lib.iwvi_sample_stats(buf, 1, 100, buf, 0, 100, buf, None, 0, buf, buf, buf, buf, None, None) == 0              # nothing to do


def test_predict_samples_refuses_bad_arguments_before_any_launch():
    _abi, lib = _lib()
    d = (_abi.LayerDesc * 1)()
    buf = ctypes.c_void_p(16)
    f = lib.iwvi_dgp_predict_samples
    assert f(d, 1, buf, 8, 1, 10, 0, 0.1, None, None, 0, buf, buf, None) == _abi.ERR_ARG
    assert b"S=0" in lib.iwvi_last_error()
    assert f(d, 1, buf, 8, 1, 10, 4, 0.1, None, None, 0, buf, None, None) == _abi.ERR_ARG          # no output
    assert f(d, 1, buf, 8, 0, 10, 4, 0.1, None, None, 0, buf, buf, None) == _abi.ERR_ARG           # Dy
    assert f(d, 1, buf, 8, 1, 10, 4, 0.0, None, None, 0, buf, buf, None) == _abi.ERR_ARG           # likelihood variance
    assert f(d, 1, buf, 8, 1, 10, 4, 0.1, None, None, 0, None, buf, None) == _abi.ERR_ARG          # draws its own noise, no rng_state
    assert f(d, 1, buf, 8, 1, 1 << 20, 1 << 12, 0.1, None, None, 0, buf, buf, None) == _abi.ERR_ARG
    assert b"rows" in lib.iwvi_last_error()
    assert f(d, 1, buf, 8, 1, 0, 4, 0.1, None, None, 0, buf, buf, None) == 0                       # nothing to do


def test_python_side_refuses_probabilities_outside_the_unit_interval_and_bad_sizes():
    import torch
    from dgps_with_iwvi_amd import evaluation
    x = torch.zeros(8, 3)
    for bad in ([-0.1], [0.5, 1.5], [float("nan")]):
        with pytest.raises(ValueError):
            evaluation.sample_stats(x, quantiles=bad)
        with pytest.raises(ValueError):
            evaluation.evaluate(None, np.zeros((2, 1)), np.zeros((2, 1)), on_device=True, quantiles=bad)
    with pytest.raises(ValueError):
        evaluation.evaluate(None, np.zeros((2, 1)), np.zeros((2, 1)), quantiles=[0.5])             # quantiles are the device route's
    with pytest.raises(ValueError):
        evaluation.sample_stats(torch.zeros(1, 3))
    with pytest.raises(ValueError):
        evaluation.sample_stats(torch.zeros(16385, 1))
    for S in (1, 16385):
        with pytest.raises(ValueError):
            evaluation.shapiro_coefficients(S)


def test_new_kernels_are_built_without_scratch():
    from dgps_with_iwvi_amd import kernel_resources as kr
    if not os.path.exists(kr.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    rows = kr.check()
    names = [r["demangled"] for r in rows]
    assert "k_sample_stats" in names and "k_sample_stats" in kr.NO_SCRATCH
    samp = [r for r in rows if re.match(r"k_dgp_forward<\d+,(true|false),(true|false),4,(true|false)>", r["demangled"])]
    assert len(samp) == 15                                       # NS in {1, 3, 5} x (S16, BIG) + the three float64 stage-1 variants
    assert all(r["private_segment_fixed_size"] == 0 for r in samp)


def _draws(rng, n, kind):
    x = rng.standard_normal(n)
    if kind == "bimodal":
        x = np.where(rng.random(n) < 0.4, x * 0.3 - 2, x * 0.5 + 1.5)
    elif kind == "lognormal":
        x = np.exp(x)
    elif kind == "offset":
        x = 50 + 1e-3 * x
    return x.astype(np.float32).astype(np.float64)               # float32 values, widened


def test_small_sizes_have_their_exact_forms():
    from dgps_with_iwvi_amd.evaluation import shapiro_coefficients
    assert shapiro_coefficients(3).tolist() == [np.sqrt(0.5)]
    for S in SIZES:
        a = shapiro_coefficients(S)
        assert a.dtype == np.float64 and a.shape == (S // 2,)
        assert abs(2.0 * float(np.dot(a, a)) - 1.0) < 1e-12       # normalised: W <= 1
        assert np.all(a > 0) and np.all(np.diff(a) < 0)
    for S in (4, 5):                                             # only the first coefficient carries the polynomial correction:
        from statistics import NormalDist                        # the rest are the normal scores, rescaled
        a = shapiro_coefficients(S)
        m = np.array([NormalDist().inv_cdf((i - 0.375) / (S + 0.25)) for i in range(1, S // 2 + 1)])
        fac = np.sqrt((2.0 * np.dot(m, m) - 2.0 * m[0] ** 2) / (1.0 - 2.0 * a[0] ** 2))
        np.testing.assert_allclose(a[1], -m[1] / fac, rtol=1e-14)
        assert abs(a[0] + m[0] / np.sqrt(2.0 * np.dot(m, m))) > 1e-4      # (a_1 is NOT the plain rescaled score)


@pytest.mark.parametrize("S", SIZES)
def test_coefficients_reproduce_scipy_shapiro(S):
    """W from the direct formula in NumPy float64 with ``shapiro_coefficients(S)`` against ``scipy.stats.shapiro``.  Bound 1e-7: the
    largest gap measured over these 13 sizes x 4 kinds is 6.4e-9 (log-normal, S = 16384), typical gaps are 1e-11 .. 6e-10."""
    from scipy.stats import shapiro
    from dgps_with_iwvi_amd.evaluation import shapiro_coefficients
    a = shapiro_coefficients(S)
    rng = np.random.default_rng(S)
    for kind in ("normal", "bimodal", "lognormal", "offset"):
        x = np.sort(_draws(rng, S, kind))
        h = S // 2
        W = float(np.dot(a, x[::-1][:h] - x[:h])) ** 2 / float(((x - x.mean()) ** 2).sum())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                      # (SciPy warns about its p-value above N = 5000; W is what is compared)
            ref = float(shapiro(x)[0])
        print("S=%d %s: W=%.12f scipy=%.12f gap=%.2e" % (S, kind, W, ref, abs(W - ref)))
        assert abs(W - ref) <= 1e-7
