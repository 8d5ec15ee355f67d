"""Entry points around the hot path, called directly with the arguments the Python wrappers never pass: ``iwvi_gaussian_var_exp`` and
``iwvi_gaussian_log_density`` under the three documented tilings of Y (explicit, IW, VI), past one pass of their grid, with a device
variance and without Fvar -- against float64 -- and ``iwvi_kde_loglik`` on point-major and padded sample layouts against
oracle/kde_oracle.py."""
import numpy as np
import pytest
import torch

from oracle.kde_oracle import kde_loglik

pytestmark = pytest.mark.gpu

NAN = float("nan")
U32 = 2.0 ** -24
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
LIK_VAR = 0.37


def _dev(a, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _tiling(name, rng, Dy):
    """-> (T, row_div, row_mod, Y [rows, Dy], row(t) for every t)."""
    if name == "explicit":                       # Y already has one row per sample
        T = 45
        return T, 1, T, rng.standard_normal((T, Dy)), np.arange(T)
    if name == "iw":                             # [B, K, .]: sample t = b K + k
        B, K = 13, 7
        return B * K, K, B, rng.standard_normal((B, Dy)), np.arange(B * K) // K
    if name == "vi":                             # tile(Y, [3, 1])
        N = 17
        return 3 * N, 1, N, rng.standard_normal((N, Dy)), np.arange(3 * N) % N
    if name == "iw_past_the_grid":               # 1 048 593 elements at Dy = 3: 17 more than 4096 blocks x 256 threads cover in one pass
        B, K = 49933, 7
        return B * K, K, B, rng.standard_normal((B, Dy)), np.arange(B * K) // K
    raise ValueError(name)


def _reference(Fmu, Fvar, Yrow, var, density):
    """float64 value and the sum of the magnitudes of its terms, from the float32 inputs.  variational expectation:
    -1/2 log 2pi - 1/2 log var - 1/2 ((y - m)^2 + v) / var;  log density: the same with s = v + var in both places and no v on top."""
    m, y = Fmu.astype(np.float64), Yrow.astype(np.float64)
    v = 0.0 if Fvar is None else Fvar.astype(np.float64)
    var = float(np.float32(var))
    s = (v + var) if density else var
    quad = 0.5 * ((y - m) ** 2 + (0.0 if density else v)) / s
    half_log = 0.5 * np.log(s) * np.ones_like(m)
    return -HALF_LOG_2PI - half_log - quad, HALF_LOG_2PI + np.abs(half_log) + quad


def _check(got, ref, mag):
    """8 float32 roundings of the sum of the terms' magnitudes: a handful of float32 operations and logf."""
    assert not np.isnan(got).any()
    err = np.abs(got - ref)
    assert np.all(err <= 8 * U32 * mag), (float((err / mag).max() / U32), np.argwhere(err > 8 * U32 * mag)[:3])
    return float((err / mag).max() / U32)


CASES = [("explicit", 1), ("explicit", 3), ("iw", 1), ("iw", 3), ("vi", 1), ("vi", 3), ("iw_past_the_grid", 3)]


@pytest.mark.parametrize("tiling,Dy", CASES)
def test_gaussian_var_exp_tilings(gpu_device, tiling, Dy):
    """Observed max error / (2^-24 sum |terms|) on an MI355X: <= 3.7 (bound 8)."""
    from dgps_with_iwvi_amd import _abi
    rng = np.random.default_rng(len(tiling) + Dy)
    T, row_div, row_mod, Y, rows = _tiling(tiling, rng, Dy)
    Fmu, Fvar = rng.standard_normal((T, Dy)).astype(np.float32), rng.random((T, Dy)).astype(np.float32)
    Y = Y.astype(np.float32)
    d = [_dev(a, gpu_device) for a in (Fmu, Fvar, Y)]
    out = torch.full((T, Dy), NAN, device=gpu_device)
    _abi.check(_abi.lib().iwvi_gaussian_var_exp(_abi.ptr(d[0]), _abi.ptr(d[1]), _abi.ptr(d[2]), LIK_VAR, T, Dy, row_div, row_mod,
                                                _abi.ptr(out), _abi.stream_ptr()))
    ref, mag = _reference(Fmu, Fvar, Y[rows], LIK_VAR, density=False)
    print("var_exp %s Dy=%d: max err = %.2f x 2^-24 sum|terms|" % (tiling, Dy, _check(out.double().cpu().numpy(), ref, mag)))


@pytest.mark.parametrize("mode", ["fvar", "no_fvar", "device_variance", "device_variance_no_fvar"])
@pytest.mark.parametrize("tiling,Dy", CASES)
def test_gaussian_log_density_tilings(gpu_device, tiling, Dy, mode):
    """Fvar given / NULL (logp), the variance as an argument / as a device scalar (the argument is then ignored), under every tiling.
    Observed max error / (2^-24 sum |terms|): <= 4.6 (bound 8)."""
    from dgps_with_iwvi_amd import _abi
    rng = np.random.default_rng(10 + len(tiling) + Dy)
    T, row_div, row_mod, Y, rows = _tiling(tiling, rng, Dy)
    Fmu = rng.standard_normal((T, Dy)).astype(np.float32)
    Fvar = None if mode.endswith("no_fvar") else rng.random((T, Dy)).astype(np.float32)
    Y = Y.astype(np.float32)
    on_device = mode.startswith("device_variance")
    var_dev = torch.tensor([LIK_VAR], dtype=torch.float32, device=gpu_device) if on_device else None
    d = [_dev(a, gpu_device) for a in (Fmu, Fvar, Y)]
    out = torch.full((T, Dy), NAN, device=gpu_device)
    _abi.check(_abi.lib().iwvi_gaussian_log_density(_abi.ptr(d[0]), _abi.ptr(d[1]), _abi.ptr(d[2]), -5.0 if on_device else LIK_VAR,
                                                    _abi.ptr(var_dev), T, Dy, row_div, row_mod, _abi.ptr(out), _abi.stream_ptr()))
    ref, mag = _reference(Fmu, Fvar, Y[rows], LIK_VAR, density=True)
    print("log_density %s Dy=%d %s: max err = %.2f x 2^-24 sum|terms|" % (tiling, Dy, mode, _check(out.double().cpu().numpy(), ref, mag)))


def test_gaussian_callables_arguments(gpu_device):
    """T == 0 is a no-op that needs no buffers; bad sizes, a non-positive variance and missing buffers are refused."""
    from dgps_with_iwvi_amd import _abi
    lib, sp = _abi.lib(), _abi.stream_ptr()
    a = torch.zeros(4, 2, device=gpu_device)
    out = torch.full((4, 2), NAN, device=gpu_device)
    p, po = _abi.ptr(a), _abi.ptr(out)
    assert lib.iwvi_gaussian_var_exp(None, None, None, LIK_VAR, 0, 2, 1, 1, None, sp) == 0
    assert lib.iwvi_gaussian_log_density(None, None, None, LIK_VAR, None, 0, 2, 1, 1, None, sp) == 0
    assert lib.iwvi_gaussian_var_exp(p, p, p, LIK_VAR, 0, 2, 1, 4, po, sp) == 0
    for T, Dy, div, mod, var in ((-1, 2, 1, 4, LIK_VAR), (4, 0, 1, 4, LIK_VAR), (4, 2, 0, 4, LIK_VAR), (4, 2, 1, 0, LIK_VAR), (4, 2, 1, 4, 0.0)):
        assert lib.iwvi_gaussian_var_exp(p, p, p, var, T, Dy, div, mod, po, sp) == _abi.ERR_ARG
        assert lib.iwvi_gaussian_log_density(p, p, p, var, None, T, Dy, div, mod, po, sp) == _abi.ERR_ARG
    assert lib.iwvi_gaussian_var_exp(p, None, p, LIK_VAR, 4, 2, 1, 4, po, sp) == _abi.ERR_ARG      # the expectation needs Fvar
    assert lib.iwvi_gaussian_log_density(p, None, None, LIK_VAR, None, 4, 2, 1, 4, po, sp) == _abi.ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------
# iwvi_kde_loglik: element (s, n) at samples[s * sample_stride + n * point_stride]
# ------------------------------------------------------------------------------------------
def _kde_call(dev, buf, sample_stride, point_stride, y, N, S):
    from dgps_with_iwvi_amd import _abi
    bd, yd = _dev(buf, dev), _dev(y, dev)
    lp, sq, ms = (torch.full(s, NAN, device=dev) for s in ((N,), (N,), (N, 2)))
    _abi.check(_abi.lib().iwvi_kde_loglik(_abi.ptr(bd), sample_stride, point_stride, _abi.ptr(yd), N, S,
                                          _abi.ptr(lp), _abi.ptr(sq), _abi.ptr(ms), _abi.stream_ptr()))
    torch.cuda.synchronize()
    return lp.cpu().numpy(), sq.cpu().numpy(), ms.cpu().numpy()


@pytest.mark.parametrize("layout", ["point_major", "padded_sample_major", "padded_point_major", "padded_both"])
@pytest.mark.parametrize("S,N", [(2, 1), (2, 5), (63, 1), (63, 5), (65, 1), (65, 5)])
def test_kde_loglik_layouts(gpu_device, S, N, layout):
    """The layouts the Python wrapper never passes (it always has (sample_stride, point_stride) = (N, 1)): a point's samples contiguous,
    and strides larger than the extents with NaN in the gaps -- a read outside the addressed elements poisons the result.  S on both
    sides of the 64-lane wave.  Tolerances of tests/test_gpu_evaluation.py::test_kde_kernel_matches_oracle."""
    rng = np.random.default_rng(100 * S + N)
    samples = (rng.standard_normal((S, N)) * rng.uniform(0.1, 2.0, N) + rng.standard_normal(N) * 3).astype(np.float32)
    y = (rng.standard_normal(N) * 2).astype(np.float32)
    if layout == "point_major":
        ss, ps = 1, S
    elif layout == "padded_sample_major":
        ss, ps = N + 3, 1
    elif layout == "padded_point_major":
        ss, ps = 1, S + 5
    else:
        ss, ps = 2, 2 * S + 3
    buf = np.full((S - 1) * ss + (N - 1) * ps + 1, np.nan, np.float32)
    idx = np.arange(S)[:, None] * ss + np.arange(N)[None, :] * ps
    assert np.unique(idx).size == S * N
    buf[idx] = samples
    lp, sq, ms = _kde_call(gpu_device, buf, ss, ps, y, N, S)
    ref_lp, ref_sq = kde_loglik(samples, y)
    np.testing.assert_allclose(lp, ref_lp, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(sq, ref_sq, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(ms[:, 0], samples.astype(np.float64).mean(0), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(ms[:, 1], samples.astype(np.float64).std(0), rtol=2e-5)
