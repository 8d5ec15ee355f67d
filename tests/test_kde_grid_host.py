"""The KDE density grid on a GPU-less host: the float64 restatement (tests/kde_grid_reference.py) against
``sklearn.neighbors.KernelDensity``, the surface of ``iwvi_kde_density_grid`` (declared, exported, prototyped completely; the ABI number
stays 19; bad arguments refused before any HIP call), the kernel's place in the scratch guard, and the Python side's own checks."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import kde_grid_reference as R   # noqa: E402

NAME = "iwvi_kde_density_grid"
CASES = [(2, "normal"), (3, "normal"), (65, "bimodal"), (257, "bimodal"), (2000, "bimodal"), (4099, "offset")]


def _sklearn_logdens(x64, levels64, h):
    from sklearn.neighbors import KernelDensity
    kde = KernelDensity(bandwidth=float(h), kernel="gaussian", rtol=0.0, atol=0.0).fit(x64.reshape(-1, 1))
    return kde.score_samples(levels64.reshape(-1, 1))


@pytest.mark.parametrize("S,kind", CASES)
def test_restatement_reproduces_sklearn_with_silverman_bandwidth(S, kind):
    """37 levels across +-4 std, mean - 80 std, mean + 300 std and a level equal to a sample.  Bound 1e-12 max(1, |ref|); measured:
    the largest gap is 6.9e-14 (S = 2000), every far-tail value is finite (-3.7e3 .. -1.1e6) where the unshifted formula gives -inf."""
    assert R.kind_for(S) == kind
    x = R.draws(np.random.default_rng(S), S, kind)                # float32 values ...
    x64 = x.astype(np.float64)                                    # ... widened
    lev = R.tail_levels(x).astype(np.float64)
    ref, ms, bw = R.kde_log_density_grid(x[:, None], lev)
    h = 1.06 * x64.std() * S ** -0.2
    assert bw[0] == pytest.approx(h, rel=1e-15) and ms[0, 0] == pytest.approx(x64.mean(), rel=1e-15) and ms[0, 1] == pytest.approx(x64.std(), rel=1e-15)
    sk = _sklearn_logdens(x64, lev, h)
    gap = np.abs(ref[0] - sk) / np.maximum(1.0, np.abs(ref[0]))
    print("S=%d %s: worst scaled gap %.2e; far tails %.6g, %.6g; at a sample %.6g" % (S, kind, gap.max(), ref[0, -3], ref[0, -2], ref[0, -1]))
    assert np.all(gap <= 1e-12)
    assert np.isfinite(ref[0]).all() and -1.2e6 < ref[0, -2] < ref[0, -3] < -1e3
    assert R.naive_log_density(x64, lev[-3], h) == -np.inf and R.naive_log_density(x64, lev[-2], h) == -np.inf


def test_restatement_reproduces_sklearn_with_the_fixed_bandwidth():
    x = R.draws(np.random.default_rng(7), 1000, "bimodal")
    x = (x * 0.3 + 0.5).astype(np.float32)
    lev = np.linspace(-1.0, 2.0, 200)
    ref, _, bw = R.kde_log_density_grid(x[:, None], lev, bandwidth=0.01)
    sk = _sklearn_logdens(x.astype(np.float64), lev, 0.01)
    assert bw[0] == 0.01 and np.isfinite(ref).all()
    gap = np.abs(ref[0] - sk) / np.maximum(1.0, np.abs(ref[0]))
    print("fixed bandwidth 0.01, S=1000: worst scaled gap %.2e, log density %.4g .. %.4g" % (gap.max(), ref.min(), ref.max()))
    assert np.all(gap <= 1e-12)


def test_restatement_rules_for_degenerate_and_nan_inputs():
    x = R.sample_matrix(65, 5)
    x[:, 1] = 1.25
    x[7, 3] = np.nan
    lev = np.array([1.25, 0.0, np.nan, 2.0], dtype=np.float32)
    out, ms, bw = R.kde_log_density_grid(x, lev)
    assert out[1, 0] == np.inf and out[1, 1] == -np.inf and np.isnan(out[1, 2]) and out[1, 3] == -np.inf and bw[1] == 0.0
    assert np.isnan(out[3]).all() and np.isnan(ms[3]).all() and np.isnan(bw[3])
    for n in (0, 2, 4):
        assert np.isfinite(out[n, [0, 1, 3]]).all() and np.isnan(out[n, 2])
    fixed, _, _ = R.kde_log_density_grid(x, lev, bandwidth=0.5)   # a fixed bandwidth: equal samples are no special case
    assert np.isfinite(fixed[1, [0, 1, 3]]).all()
    # per-point levels that repeat the shared ones: the same numbers
    out2, _, _ = R.kde_log_density_grid(x, np.tile(lev, (5, 1)))
    assert np.array_equal(out, out2, equal_nan=True)


def test_trapezoid_of_the_estimate_integrates_to_one():
    """What tests/test_gpu_kde_grid.py asks of the model route, on stand-in samples: 401 levels over the samples' range widened by 8
    bandwidths, S = 2000.  The KDE integrates to one exactly; the trapezoid's own error at this spacing is measured here."""
    worst = 0.0
    for seed, kind in enumerate(("normal", "bimodal", "offset")):
        x = R.draws(np.random.default_rng(seed), 2000, kind)
        x64 = x.astype(np.float64)
        h = 1.06 * x64.std() * 2000 ** -0.2
        lev = np.linspace(x64.min() - 8 * h, x64.max() + 8 * h, 401).astype(np.float32)
        ref, _, _ = R.kde_log_density_grid(x[:, None], lev)
        p, l64 = np.exp(ref[0]), lev.astype(np.float64)
        integral = float(np.sum(0.5 * (p[1:] + p[:-1]) * np.diff(l64)))
        worst = max(worst, abs(integral - 1.0))
    print("trapezoid of exp(logdens) over 401 levels: worst |integral - 1| = %.2e" % worst)
    assert worst <= 1e-4                                          # (the GPU test's bound is 1e-3)


# ---- the entry point's surface ---------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "iwvi_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


def test_entry_point_is_declared_exported_and_prototyped_completely():
    decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % NAME, _header())
    assert decl, "%s is not declared in include/iwvi_hip.h" % NAME
    from dgps_with_iwvi_amd import _abi
    nargs = len([a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"])
    assert nargs == 13 and len(_abi.PROTOTYPES[NAME][1]) == nargs
    _abi, lib = _lib()
    assert hasattr(lib, NAME)
    assert lib.iwvi_version() == _abi.ABI_VERSION == 19          # additive: the number did not move


def test_grid_refuses_bad_arguments_before_any_launch():
    _abi, lib = _lib()
    buf = ctypes.c_void_p(16)                                    # never dereferenced: every call below is refused on its arguments

    def call(samples=buf, ss=1, sn=100, N=4, S=100, levels=buf, lps=0, G=8, bw=0.0, out=buf):
        return getattr(lib, NAME)(samples, ss, sn, N, S, levels, lps, G, bw, out, None, None, None)

    def refused(text, **kw):
        assert call(**kw) == _abi.ERR_ARG, kw
        msg = lib.iwvi_last_error()
        assert NAME.encode() in msg and text in msg, (kw, msg)

    refused(b"null samples", samples=None)
    refused(b"null levels", levels=None)
    refused(b"null out_logdens", out=None)
    refused(b"strides 0 / 100", ss=0)
    refused(b"strides 1 / -3", sn=-3)
    refused(b"S=1", S=1)                                         # Silverman needs two samples
    refused(b"S=1", S=1, bw=-1.0)
    assert call(S=1, bw=0.5, N=0) == 0                           # ... a fixed bandwidth one
    refused(b"S=0", S=0, bw=0.5)
    refused(b"S=-2", S=-2)
    refused(b"G=0", G=0)
    refused(b"level_point_stride=7", lps=7)                      # neither 0 nor >= G
    refused(b"level_point_stride=-8", lps=-8)
    refused(b"N=-1", N=-1)
    refused(b"bandwidth=inf", bw=float("inf"))
    refused(b"bandwidth=nan", bw=float("nan"))
    refused(b"bandwidth=-inf", bw=float("-inf"))
    assert call(N=0) == 0 and call(N=0, lps=8) == 0 and call(N=0, S=20000, G=200, lps=4096, bw=0.01) == 0      # nothing to do


def test_grid_kernel_is_listed_and_built_without_scratch():
    from dgps_with_iwvi_amd import kernel_resources as kr
    assert "k_kde_grid" in kr.NO_SCRATCH
    if not os.path.exists(kr.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    rows = [r for r in kr.check() if r["demangled"] == "k_kde_grid"]
    assert len(rows) == 1 and rows[0]["private_segment_fixed_size"] == 0 and rows[0]["vgpr_spill_count"] == 0


def test_tile_constants_match_the_kernel_source():
    from dgps_with_iwvi_amd import evaluation
    src = open(os.path.join(ROOT, "dgps_with_iwvi_amd", "csrc", "kde_grid.hip")).read()
    assert int(re.search(r"constexpr int KG_TILE = (\d+);", src).group(1)) == evaluation.KDE_GRID_TILE
    assert int(re.search(r"constexpr int KG_CHUNK = (\d+);", src).group(1)) == evaluation.KDE_GRID_CHUNK


# ---- the Python side's own checks: ValueError before the library is touched --------------------------------------------------------------
def test_python_side_refuses_bad_shapes_dtypes_and_bandwidths():
    import torch
    from dgps_with_iwvi_amd import evaluation
    import dgps_with_iwvi.evaluation as alias
    assert alias.kde_log_density_grid is evaluation.kde_log_density_grid and alias.predictive_density_grid is evaluation.predictive_density_grid
    x = torch.zeros(8, 3)
    for bad_levels in (torch.zeros(2, 4), torch.zeros(3, 4, 1), torch.zeros(0), torch.zeros(()), torch.zeros(3, 0)):
        with pytest.raises(ValueError):
            evaluation.kde_log_density_grid(x, bad_levels)
    for bad_bw in (float("inf"), float("nan"), 0.0, -0.5):
        with pytest.raises(ValueError):
            evaluation.kde_log_density_grid(x, torch.zeros(4), bandwidth=bad_bw)
        with pytest.raises(ValueError):
            evaluation.predictive_density_grid(None, np.zeros((3, 1)), np.zeros(4), bandwidth=bad_bw)
    with pytest.raises(ValueError):
        evaluation.kde_log_density_grid(torch.zeros(8), torch.zeros(4))                       # samples not [S, N]
    with pytest.raises(ValueError):
        evaluation.kde_log_density_grid(x.double(), torch.zeros(4))                           # float32 only
    with pytest.raises(ValueError):
        evaluation.kde_log_density_grid(x, torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError):
        evaluation.kde_log_density_grid(torch.zeros(1, 3), torch.zeros(4))                    # Silverman on one sample
    with pytest.raises(Exception) as e:
        evaluation.kde_log_density_grid(x, torch.zeros(4))                                    # a CPU tensor: no fallback
    assert "no CPU fallback" in str(e.value)


def test_evaluate_and_the_model_route_refuse_before_any_launch():
    import torch
    from dgps_with_iwvi_amd import evaluation
    X, Y = np.zeros((2, 1)), np.zeros((2, 1))
    with pytest.raises(ValueError, match="on_device"):
        evaluation.evaluate(None, X, Y, density_levels=[0.0, 1.0])                            # the grid is the device route's
    with pytest.raises(ValueError):
        evaluation.evaluate(None, X, Y, on_device=True, density_levels=np.zeros((3, 4)))      # [N, G] with another N
    with pytest.raises(ValueError):
        evaluation.evaluate(None, X, Y, on_device=True, density_levels=np.zeros(()))
    stub = types.SimpleNamespace(X=torch.zeros(1, 1), _output_dim=lambda: 2)
    with pytest.raises(ValueError, match="one output column"):
        evaluation.evaluate(stub, X, np.zeros((2, 2)), on_device=True, density_levels=[0.0, 1.0])
    with pytest.raises(ValueError, match="one output column"):
        evaluation.predictive_density_grid(stub, X, np.zeros(4), num_samples=10)
    stub1 = types.SimpleNamespace(X=torch.zeros(1, 1), _output_dim=lambda: 1)
    with pytest.raises(ValueError):
        evaluation.predictive_density_grid(stub1, X, np.zeros((3, 4)), num_samples=10)         # levels for another N
    with pytest.raises(ValueError):
        evaluation.predictive_density_grid(stub1, X, np.zeros(4), num_samples=1)
