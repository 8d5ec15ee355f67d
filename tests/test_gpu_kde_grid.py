"""``iwvi_kde_density_grid`` (csrc/kde_grid.hip) on the MI355X against the float64 restatement tests/kde_grid_reference.py (pinned to
sklearn by tests/test_kde_grid_host.py) on the same float32 values: every code path of the kernel's sample streaming and level tiling,
the layouts, both kinds of bandwidth, the far tails, the degenerate and NaN rules, the output's bounds, determinism, the existing
single-level kernel, and the model routes ``predictive_density_grid`` and ``evaluate(on_device=True, density_levels=...)``.

Tolerance |got - ref| <= a + r |ref|.  The kernel works in float64 and rounds once to float32, so the floor is that rounding: half a unit
in the last place, 6.0e-8 |ref| (0.06 absolute at -1e6), and 3.0e-8 absolute for |ref| <= 1.
Measured on an MI355X over every comparison of this file (each prints its own figures): the largest |got - ref| where |ref| <= 1 is
2.967e-8 (the a-part), the largest |got - ref| / |ref| elsewhere 5.877e-8 (the r-part) -- the rounding of the output and nothing else;
asserted at four times these records, a = 1.19e-7 and r = 2.35e-7.  Where the restatement is +-inf or NaN the kernel must give the same."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import kde_grid_reference as R   # noqa: E402
from dgps_with_iwvi_amd.evaluation import KDE_GRID_CHUNK as C, KDE_GRID_TILE as TL   # noqa: E402

pytestmark = pytest.mark.gpu

A_REC, R_REC = 2.967e-8, 5.877e-8                # the record: largest |got - ref| where |ref| <= 1, largest |got - ref| / |ref| elsewhere
A_TOL, R_TOL = 4.0 * A_REC, 4.0 * R_REC           # asserted at four times the record
WORST = {"a": 0.0, "r": 0.0}

S_ALL = (2, 3, 63, 64, 65, 257, C - 1, C, C + 1, 2 * C + 17, 20000)
# every S meets G = 1 at N = 5 (all the parallelism over samples), a G below the tile (the splits share a level's samples) and G = 200
# (four tiles, the last one partly filled); G = TL and TL + 1 at sizes on both sides of a chunk
CASES = [(S, N, G) for S in S_ALL for N, G in ((5, 1), (5, 7), (1, 200))]
CASES += [(65, 5, TL), (257, 1, TL), (C + 1, 1, TL + 1), (2 * C + 17, 5, TL + 1), (2 * C + 17, 5, 200), (C, 5, TL)]
LAYOUTS = ("contiguous", "transposed", "strided")


def _to_device(samples, layout, dev):
    """[S, N] float32 array -> a device tensor of that shape in one of the three layouts."""
    S, N = samples.shape
    if layout == "contiguous":
        t = torch.as_tensor(samples, device=dev)
    elif layout == "transposed":                                  # the fused sampling route's: a [S, N] view of [N, S]
        t = torch.as_tensor(np.ascontiguousarray(samples.T), device=dev).t()
    else:                                                         # every second column of a wider buffer
        wide = torch.full((S, 2 * N), 7.0, dtype=torch.float32, device=dev)
        wide[:, ::2] = torch.as_tensor(samples, device=dev)
        t = wide[:, ::2]
    assert tuple(t.shape) == (S, N)
    return t


def _check(got, ref, tag):
    """Exact where the reference is +-inf or NaN, a + r |ref| elsewhere; prints this comparison's a-part and r-part and the running worst."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    special = ~np.isfinite(ref)
    assert np.array_equal(got[special], ref[special], equal_nan=True), tag
    g, r = got[~special], ref[~special]
    err = np.abs(g - r)
    small = np.abs(r) <= 1.0
    a_part = float(err[small].max()) if small.any() else 0.0
    r_part = float((err[~small] / np.abs(r[~small])).max()) if (~small).any() else 0.0
    WORST["a"], WORST["r"] = max(WORST["a"], a_part), max(WORST["r"], r_part)
    print("%s: a-part %.3e, r-part %.3e (running worst %.3e / %.3e); ref in [%.6g, %.6g]" % (
        tag, a_part, r_part, WORST["a"], WORST["r"], r.min() if r.size else np.nan, r.max() if r.size else np.nan))
    assert np.all(np.isfinite(g)), tag
    assert np.all(err <= A_TOL + R_TOL * np.abs(r)), (tag, float((err - R_TOL * np.abs(r)).max()))


@pytest.mark.parametrize("S,N,G", CASES)
def test_grid_matches_the_restatement(gpu_device, S, N, G):
    from dgps_with_iwvi_amd import evaluation
    layout = LAYOUTS[(S + N + G) % 3]
    samples = R.sample_matrix(S, N)
    levels = R.level_matrix(samples, G)                           # [N, G]: for G >= 4 the last three are -80 std, +300 std, a sample
    out = evaluation.kde_log_density_grid(_to_device(samples, layout, gpu_device), torch.as_tensor(levels, device=gpu_device))
    assert set(out) == {"logdens", "mean_std", "bandwidth"} and all(v.is_cuda and v.dtype == torch.float32 for v in out.values())
    ref, ms, bw = R.kde_log_density_grid(samples, levels)
    _check(out["logdens"].cpu().numpy(), ref, "S=%d N=%d G=%d %s" % (S, N, G, layout))
    np.testing.assert_allclose(out["bandwidth"].cpu().numpy(), bw, rtol=1e-6)
    np.testing.assert_allclose(out["mean_std"].cpu().numpy(), ms, rtol=1e-6, atol=1e-7)
    if S <= evaluation.MAX_SAMPLES:                               # the sort-based launch: the same mean and standard deviation, bit for bit
        ss = evaluation.sample_stats(_to_device(samples, layout, gpu_device), None, shapiro=False)
        assert torch.equal(out["mean_std"], ss["mean_std"])


@pytest.mark.parametrize("S", [1, 2, C + 1, 2 * C + 17])
@pytest.mark.parametrize("bandwidth", [0.01, 0.5])
def test_fixed_bandwidth(gpu_device, S, bandwidth):
    from dgps_with_iwvi_amd import evaluation
    N, G = 5, TL + 1
    samples = R.sample_matrix(S, N)
    levels = R.level_matrix(samples, G) if S > 1 else (samples[0][:, None] + np.linspace(-2, 2, G)[None, :]).astype(np.float32)
    out = evaluation.kde_log_density_grid(_to_device(samples, LAYOUTS[S % 3], gpu_device), torch.as_tensor(levels, device=gpu_device), bandwidth)
    ref, ms, bw = R.kde_log_density_grid(samples, levels, bandwidth)
    _check(out["logdens"].cpu().numpy(), ref, "fixed bandwidth %g S=%d" % (bandwidth, S))
    assert np.array_equal(out["bandwidth"].cpu().numpy(), np.full(N, bandwidth, dtype=np.float32))
    np.testing.assert_allclose(out["mean_std"].cpu().numpy(), ms, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("S", [2, 2 * C + 17])
def test_far_tails_are_finite(gpu_device, S):
    """mean - 80 std, mean + 300 std and a level equal to a sample: the float64 formula's finite values (-3e3 .. -1.1e6), where
    log(sum(exp(...))) without the shift returns -inf."""
    from dgps_with_iwvi_amd import evaluation
    samples = R.sample_matrix(S, 5)
    levels = np.stack([R.tail_levels(samples[:, n])[-3:] for n in range(5)])          # [5, 3]
    ref, _, bw = R.kde_log_density_grid(samples, levels)
    assert np.isfinite(ref).all() and np.all(ref[:, :2] < -1e3)
    assert all(R.naive_log_density(samples[:, n], float(levels[n, k]), bw[n]) == -np.inf for n in range(5) for k in (0, 1))
    got = evaluation.kde_log_density_grid(torch.as_tensor(samples, device=gpu_device), torch.as_tensor(levels, device=gpu_device))["logdens"]
    _check(got.cpu().numpy(), ref, "far tails S=%d" % S)


@pytest.mark.parametrize("S,G", [(257, 7), (2 * C + 17, 200)])
def test_shared_and_per_point_levels_give_the_same_bits(gpu_device, S, G):
    from dgps_with_iwvi_amd import evaluation
    samples = R.sample_matrix(S, 5)
    lev = R.level_matrix(samples, G)[0]
    smp = torch.as_tensor(samples, device=gpu_device)
    shared = evaluation.kde_log_density_grid(smp, torch.as_tensor(lev, device=gpu_device))
    own = evaluation.kde_log_density_grid(smp, torch.as_tensor(np.tile(lev, (5, 1)), device=gpu_device))
    for k in shared:
        assert torch.equal(shared[k], own[k]), k
    ref, _, _ = R.kde_log_density_grid(samples, lev)
    _check(shared["logdens"].cpu().numpy(), ref, "shared levels S=%d G=%d" % (S, G))


@pytest.mark.parametrize("S", [65, C + 1])
def test_degenerate_and_nan_inputs(gpu_device, S):
    from dgps_with_iwvi_amd import evaluation
    samples = R.sample_matrix(S, 5)
    clean_levels = R.level_matrix(samples, 9)
    clean = evaluation.kde_log_density_grid(torch.as_tensor(samples, device=gpu_device), torch.as_tensor(clean_levels, device=gpu_device))
    bad = samples.copy()
    bad[:, 1] = 1.25                                             # all samples equal: a point mass under Silverman
    bad[S // 2, 3] = np.nan                                      # one NaN: that point's row, nobody else's
    levels = clean_levels.copy()
    levels[1, :3] = (1.25, 1.2500001, 0.0)
    levels[4, 2] = np.nan                                        # one NaN level
    out = evaluation.kde_log_density_grid(torch.as_tensor(bad, device=gpu_device), torch.as_tensor(levels, device=gpu_device))
    ref, ms, bw = R.kde_log_density_grid(bad, levels)
    got = out["logdens"].cpu().numpy()
    assert got[1, 0] == np.inf and np.all(got[1, 1:] == -np.inf) and float(out["bandwidth"][1]) == 0.0 and out["mean_std"][1].tolist() == [1.25, 0.0]
    assert np.isnan(got[3]).all() and torch.isnan(out["mean_std"][3]).all() and torch.isnan(out["bandwidth"][3])
    assert np.isnan(got[4, 2]) and np.isfinite(np.delete(got[4], 2)).all()
    _check(got, ref, "degenerate / NaN S=%d" % S)
    for n in (0, 2):                                             # untouched points: bit for bit what the clean call gave
        assert torch.equal(out["logdens"][n], clean["logdens"][n]) and torch.equal(out["mean_std"][n], clean["mean_std"][n])
    fixed = evaluation.kde_log_density_grid(torch.as_tensor(bad, device=gpu_device), torch.as_tensor(levels, device=gpu_device), 0.5)
    _check(fixed["logdens"].cpu().numpy(), R.kde_log_density_grid(bad, levels, 0.5)[0], "degenerate / NaN, fixed bandwidth, S=%d" % S)


@pytest.mark.parametrize("S,N,G", [(2 * C + 17, 5, 7), (C + 1, 5, 200), (65, 5, 1), (257, 3, TL + 1)])
def test_output_margins_are_untouched(gpu_device, S, N, G):
    """The library called directly on the middle of a sentinel-filled buffer: nothing outside [N, G], [N, 2] and [N] is written."""
    from dgps_with_iwvi_amd import _abi
    samples = R.sample_matrix(S, N)
    levels = R.level_matrix(samples, G)
    smp = torch.as_tensor(np.ascontiguousarray(samples.T), device=gpu_device)         # [N, S]
    lev = torch.as_tensor(levels, device=gpu_device)
    margin, sentinel = 512, -12345.0
    bufs = {k: torch.full((2 * margin + n,), sentinel, dtype=torch.float32, device=gpu_device) for k, n in (("out", N * G), ("ms", 2 * N), ("bw", N))}
    p = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * margin)
    _abi.check(_abi.lib().iwvi_kde_density_grid(_abi.ptr(smp), 1, S, N, S, _abi.ptr(lev), G, G, 0.0, p(bufs["out"]), p(bufs["ms"]), p(bufs["bw"]),
                                               _abi.stream_ptr()))
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert torch.all(t[:margin] == sentinel) and torch.all(t[-margin:] == sentinel), k
        assert not torch.any(t[margin:-margin] == sentinel), k
    ref, _, _ = R.kde_log_density_grid(samples, levels)
    _check(bufs["out"][margin:-margin].reshape(N, G).cpu().numpy(), ref, "direct call S=%d N=%d G=%d" % (S, N, G))
    # the optional outputs left out: the same densities
    out2 = torch.empty(N, G, dtype=torch.float32, device=gpu_device)
    _abi.check(_abi.lib().iwvi_kde_density_grid(_abi.ptr(smp), 1, S, N, S, _abi.ptr(lev), G, G, 0.0, _abi.ptr(out2), None, None, _abi.stream_ptr()))
    assert torch.equal(out2.reshape(-1), bufs["out"][margin:-margin])


def test_two_calls_give_the_same_bits(gpu_device):
    from dgps_with_iwvi_amd import evaluation
    samples = R.sample_matrix(2 * C + 17, 5)
    smp = torch.as_tensor(samples, device=gpu_device)
    lev = torch.as_tensor(R.level_matrix(samples, 7), device=gpu_device)
    a = evaluation.kde_log_density_grid(smp, lev)
    b = evaluation.kde_log_density_grid(smp, lev)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_one_level_per_point_agrees_with_sample_stats(gpu_device):
    """Per-point levels [N, 1] equal to y: the grid and the sort-based launch's ``logp`` both within the tolerance of the restatement."""
    from dgps_with_iwvi_amd import evaluation
    S, N = 2000, 37
    samples = R.sample_matrix(S, N)
    y = R.level_matrix(samples, 1)                                # [N, 1]
    smp = torch.as_tensor(np.ascontiguousarray(samples.T), device=gpu_device).t()
    grid = evaluation.kde_log_density_grid(smp, torch.as_tensor(y, device=gpu_device))
    ss = evaluation.sample_stats(smp, torch.as_tensor(y[:, 0], device=gpu_device), shapiro=False)
    ref, _, _ = R.kde_log_density_grid(samples, y)
    _check(grid["logdens"].cpu().numpy(), ref, "grid at y, S=2000")
    _check(ss["logp"].cpu().numpy()[:, None], ref, "sample_stats logp at y, S=2000")
    assert torch.equal(grid["mean_std"], ss["mean_std"])


def test_python_interface_edges(gpu_device):
    from dgps_with_iwvi_amd import evaluation
    samples = R.sample_matrix(300, 4)
    smp = torch.as_tensor(samples, device=gpu_device)
    lev = np.linspace(-3, 3, 11).astype(np.float32)
    full = evaluation.kde_log_density_grid(smp, lev)              # levels from NumPy
    expanded = smp[:, :1].expand(300, 3)                          # a zero stride: made contiguous
    e = evaluation.kde_log_density_grid(expanded, torch.as_tensor(lev, device=gpu_device))
    assert torch.equal(e["logdens"], full["logdens"][:1].expand(3, 11))
    empty = evaluation.kde_log_density_grid(smp[:, :0], torch.as_tensor(lev, device=gpu_device))
    assert tuple(empty["logdens"].shape) == (0, 11) and tuple(empty["bandwidth"].shape) == (0,)
    with pytest.raises(Exception):
        evaluation.kde_log_density_grid(torch.zeros(8, 3), torch.zeros(4))             # a CPU tensor: no fallback


# ---- the model routes --------------------------------------------------------------------------------------------------------------------
def _factory_model(dev):
    """The small factory model of tests/test_build_models.py: IWAE, L1_G5, M = 16, on 3-D inputs."""
    from dgps_with_iwvi_amd import build_models as bm
    rng = np.random.default_rng(0)
    X = rng.standard_normal((200, 3))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((200, 1))
    args = types.SimpleNamespace(mode="IWAE", configuration="L1_G5", M=16, likelihood_variance=0.01, minibatch_size=32, num_IW_samples=4)
    np.random.seed(1)
    model = bm.build_model(args, X.astype(np.float32), Y.astype(np.float32), device=dev)
    rng = np.random.default_rng(2)
    for layer in model.layers:                                    # away from the initial state: a predictive that is not one Gaussian
        if hasattr(layer, "q_mu"):
            layer.q_mu = layer.q_mu + torch.as_tensor(rng.standard_normal(tuple(layer.q_mu.shape)), dtype=torch.float32, device=dev)
    return model, X.astype(np.float32), Y.astype(np.float32)


def _reset_noise(model):
    from dgps_with_iwvi_amd import settings
    settings.set_seed(5)
    model._words().zero_()


def test_fused_samples_through_the_grid_match_the_restatement(gpu_device):
    from dgps_with_iwvi_amd import evaluation
    from dgps_with_iwvi_amd.layers import LatentVariableLayer
    model, X, _ = _factory_model(gpu_device)
    S, N = 257, 6
    rng = np.random.default_rng(11)
    zs = [torch.as_tensor(rng.standard_normal((S, N, l.latent_dim if isinstance(l, LatentVariableLayer) else l.num_outputs)).astype(np.float32),
                          device=gpu_device) for l in model.layers]
    z_y = torch.as_tensor(rng.standard_normal((S, N, 1)).astype(np.float32), device=gpu_device)
    smp = model.predict_y_samples_fused(X[:N], S, zs, z_y)[:, :, 0]                     # [S, N], a point's samples contiguous
    host = smp.cpu().numpy()
    levels = R.level_matrix(host, 40)
    out = evaluation.kde_log_density_grid(smp, torch.as_tensor(levels, device=gpu_device))
    _check(out["logdens"].cpu().numpy(), R.kde_log_density_grid(host, levels)[0], "fused samples of the factory model")


def test_predictive_density_grid_integrates_to_one(gpu_device):
    from dgps_with_iwvi_amd import evaluation
    model, X, _ = _factory_model(gpu_device)
    S, G = 2000, 401
    _reset_noise(model)
    host = model.predict_y_samples_fused(X[:4], S)[:, :, 0].cpu().numpy().astype(np.float64)   # to place the levels
    h = 1.06 * host.std(0) * S ** -0.2
    levels = np.stack([np.linspace(host[:, n].min() - 8 * h[n], host[:, n].max() + 8 * h[n], G) for n in range(4)]).astype(np.float32)
    _reset_noise(model)
    got = evaluation.predictive_density_grid(model, X[:4], levels, num_samples=S)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (4, G) and bool(torch.isfinite(got).all())
    p, l64 = np.exp(got.cpu().numpy().astype(np.float64)), levels.astype(np.float64)
    integral = np.sum(0.5 * (p[:, 1:] + p[:, :-1]) * np.diff(l64, axis=1), axis=1)
    print("predictive_density_grid: trapezoid of exp(logdens) over 401 levels = %s" % integral)
    assert np.all(np.abs(integral - 1.0) <= 1e-3)
    # batches of points and a fixed bandwidth: the same shape, finite
    again = evaluation.predictive_density_grid(model, X[:5], levels[0], num_samples=300, predict_batch_size=2, bandwidth=0.05)
    assert tuple(again.shape) == (5, G) and bool(torch.isfinite(again).all())


def test_evaluate_adds_the_grid_and_keeps_the_other_results(gpu_device):
    from dgps_with_iwvi_amd import evaluation
    model, X, Y = _factory_model(gpu_device)
    Xt, Yt = X[100:150], Y[100:150]
    levels = np.linspace(-2.5, 2.5, 33).astype(np.float32)
    _reset_noise(model)
    plain = evaluation.evaluate(model, Xt, Yt, num_predict_samples=256, predict_batch_size=20, on_device=True)
    _reset_noise(model)
    res = evaluation.evaluate(model, Xt, Yt, num_predict_samples=256, predict_batch_size=20, on_device=True, density_levels=levels)
    assert set(res) == set(plain) | {"test_density_grid"}
    for k in ("test_loglik", "test_rmse", "test_shapiro_W_median"):
        assert res[k] == plain[k], k                              # the same samples, the same statistics
    grid = res["test_density_grid"]
    assert isinstance(grid, np.ndarray) and grid.shape == (50, 33) and grid.dtype == np.float32 and not np.isnan(grid).any()
    _reset_noise(model)
    own = evaluation.evaluate(model, Xt, Yt, num_predict_samples=256, predict_batch_size=20, on_device=True,
                              density_levels=np.tile(levels, (50, 1)))
    assert np.array_equal(own["test_density_grid"], grid)
