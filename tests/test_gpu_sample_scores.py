"""``iwvi_sample_scores`` (one sort per point -> CRPS in both forms, the PIT's counts, quantiles and their pinball loss) against the
float64 restatement by the definitions (tests/scoring_reference.py) on the same float32 samples.

Sizes: S = 2, 3 (below a wave), 63 / 64 / 65 (the padding to 64 and the first size that pads to 128), 128 / 129 and 257 (each change of the
points-per-workgroup rule, the first LDS merge), 1000, 2049 (the first size on 1024 threads), 4097, 16384 (the cap); N = 5 leaves a group
of the four-point workgroup without a point.  The restatement sums S^2 terms per point, so the two largest sizes take one point.

Bounds.  CRPS, both forms: |device - restatement| <= 2^-23 (A + G / S^2) with the restatement's terms -- the device sums are float64, what
remains is one rounding of the result to float32 (<= 2^-24 of the result, and the result is <= A + G / S^2); the factor 2 covers the
reference's own rounding.  Pinball: the same with |y - Q| in place of the terms.  Counts: exact.  Quantiles: the bits of ``sample_stats``.
Measured on an MI355X over every case below: worst gap 0.27 of the CRPS bound, 0.41 of the pinball bound (each test prints its own)."""
import numpy as np
import pytest
import torch

import scoring_reference as SR

pytestmark = pytest.mark.gpu

PROBS = [0.0, 0.05, 0.25, 0.5, 0.75, 0.975, 1.0]
SIZES = [(2, 5), (3, 1), (3, 5), (63, 5), (64, 1), (64, 5), (65, 5), (128, 5), (129, 5), (257, 1), (257, 5), (1000, 5), (2049, 5), (4097, 1),
         (16384, 1)]
EPS = 2.0 ** -23
_cache = {}


def _inputs(kind, S, N):
    rng = np.random.default_rng(1000 * S + 10 * N + len(kind))
    if kind == "normal":
        x = rng.standard_normal((S, N)) * rng.uniform(0.3, 2.0, N) + rng.standard_normal(N)
        y = rng.standard_normal(N) * 1.5
    elif kind == "offset":                                               # offset against spread: the float32 spacing at 1e4 is 1e-3
        x = rng.standard_normal((S, N)) + 1e4
        y = rng.standard_normal(N) + 1e4
    elif kind == "ties":                                                 # integer-valued draws, y one of them
        x = np.round(rng.standard_normal((S, N)) * 3.0)
        y = x[rng.integers(0, S, N), np.arange(N)].copy()
    else:
        raise KeyError(kind)
    return x.astype(np.float32), y.astype(np.float32)


def _case(kind, S, N):
    """Inputs and the restatement's results, computed once per (kind, S, N) and left unchanged."""
    key = (kind, S, N)
    if key not in _cache:
        x, y = _inputs(kind, S, N)
        ref = SR.crps(x, y)
        ref["below"], ref["equal"] = SR.counts(x, y)
        ref["pinball"], ref["absd"] = SR.pinball(x, y, PROBS)
        _cache[key] = (x, y, ref)
    return _cache[key]


def _layout(x, layout, dev):
    S, N = x.shape
    if layout == "contiguous":
        return torch.as_tensor(x, device=dev)
    if layout == "transposed":                                           # the [S, N] view of [N, S]: a point's samples contiguous
        return torch.as_tensor(np.ascontiguousarray(x.T), device=dev).t()
    buf = torch.full((S, 2 * N + 1, 3), -7.0, device=dev)              # a strided slice: neither stride is 1
    buf[:, 1::2, 1] = torch.as_tensor(x, device=dev)
    return buf[:, 1::2, 1]


def _check(out, ref, stats_q, tag):
    crps, fair = out["crps"].cpu().numpy().astype(np.float64), out["crps_fair"].cpu().numpy().astype(np.float64)
    bound = EPS * (ref["A"] + ref["G_over_S2"])
    gap, gap_f = np.abs(crps - ref["crps"]), np.abs(fair - ref["crps_fair"])
    pin = out["pinball"].cpu().numpy().astype(np.float64)
    gap_p = np.abs(pin - ref["pinball"])
    print("%s: CRPS gap / bound %.3f, fair %.3f, pinball %.3f" % (tag, (gap / bound).max(), (gap_f / bound).max(),
                                                                   (gap_p / np.maximum(EPS * ref["absd"], 1e-300)).max()))
    assert np.array_equal(out["below"].cpu().numpy(), ref["below"]) and np.array_equal(out["equal"].cpu().numpy(), ref["equal"])
    assert out["below"].dtype == torch.int32 and out["crps"].dtype == torch.float32
    assert torch.equal(out["quantiles"], stats_q)                        # bit for bit
    assert np.all(gap <= bound), (tag, gap, bound)
    assert np.all(gap_f <= bound), (tag, gap_f, bound)
    assert np.all(gap_p <= EPS * ref["absd"]), (tag, gap_p, EPS * ref["absd"])


@pytest.mark.parametrize("layout", ["contiguous", "transposed", "strided"])
@pytest.mark.parametrize("kind", ["normal", "offset", "ties"])
@pytest.mark.parametrize("S,N", SIZES)
def test_scores_match_the_restatement(gpu_device, S, N, kind, layout):
    from dgps_with_iwvi_amd import evaluation
    x, y, ref = _case(kind, S, N)
    smp = _layout(x, layout, gpu_device)
    assert tuple(smp.shape) == (S, N) and (layout == "contiguous" or not smp.is_contiguous() or N == 1)
    yt = torch.as_tensor(y, device=gpu_device)
    out = evaluation.sample_scores(smp, yt, quantiles=PROBS)
    assert set(out) == {"crps", "crps_fair", "below", "equal", "quantiles", "pinball"} and all(v.is_cuda for v in out.values())
    stats_q = evaluation.sample_stats(smp, None, shapiro=False, quantiles=PROBS)["quantiles"]
    _check(out, ref, stats_q, "S=%d N=%d %s %s" % (S, N, kind, layout))
    again = evaluation.sample_scores(smp, yt, quantiles=PROBS)
    for k in out:
        assert torch.equal(out[k], again[k]), k                          # two calls: the same bits
    bare = evaluation.sample_scores(smp, yt)                             # no quantile outputs
    assert set(bare) == {"crps", "crps_fair", "below", "equal"} and all(torch.equal(bare[k], out[k]) for k in bare)


@pytest.mark.parametrize("S", [2, 64, 129, 1000, 4097])
def test_constant_samples_and_targets_outside_the_range(gpu_device, S):
    """All samples equal with y equal, above and below (G = 0: the score is |x - y|, exactly), and y beyond either end of a normal sample."""
    from dgps_with_iwvi_amd import evaluation
    rng = np.random.default_rng(S)
    x = np.full((S, 5), 1.25, dtype=np.float32)
    x[:, 3:] = rng.standard_normal((S, 2)).astype(np.float32)
    y = np.array([1.25, 3.0, -0.5, x[:, 3].max() + 1.0, x[:, 4].min() - 1.0], dtype=np.float32)
    out = evaluation.sample_scores(torch.as_tensor(x, device=gpu_device), torch.as_tensor(y, device=gpu_device), quantiles=[0.5])
    assert out["crps"][:3].tolist() == [0.0, 1.75, 1.75] and out["crps_fair"][:3].tolist() == [0.0, 1.75, 1.75]
    assert out["below"].tolist() == [0, S, 0, S, 0] and out["equal"].tolist() == [S, 0, 0, 0, 0]
    assert out["quantiles"][:3, 0].tolist() == [1.25] * 3 and out["pinball"][:3, 0].tolist() == [0.0, 0.875, 0.875]
    ref = SR.crps(x, y)
    bound = EPS * (ref["A"] + ref["G_over_S2"])
    assert np.all(np.abs(out["crps"].cpu().numpy() - ref["crps"]) <= bound) and np.all(np.abs(out["crps_fair"].cpu().numpy() - ref["crps_fair"]) <= bound)


@pytest.mark.parametrize("S", [3, 65, 257, 2049])
def test_a_nan_marks_its_point_alone(gpu_device, S):
    from dgps_with_iwvi_amd import evaluation
    x, y = _inputs("normal", S, 5)
    clean = evaluation.sample_scores(torch.as_tensor(x, device=gpu_device), torch.as_tensor(y, device=gpu_device), quantiles=PROBS)
    bad_x, bad_y = x.copy(), y.copy()
    bad_x[S // 2, 1] = np.nan                                            # one NaN sample in one point of five
    bad_y[3] = np.nan                                                    # one NaN target
    out = evaluation.sample_scores(torch.as_tensor(bad_x, device=gpu_device), torch.as_tensor(bad_y, device=gpu_device), quantiles=PROBS)
    for n in (1, 3):
        assert torch.isnan(out["crps"][n]) and torch.isnan(out["crps_fair"][n])
        assert torch.isnan(out["quantiles"][n]).all() and torch.isnan(out["pinball"][n]).all()
        assert int(out["below"][n]) == -1 and int(out["equal"][n]) == -1
    keep = [0, 2, 4]
    for k in clean:
        assert torch.equal(out[k][keep], clean[k][keep]), k             # bit for bit


def test_a_captured_call_replays_on_new_samples(gpu_device):
    from dgps_with_iwvi_amd import evaluation
    S, N = 300, 9
    x0, y0 = _inputs("normal", S, N)
    x1, y1 = _inputs("ties", S, N)
    smp, yt = torch.as_tensor(x0, device=gpu_device), torch.as_tensor(y0, device=gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        evaluation.sample_scores(smp, yt)                                # (warm-up outside the capture)
        with torch.cuda.graph(graph, stream=side):
            out = evaluation.sample_scores(smp, yt)
    torch.cuda.current_stream().wait_stream(side)
    smp.copy_(torch.as_tensor(x1, device=gpu_device))
    yt.copy_(torch.as_tensor(y1, device=gpu_device))
    graph.replay()
    torch.cuda.synchronize()
    want = evaluation.sample_scores(torch.as_tensor(x1, device=gpu_device), torch.as_tensor(y1, device=gpu_device))
    first = evaluation.sample_scores(torch.as_tensor(x0, device=gpu_device), torch.as_tensor(y0, device=gpu_device))
    for k in want:
        assert torch.equal(out[k], want[k]), k
    assert not torch.equal(want["crps"], first["crps"])


def test_empty_and_expanded_inputs(gpu_device):
    from dgps_with_iwvi_amd import evaluation
    out = evaluation.sample_scores(torch.zeros(8, 0, device=gpu_device), torch.zeros(0, device=gpu_device), quantiles=[0.5])
    assert out["crps"].shape == (0,) and out["pinball"].shape == (0, 1)
    x, y = _inputs("normal", 100, 1)
    smp = torch.as_tensor(x, device=gpu_device)
    e = evaluation.sample_scores(smp.expand(100, 4), torch.as_tensor(np.repeat(y, 4), device=gpu_device))    # a zero stride
    one = evaluation.sample_scores(smp, torch.as_tensor(y, device=gpu_device))
    assert torch.equal(e["crps"], one["crps"].expand(4)) and torch.equal(e["below"], one["below"].expand(4))
