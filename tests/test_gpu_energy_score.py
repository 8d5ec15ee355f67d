"""``iwvi_energy_score`` (the multivariate CRPS over all pairs of a point's draws, one launch) against the float64 restatement by the
definition (tests/scoring_reference.py: the double sum over ALL ordered pairs) on the same float32 samples.

Bound: |device - restatement| <= (D + 6) 2^-24 (A + B / S^2) with the restatement's terms.  Per distance: one rounding of each difference
(relative to the difference), D roundings of the float32 square-sum, a square root allowed 2 ulp, and one rounding of the result; everything
across pairs is float64.  An excess over this bound is a defect to find, not a tolerance to widen.  Measured on an MI355X over every case
below: worst gap 0.19 of the bound (each test prints its own).

The ``tight`` input (1e3 + 1e-3 z in every coordinate) is the one a Gram-form distance |x_s|^2 + |x_t|^2 - 2 x_s . x_t fails: its terms are
~D 1e6 with a float32 spacing of ~0.1 D against squared distances of ~D 1e-6."""
import numpy as np
import pytest
import torch

import scoring_reference as SR

pytestmark = pytest.mark.gpu

# (S, D, N): every S of {2, 3, 64, 65, 200, 1000}, every D of {1, 2, 3, 8, 32}, every N of {1, 3, 70}; 64 / 65: one tile of one wave and
# of two; 200: one tile of four waves, the last one ragged; 1000: four tiles, the last one ragged
CASES = [(2, 1, 1), (3, 2, 3), (64, 3, 70), (65, 8, 3), (200, 32, 3), (1000, 8, 3), (64, 32, 1), (200, 1, 70), (65, 2, 1)]
_cache = {}


def _inputs(kind, S, D, N):
    rng = np.random.default_rng(100000 * D + 100 * S + N + 7 * len(kind))
    x = rng.standard_normal((S, N, D)) * rng.uniform(0.3, 2.0, (N, D)) + rng.standard_normal((N, D))
    y = rng.standard_normal((N, D))
    if kind == "tight":
        x, y = x * 1e-3 + 1e3, y * 1e-3 + 1e3
    elif kind == "duplicated":                                           # every sample once more: exact zero distances
        x[S - S // 2:] = x[:S // 2]
    elif kind == "equal":                                                # all samples equal: B = 0, the score is |x - y|
        x[:] = x[:1]
    elif kind != "normal":
        raise KeyError(kind)
    return x.astype(np.float32), y.astype(np.float32)


def _case(kind, S, D, N):
    key = (kind, S, D, N)
    if key not in _cache:
        x, y = _inputs(kind, S, D, N)
        _cache[key] = (x, y, SR.energy(x, y))
    return _cache[key]


def _layout(x, layout, dev):
    S, N, D = x.shape
    if layout == "contiguous":
        return torch.as_tensor(x, device=dev)
    if layout == "point_major":                                          # the [S, N, D] view of [N, S, D] that predict_y_draws returns
        return torch.as_tensor(np.ascontiguousarray(x.transpose(1, 0, 2)), device=dev).permute(1, 0, 2)
    buf = torch.full((S, N, 2 * D + 1), -7.0, device=dev)               # a strided D
    buf[:, :, 1::2] = torch.as_tensor(x, device=dev)
    return buf[:, :, 1::2]


@pytest.mark.parametrize("layout", ["contiguous", "point_major", "strided_d"])
@pytest.mark.parametrize("kind", ["normal", "tight", "duplicated", "equal"])
@pytest.mark.parametrize("S,D,N", CASES)
def test_energy_score_matches_the_restatement(gpu_device, S, D, N, kind, layout):
    from dgps_with_iwvi_amd import evaluation
    x, y, ref = _case(kind, S, D, N)
    smp, Y = _layout(x, layout, gpu_device), torch.as_tensor(y, device=gpu_device)
    assert tuple(smp.shape) == (S, N, D)
    out = evaluation.energy_score(smp, Y)
    assert set(out) == {"energy", "energy_fair"} and all(v.is_cuda and v.dtype == torch.float32 and v.shape == (N,) for v in out.values())
    bound = (D + 6) * 2.0 ** -24 * (ref["A"] + ref["B_over_S2"])
    gap = np.abs(out["energy"].cpu().numpy().astype(np.float64) - ref["energy"])
    gap_f = np.abs(out["energy_fair"].cpu().numpy().astype(np.float64) - ref["energy_fair"])
    print("S=%d D=%d N=%d %s %s: gap / bound %.3f, fair %.3f" % (S, D, N, kind, layout, (gap / bound).max(), (gap_f / bound).max()))
    assert np.all(gap <= bound), (gap, bound)
    assert np.all(gap_f <= bound), (gap_f, bound)
    if kind == "equal":
        assert torch.equal(out["energy"], out["energy_fair"])            # B = 0 exactly
    again = evaluation.energy_score(smp, Y)
    assert torch.equal(out["energy"], again["energy"]) and torch.equal(out["energy_fair"], again["energy_fair"])    # the same bits


@pytest.mark.parametrize("S,N", [(2, 1), (200, 70), (1000, 3)])
def test_one_dimension_is_the_crps_of_sample_scores(gpu_device, S, N):
    """D = 1: the energy score is the CRPS; the two kernels agree within the sum of their bounds against the restatement."""
    from dgps_with_iwvi_amd import evaluation
    x, y, ref = _case("normal", S, 1, N)
    smp, Y = torch.as_tensor(x, device=gpu_device), torch.as_tensor(y, device=gpu_device)
    es = evaluation.energy_score(smp, Y)
    sc = evaluation.sample_scores(smp[:, :, 0], Y[:, 0])
    terms = ref["A"] + ref["B_over_S2"]
    bound = (7 * 2.0 ** -24 + 2.0 ** -23) * terms
    for a, b in (("energy", "crps"), ("energy_fair", "crps_fair")):
        gap = np.abs(es[a].cpu().numpy().astype(np.float64) - sc[b].cpu().numpy().astype(np.float64))
        print("S=%d N=%d %s vs %s: gap / bound %.3f" % (S, N, a, b, (gap / bound).max()))
        assert np.all(gap <= bound)


@pytest.mark.parametrize("S,D", [(3, 2), (65, 8), (1000, 8)])
def test_a_nan_marks_its_point_alone(gpu_device, S, D):
    from dgps_with_iwvi_amd import evaluation
    x, y, _ = _case("normal", S, D, 3)
    clean = evaluation.energy_score(torch.as_tensor(x, device=gpu_device), torch.as_tensor(y, device=gpu_device))
    for where in ("sample", "last_sample", "target"):
        bx, by = x.copy(), y.copy()
        if where == "target":
            by[1, D - 1] = np.nan
        else:
            bx[S // 2 if where == "sample" else S - 1, 1, 0] = np.nan
        out = evaluation.energy_score(torch.as_tensor(bx, device=gpu_device), torch.as_tensor(by, device=gpu_device))
        assert torch.isnan(out["energy"][1]) and torch.isnan(out["energy_fair"][1]), where
        for k in clean:
            assert torch.equal(out[k][[0, 2]], clean[k][[0, 2]]), (where, k)


def test_empty_input_and_the_largest_dimension_count(gpu_device):
    from dgps_with_iwvi_amd import evaluation
    out = evaluation.energy_score(torch.zeros(8, 0, 3, device=gpu_device), torch.zeros(0, 3, device=gpu_device))
    assert out["energy"].shape == (0,)
    e = evaluation.energy_score(torch.zeros(4, 2, 3, device=gpu_device).expand(4, 2, 3)[:, :, :], torch.ones(2, 3, device=gpu_device))
    assert e["energy"].tolist() == pytest.approx([3 ** 0.5] * 2, rel=1e-6)
