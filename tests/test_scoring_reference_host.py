"""The float64 restatement of the proper scoring rules (tests/scoring_reference.py) against identities and a closed form it does not use,
the host side of ``pit_values`` / ``pit_histogram`` on hand-made counts, and the argument checks that must raise without a device."""
import os

import numpy as np
import pytest
import torch

import scoring_reference as SR


def test_sorted_sum_identity_holds_for_the_restatement():
    """G = sum_i (2i - S - 1) x_(i) (what the kernel sums) equals the restatement's 1/2 sum_s sum_t |x_s - x_t| (what it is defined as)."""
    rng = np.random.default_rng(0)
    for S in (2, 3, 64, 257):
        x = rng.standard_normal((S, 4)).astype(np.float32)
        x[:, 1] = np.round(x[:, 1] * 2)                                  # ties
        ref = SR.crps(x, np.zeros(4))
        xs = np.sort(x.astype(np.float64), axis=0)
        G = ((2.0 * np.arange(1, S + 1) - S - 1.0)[:, None] * xs).sum(0)
        np.testing.assert_allclose(G / S ** 2, ref["G_over_S2"], rtol=1e-12, atol=1e-14)


def test_energy_score_at_one_dimension_is_the_crps():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((100, 3)).astype(np.float32)
    y = rng.standard_normal(3).astype(np.float32)
    c, e = SR.crps(x, y), SR.energy(x[:, :, None], y[:, None])
    for a, b in (("crps", "energy"), ("crps_fair", "energy_fair"), ("A", "A"), ("G_over_S2", "B_over_S2")):
        np.testing.assert_allclose(c[a], e[b], rtol=1e-13, atol=1e-15)


def test_crps_of_normal_draws_matches_the_closed_form():
    """20 000 standard-normal draws against sigma [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)].  The fair CRPS is the U-statistic
    mean_s |x_s - y| - mean_{s != t} |x_s - x_t| / 2, unbiased for the closed form; its variance is estimated here from the draws by the
    first-order (Hoeffding) projection h(x) = |x - y| - E_t |x - x_t|: Var ~ Var(h) / S, and the margin is five of those standard errors."""
    S = 20000
    x = np.random.default_rng(2).standard_normal((S, 1))
    xs = np.sort(x[:, 0])
    csum = np.concatenate([[0.0], np.cumsum(xs)])
    rank = np.arange(S)
    mean_abs_to_others = (xs * rank - csum[:-1] + (csum[-1] - csum[1:]) - xs * (S - 1 - rank)) / (S - 1)     # E_t |x - x_t| per sorted x
    for z in (0.0, 1.0, -2.5):
        got = SR.crps(x, np.array([z]))
        h = np.abs(xs - z) - mean_abs_to_others
        se = h.std(ddof=1) / np.sqrt(S)
        want = SR.crps_normal(z)
        print("z=%.1f: fair CRPS %.6f, ensemble %.6f, closed form %.6f, standard error %.2e" % (z, got["crps_fair"][0], got["crps"][0], want, se))
        assert abs(got["crps_fair"][0] - want) <= 5.0 * se
        assert abs(got["crps"][0] - want) <= 5.0 * se + got["G_over_S2"][0] / (S - 1)      # the ensemble form's known bias G / (S^2 (S - 1))


def test_pit_of_targets_below_every_draw_falls_in_the_first_bin():
    from dgps_with_iwvi_amd import evaluation
    N, S = 40, 99
    below, equal = torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
    pit = evaluation.pit_values(below, equal, S)
    assert pit.dtype == torch.float64 and torch.allclose(pit, torch.full((N,), 0.5 / (S + 1), dtype=torch.float64))
    h = evaluation.pit_histogram(pit, bins=10)
    assert h["counts"].tolist() == [N] + [0] * 9
    assert h["calibration_error"] == pytest.approx(1.0 - 0.5 / (S + 1))
    np.testing.assert_array_equal(h["counts"], SR.pit_hist(pit.numpy(), 10))
    assert h["calibration_error"] == pytest.approx(SR.calibration_error(pit.numpy()))


def test_pit_of_perfectly_spread_ranks_is_calibrated():
    from dgps_with_iwvi_amd import evaluation
    S = 49
    N = S + 1
    below = torch.arange(N, dtype=torch.int32)                           # every rank 0 .. S once
    equal = torch.zeros(N, dtype=torch.int32)
    pit = evaluation.pit_values(below, equal, S)
    np.testing.assert_allclose(pit.numpy(), SR.pit_midrank(below.numpy(), equal.numpy(), S), rtol=0, atol=1e-15)
    h = evaluation.pit_histogram(pit, bins=10)
    assert h["counts"].tolist() == [5] * 10
    assert h["calibration_error"] <= 1.0 / N
    assert h["calibration_error"] == pytest.approx(SR.calibration_error(pit.numpy()))


def test_randomized_pit_stays_inside_its_tie_and_marks_invalid_points():
    from dgps_with_iwvi_amd import evaluation
    S = 20
    below = torch.tensor([0, 3, 20, 5, -1], dtype=torch.int32)
    equal = torch.tensor([20, 4, 0, 0, -1], dtype=torch.int32)
    g = torch.Generator().manual_seed(1)
    pit = evaluation.pit_values(below, equal, S, randomized=True, generator=g)
    again = evaluation.pit_values(below, equal, S, randomized=True, generator=torch.Generator().manual_seed(1))
    assert torch.equal(pit[:4], again[:4]) and torch.isnan(pit[4]) and torch.isnan(evaluation.pit_values(below, equal, S)[4])
    lo, hi = below[:4].double() / (S + 1), (below[:4] + equal[:4] + 1).double() / (S + 1)
    assert bool(((pit[:4] >= lo) & (pit[:4] < hi)).all())
    many = evaluation.pit_values(torch.zeros(4000, dtype=torch.int32), torch.full((4000,), S, dtype=torch.int32), S, randomized=True, generator=g)
    assert evaluation.pit_histogram(many, 10)["calibration_error"] < 5.0 / np.sqrt(4000)       # all ties: uniform on [0, 1)


def test_argument_checks_raise_without_a_device():
    from dgps_with_iwvi_amd import _abi, evaluation
    x, y = torch.zeros(8, 3), torch.zeros(3)
    with pytest.raises(_abi.IwviError):
        evaluation.sample_scores(x, y)                                   # a CPU tensor: no fallback
    with pytest.raises(_abi.IwviError):
        evaluation.energy_score(torch.zeros(8, 3, 2), torch.zeros(3, 2))
    for S in (1, evaluation.MAX_SAMPLES + 1):
        with pytest.raises(ValueError, match="out of range"):
            evaluation.sample_scores(torch.zeros(S, 2), torch.zeros(2))
        with pytest.raises(ValueError, match="out of range"):
            evaluation.energy_score(torch.zeros(S, 2, 1), torch.zeros(2, 1))
    with pytest.raises(ValueError, match="out of range"):
        evaluation.energy_score(torch.zeros(4, 2, 33), torch.zeros(2, 33))
    with pytest.raises(ValueError):
        evaluation.sample_scores(x, torch.zeros(4))                     # shape mismatch
    with pytest.raises(ValueError):
        evaluation.sample_scores(torch.zeros(8), y)
    with pytest.raises(ValueError):
        evaluation.energy_score(torch.zeros(8, 3, 2), torch.zeros(3, 3))
    for bad in ([1.5], [-0.1], [float("nan")]):
        with pytest.raises(ValueError, match="quantiles"):
            evaluation.sample_scores(x, y, quantiles=bad)
    with pytest.raises(ValueError):
        evaluation.pit_histogram(torch.zeros(0))
    with pytest.raises(ValueError):
        evaluation.pit_values(torch.zeros(3), torch.zeros(4), 10)


def test_the_library_refuses_bad_arguments_before_any_hip_call():
    import ctypes
    from dgps_with_iwvi_amd import _abi
    for name in ("iwvi_sample_scores", "iwvi_energy_score"):
        assert name in _abi.PROTOTYPES
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    lib = _abi.lib()
    p = ctypes.c_void_p(256)                                             # never dereferenced: every call below is refused or has N = 0
    sc = lambda *a: lib.iwvi_sample_scores(*a)
    assert sc(p, 1, 8, p, 4, 1, None, 0, p, p, None, None, None) == _abi.ERR_ARG and b"iwvi_sample_scores: S=1" in lib.iwvi_last_error()
    assert sc(p, 1, 8, p, 4, 16385, None, 0, p, p, None, None, None) == _abi.ERR_ARG
    assert sc(None, 1, 8, p, 4, 8, None, 0, p, p, None, None, None) == _abi.ERR_ARG
    assert sc(p, 1, 8, None, 4, 8, None, 0, p, p, None, None, None) == _abi.ERR_ARG and b"null y" in lib.iwvi_last_error()
    assert sc(p, 0, 8, p, 4, 8, None, 0, p, p, None, None, None) == _abi.ERR_ARG and b"strides" in lib.iwvi_last_error()
    assert sc(p, 1, 8, p, -1, 8, None, 0, p, p, None, None, None) == _abi.ERR_ARG
    assert sc(p, 1, 8, p, 4, 8, None, 2, p, p, p, p, None) == _abi.ERR_ARG and b"n_probs=2" in lib.iwvi_last_error()
    assert sc(p, 1, 8, p, 0, 8, None, 0, None, None, None, None, None) == 0           # N = 0: nothing to do, no launch
    es = lambda *a: lib.iwvi_energy_score(*a)
    assert es(p, 2, 16, 1, p, 4, 1, 2, p, None) == _abi.ERR_ARG and b"iwvi_energy_score: S=1" in lib.iwvi_last_error()
    assert es(p, 2, 16, 1, p, 4, 8, 0, p, None) == _abi.ERR_ARG and b"D=0" in lib.iwvi_last_error()
    assert es(p, 2, 16, 1, p, 4, 8, 33, p, None) == _abi.ERR_ARG
    assert es(p, 2, 16, 0, p, 4, 8, 2, p, None) == _abi.ERR_ARG and b"strides" in lib.iwvi_last_error()
    assert es(p, 2, 16, 1, None, 4, 8, 2, p, None) == _abi.ERR_ARG
    assert es(p, 2, 16, 1, p, 4, 8, 2, None, None) == _abi.ERR_ARG
    assert es(p, 2, 16, 1, p, 0, 8, 2, p, None) == 0
