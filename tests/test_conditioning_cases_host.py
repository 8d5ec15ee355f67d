"""tests/conditioning_cases.py on the host: every case of its tables lands on the side of the K_uf switch it promises, with room, and keeps
its rows live; ``expected_constants`` restates the device's rounding; ``per_column_close`` sees an error that is confined to the
smallest-scale latent GP, which the whole-array max-norm does not."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_cases as cc   # noqa: E402


def _check(c, geometry):
    assert c.geometry == geometry
    if geometry == "compact":
        assert c.zmax2 <= cc.COMPACT_MAX < cc.SWITCH and c.multiplier >= 1.0
    else:
        assert c.zmax2 >= cc.SPREAD_MIN > cc.SWITCH and c.multiplier <= 0.4
    assert c.live_mean_fraction >= 0.8 and c.live_a2_min > 0.1
    lay = c.spec["layers"][c.li]
    for k in ("Z", "ls", "q_mu", "q_sqrt"):                      # what the device, the oracle and the autograd reference all read
        assert np.array_equal(np.asarray(lay[k], dtype=np.float32).astype(np.float64), lay[k]), k
    assert np.array_equal(c.spec["X"].astype(np.float32).astype(np.float64), c.spec["X"])


@pytest.mark.parametrize("M,D", cc.SHAPES_A)
@pytest.mark.parametrize("geometry", ["compact", "spread"])
def test_cases_of_part_a_keep_their_side_and_stay_live(M, D, geometry):
    _check(cc.conditioned_case(M, D, cc.R_B, geometry, 10, seed=cc.case_seed(M, D)), geometry)


@pytest.mark.parametrize("M,D,geometry,offset,kern", cc.CASES_B)
def test_cases_of_part_b_keep_their_side_and_stay_live(M, D, geometry, offset, kern):
    c = cc.conditioned_case(M, D, cc.R_B, geometry, offset, kern=kern, seed=cc.case_seed(M, D))
    _check(c, geometry)
    # the cloud really is off-centre: the centre the state publishes is the offset, in lengthscale units
    zc = cc.expected_constants(c.spec, c.li)[1]
    assert np.all(np.abs(zc - offset) < 0.5)
    # and the first layer hands on rows near F: its mean function alone gives F back to float32 rounding
    first = c.spec["layers"][0]
    back = c.spec["X"][:len(c.F)] @ first["mf"][1] + first["mf"][2]
    assert np.abs(back - c.F).max() <= 4e-6 * max(1.0, float(np.abs(c.F).max()))
    # ... and with its GP part they stay live
    handed = cc.first_layer_reference(c)[0]
    assert np.abs((handed - c.F) / c.spec["layers"][c.li]["ls"]).max() < 0.5
    live, a2 = cc.liveness(c, handed)
    assert live >= 0.8 and a2 > 0.1, (live, a2)


def test_the_tables_of_part_b_show_every_geometry_kernel_and_offset():
    assert {(g, k) for _, _, g, _, k in cc.CASES_B} == {(g, k) for g in ("compact", "spread") for k in ("rbf", "matern52")}
    for M, D in {(m, d) for m, d, _, _, _ in cc.CASES_B}:
        rows = [r for r in cc.CASES_B if r[:2] == (M, D)]
        assert {r[2] for r in rows} == {"compact", "spread"} and {r[4] for r in rows} == {"rbf", "matern52"}
        assert {10, 30} <= {r[3] for r in rows}
    assert {(m, d) for m, d, _, _, _ in cc.CASES_B} == {(32, 4), (48, 8), (100, 5), (128, 8), (96, 12), (250, 8), (64, 2)}


@pytest.mark.parametrize("M", cc.M_C)
def test_cases_of_part_c_keep_their_side_and_stay_live(M):
    for q, qmu in ((cc.Q_FORWARD, cc.QMU_HETERO), (cc.Q_ADJOINT, cc.QMU_HETERO), (None, cc.QMU_ZERO)):
        c = cc.conditioned_case(M, cc.D_C, 4, "compact", 0, q, qmu, seed=cc.case_seed(M, cc.D_C))
        _check(c, "compact")
        lay = c.spec["layers"][c.li]
        base = cc.conditioned_case(M, cc.D_C, 4, "compact", 0, seed=cc.case_seed(M, cc.D_C)).spec["layers"][c.li]
        for r in range(4):
            assert np.array_equal(lay["q_mu"][:, r], (qmu[r] * base["q_mu"][:, r]).astype(np.float32).astype(np.float64))
            if q is not None:
                assert np.array_equal(lay["q_sqrt"][r], (q[r] * base["q_sqrt"][r]).astype(np.float32).astype(np.float64))
        if q is cc.Q_FORWARD:
            assert not lay["q_sqrt"][3].any() and not lay["q_mu"][:, 3].any()
            # every latent GP gets another exponent: 13 - ilogb(max|tril L_r|) (csrc/precompute_dev.h), 0 for the zero matrix
            er = [13 - int(np.floor(np.log2(np.abs(np.tril(L)).max()))) if L.any() else 0 for L in lay["q_sqrt"]]
            assert len(set(er)) == 4, er


@pytest.mark.parametrize("cid,M,D,T,geometry,offset,q,qmu,kern", cc.CASES_D, ids=[c[0] for c in cc.CASES_D])
def test_cases_of_part_d_keep_their_side_and_stay_live(cid, M, D, T, geometry, offset, q, qmu, kern):
    c = cc.conditioned_case(M, D, cc.R_D, geometry, offset, q, qmu, kern=kern, seed=cc.case_seed(M, D), T=T)
    _check(c, geometry)
    assert c.F.shape == (T, D) and c.cs.shape == c.cm.shape == c.cv.shape == c.z.shape == (T, cc.R_D)
    assert (T % 16 == 0) == (M % 16 == 0)
    assert np.all(np.diagonal(c.spec["layers"][c.li]["q_sqrt"], axis1=1, axis2=2) != 0)      # the KL's log diag stays finite


@pytest.mark.parametrize("M,v", cc.CASES_E)
def test_cases_of_part_e_keep_their_side_and_stay_live(M, v):
    c = cc.conditioned_case(M, cc.D_E, cc.R_E, "compact", 0, seed=cc.case_seed(M, cc.D_E), T=cc.T_CHAIN, variance=v)
    _check(c, "compact")
    assert c.spec["layers"][c.li]["var"] == float(np.float32(v))
    # the device value and the stale host copy 1.0 imply different scale exponents: ceil(log2(v) / 2) = -2 (0.02) and +3 (60)
    assert int(np.ceil(0.5 * np.log2(np.float32(v)))) == {0.02: -2, 60.0: 3}[v]


@pytest.mark.parametrize("cid,L,M,D,geometry,kern,fetch", cc.CASES_L2, ids=[c[0] for c in cc.CASES_L2])
def test_stacks_of_the_l2_fetches_overflow_the_lds_and_stay_live(cid, L, M, D, geometry, kern, fetch):
    assert cc.staged_image_floor(L, M, D) > cc.LDS_MAX                       # the images cannot all be staged: ZtP is read from L2
    assert M > 128 and fetch == {"compact": "prefetched", "spread": "direct"}[geometry]
    c = cc.conditioned_case(M, D, cc.R_B, geometry, 0, kern=kern, seed=cc.case_seed(M, D), L=L)
    _check(c, geometry)
    assert c.li == L - 1 and len(c.spec["layers"]) == L
    handed = cc.handed_on_reference(c)
    assert np.abs((handed - c.F) / c.spec["layers"][c.li]["ls"]).max() < 0.5
    live, a2 = cc.liveness(c, handed)
    assert live >= 0.8 and a2 > 0.1, (live, a2)


def test_d5_at_m100_needs_a_larger_multiplier():
    """(100, 5) at multiplier 1.0 sits above the compact bound: the ladder moves it, and the helper says by how much."""
    c = cc.conditioned_case(100, 5, 2, "compact", 0, seed=cc.case_seed(100, 5))
    assert c.multiplier > 1.0 and c.zmax2 <= cc.COMPACT_MAX
    lay = c.spec["layers"][c.li]
    assert cc._zmax2(lay["Z"], lay["ls"] / c.multiplier) > cc.COMPACT_MAX


def test_expected_constants_restate_the_device_rounding():
    spec = dict(layers=[None, dict(Z=np.array([[1.0, 2.0], [3.0, 4.0]]), ls=np.array([1.0, 2.0]))])
    invls, zc, zmax2 = cc.expected_constants(spec, 1)
    assert np.array_equal(invls, [1.0, 0.5]) and np.array_equal(zc, [2.0, 1.5]) and zmax2 == 1.25
    # float32 at every step: a lengthscale whose reciprocal is not representable, an offset that costs the centred values their low bits
    rng = np.random.default_rng(0)
    Z = (rng.standard_normal((50, 3)) + 30.0).astype(np.float32).astype(np.float64)
    ls = np.array([0.3, 1.7, 0.9], dtype=np.float32).astype(np.float64)
    invls, zc, zmax2 = cc.expected_constants(dict(layers=[None, dict(Z=Z, ls=ls)]), 1)
    Zs = np.float32(Z / ls)
    assert np.array_equal(zc, np.float32(Zs.astype(np.float64).sum(0) / 50).astype(np.float64))
    assert zmax2 == max(float(((np.float32(Zs[m] - np.float32(zc))).astype(np.float64) ** 2).sum()) for m in range(50))
    exact = (((Z / ls) - (Z / ls).mean(0)) ** 2).sum(1).max()
    assert zmax2 != exact and abs(zmax2 - exact) < 1e-3 * exact            # the rounding is visible, and small


def test_per_column_close_sees_what_the_max_norm_hides():
    rng = np.random.default_rng(1)
    ref = rng.standard_normal((64, 4)) * np.array([1.0, 1e-4, 1e3, 0.0])
    got = ref.copy()
    got[:, 1] *= 1.5                                                       # 50 % off, in the smallest live column alone
    assert cc.max_norm_close(got, ref, 2e-3) < 1e-3                        # the whole-array form accepts it
    with pytest.raises(AssertionError, match=r"x\[1\]"):
        cc.per_column_close(got, ref, 1, 2e-3, name="x")
    assert max(cc.per_column_close(ref, ref, 1, 2e-3)) == 0.0
    ok = ref.copy()
    ok[:, 1] *= 1.001
    ok[:, 2] *= 1.001
    ratios = cc.per_column_close(ok, ref, 1, 2e-3)
    assert 0.4 < ratios[1] < 0.6 and 0.4 < ratios[2] < 0.6 and ratios[0] == ratios[3] == 0.0
    # along another axis: the slices of a [R, M, M] array
    ref3 = rng.standard_normal((3, 5, 5)) * np.array([1.0, 1e-5, 30.0])[:, None, None]
    got3 = ref3.copy()
    got3[1, 2, 2] += 1e-6
    assert cc.max_norm_close(got3, ref3, 3e-3) < 1e-3
    with pytest.raises(AssertionError, match=r"y\[1\]"):
        cc.per_column_close(got3, ref3, 0, 3e-3, name="y")


def test_per_column_close_wants_an_exact_zero_for_a_zero_reference():
    ref = np.zeros((8, 2))
    ref[:, 0] = 1.0
    got = ref.copy()
    got[3, 1] = 1e-30
    with pytest.raises(AssertionError, match=r"x\[1\]"):
        cc.per_column_close(got, ref, 1, 2e-3, name="x")
    # ... unless the case states the scale of what the slice was computed from
    assert cc.per_column_close(got, ref, 1, 2e-3, atol_rel=1e-6, input_scale=[1.0, 1.0])[1] < 1e-20
    got[3, 1] = 1e-5
    with pytest.raises(AssertionError, match=r"x\[1\]"):
        cc.per_column_close(got, ref, 1, 2e-3, atol_rel=1e-6, input_scale=[1.0, 1.0], name="x")
    with pytest.raises(AssertionError):
        cc.per_column_close(np.full((2, 2), np.nan), np.ones((2, 2)), 1, 1.0)
