"""Cases that move a GP layer's data to where its packed state adapts (test_gpu_layer_conditioning.py, test_conditioning_cases_host.py):
the geometry of the inducing cloud in lengthscale units (``zmax2`` of csrc/precompute_dev.h: role_factor, on either side of the 4.0 that
selects the form of K_uf), its distance from the origin, and the power-of-two scales of the split-f16 operands (per latent GP from
max|tril q_sqrt[r]|, one for the matrix from max|q_mu|).

A case is an edited ``synthetic.make_spec`` spec of two GP layers whose FINAL layer (index ``LI``) is the layer under test -- the device
model, the float64 oracle and the float64 autograd adjoint all read the same float32 numbers -- plus the rows that layer is evaluated on:

  * ARD lengthscales ``(0.8 + 0.4 u) sqrt(D) * multiplier``; the multiplier is the largest (compact) / smallest (spread) of a fixed ladder at
    which the float64 restatement of the device's ``zmax2`` is <= 3 / >= 8, so float32 rounding cannot flip the side the case promises;
  * ``offset`` moves Z, and the inputs with it, by ``offset * lengthscale`` in every coordinate;
  * inputs near the cloud, ``F = Z[idx] + 0.3 l N(0, 1)``: a spread layer is then not tested on rows where k = 0.  Asserted on the float64
    reference alone: >= 80 % of the means (unit q scales) have |mean| > 0.05 and every row has |a|^2 / variance > 0.1;
  * ``q_scales[r]`` multiplies q_sqrt[r], ``qmu_scales[r]`` multiplies q_mu[:, r].

For the route through the fused forward the first layer is made to hand the same rows on: model inputs ``X = F - offset * l``, a Linear
mean function with the identity and the bias ``offset * l``, and a mixing matrix shrunk to a twentieth of the smallest lengthscale -- the
second layer's inputs are then the first layer's own samples, within a fraction of a lengthscale of F (``first_layer_reference``)."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import iwvi_oracle as O   # noqa: E402

LI = 1                   # the layer under test: the final layer of the two-layer spec
T_ROWS = 70              # four whole 16-row sub-tiles and a ragged one
T_CHAIN = 80             # the adjoint's streaming chain (and with it the split-f16 images of S_r) needs whole 16-row tiles
COMPACT_MAX, SPREAD_MIN, SWITCH = 3.0, 8.0, 4.0
LADDER = 1.25            # the multiplier moves in these steps from 1.0 (compact, upwards) or 0.4 (spread, downwards)

Conditioned = namedtuple("Conditioned", "spec li F z cs cm cv kern geometry offset multiplier zmax2 live_mean_fraction live_a2_min shift")


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def oracle_kernel(lay):
    """The float64 kernel of a spec layer (``lay["kern"]``: "rbf" when absent, or "matern52")."""
    cls = O.Matern52 if lay.get("kern") == "matern52" else O.RBF
    return cls(lay["Z"].shape[1], variance=float(lay["var"]), lengthscales=np.asarray(lay["ls"], dtype=np.float64))


def scaled_centred(Z, ls):
    """What the device factorises and K_uf sees: Zs = fl32(Z / l), zc = fl32(mean_m Zs), fl32(Zs - zc) -> (1 / l, zc, centred), float64
    arrays of float32-representable values (1 / l is NOT rounded: the state holds its float32 rounding)."""
    Z32, l32 = np.asarray(Z, dtype=np.float32), np.asarray(ls, dtype=np.float32)
    Zs = (Z32.astype(np.float64) / l32.astype(np.float64)).astype(np.float32)
    zc = Zs.astype(np.float64).mean(0).astype(np.float32)
    return 1.0 / l32.astype(np.float64), zc.astype(np.float64), (Zs - zc).astype(np.float32).astype(np.float64)


def expected_constants(spec, li):
    """-> float64 (1 / l [D], zc [D], zmax2 = max_m |Z_m / l - zc|^2) as the precompute launch rounds them (``scaled_centred``)."""
    lay = spec["layers"][li]
    invls, zc, Zc = scaled_centred(lay["Z"], lay["ls"])
    return invls, zc, float((Zc ** 2).sum(1).max())


def _zmax2(Z, ls):
    return float((scaled_centred(Z, ls)[2] ** 2).sum(1).max())


def _multiplier(Z0, base_ls, offset, geometry):
    """The first multiplier of the ladder that puts the case on its side with room: compact from 1.0 upwards, spread from 0.4 downwards."""
    mult = 1.0 if geometry == "compact" else 0.4
    for _ in range(40):
        ls = _f32(base_ls * mult)
        z2 = _zmax2(_f32(Z0 + offset * ls), ls)
        if (z2 <= COMPACT_MAX) if geometry == "compact" else (z2 >= SPREAD_MIN):
            return mult
        mult = mult * LADDER if geometry == "compact" else mult / LADDER
    raise AssertionError("no multiplier puts the case on the %s side" % geometry)


def solve_a(lay, F):
    """a = Lm^-1 k(Z, F) in float64 -> [M, T]."""
    k = oracle_kernel(lay)
    Z = np.asarray(lay["Z"], dtype=np.float64)
    Lm = np.linalg.cholesky(k.K(Z) + O.DEFAULT_JITTER * np.eye(len(Z)))
    return np.linalg.solve(Lm, k.K(Z, np.asarray(F, dtype=np.float64)))


def reference_layer(lay, F, z=None):
    """The float64 conditional of a spec layer on rows F [T, D] (zero mean function, no mixing) -> (sample, mean, var, kl)."""
    layer = O.GPLayer(oracle_kernel(lay), lay["Z"], lay["q_mu"].shape[1], None)
    layer.q_mu, layer.q_sqrt = np.asarray(lay["q_mu"], dtype=np.float64), np.asarray(lay["q_sqrt"], dtype=np.float64)
    s, m, v, kl = layer.propagate(np.asarray(F, dtype=np.float64)[None], full_cov=False,
                                  z=None if z is None else np.asarray(z, dtype=np.float64)[None])
    return s[0], m[0], v[0], kl


def conditioned_case(M, D, R, geometry, offset, q_scales=None, qmu_scales=None, kern="rbf", seed=0, T=T_ROWS, variance=1.0, L=2):
    """-> ``Conditioned``: the edited spec (layer ``li`` under test), its rows F [T, D] and z [T, R], cotangents cs, cm, cv [T, R] (float32),
    the multiplier chosen, the float64 ``zmax2`` and the two liveness figures -- all asserted before anything is returned."""
    from dgps_with_iwvi_amd import synthetic
    if geometry not in ("compact", "spread") or kern not in ("rbf", "matern52"):
        raise ValueError((geometry, kern))
    spec = synthetic.make_spec(L=L, M=M, B=T, K=1, Dx=D, Dy=R, R=2, with_lv=False, seed=seed)
    first, lay, li = spec["layers"][0], spec["layers"][L - 1], L - 1
    assert L == 2 or offset == 0                   # a deeper stack (``L`` > 2: every inner layer hands its rows on) stays at the origin
    rng = np.random.default_rng([seed, M, D, 0x636f6e64])
    base_ls = (0.8 + 0.4 * rng.random(D)) * np.sqrt(D)
    Z0 = np.asarray(lay["Z"], dtype=np.float64)
    mult = _multiplier(Z0, base_ls, offset, geometry)
    ls = _f32(base_ls * mult)
    shift = _f32(offset * ls)
    lay["ls"], lay["Z"], lay["kern"], lay["var"] = ls, _f32(Z0 + shift), kern, float(np.float32(variance))
    zmax2 = expected_constants(spec, li)[2]
    assert (zmax2 <= COMPACT_MAX) if geometry == "compact" else (zmax2 >= SPREAD_MIN), (geometry, zmax2)
    # rows near the cloud, and what makes the first layer hand (nearly) the same rows on
    idx = rng.integers(0, M, T)
    F = np.asarray(lay["Z"][idx] + 0.3 * ls * rng.standard_normal((T, D)), dtype=np.float32)
    z = rng.standard_normal((T, R)).astype(np.float32)
    cs, cm, cv = (rng.standard_normal((T, R)).astype(np.float32) for _ in range(3))
    spec["X"][:T] = _f32(F.astype(np.float64) - shift)
    for inner in spec["layers"][:li]:
        inner["W"] = _f32(0.05 * ls.min() * inner["W"])
    first["mf"] = ("linear", first["mf"][1], shift.copy())
    # liveness, on the reference alone and at unit q scales
    a = solve_a(dict(lay, Z=lay["Z"] - shift), F.astype(np.float64) - shift)
    a2 = (a ** 2).sum(0) / float(lay["var"])
    live = float((np.abs(a.T @ np.asarray(lay["q_mu"], dtype=np.float64)) > 0.05 * np.sqrt(float(lay["var"]))).mean())
    assert live >= 0.8 and a2.min() > 0.1, ("the rows are not live", M, D, geometry, kern, live, float(a2.min()))
    if q_scales is not None:
        assert len(q_scales) == R
        lay["q_sqrt"] = _f32(np.asarray(lay["q_sqrt"]) * np.asarray(q_scales, dtype=np.float64)[:, None, None])
    if qmu_scales is not None:
        assert len(qmu_scales) == R
        lay["q_mu"] = _f32(np.asarray(lay["q_mu"]) * np.asarray(qmu_scales, dtype=np.float64)[None, :])
    return Conditioned(spec, li, F, z, cs, cm, cv, kern, geometry, offset, mult, zmax2, live, float(a2.min()), shift)


def inner_noise(c):
    """The draws of the layers in front of the one under test on the fused route, [T, 2] float32 each (a stream of their own)."""
    rng = np.random.default_rng([len(c.F), c.F.shape[1], 0x7a30])
    return [rng.standard_normal((len(c.F), 2)).astype(np.float32) for _ in range(c.li)]


def first_layer_noise(c):
    return inner_noise(c)[0]


def inner_layer_reference(c, i, rows, z):
    """The float64 inner layer i (mixing, Linear mean function with its bias) on ``rows`` -> (sample, mean, var) [T, D]."""
    inner = c.spec["layers"][i]
    kern = O.SharedMixedMok(O.RBF(inner["Z"].shape[1], variance=float(inner["var"]), lengthscales=inner["ls"]), inner["W"])
    layer = O.GPLayer(kern, inner["Z"], inner["q_mu"].shape[1], O.Linear(inner["mf"][1], inner["mf"][2]))
    layer.q_mu, layer.q_sqrt = inner["q_mu"], inner["q_sqrt"]
    s, m, v, _ = layer.propagate(np.asarray(rows, dtype=np.float64)[None], full_cov=False, z=np.asarray(z, dtype=np.float64)[None])
    return s[0], m[0], v[0]


def first_layer_reference(c, z0=None):
    """The float64 first layer on the model's inputs: the rows the layer under test gets on the fused two-layer route."""
    return inner_layer_reference(c, 0, c.spec["X"][:len(c.F)], first_layer_noise(c) if z0 is None else z0)


def handed_on_reference(c):
    """The float64 samples of the whole stack in front of the layer under test, each layer fed the one before -> [T, D]."""
    rows = c.spec["X"][:len(c.F)]
    for i, z in enumerate(inner_noise(c)):
        rows = inner_layer_reference(c, i, rows, z)[0]
    return rows


def liveness(c, rows):
    """(share of |mean| > 0.05 sigma at the case's q_mu, min over rows of |a|^2 / variance) of the layer under test on ``rows``."""
    lay = centred_layer(c)
    a = solve_a(lay, centred_rows(c, rows))
    sd = np.sqrt(float(lay["var"]))
    return float((np.abs(a.T @ lay["q_mu"]) > 0.05 * sd).mean()), float(((a ** 2).sum(0) / float(lay["var"])).min())


def centred_layer(c):
    """The layer under test with its inducing inputs moved back by the case's shift, for the float64 references: a stationary kernel
    sees differences only, so this is the same function of ``rows - shift`` -- and the subtraction of two float32 values is exact in
    float64.  (Evaluated where the data lies, the oracle's own expanded square distance |x|^2 + |z|^2 - 2 x.z cancels to ~1e-12 at
    offset 30 -- the size of the 1e-12 under Matern52's square root, which then goes negative.)"""
    lay = c.spec["layers"][c.li]
    return dict(lay, Z=lay["Z"] - c.shift)


def centred_spec(c):
    """The case's spec with ``centred_layer`` in place of the layer under test (for ``adjoint_reference.layer_reference``; its
    gradients with respect to Z, the rows, the lengthscales and everything else are those of the spec itself)."""
    layers = list(c.spec["layers"])
    layers[c.li] = centred_layer(c)
    return dict(c.spec, layers=layers)


def centred_rows(c, rows=None):
    """``rows - shift`` in float64 (``rows``: the case's F when None)."""
    return np.asarray(c.F if rows is None else rows, dtype=np.float64) - c.shift


def per_column_close(got, ref, axis, rtol, atol_rel=0.0, input_scale=None, name="array"):
    """Every slice along ``axis`` (one latent GP each) against that slice's OWN max|ref|: max|got - ref| <= rtol max|ref_slice|.  A slice
    whose reference is exactly zero must be exactly zero -- or, where the caller says why, within ``atol_rel * input_scale[i]``
    (``input_scale``: the scale of what that slice was computed from).  -> the per-slice error / allowance; raises AssertionError naming
    every slice that misses."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s is not finite" % name
    n = got.shape[axis]
    g, r = np.moveaxis(got, axis, 0).reshape(n, -1), np.moveaxis(ref, axis, 0).reshape(n, -1)
    ratios, misses = [], []
    for i in range(n):
        scale, err = np.abs(r[i]).max(), np.abs(g[i] - r[i]).max()
        allow = rtol * scale + (atol_rel * float(input_scale[i]) if input_scale is not None else 0.0)
        ratio = 0.0 if err == 0.0 else (err / allow if allow > 0.0 else np.inf)
        ratios.append(float(ratio))
        if ratio > 1.0:
            misses.append("%s[%d]: max err %.3e, allowed %.3e (slice scale %.3e)" % (name, i, err, allow, scale))
    assert not misses, misses
    return ratios


def max_norm_close(got, ref, rtol):
    """The whole-array form (test_gpu_backward._close): max|got - ref| <= rtol max|ref| -> error / allowance."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / (rtol * max(np.abs(ref).max(), 1e-12)))


# ------------------------------------------------------------------------------------------------------------------------------------
# the tables: one place for the host test (bounds and liveness of every case) and the GPU test
# ------------------------------------------------------------------------------------------------------------------------------------
# A: published constants and the switch -- (M, D); every shape at both geometries, offset 10.  D = 2 takes the float64 stage-1 route.
SHAPES_A = [(32, 4), (100, 5), (128, 8), (96, 12), (250, 8), (64, 2)]

# B: the forward on both sides of the switch, off-centre -- (M, D, geometry, offset, kernel).  The full cross product for (32, 4) and
# (128, 8); for every other shape a diagonal through geometry x offset x kernel that shows both geometries, both kernels and both
# non-zero offsets
_G, _K = ("compact", "spread"), ("rbf", "matern52")
CASES_B = [(M, D, g, o, k) for M, D in ((32, 4), (128, 8)) for g in _G for o in (0, 10, 30) for k in _K]
CASES_B += [(48, 8, "compact", 10, "matern52"), (48, 8, "spread", 30, "rbf"), (48, 8, "compact", 0, "rbf"),
            (100, 5, "compact", 30, "rbf"), (100, 5, "spread", 10, "matern52"), (100, 5, "spread", 0, "rbf"),
            (96, 12, "compact", 10, "rbf"), (96, 12, "spread", 30, "matern52"), (96, 12, "spread", 10, "rbf"), (96, 12, "compact", 0, "matern52"),
            (250, 8, "compact", 10, "matern52"), (250, 8, "spread", 10, "rbf"), (250, 8, "spread", 30, "matern52"), (250, 8, "compact", 30, "rbf"),
            (64, 2, "compact", 10, "rbf"), (64, 2, "spread", 30, "matern52"), (64, 2, "spread", 10, "rbf"), (64, 2, "compact", 30, "matern52")]
R_B = 2

# C: heterogeneous operand scales -- R = 4 latent GPs, compact, offset 0, D = 8
M_C, D_C = (32, 128, 256), 8
Q_FORWARD = (1.0, 2.0 ** -17, 30.0, 0.0)          # the last latent GP has q_sqrt exactly 0: forward only (log diag is infinite in the KL)
Q_ADJOINT = (1.0, 2.0 ** -17, 30.0, 1e-5)
QMU_HETERO = (1.0, 1e-4, 1e3, 0.0)
QMU_ZERO = (0.0, 0.0, 0.0, 0.0)

# D: the adjoint at the same edges -- (id, M, D, T, geometry, offset, q_scales, qmu_scales, kernel).  T = 80 where the shape can take the
# streaming chain (M a multiple of 16), T = 70 on the GEMM path of the padded shape
_ONES = (1.0, 1.0, 1.0, 1.0)
CASES_D = [("spread-m32", 32, 4, T_CHAIN, "spread", 10, _ONES, _ONES, "rbf"),
           ("spread-m128", 128, 8, T_CHAIN, "spread", 10, _ONES, _ONES, "matern52"),
           ("spread-m100", 100, 5, T_ROWS, "spread", 10, _ONES, _ONES, "rbf"),
           ("spread-m256", 256, 8, T_CHAIN, "spread", 10, _ONES, _ONES, "rbf"),
           ("hetero-m32", 32, 4, T_CHAIN, "compact", 0, Q_ADJOINT, QMU_HETERO, "rbf"),
           ("hetero-m128", 128, 8, T_CHAIN, "compact", 0, Q_ADJOINT, QMU_HETERO, "rbf"),
           ("hetero-m100", 100, 5, T_ROWS, "compact", 0, Q_ADJOINT, QMU_HETERO, "matern52"),
           ("hetero-m256", 256, 8, T_CHAIN, "compact", 0, Q_ADJOINT, QMU_HETERO, "rbf"),
           ("both-m128", 128, 8, T_CHAIN, "spread", 10, Q_ADJOINT, QMU_HETERO, "rbf")]
R_D = 4
MOVES_D = [(32, 4), (128, 8), (256, 8)]            # the scale moves: shapes with an even block count (the state then carries the scales)

# E: a device-resident kernel variance against a stale host copy of 1.0 -- (M, device value); D = 8
CASES_E = [(M, v) for M in (64, 256) for v in (0.02, 60.0)]
D_E, R_E = 8, 2


# the fetches of ZtP from L2: stacks whose Z~ images cannot all be staged -- (id, layers, M, D, geometry, kernel, fetch).  The LDS image of
# a launch holds at least its staged Z~ images (16 ceil((D + 2) / 4) M bytes per layer), one [Mp x 16] float32 tile, three [16 x
# (D + 2 rounded up to 4, + 1)] activation tiles and every layer's constant block with the inner layers' W [D, 2] and A [D, D] (csrc/
# dgp_forward.hip: fw_plan_lds); beyond 160 KiB the plan reads every layer's ZtP from L2 (plan_fit).
# M > 128 and at most three sub-tiles: the expanded form prefetches it; the direct form reads it in place.  (The expanded form's plain
# read needs an overflowing stack of M <= 128 layers, or four sub-tiles and more at M > 128: eight layers of D >= 28, where rows drawn
# 0.3 l from the cloud are no longer live -- |a|^2 / variance falls to 0.03 at M = 128, D = 32 -- or T > 12288.  Not in the table.)
CASES_L2 = [("m512-compact-rbf", 4, 512, 12, "compact", "rbf", "prefetched"), ("m512-compact-matern52", 4, 512, 12, "compact", "matern52", "prefetched"),
            ("m512-spread-rbf", 4, 512, 12, "spread", "rbf", "direct"), ("m512-spread-matern52", 4, 512, 12, "spread", "matern52", "direct")]
LDS_MAX = 160 * 1024


def staged_image_floor(L, M, D, T_tile=16):
    """A lower bound, in bytes, of the LDS image of an L-layer stack with every Z~ image staged (see CASES_L2)."""
    Mp, w = (M + 15) // 16 * 16, (D + 2 + 3) // 4 * 4
    return L * (Mp // 16) * (w // 4) * 64 * 4 + Mp * T_tile * 4 + 3 * T_tile * (w + 1) * 4 + L * 104 * 4 + (L - 1) * (2 * D + D * D) * 4


def case_seed(M, D):
    return 100 * M + D
