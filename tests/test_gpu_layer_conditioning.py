"""The GP layer where its packed state adapts to the data (tests/conditioning_cases.py): the inducing cloud compact (``zmax2`` <= 3: the
expanded MFMA form of K_uf) and spread (>= 8: the direct-difference form), 0 / 10 / 30 lengthscales away from the origin, latent GPs
whose q_sqrt and q_mu differ by many powers of two (one of them exactly zero), and a kernel variance that lives on the device while the
host copy is stale -- forward and adjoint against the float64 oracle and float64 autograd.

The float64 references are evaluated on ``rows - shift`` with ``Z - shift`` (conditioning_cases.centred_layer): the same function for a
stationary kernel, without the cancellation of the oracle's own expanded square distance 30 lengthscales out.

Part A  the constant block of the state (1 / l, zc, zeros beyond D, zmax2 within 4 float32 ulp and on the promised side of 4.0) and the
        factorisation's residuals at offset 10.
Part B  ``GPLayer.propagate`` as one layer call, and the same layer as layer 1 of a fused two-layer forward, where the first layer's
        epilogue builds x~ -- the second implementation of the centring.  Mean rtol 2e-3 + atol 1e-3, variance rtol 2e-3 + atol 1e-4,
        sample rtol 2e-3 + atol 2e-3 (test_gpu_parity.py), unchanged.
Part C  q_sqrt scales (1, 2^-17, 30, 0) and q_mu scales (1, 1e-4, 1e3, 0): every latent GP's mean and variance against that column's own
        max|reference| at rtol 2e-3, the zero columns exact, the KL shares of the proper columns at rtol 1e-6; and q_mu all zero.
Part D  the adjoint (max-norm relative 3e-3 per array, test_gpu_backward.py; dq_mu and dq_sqrt per latent GP) at spread / offset 10,
        at the scales of C, and both; IWVI_BW_OWN_QSCALE on a state whose scales are stale and IWVI_GP_REUSE_FACTOR after the same move,
        bit for bit against a fresh precompute.
Part E  a bound device variance of 0.02 / 60 under a host copy of 1.0 (scale exponents -2 / +3 away): the fused forward and the adjoint
        against the oracle at the device value, and bit for bit what the run with a matching host copy gives.  (``GPLayer.propagate``
        hands the host copy over by value and is not part of E: its contract is that the owner marks a moved device value.)

Forward variants reached at T = 70 (iwvi_debug_last_forward_variant, asserted per case): one sub-tile per workgroup; split-f16 stage 2 and
solve at an even block count (M = 32, 96, 128), the fp32 variant at an odd one (M = 48, 100), the super-block solve with split-f16 dense
part (M = 250), the float64 stage-1 route (D = 2) -- each with compact and spread geometry and with RBF and Matern52.  Every stack of
these shapes fits the LDS with its Z~ images staged, so K_uf reads ZtP from LDS in both forms there.  The fetches from L2 need a stack
whose images overflow 160 KiB: four layers of M = 512, D = 12 (conditioning_cases.CASES_L2) reach the expanded form's prefetch and the
direct form's read in place, both kernels each.  NOT reached: the expanded form's plain L2 read (an overflowing stack of M <= 128
layers -- eight layers of D >= 28, where rows 0.3 l from the cloud are not live -- or T > 12288 at M > 128) and the column-at-a-time
solve (128 < M <= 240: not among the shapes; test_gpu_parity.py runs it at the origin).  The float64 route reads the plain z~ image of
the state from global memory whatever the stack.

Observed on an MI355X, worst error / tolerance per family (every case prints its own line):
A  cst[0:D], cst[32:32+D] equal, zmax2 <= 0.5 float32 ulp from the float64 value (bound 4); |Lm Lm^T - K_uu| <= 5.1e-15 (1e-12),
   |Lm^-1 Lm - I| <= 3.1e-12 (1e-7, the D = 2 layer; <= 9.7e-14 elsewhere).
B  one layer call -- compact, offset 0: mean 4.9e-3, variance 3.1e-4, sample 3.9e-3 of the tolerance; compact, offset 10 / 30: mean 1.0e-1
   (M = 250, offset 30, RBF), variance 6.2e-4, sample 5.0e-2; spread, offset 0: 5.6e-4, 3.7e-4, 4.4e-4; spread, offset 10 / 30: 2.9e-3,
   5.7e-4, 1.8e-3; KL 2.2e-10 of rtol 1e-6.  Layer 1 of the fused forward -- compact, offset 0: 5.6e-3, 3.1e-4, 3.6e-3; compact, offset
   10 / 30: 4.2e-2, 6.1e-4, 3.2e-2; spread, offset 0: 5.3e-4, 3.0e-4, 5.6e-4; spread, offset 10 / 30: 3.8e-3, 3.8e-4, 1.9e-3; its first
   layer <= 6.1e-4.  ZtP from L2, final layer -- prefetched: 2.1e-2, 5.1e-4, 2.7e-2; direct form: 6.4e-4, 2.2e-4, 3.3e-4; the layers in
   front of it <= 3.0e-3.
C  error / (2e-3 x the column's max), columns (1, 1e-4 | 2^-17, 1e3 | 30, 0): mean M = 32: 3.2e-4, 1.8e-2, 2.4e-4, 0 (fp32 stage 2: 2.4e-4,
   2.0e-4, 1.9e-4, 0); M = 128: 9.5e-4, 2.9e-2, 3.4e-3, 0 (9.6e-4, 1.4e-3, 3.3e-3, 0); M = 256: 1.5e-2, 2.7e-2, 1.4e-2, 0 (7.1e-3, 1.2e-2,
   4.9e-3, 0); variance <= 3.0e-3, sample <= 1.4e-2 in every column of both variants.  q_mu all zero: mean 0, variance 6.3e-4, sample
   1.8e-4 of the tolerance, KL 4.3e-8 of rtol 1e-6.
D  error / (3e-3 x max-norm; dq_mu, dq_sqrt per latent GP): dF 7.8e-3, dZ 1.4e-2, dls 4.8e-2, dvariance 6.7e-3, dq_mu 8.0e-3, dq_sqrt 7.5e-3;
   the saved forward per column (2e-3): mean 3.6e-2, variance 3.1e-3.  IWVI_BW_OWN_QSCALE and IWVI_GP_REUSE_FACTOR: identical bits.
E  mean 5.3e-2, variance 5.9e-4, sample 2.6e-2 of the tolerance scaled by sigma / sigma^2, KL 1.6e-10 of 1e-6; dF 1.0e-2, dZ 1.8e-2, dls 5.8e-3,
   dvariance 1.9e-2, dq_mu 6.6e-3, dq_sqrt 1.1e-2 of 3e-3; identical bits under either host copy.
With a library whose forward reads cst[IWVI_CST_FR] for every latent GP, part C fails in the default variant (variance of the 2^-17
column off by 1.0 against 5e-4 .. 1.5e-3 allowed, of the 30 column by 9e2 against 1.8) and with it the heterogeneous cases of D; with
the centre left out of the x~ that a layer's epilogue builds for the next one, every fused case of B fails (mean 60 - 770 x the tolerance at
offset 0, 370 - 430 x at offsets 10 and 30) and every one-layer call passes; with the RBF constant for Matern52 in the direct form, the
spread Matern52 cases of B fail (mean 700 - 1800 x the tolerance) except on the float64 route, which forms its own Gram; with the values
that K_uf takes from L2 (the prefetched steps, the direct form's read in place) 1 % too large, the four M = 512 stacks fail (final mean
14 - 21 x the tolerance) and nothing else does: they, and only they, read ZtP from L2.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_reference as ar   # noqa: E402
import conditioning_cases as cc   # noqa: E402
from oracle import iwvi_oracle as O   # noqa: E402

pytestmark = pytest.mark.gpu

MEAN_TOL = dict(rtol=2e-3, atol=1e-3)             # test_gpu_parity.py
VAR_TOL = dict(rtol=2e-3, atol=1e-4)
SAMPLE_TOL = dict(rtol=2e-3, atol=2e-3)
COLUMN_RTOL = 2e-3
KL_RTOL = 1e-6
CST_SA, CST_FMEAN, CST_FR, CST_FLOATS = 65, 66, 72, 104      # csrc/iwvi_common.h


@functools.lru_cache(maxsize=None)
def _case(*args, **kw):
    """A case of the tables -- built once, shared, never written to."""
    c = cc.conditioned_case(*args, **kw)
    for a in (c.F, c.z, c.cs, c.cm, c.cv):
        a.setflags(write=False)
    return c


def _b_case(M, D, geometry, offset, kern):
    return _case(M, D, cc.R_B, geometry, offset, None, None, kern, seed=cc.case_seed(M, D))


@functools.lru_cache(maxsize=None)
def _forward_reference(key):
    c = _case(*key[0], **dict(key[1]))
    out = cc.reference_layer(cc.centred_layer(c), cc.centred_rows(c), c.z)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _key(*args, **kw):
    return (args, tuple(sorted(kw.items())))


def _t(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)


def _np(t):
    return t.detach().double().cpu().numpy()


def _model(c, dev):
    """The device model of the case's spec, the layers marked ``kern = "matern52"`` with that kernel."""
    from dgps_with_iwvi_amd import kernels, synthetic
    model = synthetic.build_model(c.spec, dev)
    for lay, layer in zip(c.spec["layers"], model.layers):
        if lay.get("kern") == "matern52":
            old = layer._base_kern()
            new = kernels.Matern52(old.input_dim, variance=old.variance, lengthscales=old.lengthscales, ARD=True).to(dev)
            if hasattr(layer.kern, "kernel"):
                layer.kern.kernel = new
            else:
                layer.kern = new
    return model


def _ratio(got, ref, rtol, atol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def _moments_ratios(s, m, v, so, mo, vo, sd=1.0):
    """error / tolerance of sample, mean, variance at the stated tolerances, the absolute parts scaled by sigma / sigma^2."""
    return dict(mean=_ratio(m, mo, MEAN_TOL["rtol"], MEAN_TOL["atol"] * sd), var=_ratio(v, vo, VAR_TOL["rtol"], VAR_TOL["atol"] * sd * sd),
                sample=_ratio(s, so, SAMPLE_TOL["rtol"], SAMPLE_TOL["atol"] * sd))


def _report(family, cid, ratios):
    print("layer-conditioning %s %s: " % (family, cid) + " ".join("%s=%.1e" % kv for kv in ratios.items()))
    assert all(r <= 1.0 for r in ratios.values()), (family, cid, {k: r for k, r in ratios.items() if r > 1.0})


def _variant():
    from dgps_with_iwvi_amd import _abi
    w = _abi.lib().iwvi_debug_last_forward_variant()
    return dict(ns=w & 0xff, s16=bool(w >> 8 & 1), big=bool(w >> 9 & 1), f64=bool(w >> 12 & 1))


def _expected_variant(M, D, f32=False):
    """What the plan gives a T <= 4096 call on layers of M inducing points and D inputs (csrc/dgp_forward.hip: plan_check_call, choose_variant)."""
    nbk, f64 = (M + 15) // 16, D <= 3
    return dict(ns=1, s16=(nbk % 2 == 0) and not f64 and not f32, big=nbk > 8 or f64, f64=f64)


def _cst(layer):
    st = layer.state()
    return st.view("cst", torch.float32, CST_FLOATS).cpu().numpy().copy()


def _cst_written(cst, R):
    """The entries of a constant block that a precompute writes: 1 / l, zc, zmax2 and the five scales, then one scale per latent GP (the
    pad words keep whatever the buffer held)."""
    return np.concatenate([cst[:69], cst[CST_FR:CST_FR + R]])


# ------------------------------------------------------------------------------------------------------------------------------------
# A: published constants and the switch
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["compact", "spread"])
@pytest.mark.parametrize("M,D", cc.SHAPES_A)
def test_published_constants_and_the_side_of_the_switch(gpu_device, M, D, geometry):
    c = _b_case(M, D, geometry, 10, "rbf")
    layer = _model(c, gpu_device).layers[c.li]
    layer.precompute()
    torch.cuda.synchronize()
    cst = _cst(layer)
    invls, zc, zmax2 = cc.expected_constants(c.spec, c.li)
    assert np.array_equal(cst[:D], invls.astype(np.float32)), (cst[:D], invls)
    assert np.array_equal(cst[32:32 + D], zc.astype(np.float32)), (cst[32:32 + D], zc)
    assert not cst[D:32].any() and not cst[32 + D:64].any()
    ulp = float(np.spacing(np.float32(zmax2)))
    assert abs(float(cst[64]) - zmax2) <= 4 * ulp, (float(cst[64]), zmax2)
    assert (float(cst[64]) <= 4.0) == (geometry == "compact")
    assert np.all(np.abs(zc - 10.0) < 0.5)                       # the centre is the offset, in lengthscale units
    # the factorisation of the Gram of exactly these centred values (test_gpu_parity.py: test_precompute_factorisation)
    st, lay = layer.state(), c.spec["layers"][c.li]
    Zs = cc.scaled_centred(lay["Z"], lay["ls"])[2]
    Kuu = O.RBF(D, variance=float(np.float32(lay["var"])), lengthscales=1.0).K(Zs) + 1e-6 * np.eye(M)
    Lm, Linv = _np(st.Lm), _np(st.Linv)
    assert np.all(np.triu(Lm, 1) == 0) and np.all(np.triu(Linv, 1) == 0)
    np.testing.assert_allclose(Lm @ Lm.T, Kuu, rtol=0, atol=1e-12)
    np.testing.assert_allclose(Linv @ Lm, np.eye(M), atol=1e-7)
    np.testing.assert_allclose(float(st.kl.item()), O.gauss_kl(lay["q_mu"], lay["q_sqrt"]), rtol=KL_RTOL)
    print("layer-conditioning A M%d-D%d-%s: zmax2=%.4f (float64 %.4f, %.1f ulp) |Lm Lm^T - Kuu|=%.1e |Linv Lm - I|=%.1e"
          % (M, D, geometry, cst[64], zmax2, abs(float(cst[64]) - zmax2) / ulp, np.abs(Lm @ Lm.T - Kuu).max(), np.abs(Linv @ Lm - np.eye(M)).max()))


# ------------------------------------------------------------------------------------------------------------------------------------
# B: the forward on both sides of the switch, off-centre
# ------------------------------------------------------------------------------------------------------------------------------------
_B_IDS = ["M%d-D%d-%s-off%d-%s" % r for r in cc.CASES_B]


@pytest.mark.parametrize("M,D,geometry,offset,kern", cc.CASES_B, ids=_B_IDS)
def test_one_layer_call_on_both_sides_of_the_switch(gpu_device, M, D, geometry, offset, kern):
    c = _b_case(M, D, geometry, offset, kern)
    layer = _model(c, gpu_device).layers[c.li]
    s, m, v, kl = layer.propagate(_t(c.F, gpu_device), z=_t(c.z, gpu_device))
    torch.cuda.synchronize()
    assert _variant() == _expected_variant(M, D)
    assert (float(_cst(layer)[64]) <= 4.0) == (geometry == "compact")            # the side that ran
    so, mo, vo, klo = _forward_reference(_key(M, D, cc.R_B, geometry, offset, None, None, kern, seed=cc.case_seed(M, D)))
    ratios = _moments_ratios(_np(s), _np(m), _np(v), so, mo, vo)
    ratios["kl"] = abs(float(kl.item()) - klo) / (KL_RTOL * abs(klo))
    _report("B-layer", _B_IDS[cc.CASES_B.index((M, D, geometry, offset, kern))], ratios)


@pytest.mark.parametrize("M,D,geometry,offset,kern", cc.CASES_B, ids=_B_IDS)
def test_layer_one_of_a_fused_forward_on_both_sides_of_the_switch(gpu_device, M, D, geometry, offset, kern):
    """The layer under test reads the x~ that the first layer's epilogue left for it.  Its reference is the float64 conditional at the
    rows the device's first layer actually handed on (so the comparison holds this layer alone to the stated tolerances); the first
    layer's own outputs are held to the same tolerances against the oracle, and the rows are live by the reference alone."""
    c = _b_case(M, D, geometry, offset, kern)
    T = len(c.F)
    model = _model(c, gpu_device)
    z0 = cc.first_layer_noise(c)
    model.precompute()
    _, outs, _ = model._fused_forward(T, 1, T, (T,), zs=[_t(z0, gpu_device), _t(c.z, gpu_device)], want_layers=True, want_logw=False)
    torch.cuda.synchronize()
    assert _variant() == _expected_variant(M, D)
    s0o, m0o, v0o = cc.first_layer_reference(c, z0)
    live, a2 = cc.liveness(c, s0o)
    assert live >= 0.8 and a2 > 0.1, (live, a2)
    s0, m0, v0 = (_np(outs[0][k]) for k in ("sample", "mean", "var"))
    first = {"first-" + k: r for k, r in _moments_ratios(s0, m0, v0, s0o, m0o, v0o).items()}
    so, mo, vo, _ = cc.reference_layer(cc.centred_layer(c), cc.centred_rows(c, s0), c.z)
    ratios = _moments_ratios(*(_np(outs[1][k]) for k in ("sample", "mean", "var")), so, mo, vo)
    _report("B-fused", _B_IDS[cc.CASES_B.index((M, D, geometry, offset, kern))], dict(ratios, **first))


_L2_BY_ID = {r[0]: r for r in cc.CASES_L2}


@pytest.mark.parametrize("cid", [r[0] for r in cc.CASES_L2])
def test_final_layer_of_a_stack_whose_inducing_images_stay_in_l2(gpu_device, cid):
    """Four M = 512, D = 12 layers: their Z~ images cannot all be staged beside the solve's tile (conditioning_cases.staged_image_floor), so
    every layer's K_uf reads ZtP from L2 -- the expanded form through its prefetch (three steps ahead, the fourth in place), the direct form
    in place.  The layer under test is the last one; every layer is held to the stated tolerances against the float64 conditional at the
    rows the device's previous layer handed on."""
    _, L, M, D, geometry, kern, fetch = _L2_BY_ID[cid]
    assert cc.staged_image_floor(L, M, D) > cc.LDS_MAX
    c = _case(M, D, cc.R_B, geometry, 0, None, None, kern, seed=cc.case_seed(M, D), L=L)
    T = len(c.F)
    model = _model(c, gpu_device)
    zs = cc.inner_noise(c) + [c.z]
    model.precompute()
    _, outs, _ = model._fused_forward(T, 1, T, (T,), zs=[_t(z, gpu_device) for z in zs], want_layers=True, want_logw=False)
    torch.cuda.synchronize()
    assert _variant() == dict(ns=1, s16=True, big=True, f64=False)
    assert (float(_cst(model.layers[c.li])[64]) <= 4.0) == (geometry == "compact")
    live, a2 = cc.liveness(c, cc.handed_on_reference(c))
    assert live >= 0.8 and a2 > 0.1, (live, a2)
    rows, ratios = c.spec["X"][:T], {}
    for i in range(c.li):
        so, mo, vo = cc.inner_layer_reference(c, i, rows, zs[i])
        got = [_np(outs[i][k]) for k in ("sample", "mean", "var")]
        ratios.update({"l%d-%s" % (i, k): r for k, r in _moments_ratios(*got, so, mo, vo).items()})
        rows = got[0]
    so, mo, vo, _ = cc.reference_layer(cc.centred_layer(c), cc.centred_rows(c, rows), c.z)
    ratios.update(_moments_ratios(*(_np(outs[c.li][k]) for k in ("sample", "mean", "var")), so, mo, vo))
    _report("B-l2-" + fetch, cid, ratios)


# ------------------------------------------------------------------------------------------------------------------------------------
# C: heterogeneous operand scales
# ------------------------------------------------------------------------------------------------------------------------------------
def _propagate(layer, c, dev, f32):
    from dgps_with_iwvi_amd import settings
    old, settings.fw_f32_stage2 = settings.fw_f32_stage2, bool(f32)
    try:
        s, m, v, _ = layer.propagate(_t(c.F, dev), z=_t(c.z, dev))
        torch.cuda.synchronize()
    finally:
        settings.fw_f32_stage2 = old
    return _np(s), _np(m), _np(v)


@pytest.mark.parametrize("f32", [False, True], ids=["default", "fp32-stage2"])
@pytest.mark.parametrize("M", cc.M_C)
def test_forward_with_a_scale_of_its_own_per_latent_gp(gpu_device, M, f32):
    """q_sqrt scales (1, 2^-17, 30, 0), q_mu scales (1, 1e-4, 1e3, 0).  The one scale 2^eq of the whole q_mu matrix is set by the 1e3
    column: the 1e-4 column's f16 planes then hold seven orders of magnitude less, which its split h1 + h2 still carries -- measured
    against float64, relative to the column's own max: 3.6e-5 (M = 32), 5.8e-5 (128), 5.4e-5 (256) in the default variant, 4.0e-7, 2.8e-6, 2.4e-5
    with the fp32-MFMA stage 2 (which reads the unscaled float32 q_mu) -- 3 % of the rtol 2e-3 it is held to, per column."""
    c = _case(M, cc.D_C, 4, "compact", 0, cc.Q_FORWARD, cc.QMU_HETERO, "rbf", seed=cc.case_seed(M, cc.D_C))
    layer = _model(c, gpu_device).layers[c.li]
    s, m, v = _propagate(layer, c, gpu_device, f32)
    assert _variant() == _expected_variant(M, cc.D_C, f32)
    cst, lay = _cst(layer), c.spec["layers"][c.li]
    # the published scales: a different exponent for every latent GP (csrc/precompute_dev.h: e_r = 13 - ilogb(max|tril L_r|), 0 for a zero matrix)
    er = [13 - int(np.floor(np.log2(np.abs(np.tril(L)).max()))) if L.any() else 0 for L in lay["q_sqrt"]]
    ea = -np.log2(cst[CST_FR:CST_FR + 4].astype(np.float64)) - np.array(er)
    assert len(set(er)) == 4 and np.all(ea == ea[0]) and float(ea[0]).is_integer(), (er, ea)
    eq = 13 - int(np.floor(np.log2(np.abs(lay["q_mu"]).max())))
    assert -np.log2(float(cst[CST_FMEAN])) == ea[0] + eq and cst[CST_SA] == 2.0 ** ea[0]
    so, mo, vo, _ = _forward_reference(_key(M, cc.D_C, 4, "compact", 0, cc.Q_FORWARD, cc.QMU_HETERO, "rbf", seed=cc.case_seed(M, cc.D_C)))
    rm = cc.per_column_close(m, mo, 1, COLUMN_RTOL, name="mean")
    rv = cc.per_column_close(v, vo, 1, COLUMN_RTOL, name="var")
    rs = cc.per_column_close(s, so, 1, COLUMN_RTOL, name="sample")
    assert not m[:, 3].any()                                     # q_mu[:, 3] = 0, no mean function: exactly zero
    # q_sqrt[3] = 0: var = variance - |a|^2, the oracle's column with no q(u) covariance term
    a2 = (cc.solve_a(cc.centred_layer(c), cc.centred_rows(c)) ** 2).sum(0)
    np.testing.assert_allclose(vo[:, 3], float(lay["var"]) - a2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(v[:, 3], float(lay["var"]) - a2, **VAR_TOL)
    # the KL shares of the proper latent GPs; the zero q_sqrt has none (log diag)
    kl = layer.state().kl_parts.cpu().numpy()
    for r in range(3):
        np.testing.assert_allclose(kl[r], O.gauss_kl(lay["q_mu"][:, r:r + 1], lay["q_sqrt"][r:r + 1]), rtol=KL_RTOL)
    assert np.isinf(kl[3]) and kl[3] > 0
    print("layer-conditioning C M%d-%s: err / (2e-3 column max) mean=%s var=%s sample=%s"
          % (M, "fp32" if f32 else "default", *(" ".join("%.1e" % x for x in r) for r in (rm, rv, rs))))


@pytest.mark.parametrize("M", cc.M_C)
def test_forward_with_q_mu_all_zero(gpu_device, M):
    """The value every model starts from: max|q_mu| = 0 takes the zero guard of the matrix scale (eq = 0)."""
    c = _case(M, cc.D_C, 4, "compact", 0, None, cc.QMU_ZERO, "rbf", seed=cc.case_seed(M, cc.D_C))
    layer = _model(c, gpu_device).layers[c.li]
    so, mo, vo, klo = _forward_reference(_key(M, cc.D_C, 4, "compact", 0, None, cc.QMU_ZERO, "rbf", seed=cc.case_seed(M, cc.D_C)))
    assert not mo.any()
    for f32 in (False, True):
        s, m, v = _propagate(layer, c, gpu_device, f32)
        assert _variant() == _expected_variant(M, cc.D_C, f32)
        assert not m.any()
        cst = _cst(layer)
        assert cst[CST_FMEAN] == 1.0 / cst[CST_SA]               # 2^-(ea + 0)
        ratios = _moments_ratios(s, m, v, so, mo, vo)
        ratios["kl"] = abs(float(layer.state().kl.item()) - klo) / (KL_RTOL * abs(klo))
        _report("C-zero-q_mu", "M%d-%s" % (M, "fp32" if f32 else "default"), ratios)


# ------------------------------------------------------------------------------------------------------------------------------------
# D: the adjoint at the same edges
# ------------------------------------------------------------------------------------------------------------------------------------
_D_BY_ID = {r[0]: r for r in cc.CASES_D}


def _d_case(cid):
    _, M, D, T, geometry, offset, q, qmu, kern = _D_BY_ID[cid]
    return _case(M, D, cc.R_D, geometry, offset, q, qmu, kern, seed=cc.case_seed(M, D), T=T)


@functools.lru_cache(maxsize=None)
def _adjoint_reference(key):
    c = _case(*key[0], **dict(key[1]))
    return ar.layer_reference(cc.centred_spec(c), c.li, cc.centred_rows(c), c.z, c.cs, c.cm, c.cv, ar.KL_WEIGHT,
                              kern="matern52" if c.kern == "matern52" else None)


def _adjoint_ratios(out, ref):
    """error / tolerance of every gradient array: dF, dZ, dls, dvariance in the max-norm of the array (test_gpu_backward._close), dq_mu
    and dq_sqrt per latent GP."""
    r = {k: cc.max_norm_close(_np(out["d" + k]), ref[k], ar.RTOL) for k in ("F", "Z", "ls")}
    r["variance"] = cc.max_norm_close(_np(out["dvariance"])[0], ref["var"], ar.RTOL)
    misses = []
    for name, got, want, axis in (("q_mu", _np(out["dq_mu"]), ref["q_mu"], 1), ("q_sqrt", _np(out["dq_sqrt"]), np.tril(ref["q_sqrt"]), 0)):
        try:
            r[name] = max(cc.per_column_close(got, want, axis, ar.RTOL, name="d" + name))
        except AssertionError as e:
            misses.append(str(e))
            r[name] = np.inf
    assert float(torch.triu(out["dq_sqrt"], 1).abs().max()) == 0.0
    return r, misses


def _run_adjoint(layer, c, dev, prepared=None, saved=None):
    from dgps_with_iwvi_amd import backward
    saved = backward.gp_forward_saved(layer, _t(c.F, dev), _t(c.z, dev)) if saved is None else saved
    out = backward.gp_backward(layer, saved, _t(c.cs, dev), _t(c.cm, dev), _t(c.cv, dev), kl_weight=ar.KL_WEIGHT, prepared=prepared)
    torch.cuda.synchronize()
    return saved, out


@pytest.mark.parametrize("cid", [r[0] for r in cc.CASES_D])
def test_adjoint_at_the_edges_of_the_packed_state(gpu_device, cid):
    from dgps_with_iwvi_amd import _abi
    _, M, D, T, geometry, offset, q, qmu, kern = _D_BY_ID[cid]
    c = _d_case(cid)
    layer = _model(c, gpu_device).layers[c.li]
    _abi.backward_routes()                                       # (empties the log)
    saved, out = _run_adjoint(layer, c, gpu_device)
    routes = _abi.backward_routes()
    assert len(routes) == 1 and routes[0][0] == (_abi.BW_ROUTE_CHAIN if T % 16 == 0 else _abi.BW_ROUTE_GEMM), routes
    assert (float(_cst(layer)[64]) <= 4.0) == (geometry == "compact")
    ref = _adjoint_reference(_key(M, D, cc.R_D, geometry, offset, q, qmu, kern, seed=cc.case_seed(M, D), T=T))
    ratios, misses = _adjoint_ratios(out, ref)
    # the saved forward against the same reference's conditional
    so, mo, vo, _ = _forward_reference(_key(M, D, cc.R_D, geometry, offset, q, qmu, kern, seed=cc.case_seed(M, D), T=T))
    ratios["fw-mean"] = max(cc.per_column_close(_np(saved.mean), mo, 1, COLUMN_RTOL, name="mean"))
    ratios["fw-var"] = max(cc.per_column_close(_np(saved.var), vo, 1, COLUMN_RTOL, name="var"))
    print("layer-conditioning D route", routes[0])
    assert not misses, misses
    _report("D", cid, ratios)


def _dense_precompute(layer, state):
    from dgps_with_iwvi_amd import _abi
    from dgps_with_iwvi_amd.temp_workaround import precompute_states
    d = layer.state_desc(state=state)
    d.flags |= _abi.GP_WANT_DENSE
    precompute_states([d])


@pytest.mark.parametrize("batched", [False, True], ids=["k_pack_bw", "k_prepare_all"])
@pytest.mark.parametrize("M,D", cc.MOVES_D)
def test_own_qscale_on_a_state_with_stale_scales(gpu_device, M, D, batched):
    """Precompute at q scales (1, 1, 1, 1), move q to the scales of C without a precompute, prepare the adjoint with IWVI_BW_OWN_QSCALE on
    the stale state: every gradient equals, bit for bit, what a fresh precompute and a plain prepare give."""
    from dgps_with_iwvi_amd import _abi, backward
    dev, seed = gpu_device, cc.case_seed(M, D)
    c1 = _case(M, D, cc.R_D, "compact", 0, cc._ONES, cc._ONES, "rbf", seed=seed, T=cc.T_CHAIN)
    c2 = _case(M, D, cc.R_D, "compact", 0, cc.Q_ADJOINT, cc.QMU_HETERO, "rbf", seed=seed, T=cc.T_CHAIN)
    assert np.array_equal(c1.F, c2.F) and np.array_equal(c1.spec["layers"][1]["Z"], c2.spec["layers"][1]["Z"])
    layer = _model(c1, dev).layers[c1.li]
    dense = layer.state_dense()
    _dense_precompute(layer, dense)                               # the scales of q at (1, 1, 1, 1)
    stale = _cst_written(dense.view("cst", torch.float32, CST_FLOATS).cpu().numpy().copy(), cc.R_D)
    lay2 = c2.spec["layers"][c2.li]
    layer.q_mu, layer.q_sqrt = _t(lay2["q_mu"], dev), _t(lay2["q_sqrt"], dev)
    saved = backward.gp_forward_saved(layer, _t(c2.F, dev), _t(c2.z, dev))        # (the forward's own state: a precompute of the moved q)
    T = len(c2.F)
    ws = backward._workspace(layer, T, D, dev)
    backward._pack_operands([(1, layer)], {1: (ws, dense)}, T, batched=batched, flags=_abi.BW_OWN_QSCALE)
    _abi.backward_routes()
    _, own = _run_adjoint(layer, c2, dev, prepared=(ws, dense), saved=saved)
    routes = _abi.backward_routes()
    assert len(routes) == 1 and routes[0][0] == _abi.BW_ROUTE_CHAIN, routes      # the route whose split-f16 images carry the scales
    assert np.array_equal(_cst_written(dense.view("cst", torch.float32, CST_FLOATS).cpu().numpy(), cc.R_D), stale)      # nothing refreshed the state meanwhile
    _dense_precompute(layer, dense)
    fresh = _cst_written(dense.view("cst", torch.float32, CST_FLOATS).cpu().numpy().copy(), cc.R_D)
    assert fresh[69] == stale[69] and np.all(fresh[70:73] != stale[70:73]) and fresh[CST_FMEAN] != stale[CST_FMEAN]      # the scales did move
    ws2 = backward._workspace(layer, T, D, dev)
    backward._pack_operands([(1, layer)], {1: (ws2, dense)}, T, batched=batched, flags=0)
    _, plain = _run_adjoint(layer, c2, dev, prepared=(ws2, dense), saved=saved)
    for k in plain:
        assert torch.equal(own[k], plain[k]), k
    # and they are the right gradients
    ref = _adjoint_reference(_key(M, D, cc.R_D, "compact", 0, cc.Q_ADJOINT, cc.QMU_HETERO, "rbf", seed=seed, T=cc.T_CHAIN))
    ratios, misses = _adjoint_ratios(own, ref)
    assert not misses, misses
    _report("D-own-qscale", "M%d-%s" % (M, "batched" if batched else "single"), ratios)


@pytest.mark.parametrize("M,D", cc.MOVES_D)
def test_reuse_factor_after_a_move_of_the_scales(gpu_device, M, D):
    """IWVI_GP_REUSE_FACTOR after q moved from scales (1, 1, 1, 1) to those of C, and again after q_mu went to zero: the state equals a
    full precompute byte for byte (tests/test_gpu_reuse_factor.py moves q by O(0.1) only: no exponent changes there)."""
    from dgps_with_iwvi_amd import _abi
    from dgps_with_iwvi_amd.temp_workaround import precompute_states
    dev, seed = gpu_device, cc.case_seed(M, D)
    c1 = _case(M, D, cc.R_D, "compact", 0, cc._ONES, cc._ONES, "rbf", seed=seed, T=cc.T_CHAIN)
    lay2 = _case(M, D, cc.R_D, "compact", 0, cc.Q_ADJOINT, cc.QMU_HETERO, "rbf", seed=seed, T=cc.T_CHAIN).spec["layers"][1]
    layer = _model(c1, dev).layers[c1.li]
    precompute_states([layer.state_desc()])
    for q_mu, q_sqrt in ((lay2["q_mu"], lay2["q_sqrt"]), (np.zeros_like(lay2["q_mu"]), lay2["q_sqrt"])):
        before = layer.state().buf.clone()
        layer.q_mu, layer.q_sqrt = _t(q_mu, dev), _t(q_sqrt, dev)
        d = layer.state_desc()
        d.flags |= _abi.GP_REUSE_FACTOR
        precompute_states([d])
        torch.cuda.synchronize()
        reused = layer.state().buf.clone()
        precompute_states([layer.state_desc()])
        torch.cuda.synchronize()
        assert torch.equal(reused, layer.state().buf)
        assert bool((reused != before).any())


# ------------------------------------------------------------------------------------------------------------------------------------
# E: a device-resident kernel variance against a stale host copy
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,v", cc.CASES_E)
def test_device_variance_under_a_stale_host_copy(gpu_device, M, v):
    from dgps_with_iwvi_amd import _abi
    dev, D = gpu_device, cc.D_E
    c = _case(M, D, cc.R_E, "compact", 0, None, None, "rbf", seed=cc.case_seed(M, D), T=cc.T_CHAIN, variance=v)
    v32 = float(np.float32(v))
    assert c.spec["layers"][c.li]["var"] == v32

    def run(host_value):
        layer = _model(c, dev).layers[c.li]
        k = layer._base_kern()
        k.variance = host_value
        k.bind_device_variance(torch.full((1,), v32, dtype=torch.float32, device=dev))
        assert k.desc_variance()[0] == host_value and k.desc_variance()[1] is not None     # nobody marked the device value as moved
        _abi.backward_routes()
        saved, out = _run_adjoint(layer, c, dev)
        assert k.desc_variance()[0] == host_value
        return saved, out, _cst(layer), layer.state().kl_parts.clone(), _abi.backward_routes()

    saved, out, cst, kl, routes = run(1.0)
    saved2, out2, cst2, kl2, _ = run(v32)
    # identical bits, whatever the host believed
    assert np.array_equal(_cst_written(cst, cc.R_E), _cst_written(cst2, cc.R_E)) and torch.equal(kl, kl2)
    for k in ("sample", "mean", "var", "A", "GMV"):
        assert torch.equal(getattr(saved, k), getattr(saved2, k)), k
    for k in out:
        assert torch.equal(out[k], out2[k]), k
    # the exponents are the device value's: 2^ea with ea = (7 | 10) - ceil(log2(v) / 2), three (60) or minus two (0.02) away from the host's
    lg = int(np.ceil(0.5 * np.log2(np.float32(v))))
    assert lg == {0.02: -2, 60.0: 3}[v]
    assert cst[CST_SA] == 2.0 ** ((7 if M <= 128 else 10) - lg), cst[CST_SA]
    assert routes[0][0] == _abi.BW_ROUTE_CHAIN, routes
    # against float64 at the device value
    sd = float(np.sqrt(v32))
    so, mo, vo, klo = _forward_reference(_key(M, D, cc.R_E, "compact", 0, None, None, "rbf", seed=cc.case_seed(M, D), T=cc.T_CHAIN, variance=v))
    ratios = _moments_ratios(_np(saved.sample), _np(saved.mean), _np(saved.var), so, mo, vo, sd=sd)
    ratios["kl"] = abs(float(kl.sum().item()) - klo) / (KL_RTOL * abs(klo))
    ref = _adjoint_reference(_key(M, D, cc.R_E, "compact", 0, None, None, "rbf", seed=cc.case_seed(M, D), T=cc.T_CHAIN, variance=v))
    adj, misses = _adjoint_ratios(out, ref)
    assert not misses, misses
    _report("E", "M%d-var%g" % (M, v), dict(ratios, **adj))
