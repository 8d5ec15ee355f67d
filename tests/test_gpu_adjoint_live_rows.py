"""``iwvi_gp_layer_backward`` against float64 autograd with live cotangents in every workgroup (tests/adjoint_reference.py): the
instantiations that exist only at large T -- k_bw_chain<NS, DM> for NS = 1 .. 5 and DM = 8 / 16 / 32, k_bw_mid forced and by the default
rule, the split-K GEMM path with 4, 16 and 33 splits, k_reduce_parts / k_reduce_multi over hundreds of partials, the dLm / G_r shares
formed inside and outside the chain -- and IWVI_BW_F32_CHAIN (``settings.bw_f32_chain``) at even block counts.

Each case: F, z, cs, cm, cv ~ N(0, 1) float32 on T rows, the cotangents zeroed outside ``live_rows(T)`` (a live row in every 16-row tile,
hence in every workgroup of every route and in every 512-row split; test_adjoint_reference_host.py checks that the loss of any one
workgroup's live rows would show), kl_weight = 0.7, one saving forward and one adjoint.  dF on the live rows, dq_mu, tril(dq_sqrt), dZ,
dls, dvariance, dW and dmf_A against the reference at the tolerance test_gpu_backward.py states for this comparison (max-norm relative
3e-3 per array); dF exactly zero on the dead rows, dq_sqrt exactly zero above the diagonal; the route as derived from the code; a second
call bit for bit.  A final layer gets d_sample = None, as in the model.

Not reached: k_bw_chain<5, 32> on split-f16 operands at M = 128 -- three [128 x 84] tiles and the staging of D > 16 need ~182 KB of LDS,
the chain plan's `fits` is false there at any T > 16384 and the default rule launches k_bw_mid; <5, 32> runs here at M = 64 (split f16) and at
M = 128 with IWVI_BW_F32_CHAIN (two tiles).

Observed on an MI355X, worst error / tolerance over the arrays of each case (every case prints its own):
chain-ns2 3.8e-3 (dvariance), chain-ns3 3.0e-3 (dZ), chain-ns4 2.5e-3 (dls), chain-ns5-final 3.1e-3 (dvariance), chain-ns5-to-3 1.9e-3 (dZ),
chain-ns1-1031-shares 1.3e-3 (dZ), chain-ns5-dm16 7.6e-4, chain-ns5-dm32-m64 4.2e-4, chain-ns5-dm32-f32 7.8e-4 (all dvariance),
chain-m256-32 5.0e-3 (dvariance), gemm-m256-16-splits 1.6e-3 (dls), chain-m176-f32-64 2.6e-3 (dvariance), chain-m512-s16 6.7e-2 (dZ),
mid-forced-m64 5.2e-4 (dvariance), mid-forced-m256 1.5e-3 (dls), mid-default 8.6e-4 (dvariance), gemm-33-splits 3.6e-4 (dZ),
gemm-ragged 1.0e-2 (dvariance), chain-matern52 8.3e-4 (dls), flag-m128 4.0e-3 split f16 / 5.7e-3 fp32 (dvariance), flag-m256 4.1e-2 / 4.1e-2
(dZ).  dW stays below 7.1e-3 and dmf_A below 4.4e-5 of the tolerance everywhere.  With a library whose chain reductions skip the last
workgroup's partial sums every chain case fails (at T = 16384, 64 samples per workgroup: dq_mu off by 5 %, dmf_A by 10 % of its max-norm)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_reference as ar   # noqa: E402

pytestmark = pytest.mark.gpu

_BY_ID = {c.id: c for c in ar.CASES}


@functools.lru_cache(maxsize=None)
def _inputs_and_reference(M, Dx, R, li, T, kern, rows_kind):
    """(spec, inputs, rows, reference) of a case -- computed once, shared by the cases that differ only in a flag, never written to."""
    c = next(c for c in ar.CASES if (c.M, c.Dx, c.R, c.li, c.T, c.kern, c.rows) == (M, Dx, R, li, T, kern, rows_kind))
    spec = ar.case_spec(c)
    rows = ar.case_rows(c)
    F, z, cs, cm, cv = ar.case_inputs(c, spec)
    ref = ar.layer_reference(spec, li, F, z, cs, cm, cv, ar.KL_WEIGHT, rows, kern)
    return spec, (F, z, cs, cm, cv), rows, ref


def _t(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)


def _layer(model, c, dev):
    from dgps_with_iwvi_amd import kernels
    layer = model.layers[c.li]
    if c.kern == "matern52":
        old = layer._base_kern()
        new = kernels.Matern52(old.input_dim, variance=old.variance, lengthscales=old.lengthscales, ARD=True).to(dev)
        if hasattr(layer.kern, "kernel"):
            layer.kern.kernel = new
        else:
            layer.kern = new
    return layer


def _adjoint(dev, c):
    """One saving forward and two adjoint launches of the case -> (first outputs, second outputs, routes of the first)."""
    from dgps_with_iwvi_amd import _abi, backward, settings, synthetic
    spec, (F, z, cs, cm, cv), rows, _ = _inputs_and_reference(c.M, c.Dx, c.R, c.li, c.T, c.kern, c.rows)
    layer = _layer(synthetic.build_model(spec, dev), c, dev)
    d_sample = None if c.li == 1 else _t(cs, dev)                # the final layer's draw feeds nothing (its cs is zero in the reference)
    old, settings.bw_f32_chain = settings.bw_f32_chain, bool(c.f32)
    _abi.set_debug_option("IWVI_BW_FUSED", c.fused)
    try:
        saved = backward.gp_forward_saved(layer, _t(F, dev), _t(z, dev))
        _abi.backward_routes()                                   # (empties the log)
        out = backward.gp_backward(layer, saved, d_sample, _t(cm, dev), _t(cv, dev), kl_weight=ar.KL_WEIGHT)
        torch.cuda.synchronize()
        routes = _abi.backward_routes()
        out2 = backward.gp_backward(layer, saved, d_sample, _t(cm, dev), _t(cv, dev), kl_weight=ar.KL_WEIGHT)
        torch.cuda.synchronize()
    finally:
        _abi.set_debug_option("IWVI_BW_FUSED", 0)
        settings.bw_f32_chain = old
    return out, out2, routes


def _compare(c, out):
    """Every gradient array of the case against the reference -> the worst error / tolerance; on a miss, the worst entry of each failing
    array and the workgroup it belongs to are in the assertion's message."""
    _, _, rows, ref = _inputs_and_reference(c.M, c.Dx, c.R, c.li, c.T, c.kern, c.rows)
    dF = out["dF"].cpu().numpy()
    dead = np.ones(c.T, dtype=bool)
    dead[rows] = False
    pairs = [("dF", dF[rows], ref["F"]), ("dq_mu", out["dq_mu"].cpu().numpy(), ref["q_mu"]),
             ("dq_sqrt", out["dq_sqrt"].cpu().numpy(), np.tril(ref["q_sqrt"])), ("dZ", out["dZ"].cpu().numpy(), ref["Z"]),
             ("dls", out["dls"].cpu().numpy(), ref["ls"]), ("dvariance", out["dvariance"].cpu().numpy()[0], ref["var"])]
    assert ("dW" in out) == ("W" in ref) == (c.li == 0) and ("dmf_A" in out) == ("A" in ref) == (c.li == 0)
    if "W" in ref:
        pairs += [("dW", out["dW"].cpu().numpy(), ref["W"]), ("dmf_A", out["dmf_A"].cpu().numpy(), ref["A"])]
    ratios, misses = {}, []
    for name, got, want in pairs:
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.isfinite(got).all(), name
        scale = max(np.abs(want).max(), 1e-12)
        ratios[name] = np.abs(got - want).max() / (ar.RTOL * scale)
        if ratios[name] > 1.0:
            idx, err = ar.worst_entry(got, want)
            where = ""
            if name == "dF":
                where = ", row %d = workgroup %d of %d samples, lane %d" % (rows[idx[0]], rows[idx[0]] // c.route[2], c.route[2], rows[idx[0]] % 16)
            misses.append("%s: max err %.3e vs scale %.3e at %s%s (got %.6e, want %.6e)" % (name, err, scale, idx, where, got[idx], want[idx]))
    worst = max(ratios, key=ratios.get)
    print("adjoint-live-rows %s: worst err / tol = %.1e (%s)  " % (c.id, ratios[worst], worst) + " ".join("%s=%.1e" % kv for kv in ratios.items()))
    assert not misses, (c.id, misses)
    if dead.any():
        assert float(np.abs(dF[dead]).max()) == 0.0, "dF is not zero on a dead row: row %d" % np.flatnonzero(np.abs(dF).max(1) * dead)[0]
    assert float(torch.triu(out["dq_sqrt"], 1).abs().max()) == 0.0
    return ratios[worst]


@pytest.mark.parametrize("cid", [c.id for c in ar.CASES if not c.id.startswith("flag-")])
def test_layer_adjoint_with_live_rows_in_every_workgroup(gpu_device, cid):
    c = _BY_ID[cid]
    out, out2, routes = _adjoint(gpu_device, c)
    assert routes == [c.route], (cid, routes)
    _compare(c, out)
    for k in out:
        assert torch.equal(out[k], out2[k]), (cid, k)


@pytest.mark.parametrize("M", [128, 256])
def test_f32_chain_flag_changes_the_arithmetic_and_nothing_else(gpu_device, M):
    """IWVI_BW_F32_CHAIN at an even block count, every row live: the split-f16 chain and the fp32 chain both hold the float64 tolerance,
    on the same route -- and dF differs in at least one bit, or the flag never reached the kernel."""
    runs = []
    for mode in ("s16", "f32"):
        c = _BY_ID["flag-m%d-%s" % (M, mode)]
        out, out2, routes = _adjoint(gpu_device, c)
        assert routes == [c.route], (c.id, routes)
        _compare(c, out)
        for k in out:
            assert torch.equal(out[k], out2[k]), (c.id, k)
        runs.append(out)
    assert not torch.equal(runs[0]["dF"], runs[1]["dF"])
