"""Every ``k_dgp_forward`` instantiation (csrc/dgp_forward.hip: ``fw_variants[]``) against the float64 oracle, one case per runnable row of
tests/forward_variant_cases.py (whose docstring says what selects each row; tests/test_forward_variant_cases_host.py proves the table
complete).  Each case reads ``iwvi_debug_last_forward_variant()`` and asserts the row's word BEFORE it compares anything: a case that drifts
to another instantiation fails for that reason.

  bound tail    ``_fused_forward(..., want_layers=True)`` on injected noise.  Per SAMPLE, so that one wrong sub-tile (16 samples of a chunk)
                cannot hide behind a logsumexp: the log-weights [B, K] against ``oracle.log_weights`` and each layer's mean, variance and
                sample against the oracle's layer outputs; then the per-point logp and the bound.  The same call once more without
                per-layer outputs: ``logw`` bit for bit (the FWF_ANY_OUT branch must not change arithmetic).
  predict tail  ``predict_log_density(X, Y, S, zs=...)`` per point against the float64 Monte Carlo mixture of the oracle's moments
                (``_oracle_mc`` of tests/test_gpu_predict_density.py, on moments shared with the sampling case of the same stack and S).
  sample tail   ``predict_y_samples_fused`` with ``zs`` and ``z_y`` given: every draw [S, N, Dy] against the oracle's
                mean + sqrt(var + lik_var) z_y on the same noise.
  data          every call reads the LAST rows of its stack's X and Y (forward_variant_cases.data_rows): make_spec's inducing points are
                X[:M], and a test point that is an inducing point leaves every block of layer 0's solve but its own with zeros.
  partial chunk every buffer the model allocates for the call carries a NaN-filled guard behind its last element, and the whole buffer starts
                as NaN: the guard must be untouched and no valid element of a result NaN (an instantiation with a wrong ``nvalid`` writes
                past the end of the partial last chunk, or not at all).

Tolerances are the suite's own, the same for every ns of a stack: log-weights rtol 2e-4 + atol 2e-2 (test_gpu_lean_variant.py); layer
moments and samples MEAN_TOL / VAR_TOL / SAMPLE_TOL of test_gpu_layer_conditioning.py; logp rtol 3e-4 + atol 3e-2 and the bound 1e-4
relative + 2e-3 B (test_gpu_random_sweep.py); the predictive density 3e-4 max(1, |density|) (test_gpu_predict_density.py).  The F64 rows
are held to these and, for the layer on the float64 route, to the per-layer bounds of test_gpu_f64_route.py (mean 2e-5, variance 1e-5).
Each case prints error / tolerance per quantity.

Words run, per tail (the four LEAN / SHP words 0x405, 0x505, 0x805, 0x905 are covered by tests/test_gpu_lean_variant.py):
  bound    0x1..0x5, 0x101..0x105, 0x201..0x205 (M = 144 and 272), 0x301..0x305 (M = 160 and 256), 0x1201..0x1205
  predict  0x1, 0x3, 0x5, 0x101.., 0x201.. (M = 144 and 272), 0x301.. (M = 160 and 256), 0x1201, 0x1203, 0x1205
  sample   the same fifteen
Measured on an MI355X (gfx950): error / tolerance, the maximum over the ns of a stack (it grows with the number of samples a row holds, 77 to
16 387, not with ns: on the same 16 387 samples the ns = 5 and the ns = 1 instantiation gave the same log-weight bits at M = 160, 256 and 272).
  bound    stack   logw     layer 0 mean / var / sample    layer 1 mean / var / sample    logp     bound
           m32     7.2e-3   1.0e-3 / 8.5e-4 / 8.1e-4       1.9e-3 / 3.0e-4 / 9.6e-4       4.3e-3   7.0e-4
           m48     1.3e-2   1.7e-3 / 9.4e-4 / 1.2e-3       3.4e-3 / 3.4e-4 / 1.5e-3       5.7e-3   3.4e-3
           m144    3.0e-2   7.1e-3 / 5.4e-3 / 3.8e-3       9.3e-3 / 5.8e-4 / 5.2e-3       1.6e-2   3.5e-3
           m160    4.4e-2   9.9e-3 / 1.7e-3 / 5.4e-3       1.3e-2 / 5.5e-4 / 5.6e-3       2.9e-2   1.2e-2
           m256    2.2e-1   5.3e-2 / 5.5e-3 / 2.9e-2       5.6e-2 / 7.7e-4 / 3.2e-2       1.1e-1   7.5e-2
           m272    2.0e-1   2.3e-2 / 4.3e-3 / 1.5e-2       6.7e-2 / 9.4e-4 / 3.4e-2       1.2e-1   3.0e-2
           m32f64  6.3e-3   3.9e-4 / 1.0e-4 / 2.7e-4       1.7e-3 / 3.0e-4 / 9.8e-4       2.8e-3   2.6e-4   (float64 route's own bounds: mean 2.9e-2, var 9.4e-3)
  predict  density: m32 1.6e-3, m48 1.5e-3, m144 3.5e-3, m160 5.6e-3, m256 1.9e-2, m272 1.3e-2, m32f64 9.7e-4
  sample   draw:    m32 9.0e-4, m48 1.5e-3, m144 4.3e-3, m160 5.0e-3, m256 2.5e-2, m272 3.0e-2, m32f64 7.2e-4
The whole module takes 19 s; the slowest case 1.3 s (its float64 oracle of 16 387 rows at M = 272)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import forward_variant_cases as fv   # noqa: E402
from oracle.from_spec import build_oracle, oracle_noise   # noqa: E402
from test_gpu_predict_density import _logpdf, _noise, _oracle_moments   # noqa: E402

pytestmark = pytest.mark.gpu

LOGW_TOL = dict(rtol=2e-4, atol=2e-2)             # test_gpu_lean_variant.py::_read_back_vs_oracle
MEAN_TOL = dict(rtol=2e-3, atol=1e-3)             # test_gpu_layer_conditioning.py
VAR_TOL = dict(rtol=2e-3, atol=1e-4)
SAMPLE_TOL = dict(rtol=2e-3, atol=2e-3)
LOGP_TOL = dict(rtol=3e-4, atol=3e-2)             # test_gpu_random_sweep.py
ELBO_RTOL, ELBO_ATOL_PER_POINT = 1e-4, 2e-3
DENSITY_TOL = 3e-4                                # test_gpu_predict_density.py (times max(1, |density|))
F64_MEAN_ATOL, F64_VAR_ATOL = 2e-5, 1e-5          # test_gpu_f64_route.py
GUARD = 256                                       # elements behind every buffer

_STACKS = {}                                      # stack -> (spec, device model): built once, shared by every row of the stack
_PREDICT_REF = {}                                 # (stack, S) -> (noise, z_y, oracle mean, oracle variance), shared by the two predictive tails


def _stack(name, dev):
    if name not in _STACKS:
        from dgps_with_iwvi_amd import synthetic
        from dgps_with_iwvi_amd.layers import GPLayer
        spec = synthetic.make_spec(**fv.spec_kwargs(name))
        model = synthetic.build_model(spec, dev)
        if fv.STACKS[name]["f64"]:
            [l for l in model.layers if isinstance(l, GPLayer)][0].f64_stage1 = True
        _STACKS[name] = (spec, model)
    return _STACKS[name]


def _variant():
    from dgps_with_iwvi_amd import _abi
    return int(_abi.lib().iwvi_debug_last_forward_variant())


def _np(t):
    return t.detach().double().cpu().numpy()


def _ratio(got, ref, rtol, atol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


class _GuardedTorch:
    """Stands in for the ``torch`` module inside dgps_with_iwvi_amd.models for one call: every ``torch.empty`` there (the call's results
    and scratch) becomes the front of a NaN-filled buffer with GUARD more elements behind it.  ``check`` holds the number of such buffers
    to what the call is known to allocate and every result to be one of them, so an allocation that escapes the guard fails the test."""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=None, device=None):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        n = int(np.prod(shape, dtype=np.int64))
        assert dtype in (torch.float32, torch.float64), dtype
        flat = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=device)
        self.made.append((flat, n))
        return flat[:n].view(*shape)

    def owns(self, t):
        """t is (a view of) the valid front of one of the guarded buffers."""
        return any(t.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and t.numel() <= n for flat, n in self.made)

    def check(self, what, made, results):
        """``made`` buffers so far (an allocation that moves out of the guard's reach changes the count), every result one of them."""
        torch.cuda.synchronize()
        assert len(self.made) == made, "%s: %d guarded buffers, expected %d" % (what, len(self.made), made)
        assert results and all(self.owns(t) for t in results), what
        for k, (flat, n) in enumerate(self.made):
            assert bool(torch.isnan(flat[n:]).all()), "%s: buffer %d of %d elements was written past its end" % (what, k, n)


def _guarded(monkeypatch):
    from dgps_with_iwvi_amd import models
    g = _GuardedTorch()
    monkeypatch.setattr(models, "torch", g)
    return g


def _report(r, ratios):
    print("forward-variant %s T=%d: " % (fv.row_id(r), fv.total_rows(r)) + " ".join("%s=%.1e" % kv for kv in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (fv.row_id(r), bad)


_BOUND = [r for r in fv.RUNNABLE if r.tail == fv.TAIL_BOUND]
_PREDICT = [r for r in fv.RUNNABLE if r.tail == fv.TAIL_PREDICT]
_SAMPLE = [r for r in fv.RUNNABLE if r.tail == fv.TAIL_SAMPLE]


@pytest.mark.parametrize("r", _BOUND, ids=fv.row_id)
def test_bound_tail_row_matches_the_oracle_per_sample(gpu_device, monkeypatch, r):
    from dgps_with_iwvi_amd import synthetic
    spec, model = _stack(r.stack, gpu_device)
    B, K = r.shape
    T = B * K
    zs = synthetic.make_noise(spec, seed=31 + r.ns, K=K, B=B)
    zd = [torch.as_tensor(z, dtype=torch.float32, device=gpu_device) for z in zs]
    rows = fv.data_rows(B)                                                     # (the last B rows: see forward_variant_cases)
    Xd, Yd = (torch.as_tensor(np.asarray(a[rows], np.float32), device=gpu_device) for a in (spec["X"], spec["Y"]))
    el = dict(B=B, K=K, stride_b=K, stride_k=1, mode_vi=False)
    model.precompute()
    g = _guarded(monkeypatch)
    logw, outs, red = model._fused_forward(T, K, B, (B, K), zs=zd, sampled_kl=True, want_layers=True, X=Xd, Y=Yd, elbo=dict(el))
    # sample, mean, var of two layers; logw, logp, the bound, the reduction's scratch
    g.check(fv.row_id(r), 10, [logw, red[0], red[1]] + [o[k] for o in outs for k in ("sample", "mean", "var")])
    word = _variant()
    assert word == r.word, "%s ran %#x" % (fv.row_id(r), word)
    logw2, outs2, red2 = model._fused_forward(T, K, B, (B, K), zs=zd, sampled_kl=True, want_layers=False, X=Xd, Y=Yd, elbo=dict(el))
    g.check(fv.row_id(r) + " (no per-layer outputs)", 14, [logw2, red2[0], red2[1]])
    assert _variant() == r.word and all(o is None for o in outs2)
    monkeypatch.undo()
    got = dict(logw=logw, logp=red[1], elbo=red[0].reshape(1), logw2=logw2, logp2=red2[1], elbo2=red2[0].reshape(1))
    for i, o in enumerate(outs):
        assert tuple(o["mean"].shape) == (B, K, fv.DX if i == 0 else fv.DY)
        got.update({"l%d-%s" % (i, k): o[k] for k in ("sample", "mean", "var")})
    got = {k: _np(v) for k, v in got.items()}
    for k, v in got.items():
        assert np.isfinite(v).all(), "%s: %d of %d elements of %s not written or not finite" % (fv.row_id(r), (~np.isfinite(v)).sum(), v.size, k)
    # the FWF_ANY_OUT branch changes no arithmetic
    assert np.array_equal(got["logw"], got["logw2"]), "logw differs without per-layer outputs at rows %s" % np.flatnonzero(got["logw"] != got["logw2"])[:8]
    assert np.array_equal(got["logp"], got["logp2"]) and got["elbo"][0] == got["elbo2"][0]

    om = build_oracle(dict(spec, X=spec["X"][rows], Y=spec["Y"][rows]), B=B)
    L_NK, global_kls, means_o, covs_o, samples_o = om.log_weights(oracle_noise(spec, zs))
    var_o = [covs_o[0], np.diagonal(covs_o[1], axis1=-2, axis2=-1).transpose(0, 2, 1)]
    samples_o = [samples_o[0], means_o[1] + np.sqrt(var_o[1]) * zs[1]]          # (the oracle's final layer does not draw: z = None)
    ratios = dict(logw=_ratio(got["logw"].reshape(B, K), L_NK, **LOGW_TOL))
    for i in range(2):
        ratios["l%d-mean" % i] = _ratio(got["l%d-mean" % i], means_o[i], **MEAN_TOL)
        ratios["l%d-var" % i] = _ratio(got["l%d-var" % i], var_o[i], **VAR_TOL)
        ratios["l%d-sample" % i] = _ratio(got["l%d-sample" % i], samples_o[i], **SAMPLE_TOL)
    if r.word & fv.F64:                                                        # the flagged layer, at the float64 route's own bounds
        ratios["f64-mean"] = float(np.abs(got["l0-mean"] - means_o[0]).max()) / F64_MEAN_ATOL
        ratios["f64-var"] = float(np.abs(got["l0-var"] - var_o[0]).max()) / F64_VAR_ATOL
    m_o = L_NK.max(1)
    logp_o = m_o + np.log(np.exp(L_NK - m_o[:, None]).sum(1)) - np.log(K)
    ratios["logp"] = _ratio(got["logp"], logp_o, **LOGP_TOL)
    ref = logp_o.sum() * (spec["n_data"] / B) - np.sum(global_kls)
    ratios["elbo"] = abs(got["elbo"][0] - ref) / (ELBO_RTOL * abs(ref) + ELBO_ATOL_PER_POINT * B)
    _report(r, ratios)


def _predict_reference(r, spec):
    key = (r.stack, r.shape[1])
    if key not in _PREDICT_REF:
        N, S = r.shape
        zs = _noise(spec, S, N, 57 + S)
        z_y = np.random.default_rng(91 + S).standard_normal((S, N, fv.DY)).astype(np.float32)
        m, v = _oracle_moments(spec, np.broadcast_to(spec["X"][fv.data_rows(N)], (S, N, fv.DX)), zs)
        for a in zs + [z_y, m, v]:
            a.setflags(write=False)
        _PREDICT_REF[key] = (zs, z_y, m, v)
    return _PREDICT_REF[key]


@pytest.mark.parametrize("r", _PREDICT, ids=fv.row_id)
def test_predict_tail_row_matches_the_oracle_per_point(gpu_device, monkeypatch, r):
    spec, model = _stack(r.stack, gpu_device)
    N, S = r.shape
    zs, _, m, v = _predict_reference(r, spec)
    X, Y = spec["X"][fv.data_rows(N)], spec["Y"][fv.data_rows(N)]
    zd = [torch.tensor(z, device=gpu_device) for z in zs]                # (copies: the shared reference stays read-only)
    g = _guarded(monkeypatch)
    got = model.predict_log_density(X, Y, S, zs=zd, batch_size=None)
    g.check(fv.row_id(r), 2, [got])                                            # the densities and the per-chunk partials
    monkeypatch.undo()
    word = _variant()
    assert word == r.word, "%s ran %#x" % (fv.row_id(r), word)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N,)
    got = _np(got)
    assert np.isfinite(got).all(), got
    ell = _logpdf(np.asarray(Y, np.float64)[None], m, v + spec["lik_var"]).sum(-1)        # [S, N]: test_gpu_predict_density.py::_oracle_mc
    mx = ell.max(0)
    ref = mx + np.log(np.exp(ell - mx).mean(0))
    _report(r, dict(density=float(np.abs(got - ref).max()) / (DENSITY_TOL * max(1.0, np.abs(got).max()))))


@pytest.mark.parametrize("r", _SAMPLE, ids=fv.row_id)
def test_sample_tail_row_matches_the_oracle_per_draw(gpu_device, monkeypatch, r):
    spec, model = _stack(r.stack, gpu_device)
    N, S = r.shape
    zs, z_y, m, v = _predict_reference(r, spec)
    zd = [torch.tensor(z, device=gpu_device) for z in zs]                # (copies: the shared reference stays read-only)
    g = _guarded(monkeypatch)
    got = model.predict_y_samples_fused(spec["X"][fv.data_rows(N)], S, zs=zd, z_y=torch.tensor(z_y, device=gpu_device), batch_size=None)
    g.check(fv.row_id(r), 1, [got])                                            # the draws [N, S, Dy]
    monkeypatch.undo()
    word = _variant()
    assert word == r.word, "%s ran %#x" % (fv.row_id(r), word)
    assert tuple(got.shape) == (S, N, fv.DY)
    got = _np(got)
    assert np.isfinite(got).all(), "%d of %d draws not written or not finite" % ((~np.isfinite(got)).sum(), got.size)
    ref = m + np.sqrt(v + spec["lik_var"]) * z_y
    _report(r, dict(draw=_ratio(got, ref, **SAMPLE_TOL)))
