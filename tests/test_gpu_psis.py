"""``iwvi_psis_summary`` (csrc/psis.hip: k_psis_summary) against the float64 restatement of tests/psis_reference.py (pinned on the CPU by
tests/test_psis_reference_host.py) on the same float32 inputs.

S in {1, 4, 20, 21, 63, 64, 65, 128, 129, 224, 225, 226, 257, 1000, 2049, 5000, 16384}: each a rule change (no fit below 21; the tail
length changes formula at 225) or a padding / grouping edge of the sort (64, 128, 256, 2048, 4096 and the largest).  N = 5 (two
workgroups when four points share one, the second with three idle groups), N = 1 at the two largest S.  Families: lognormal weights with
sigma 0.5 / 2 / 4 at offsets 0 and -1000 (where the float32 spacing makes ties), quantised to 0.25, all equal, one dominant draw at
s = 0 and at s = S - 1, a quarter of the draws at -inf, all at -inf, one NaN.  Layouts, both input modes with 0, 1 and 4 regulariser
arrays, n_terms and Dy in {1, 3, 32}, both var_exp values, the device variance pointer, repeat calls, a captured graph, output subsets.

Where the device ASSEMBLES the log-weight (several terms, regularisers, the moments mode) its float32 value differs from the float64
assembly by rounding; khat is not a continuous function of that (a rounding can make or break a tie at the cutoff), so there the
summaries are compared with the restatement ON THE LOG-WEIGHTS THE DEVICE WROTE (out_logw), out_logw with the float64 assembly, and
raw with the restatement on the float64 assembly.

Tolerances
  raw       tol_reduce of tests/iw_reduction_reference.py (4 spacing32(max(|m|, log S)) + 2e-6) on log-weights that are inputs; plus
            tol_logw ((roundings per draw + 4) spacing32(largest |partial sum|)) when the device summed them
  out_logw  tol_logw
  khat, psis, ess   4 x the worst gap to the restatement measured over every case of this file and of tests/test_gpu_importance_model.py on
            an MI355X -- the margin is for another box's exp / log and summation order --, the constants of tests/psis_reference.py:
              khat  worst 1.15e-7 absolute (largest |khat| met: 4.29; the rounding of the float32 output is half of 4.8e-7 there)  -> 4.6e-7
              psis  worst 0.607 of the bound on raw                                                                               -> 2.43 x it
              ess   worst 1.24e-7 relative                                                                                        -> 4.96e-7
            none above what a rounding may cost: khat 1e-4 absolute, psis the raw bound + 1e-5 (gpu_psis_bound takes the smaller of the
            two), ess 1e-5 relative.  raw itself reached 0.19 of its bound, out_logw 0.21 of tol_logw.  Each test prints its worst
            gap-to-bound ratios.
Infinite and NaN outputs match exactly."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import iw_reduction_reference as IW   # noqa: E402
import psis_reference as R            # noqa: E402

pytestmark = pytest.mark.gpu

ALL_S = (1, 4, 20, 21, 63, 64, 65, 128, 129, 224, 225, 226, 257, 1000, 2049, 5000, 16384)
KHAT_TOL, ESS_RTOL = R.GPU_KHAT_TOL, R.GPU_ESS_RTOL


def _f(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _launch(**kw):
    from dgps_with_iwvi_amd import psis
    r = psis.summarise(**kw)
    torch.cuda.synchronize()
    return r


def _compare(got, ref, tol_raw, label, worst):
    """got: device results; ref: the restatement's float64 [N] each; tol_raw [N].  Non-finite entries must match exactly."""
    bounds = {"raw": tol_raw, "psis": R.gpu_psis_bound(tol_raw), "khat": np.full_like(tol_raw, KHAT_TOL), "ess": ESS_RTOL * np.abs(ref["ess"])}
    for key in ("raw", "ess", "khat", "psis"):
        g, r = _np(got[key]), ref[key]
        fin = np.isfinite(r)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key, g, r)
        assert np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), (label, key, g, r)
        if fin.any():
            gap = np.abs(g[fin] - r[fin])
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = float(np.where(gap == 0.0, 0.0, gap / bounds[key][fin]).max())     # (an exact match meets a bound of zero: ess = 0)
            worst[key] = max(worst.get(key, 0.0), ratio)
            if key == "khat":
                worst["khat_abs"] = max(worst.get("khat_abs", 0.0), float(gap.max()))
                worst["khat_largest"] = max(worst.get("khat_largest", 0.0), float(np.abs(r[fin]).max()))
            if key == "ess":
                worst["ess_rel"] = max(worst.get("ess_rel", 0.0), float((gap[r[fin] != 0] / np.abs(r[fin][r[fin] != 0])).max()) if (r[fin] != 0).any() else 0.0)
            if key == "psis":
                worst["psis_vs_raw_bound"] = max(worst.get("psis_vs_raw_bound", 0.0), float((gap / tol_raw[fin]).max()))
            assert ratio <= 1.0, (label, key, ratio, g, r, bounds[key])


def _tol_reduce(L):
    with np.errstate(invalid="ignore"):
        t = IW.tol_reduce(np.where(np.isfinite(L), L, -1e30))    # (rows without a finite maximum are compared exactly, not by a bound)
    return np.where(np.isfinite(t), t, 1.0)


@pytest.mark.parametrize("S", ALL_S)
def test_families_of_log_weights(gpu_device, S):
    N = 1 if S >= 5000 else 5
    worst = {}
    for name in R.FAMILIES:
        L = R.family(name, N, S, seed=S)
        got = _launch(N=N, S=S, stride_n=S, stride_s=1, terms=_f(L, gpu_device), want_logw=True)
        lw = _np(got["logw"])
        assert np.array_equal(lw, L, equal_nan=True), name       # one term, no regulariser: the log-weight is the input, bit for bit
        _compare(got, R.summary(L), _tol_reduce(L), (name, S), worst)
    print("S=%d gap / bound:" % S, {k: "%.3g" % v for k, v in sorted(worst.items())})


@pytest.mark.parametrize("S", [65, 1000])
def test_layouts_give_the_same_bits(gpu_device, S):
    from dgps_with_iwvi_amd import evaluation
    N = 5
    L = R.family("ln2", N, S, seed=3)
    base = evaluation.psis_summary(_f(L, gpu_device))
    ref = R.summary(L)
    worst = {}
    _compare({"raw": base["log_mean"], "psis": base["log_mean_psis"], "khat": base["khat"], "ess": base["ess"]}, ref, _tol_reduce(L), "contiguous", worst)
    t = _f(L.T, gpu_device).t()                                  # [S, N] storage seen as [N, S]: stride_n = 1, stride_s = N
    assert t.stride() == (1, N)
    big = torch.full((2 * N + 1, 2 * S + 7), float("nan"), device=gpu_device)
    big[1::2, 3:3 + 2 * S:2] = _f(L, gpu_device)
    sl = big[1::2, 3:3 + 2 * S:2]                                # a strided slice: NaN all around it
    assert sl.stride() == (2 * (2 * S + 7), 2)
    for view in (t, sl):
        r = evaluation.psis_summary(view)
        for k in base:
            assert torch.equal(r[k], base[k]), (k, view.stride())
    print("S=%d gap / bound:" % S, {k: "%.3g" % v for k, v in sorted(worst.items())})


def _kls(rng, N, S, n_kl):
    return [np.asarray(rng.uniform(-1.0, 2.0, (N, S, 1 + (i % 3))), dtype=np.float32).astype(np.float64) for i in range(n_kl)]


@pytest.mark.parametrize("n_terms,n_kl,S", [(1, 1, 21), (3, 0, 129), (3, 4, 1000), (32, 1, 257), (32, 4, 64), (1, 4, 2049)])
def test_terms_mode_assembles_the_log_weight(gpu_device, n_terms, n_kl, S):
    N = 5
    rng = np.random.default_rng([11, n_terms, n_kl, S])
    terms = np.asarray(rng.standard_normal((N, S, n_terms)) * 2.0 / np.sqrt(n_terms) - 30.0 / n_terms, dtype=np.float32).astype(np.float64)
    kls = _kls(rng, N, S, n_kl)
    got = _launch(N=N, S=S, stride_n=S, stride_s=1, terms=_f(terms.reshape(N * S, n_terms), gpu_device), n_terms=n_terms,
                  kls=[_f(k.reshape(N * S, -1), gpu_device) for k in kls], want_logw=True)
    l64, big, n_add = R.logw_terms(terms, kls)
    _check_assembled(got, l64, big, n_add, (n_terms, n_kl, S))


def _check_assembled(got, l64, big, n_add, label):
    tol_l = IW.tol_logw(big, n_add)
    lw = _np(got["logw"])
    gap = np.abs(lw - l64).max(1)
    assert (gap <= tol_l).all(), (label, gap, tol_l)
    worst = {"logw": float((gap / tol_l).max())}
    _compare(got, R.summary(lw), _tol_reduce(lw), label, worst)               # the summaries of what the device summed
    ref = R.summary(l64)
    gap = np.abs(_np(got["raw"]) - ref["raw"])
    tol = _tol_reduce(l64) + tol_l
    assert (gap <= tol).all(), (label, gap, tol)
    worst["raw_vs_f64"] = float((gap / tol).max())
    print(label, "gap / bound:", {k: "%.3g" % v for k, v in sorted(worst.items())})


@pytest.mark.parametrize("Dy,var_exp,n_kl,S,dev_var", [(1, 0, 0, 21, False), (1, 1, 1, 129, True), (3, 0, 4, 1000, True), (3, 1, 0, 257, False),
                                                        (32, 0, 1, 64, False), (32, 1, 4, 225, True), (2, 0, 1, 5000, False)])
def test_moments_mode_assembles_the_gaussian_log_weight(gpu_device, Dy, var_exp, n_kl, S, dev_var):
    N = 5
    rng = np.random.default_rng([13, Dy, var_exp, n_kl, S])
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    Y = f32(rng.standard_normal((N, Dy)))
    fm = f32(Y[:, None, :] + rng.standard_normal((N, S, Dy)) * 0.8)
    fv = f32(rng.uniform(0.01, 0.5, (N, S, Dy)))
    kls = _kls(rng, N, S, n_kl)
    s = float(np.float32(0.37))
    kw = dict(lik_variance=s)
    if dev_var:                                                  # the device word wins over the value
        kw = dict(lik_variance=123.0, lik_variance_dev=torch.tensor([s], dtype=torch.float32, device=gpu_device))
    got = _launch(N=N, S=S, stride_n=S, stride_s=1, fmean=_f(fm.reshape(N * S, Dy), gpu_device), fvar=_f(fv.reshape(N * S, Dy), gpu_device),
                  Y=_f(Y, gpu_device), Dy=Dy, var_exp=bool(var_exp), kls=[_f(k.reshape(N * S, -1), gpu_device) for k in kls], want_logw=True, **kw)
    l64, big, n_add = R.logw_moments(fm, fv, Y, s, var_exp, kls)
    _check_assembled(got, l64, big, n_add, (Dy, var_exp, n_kl, S, dev_var))


def test_sample_major_moments_and_zero_strides(gpu_device):
    """Rows s N + n (stride_n = 1, stride_s = N) give what the point-major layout gives; stride_s = 0 reads one draw S times."""
    N, S, Dy = 5, 65, 2
    rng = np.random.default_rng(17)
    Y, fm, fv = rng.standard_normal((N, Dy)), rng.standard_normal((N, S, Dy)), rng.uniform(0.1, 1.0, (N, S, Dy))
    kl = rng.uniform(0, 1, (N, S, 2))
    a = _launch(N=N, S=S, stride_n=S, stride_s=1, fmean=_f(fm.reshape(N * S, Dy), gpu_device), fvar=_f(fv.reshape(N * S, Dy), gpu_device),
                Y=_f(Y, gpu_device), Dy=Dy, lik_variance=0.5, kls=[_f(kl.reshape(N * S, 2), gpu_device)], want_logw=True)
    tr = lambda x: _f(np.swapaxes(x, 0, 1).reshape(N * S, -1), gpu_device)
    b = _launch(N=N, S=S, stride_n=1, stride_s=N, fmean=tr(fm), fvar=tr(fv), Y=_f(Y, gpu_device), Dy=Dy, lik_variance=0.5, kls=[tr(kl)],
                want_logw=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c = _launch(N=N, S=S, stride_n=S, stride_s=0, terms=a["logw"].reshape(N * S, 1).contiguous(), want_logw=True)
    assert torch.equal(c["logw"], a["logw"][:, :1].expand(N, S))
    assert torch.isinf(c["khat"]).all() and torch.equal(c["raw"], c["psis"]) and torch.equal(c["ess"], torch.full_like(c["ess"], float(S)))


@pytest.mark.parametrize("S", [64, 257, 5000])
def test_repeat_calls_and_a_captured_graph_give_the_same_bits(gpu_device, S):
    from dgps_with_iwvi_amd import psis
    N = 5
    L = _f(R.family("ln2_off", N, S, seed=5), gpu_device)
    a = _launch(N=N, S=S, stride_n=S, stride_s=1, terms=L, want_logw=True)
    b = _launch(N=N, S=S, stride_n=S, stride_s=1, terms=L, want_logw=True)
    for k in a:
        assert a[k].view(torch.int32).equal(b[k].view(torch.int32)), k
    out = {k: torch.zeros_like(v) for k, v in a.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        psis.summarise(N=N, S=S, stride_n=S, stride_s=1, terms=L, want_logw=True, out=out)
    for _ in range(2):
        for v in out.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in a:
            assert a[k].view(torch.int32).equal(out[k].view(torch.int32)), k


def test_output_subsets(gpu_device):
    N, S = 5, 300
    L = _f(R.family("ln4", N, S, seed=9), gpu_device)
    full = _launch(N=N, S=S, stride_n=S, stride_s=1, terms=L, want_logw=True)
    for want in (("raw",), ("ess",), ("khat",), ("psis",), ("khat", "psis"), ("raw", "ess")):
        r = _launch(N=N, S=S, stride_n=S, stride_s=1, terms=L, want=want)
        assert set(r) == set(want)
        for k in want:
            assert torch.equal(r[k], full[k]), (want, k)
    r = _launch(N=N, S=S, stride_n=S, stride_s=1, terms=L, want=(), want_logw=True)
    assert set(r) == {"logw"} and torch.equal(r["logw"], L)


def test_a_plus_infinity_is_refused_like_a_nan_and_spares_the_other_points(gpu_device):
    N, S = 5, 100
    L = R.family("ln2", N, S, seed=2)
    L[3, 17] = np.inf
    got = _launch(N=N, S=S, stride_n=S, stride_s=1, terms=_f(L, gpu_device))
    _compare(got, R.summary(L), _tol_reduce(L), "+inf", {})
    assert np.isnan(_np(got["raw"])[3]) and np.isfinite(_np(got["raw"])[[0, 1, 2, 4]]).all()
