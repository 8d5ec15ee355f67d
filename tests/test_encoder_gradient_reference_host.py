"""The float64 references of tests/encoder_gradient_reference.py pinned on the CPU, and the host-visible surface of the encoder-gradient
estimators ("iwae" | "dreg" | "stl") and of iwvi_moments_update: header, refusals (no HIP call is made), the models' setting.

  * "iwae" through the helper is oracle/grad_oracle.py's gradient (1e-12 relative; measured <= 2e-14);
  * the closed form the kernel implements is the gradient of the stop-gradient surrogate (1e-12; measured <= 2.5e-14);
  * at K = 1 "dreg" and "stl" are the same numbers; everywhere "dreg" is not "iwae";
  * over 3000 noise draws the mean of "dreg" is the mean of "iwae" (unbiased: max 1.69 standard errors measured, bound 4) and the mean
    of "stl" is not (biased for K > 1: 11.3 standard errors measured, bound > 6 -- the statistic has power).
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_gradient_reference as er   # noqa: E402

SPECS = [(2, 16, 3, 5), (3, 16, 70, 3), (2, 16, 1, 4)]          # (L, M, K, B)


def _rel(got, ref):
    return np.abs(np.asarray(got) - np.asarray(ref)).max() / max(np.abs(ref).max(), 1e-300)


_CACHE = {}


def _case(L, M, K, B):
    """spec, noise, and every estimator's surrogate and closed-form gradients, computed once per shape."""
    key = (L, M, K, B)
    if key not in _CACHE:
        from dgps_with_iwvi_amd import synthetic
        spec = synthetic.make_spec(L=L, M=M, B=B, K=K, with_lv=True, seed=3)
        zs = synthetic.make_noise(spec, seed=4)
        sur = {e: er.surrogate_gradients(spec, zs, e) for e in er.ESTIMATORS}
        _CACHE[key] = (spec, zs, sur, er.closed_form_gradients_of(spec, zs))
    return _CACHE[key]


@pytest.mark.parametrize("L,M,K,B", SPECS)
def test_iwae_through_the_helper_is_the_gradient_oracle(L, M, K, B):
    from oracle.grad_oracle import iw_elbo_and_gradients
    spec, zs, sur, _ = _case(L, M, K, B)
    val, ref = iw_elbo_and_gradients(spec, zs)
    bound, got = sur["iwae"]
    assert abs(bound - val) <= 1e-12 * abs(val)
    assert sorted(got) == sorted(n for n in ref if ".enc" in n) and got
    for n, g in got.items():
        print(n, _rel(g, ref[n]))
        assert _rel(g, ref[n]) <= 1e-12, n


@pytest.mark.parametrize("L,M,K,B", SPECS)
@pytest.mark.parametrize("estimator", er.ESTIMATORS)
def test_closed_form_is_the_gradient_of_the_surrogate(L, M, K, B, estimator):
    _, _, sur, closed = _case(L, M, K, B)
    got, ref = closed[estimator], sur[estimator][1]
    assert sorted(got) == sorted(ref)
    for n in ref:
        print(n, _rel(got[n], ref[n]))
        assert _rel(got[n], ref[n]) <= 1e-12, n


@pytest.mark.parametrize("L,M,K,B", SPECS)
def test_dreg_is_stl_at_one_sample_and_never_iwae(L, M, K, B):
    _, _, sur, closed = _case(L, M, K, B)
    for grads in ({e: sur[e][1] for e in er.ESTIMATORS}, closed):
        for n in grads["iwae"]:
            if K == 1:                                           # one sample: the normalised weight is exactly 1
                assert np.array_equal(grads["dreg"][n], grads["stl"][n]), n
            assert not np.allclose(grads["dreg"][n], grads["iwae"][n], rtol=1e-3, atol=0), n
    if K > 1:
        assert any(_rel(sur["dreg"][1][n], sur["stl"][1][n]) > 1e-3 for n in sur["dreg"][1])


def test_dreg_is_unbiased_and_stl_is_not():
    """3000 draws at make_spec(L=2, M=8, B=2, K=3, with_lv=True, seed=5): the largest |mean difference to "iwae"| over the encoder's
    elements in standard errors of that (paired: same draws) difference.  Measured: dreg 1.69, stl 11.3."""
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=2, M=8, B=2, K=3, with_lv=True, seed=5)
    R = 3000
    rows = {e: [] for e in er.ESTIMATORS}
    for r in range(R):
        g = er.closed_form_gradients_of(spec, synthetic.make_noise(spec, seed=100 + r))
        for e in er.ESTIMATORS:
            rows[e].append(np.concatenate([g[e][n].ravel() for n in sorted(g[e])]))
    rows = {e: np.asarray(v) for e, v in rows.items()}
    stat = {}
    for e in ("dreg", "stl"):
        d = rows[e] - rows["iwae"]
        stat[e] = float(np.abs(d.mean(0) / (d.std(0, ddof=1) / np.sqrt(R))).max())
    print(stat)
    assert stat["dreg"] < 4, stat
    assert stat["stl"] > 6, stat


def test_welford_reference_is_the_two_pass_mean_and_variance():
    rng = np.random.default_rng(0)
    xs = rng.standard_normal((7, 63)) * 3 + 100
    mean, m2, count = er.welford_reference(xs)
    assert count == 7
    assert _rel(mean, xs.mean(0)) <= 1e-14 and _rel(m2 / (count - 1), xs.var(0, ddof=1)) <= 1e-12
    mean1, m21, _ = er.welford_reference(xs[:1])
    assert np.array_equal(mean1, xs[0]) and not m21.any()


# -- surface ------------------------------------------------------------------------------------------------------------------------

def _header():
    text = open(os.path.join(ROOT, "include", "iwvi_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_estimators_additively_at_abi_19():
    text, code = _header()
    assert re.search(r"^#define IWVI_ABI_VERSION 19$", text, flags=re.M)
    m = re.search(r"enum\s*\{\s*IWVI_LV_GRAD_IWAE\s*=\s*0\s*,\s*IWVI_LV_GRAD_DREG\s*=\s*1\s*,\s*IWVI_LV_GRAD_STL\s*=\s*2\s*\}", code)
    assert m, "enum { IWVI_LV_GRAD_IWAE = 0, IWVI_LV_GRAD_DREG = 1, IWVI_LV_GRAD_STL = 2 }"
    for fn in ("iwvi_lv_layer_backward_ex", "iwvi_lv_encoder_backward_ex", "iwvi_moments_update"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, code), fn
    assert "typedef struct iwvi_moments_tensor" in code
    from dgps_with_iwvi_amd import _abi
    assert (_abi.LV_GRAD_IWAE, _abi.LV_GRAD_DREG, _abi.LV_GRAD_STL) == (0, 1, 2) and _abi.ABI_VERSION == 19
    assert ctypes.sizeof(_abi.MomentsTensor) == 32
    for fn in ("iwvi_lv_layer_backward_ex", "iwvi_lv_encoder_backward_ex", "iwvi_moments_update"):
        assert fn in _abi.PROTOTYPES


def _lib():
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    return _abi, _abi.lib()


def test_estimator_arguments_are_refused_before_any_hip_call():
    """Every refusal include/iwvi_hip.h lists, with otherwise complete arguments (host buffers: nothing may be launched on them, and on a
    GPU-less host nothing can be) -> IWVI_ERR_ARG and the function's name in iwvi_last_error()."""
    _abi, lib = _lib()
    Lw, B, K = 1, 4, 3
    buf = lambda n: (ctypes.c_float * n)()
    mu, raw, eps, w, d_enc, xy = buf(B * 2 * Lw), buf(B * 2 * Lw), buf(B * K * Lw), buf(B * K), buf(B * 2 * Lw), buf(B * 3)
    p = lambda b: ctypes.cast(b, ctypes.c_void_p)
    dims = (ctypes.c_int32 * 3)(3, 4, 2 * Lw)
    Ws, bs = [buf(12), buf(8)], [buf(4), buf(2)]
    arr = lambda bufs: (ctypes.c_void_p * len(bufs))(*[ctypes.addressof(b) for b in bufs])
    ws = (ctypes.c_char * 4096)()

    def layer(est, w_unit, sampled=1, weights=w):
        return lib.iwvi_lv_layer_backward_ex(p(mu), p(raw), 2 * Lw, 1, p(eps), None, 0, 0, None if weights is None else p(weights),
                                             Lw, B, K, sampled, est, w_unit, p(d_enc), None)

    def fused(est, w_unit, sampled=1, weights=w):
        return lib.iwvi_lv_encoder_backward_ex(p(mu), p(raw), 2 * Lw, 1, p(eps), None, 0, 0, None if weights is None else p(weights),
                                               Lw, B, K, sampled, est, w_unit, p(xy), arr(Ws), arr(bs), dims, 2, _abi.ACT_TANH,
                                               arr(Ws), arr(bs), p(ws), None)

    for call, name in ((layer, b"iwvi_lv_layer_backward"), (fused, b"iwvi_lv_encoder_backward")):
        cases = [((3, 1.0), b"estimator"), ((-1, 1.0), b"estimator"),
                 ((_abi.LV_GRAD_DREG, 1.0, 0), b"sampled"), ((_abi.LV_GRAD_STL, 1.0, 0), b"sampled"),
                 ((_abi.LV_GRAD_DREG, 1.0, 1, None), b"weights"), ((_abi.LV_GRAD_STL, 1.0, 1, None), b"weights")]
        cases += [((est, bad), b"w_unit") for est in (0, 1, 2) for bad in (0.0, -2.0, float("inf"), float("nan"))]
        for args, word in cases:
            assert call(*args) == -1, (name, args)
            msg = lib.iwvi_last_error()
            assert name in msg and word in msg, (name, args, msg)


def test_moments_update_refuses_bad_tables_before_any_hip_call():
    _abi, lib = _lib()
    x, mean, m2 = (ctypes.c_float * 4)(), (ctypes.c_double * 4)(), (ctypes.c_double * 4)()
    count = ctypes.c_int64(0)

    def table(**over):
        arr = (_abi.MomentsTensor * 1)()
        arr[0].x, arr[0].mean, arr[0].m2, arr[0].n = ctypes.addressof(x), ctypes.addressof(mean), ctypes.addressof(m2), 4
        for k, v in over.items():
            setattr(arr[0], k, v)
        return arr
    cp = ctypes.addressof(count)
    bad = [(None, 1, cp), (table(), 0, cp), (table(), -1, cp), (table(), _abi.MOMENTS_MAX_TENSORS + 1, cp), (table(), 1, None),
           (table(x=None), 1, cp), (table(mean=None), 1, cp), (table(m2=None), 1, cp), (table(n=-1), 1, cp)]
    for arr, n, c in bad:
        assert lib.iwvi_moments_update(arr, n, c, None) == -1
        assert b"iwvi_moments_update" in lib.iwvi_last_error()
    assert count.value == 0


def test_models_accept_the_estimators_their_bound_has():
    from dgps_with_iwvi_amd import likelihoods
    from dgps_with_iwvi_amd.models import DGP_IWVI, DGP_VI
    X, Y = np.zeros((3, 2)), np.zeros((3, 1))
    iw = DGP_IWVI(X, Y, [], likelihoods.Gaussian(0.1), num_samples=2)
    assert iw.encoder_gradient == "iwae"
    for name in ("dreg", "stl", "iwae"):
        iw.encoder_gradient = name
        assert iw.encoder_gradient == name
    for bad in ("DReG", "", None, 1):
        with pytest.raises(ValueError, match="encoder_gradient"):
            iw.encoder_gradient = bad
    assert iw.encoder_gradient == "iwae"
    vi = DGP_VI(X, Y, [], likelihoods.Gaussian(0.1))
    assert vi.encoder_gradient == "iwae"
    vi.encoder_gradient = "iwae"
    for bad in ("dreg", "stl", "nope"):
        with pytest.raises(ValueError, match="encoder_gradient"):
            vi.encoder_gradient = bad


def test_build_model_reads_the_setting_and_the_experiment_script_offers_it():
    import types
    from dgps_with_iwvi_amd import build_models
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((40, 2)), rng.standard_normal((40, 1))
    base = dict(mode="IWAE", configuration="L1_G1", M=8, likelihood_variance=0.01, minibatch_size=None, num_IW_samples=3, autotune_f64=False)
    import torch
    cpu = torch.device("cpu")
    assert build_models.build_model(types.SimpleNamespace(**base), X, Y, device=cpu).encoder_gradient == "iwae"
    assert build_models.build_model(types.SimpleNamespace(encoder_gradient="dreg", **base), X, Y, device=cpu).encoder_gradient == "dreg"
    with pytest.raises(ValueError, match="encoder_gradient"):
        build_models.build_model(types.SimpleNamespace(encoder_gradient="dreg", **dict(base, mode="VI")), X, Y, device=cpu)
    src = open(os.path.join(ROOT, "scripts", "run_experiment.py")).read()
    assert '"--encoder_gradient"' in src
