"""Pins tests/sghmc_reference.py (the float64 restatement the GPU tests of csrc/sghmc.hip compare with) by hand arithmetic and against
scipy, and the argument refusals of iwvi_sghmc_step / iwvi_neg_log_prior, which come before any HIP call and so need no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sghmc_reference as sr   # noqa: E402


def test_neg_log_prior_against_scipy():
    from scipy.stats import multivariate_normal
    rng = np.random.default_rng(0)
    M, R = 3, 2
    q_mu = rng.standard_normal((M, R))
    want = -sum(multivariate_normal(mean=np.zeros(M), cov=np.eye(M)).logpdf(q_mu[:, r]) for r in range(R))
    assert abs(sr.neg_log_prior(q_mu) - want) <= 1e-14 * abs(want)
    assert sr.neg_log_prior(np.zeros((M, R))) == pytest.approx(0.5 * M * R * np.log(2 * np.pi), rel=1e-15)


def test_init_state():
    s = sr.init_state([[0.5, -2.0]])
    assert s["theta"].dtype == np.float64
    assert (s["xi"] == 1).all() and (s["g"] == 1).all() and (s["g2"] == 1).all() and (s["p"] == 0).all()


# one element by hand.  State xi = 3, g = 0.5, g2 = 4, p = 0.25, theta = 1; d bound / d theta = -2 (grad of nll = +2); n = 0.5;
# epsilon = 0.1, mdecay = 0.2, num_data = 25:
#   r = 1/4;  g' = 3/4 * 0.5 + 1/4 * 2 = 0.875;  g2' = 3/4 * 4 + 1/4 * 4 = 4;  xi' = 1 + 3 (1 - 0.25 / 4) = 3.8125
#   Minv = 1 / sqrt(4) = 0.5 (the two 1e-16 move it by 1e-17 relative);  eps_s = 0.1 / 5 = 0.02
#   sigma = sqrt(2 * 0.0004 * 0.2 * 0.5) = sqrt(8e-5);  p' = 0.25 - 0.01 * 0.5 * 2 - 0.2 * 0.25 + sqrt(8e-5) * 0.5
_HAND = dict(state=dict(theta=[1.0], xi=[3.0], g=[0.5], g2=[4.0], p=[0.25]), grad_bound=[-2.0], noise=[0.5],
             epsilon=0.1, mdecay=0.2, num_data=25)
_P1 = 0.25 - 0.01 - 0.05 + 0.5 * np.sqrt(8e-5)


@pytest.mark.parametrize("burn_in", [False, True])
def test_one_element_by_hand(burn_in):
    new, mag = sr.step(burn_in=burn_in, **_HAND)
    assert new["p"][0] == pytest.approx(_P1, rel=1e-14)
    assert new["theta"][0] == pytest.approx(1.0 + _P1, rel=1e-14)
    if burn_in:
        assert new["g"][0] == pytest.approx(0.875, rel=1e-15)
        assert new["g2"][0] == pytest.approx(4.0, rel=1e-15)
        assert new["xi"][0] == pytest.approx(3.8125, rel=1e-14)
    else:                                                        # the sample op leaves xi, g, g2 alone
        assert new["xi"][0] == 3.0 and new["g"][0] == 0.5 and new["g2"][0] == 4.0
    assert mag["p"][0] == pytest.approx(0.25 + 0.01 + 0.05 + 0.5 * np.sqrt(8e-5), rel=1e-14)
    assert mag["theta"][0] == pytest.approx(1.0 + mag["p"][0], rel=1e-15)


def test_step_does_not_modify_its_input_and_floors_sigma():
    st = sr.init_state(np.array([0.0, 1.0]))
    before = {k: v.copy() for k, v in st.items()}
    new, _ = sr.step(st, [0.0, 0.0], [1.0, -1.0], epsilon=1e-9, mdecay=0.05, num_data=1e6, burn_in=True)
    for k in st:
        assert (st[k] == before[k]).all()
    # noise scale 2 eps_s^2 mdecay Minv = 1e-25 is below the floor: sigma = sqrt(1e-16) = 1e-8
    assert new["p"] == pytest.approx([1e-8, -1e-8], rel=1e-12)
    # a zero gradient: g' = (1 - r) g, g2' = (1 - r) g2 with r = 1/2; xi' = 1 + 1 (1 - 1 / (1 + 1e-16)) = 1 (to rounding)
    assert new["g"] == pytest.approx([0.5, 0.5]) and new["g2"] == pytest.approx([0.5, 0.5]) and new["xi"] == pytest.approx([1.0, 1.0], abs=1e-15)


# ---- argument refusals of the two entry points (before any HIP call: a GPU-less host can make them) ----------------------------------
def _lib():
    from dgps_with_iwvi_amd import _abi
    return _abi, _abi.lib()


def _tensor(_abi, n=4, **over):
    t = _abi.SghmcTensor()
    fake = 0x1000                                                # never dereferenced: every call below is refused first
    t.theta = t.grad = t.xi = t.g = t.g2 = t.p = t.theta64 = t.noise = fake
    t.n = n
    for k, v in over.items():
        setattr(t, k, v)
    return t


def _step(_abi, lib, tensors, n=None, epsilon=0.01, mdecay=0.05, num_data=100.0, rng_state=None):
    arr = (_abi.SghmcTensor * max(len(tensors), 1))(*tensors)
    rc = lib.iwvi_sghmc_step(arr if tensors else None, len(tensors) if n is None else n, epsilon, mdecay, num_data, 1, 0, rng_state, None)
    return rc, lib.iwvi_last_error().decode()


def test_sghmc_step_refuses_bad_arguments():
    _abi, lib = _lib()
    ok = _tensor(_abi)
    cases = [
        ([], None, {}, "tensors"),
        ([ok], 0, {}, "tensors"),
        ([ok] * (_abi.SGHMC_MAX_TENSORS + 1), None, {}, "tensors"),
        ([_tensor(_abi, n=0)], None, {}, "bad tensor 0"),
        ([ok, _tensor(_abi, theta64=None)], None, {}, "bad tensor 1"),
        ([_tensor(_abi, grad=None)], None, {}, "bad tensor 0"),
        ([_tensor(_abi, p=None)], None, {}, "bad tensor 0"),
        ([ok], None, dict(epsilon=0.0), "epsilon"),
        ([ok], None, dict(epsilon=float("nan")), "epsilon"),
        ([ok], None, dict(mdecay=-1.0), "mdecay"),
        ([ok], None, dict(num_data=0.0), "num_data"),
        ([ok], None, dict(num_data=float("inf")), "num_data"),
        ([_tensor(_abi, noise=None)], None, {}, "rng_state"),     # in-kernel noise without the device counter
    ]
    for tensors, n, kw, word in cases:
        rc, msg = _step(_abi, lib, tensors, n=n, **kw)
        assert rc == _abi.ERR_ARG, (word, rc)
        assert "iwvi_sghmc_step" in msg and word in msg, (word, msg)


def test_neg_log_prior_refuses_bad_arguments():
    _abi, lib = _lib()
    fake = ctypes.c_void_p(0x1000)
    for q, M, R, out in [(None, 3, 2, fake), (fake, 3, 2, None), (fake, 0, 2, fake), (fake, 3, 0, fake),
                         (fake, _abi.MAX_M + 1, 2, fake), (fake, 3, _abi.MAX_R + 1, fake)]:
        assert lib.iwvi_neg_log_prior(q, M, R, out, None) == _abi.ERR_ARG
        assert "iwvi_neg_log_prior" in lib.iwvi_last_error().decode()
