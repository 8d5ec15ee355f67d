"""tests/bound_family_reference.py pinned on the CPU: its weights against float64 autograd, its special cases against
tests/iw_reduction_reference.py, the orderings of the family, the effective sample size at its two ends, the float32 restatement of the
device recurrence inside the counted tolerance -- and ``models.Bound``: constructors, ``parse`` / ``repr`` and the validation."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bound_family_reference as F   # noqa: E402
import iw_reduction_reference as R   # noqa: E402

CASES = [(3, K, G) for K, G in F.KG_PAIRS]


def _torch_bound(L, G, tau, beta):
    B, K = L.shape
    X = F.f32v(tau) * L.reshape(B, G, K // G)
    lse = torch.logsumexp(X, 2) - float(np.log(K // G))
    return F.f32v(beta) * L.mean(1) + (1.0 - F.f32v(beta)) * (lse / F.f32v(tau)).mean(1)


@pytest.mark.parametrize("name", F.FAMILIES)
def test_weights_are_the_autograd_gradient_of_the_bound(name):
    for B, K, G in CASES:
        for tau, beta in F.TAU_BETA:
            L = R.family(name, B, K, seed=5)
            Lt = torch.tensor(L, dtype=torch.float64, requires_grad=True)
            val = _torch_bound(Lt, G, tau, beta)
            (grad,) = torch.autograd.grad(val.sum(), Lt)
            what = (name, K, G, tau, beta)
            assert np.allclose(val.detach().numpy(), F.bound_n(L, G, tau, beta), rtol=1e-13, atol=1e-12), what
            w = F.omega(L, G, tau, beta)
            assert np.allclose(grad.numpy(), w, rtol=1e-12, atol=1e-15), what
            assert np.allclose(w.sum(1), 1.0, rtol=0, atol=1e-13), what


@pytest.mark.parametrize("name", F.FAMILIES)
def test_special_cases_reduce_to_the_importance_weight_reference(name):
    for B, K, G in CASES:
        L = R.family(name, B, K, seed=6)
        assert np.allclose(F.bound_n(L, 1, 1.0, 0.0), R.logp(L), rtol=1e-14, atol=1e-12), (name, K)
        vi = R.logp(L, mode_vi=True)
        assert np.allclose(F.bound_n(L, G, 0.5, 1.0), vi, rtol=1e-14, atol=1e-12), (name, K, G)
        assert np.allclose(F.bound_n(L, K, 1.0, 0.0), vi, rtol=1e-13, atol=1e-9), (name, K)      # groups = K: every group one sample
        assert np.allclose(F.omega(L, K, 1.0, 0.3), 1.0 / K, rtol=1e-13), (name, K)
        w, dm, dv, dl = F.heads(L, np.zeros((B, K, 2)), np.ones((B, K, 2)), np.ones((B, 2)), 0.4, 2.5)
        wr, dmr, dvr, dlr = R.heads(L, np.zeros((B, K, 2)), np.ones((B, K, 2)), np.ones((B, 2)), 0.4, 2.5)
        assert np.allclose(w, wr, rtol=1e-13) and np.allclose(dm, dmr, rtol=1e-13) and np.allclose(dv, dvr, rtol=1e-13) and np.isclose(dl, dlr, rtol=1e-12)
        w, _, _, dl = F.heads(L, np.zeros((B, K, 2)), np.ones((B, K, 2)), np.ones((B, 2)), 0.4, 2.5, G, 1.0, 1.0)
        wr, _, _, dlr = R.heads(L, np.zeros((B, K, 2)), np.ones((B, K, 2)), np.ones((B, 2)), 0.4, 2.5, mode_vi=True)
        assert np.allclose(w, wr, rtol=1e-13) and np.isclose(dl, dlr, rtol=1e-12)


@pytest.mark.parametrize("name", F.FAMILIES)
def test_orderings_hold_per_point(name):
    """bound_n(beta = 1) <= miwae(G) <= iwae, and the tempered term does not decrease in tau (Jensen; exact arithmetic -- here up to
    float64 rounding at the magnitude of the values)."""
    for B, K, G in CASES:
        L = R.family(name, B, K, seed=7)
        # (float64 rounding of tau L + log s - log K_g at the magnitude of max(|L|, log K), divided by the smallest tau below)
        slack = 64 * np.spacing(np.maximum(np.abs(L).max(1), np.log(K) + 1.0)) / 0.05
        elbo, mi, iw = F.bound_n(L, 1, 1.0, 1.0), F.bound_n(L, G, 1.0, 0.0), F.bound_n(L, 1, 1.0, 0.0)
        assert np.all(elbo <= mi + slack) and np.all(mi <= iw + slack), (name, K, G)
        taus = (0.05, 0.25, 0.5, 0.75, 1.0)
        vals = [F.tempered(L, G, t) for t in taus]
        for lo, hi in zip(vals[:-1], vals[1:]):
            assert np.all(lo <= hi + slack), (name, K, G)
        assert np.all(elbo <= vals[0] + slack), (name, K, G)
        ci = F.bound_n(L, 1, 1.0, 0.3)
        assert np.all(elbo <= ci + slack) and np.all(ci <= iw + slack), (name, K)


def test_effective_sample_size_at_its_two_ends():
    for B, K, G in CASES:
        assert np.allclose(F.ess(R.family("ties_all", B, K, seed=8)), K, rtol=1e-14), K
        if K > 1:
            assert np.all(np.abs(F.ess(R.family("dominant", B, K, seed=8)) - 1.0) <= 1e-6), K
        e = F.ess(R.family("near_equal", B, K, seed=8))
        assert np.all(e >= 1.0 - 1e-12) and np.all(e <= K + 1e-12), K


def test_float32_restatement_of_the_device_recurrence_is_inside_the_counted_tolerance():
    """The counted tolerance holds for the device's recurrence restated in NumPy float32 (NumPy's exponential in place of the hardware's),
    over every family, (K, G) pair and (tau, beta) pair of the GPU test; prints the worst ratio the module's docstring quotes."""
    worst = 0.0
    for name in F.FAMILIES:
        for B, K, G in CASES:
            for tau, beta in F.TAU_BETA:
                L = R.family(name, B, K, seed=9)
                err = np.abs(F.restate_f32(L, G, tau, beta) - F.bound_n(L, G, tau, beta))
                tol = F.tol_bound(L, G, tau, beta)
                worst = max(worst, float((err / tol).max()))
                assert np.all(err <= tol), (name, K, G, tau, beta, float((err / tol).max()))
    print("worst |restatement - statement| / tolerance: %.3f" % worst)
    assert worst <= 1.0


def test_tolerances_are_small_where_the_inputs_are():
    """The counted tolerances stay at float32 resolution on the O(10) families (nothing fitted has crept in)."""
    for name in ("near_equal", "ties_all", "ties_two", "dominant"):
        L = R.family(name, 5, 65, seed=10)
        assert F.tol_bound(L, 5, 1.0, 0.0).max() < 1.2e-5, name
        assert F.tol_bound(L, 5, 0.05, 0.0).max() < 1e-3, name
        assert F.tol_ess(L).max() < 65 * 1e-5, name


# ---- models.Bound ----------------------------------------------------------------------------------------------------------------------
def test_bound_constructors_parse_and_repr():
    from dgps_with_iwvi_amd.models import Bound
    assert Bound() == Bound.iwae() == Bound.parse("iwae") and Bound().is_default
    assert Bound.miwae(4) == Bound(groups=4) == Bound.parse("miwae:4")
    assert Bound.ciwae(0.5) == Bound(beta=0.5) == Bound.parse("ciwae:0.5")
    assert Bound.vr(0.3) == Bound(alpha=0.3) == Bound.parse("vr:0.3") and abs(Bound.vr(0.3).tau - 0.7) < 1e-15
    assert Bound.miwae(4) != Bound.miwae(2) and Bound.miwae(4) != Bound.iwae() and not Bound.miwae(4).is_default
    assert len({Bound.miwae(4), Bound.parse("miwae:4"), Bound.iwae()}) == 2
    for b in (Bound(), Bound.miwae(5), Bound.ciwae(0.3), Bound.vr(0.1 + 0.2), Bound(groups=2, alpha=0.25, beta=1.0)):
        assert Bound.parse(repr(b)) == b and Bound.parse(str(b)) == b, repr(b)
    assert Bound.parse(Bound.miwae(3)) == Bound.miwae(3)
    assert str(Bound.miwae(4)) == "miwae:4" and str(Bound()) == "iwae"
    d = Bound(groups=3, alpha=0.5, beta=0.25).desc()
    assert (d.groups, d.tau, d.beta) == (3, 0.5, 0.25)


@pytest.mark.parametrize("bad", [dict(groups=0), dict(groups=-2), dict(groups=2.5), dict(groups=True), dict(alpha=1.0), dict(alpha=-0.1),
                                 dict(alpha=float("nan")), dict(beta=-0.1), dict(beta=1.5), dict(beta=float("nan"))])
def test_bound_validation(bad):
    from dgps_with_iwvi_amd.models import Bound
    with pytest.raises(ValueError):
        Bound(**bad)


@pytest.mark.parametrize("text", ["", "miwae", "miwae:x", "miwae:0", "ciwae:2", "vr:1", "elbo", "miwae:2+miwae:4", "iwae:1", 3])
def test_bound_parse_refuses(text):
    from dgps_with_iwvi_amd.models import Bound
    with pytest.raises(ValueError):
        Bound.parse(text)


def test_bound_is_immutable_and_checks_the_samples_at_the_point_of_use():
    from dgps_with_iwvi_amd.models import Bound
    b = Bound.miwae(4)
    with pytest.raises(AttributeError):
        b.groups = 2
    b.check_samples(20)
    with pytest.raises(ValueError, match="does not divide num_samples=6"):
        b.check_samples(6)


def test_entry_points_refuse_a_bad_descriptor_without_touching_the_gpu():
    """Validation comes before any device work: error code and text on a GPU-less host too."""
    import ctypes
    from dgps_with_iwvi_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("libiwvi_hip.so not built (run __graft_entry__.build())")
    lib = _abi.lib()
    fake = ctypes.c_void_p(4096)                                  # never dereferenced: every call below is refused first

    def reduce(desc, K=6):
        return lib.iwvi_bound_logw_reduce(desc, fake, 4, K, K, 1, None, None, 0, 1.0, fake, None, None, None, None)

    def backward(desc, K=6):
        return lib.iwvi_bound_elbo_backward(desc, fake, fake, fake, 1, None, None, 0, 4, K, 0.5, None, 1.0, None, None, None, None, None, 0,
                                            fake, fake, None)

    def desc(groups=1, tau=1.0, beta=0.0):
        d = _abi.BoundDesc()
        d.groups, d.tau, d.beta = groups, tau, beta
        return d

    for call, name in ((reduce, b"iwvi_bound_logw_reduce"), (backward, b"iwvi_bound_elbo_backward")):
        assert call(None) == _abi.ERR_ARG and name in lib.iwvi_last_error() and b"descriptor" in lib.iwvi_last_error()
        for bad, word in ((desc(groups=0), b"groups"), (desc(groups=4), b"groups"), (desc(tau=0.0), b"tau"), (desc(tau=1.5), b"tau"),
                          (desc(tau=float("nan")), b"tau"), (desc(beta=-0.1), b"beta"), (desc(beta=1.1), b"beta"), (desc(beta=float("nan")), b"beta")):
            assert call(bad) == _abi.ERR_ARG, word
            assert name in lib.iwvi_last_error() and word in lib.iwvi_last_error(), lib.iwvi_last_error()
        assert call(desc(), K=0) == _abi.ERR_ARG
    assert lib.iwvi_bound_logw_reduce(desc(), None, 4, 6, 6, 1, None, None, 0, 1.0, fake, None, None, None, None) == _abi.ERR_ARG
    assert lib.iwvi_bound_logw_reduce(desc(), fake, 4, 6, 6, 1, None, None, 0, 1.0, None, None, fake, fake, None) == _abi.ERR_ARG   # out_elbo without out_logp
    assert lib.iwvi_bound_logw_reduce(desc(), fake, 4, 6, 6, 1, None, None, 0, 1.0, fake, None, fake, None, None) == _abi.ERR_ARG   # ... without a ticket
    assert lib.iwvi_bound_logw_reduce(desc(), fake, 4, 6, 6, 1, None, None, 17, 1.0, fake, None, fake, fake, None) == _abi.ERR_ARG  # too many global arrays
