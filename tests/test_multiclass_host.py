"""MultiClass (robust-max) without a GPU: the float64 restatement (tests/multiclass_restatement.py) against a closed form and a Monte
Carlo, the Python surface, the checkpoint state, the header's enum and the refusals of the library's entry points."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import multiclass_restatement as MR   # noqa: E402

# The 20-point rule against the exact two-class probability Phi((mu_y - mu_c) / sqrt(v_y + v_c)) on mu in [-3, 3], v in [0.25, 4]: 3.76e-3 at
# most over the 4000 draws of default_rng(3) with label 0 (4.39e-3 with both labels) -- the rule integrates a cdf of the OTHER class's width
# over the label's latent; that is GPflow's default, not a transcription matter.  A missing sqrt 2, a wrong clip or a wrong one-hot is orders of magnitude larger.
# The bound is for these draws: over the whole box the rule's own maximum is 8.1e-3, at the corner v_y = 4, v_c = 0.25,
# and other seeds of 4000 draws reach 5.4e-3 .. 6.7e-3 there; nothing here asserts the corner.
RULE_BOUND = 5e-3


def _phi(x):
    return 0.5 * torch.erfc(-torch.as_tensor(x) / math.sqrt(2.0))


def test_two_classes_match_the_closed_form():
    rng = np.random.default_rng(3)
    mu = rng.uniform(-3.0, 3.0, (4000, 2))
    v = rng.uniform(0.25, 4.0, (4000, 2))
    lik = MR.MultiClass(2, cdf_jitter=0.0)
    worst = 0.0
    for y in (0, 1):
        p = lik.prob_is_largest(np.full((4000, 1), float(y)), mu, v).numpy()[:, 0]
        want = _phi((mu[:, y] - mu[:, 1 - y]) / np.sqrt(v[:, 0] + v[:, 1])).numpy()
        worst = max(worst, float(np.abs(p - want).max()))
    print("C = 2: the rule deviates from the closed form by at most %.3e" % worst)
    assert worst <= RULE_BOUND, worst


def test_ten_classes_match_a_monte_carlo_of_argmax_frequencies():
    rng = np.random.default_rng(12)
    C, n_rows, draws = 10, 6, 400000
    mu = rng.uniform(-3.0, 3.0, (n_rows, C))
    v = rng.uniform(0.25, 4.0, (n_rows, C))
    lik = MR.MultiClass(C, cdf_jitter=0.0)
    for r in range(n_rows):
        f = mu[r] + np.sqrt(v[r]) * rng.standard_normal((draws, C))
        freq = np.bincount(f.argmax(1), minlength=C) / draws
        p = np.array([float(lik.prob_is_largest(np.array([[float(k)]]), mu[r:r + 1], v[r:r + 1])) for k in range(C)])
        se = np.sqrt(np.maximum(freq * (1 - freq), 1.0 / draws) / draws)
        print("row %d: max |p - freq| %.3e (4 se <= %.3e)" % (r, np.abs(p - freq).max(), 4 * se.max()))
        assert (np.abs(p - freq) <= RULE_BOUND + 4 * se).all(), (r, p, freq)


def test_restatement_is_consistent():
    rng = np.random.default_rng(13)
    mu, v = rng.uniform(-3, 3, (200, 2)), rng.uniform(0.25, 4.0, (200, 2))
    # at C = 2 the two integrands are mirror images under the symmetric rule ONLY when the variances agree; GPflow's rule otherwise
    # leaves the two p a little apart.  The mixture P of predict_mean_and_var is what must sum to 1 where p does:
    v[:, 1] = v[:, 0]
    P, V = MR.MultiClass(2).predict_mean_and_var(mu, v)
    assert float((P.sum(-1) - 1.0).abs().max()) <= 1e-12
    assert torch.equal(V, P - P ** 2)
    lik = MR.MultiClass(4, epsilon=0.01)
    F = np.array([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0]])
    for y, want in ((np.array([[1.0], [0.0], [2.0]]), [True, True, True]), (np.array([[2.0], [1.0], [3.0]]), [False, False, False])):
        got = lik.logp(F, y).numpy()[:, 0]                       # ties go to the FIRST maximum
        np.testing.assert_allclose(got, [math.log(0.99) if w else math.log(0.01 / 3) for w in want], rtol=0, atol=1e-15)
    # the three forms on one p
    mu4, v4, y4 = rng.uniform(-3, 3, (50, 4)), rng.uniform(1e-4, 4.0, (50, 4)), rng.integers(0, 4, (50, 1)).astype(np.float64)
    p = lik.prob_is_largest(y4, mu4, v4)
    assert tuple(p.shape) == (50, 1) and float(p.min()) > 0.0 and float(p.max()) < 1.0
    np.testing.assert_allclose(lik.variational_expectations(mu4, v4, y4).numpy(), (p * math.log(0.99) + (1 - p) * math.log(0.01 / 3)).numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(lik.predict_density(mu4, v4, y4).numpy(), torch.log(p * 0.99 + (1 - p) * 0.01 / 3).numpy(), rtol=0, atol=1e-14)
    Pm = lik.predict_mean_and_var(mu4, v4)[0]
    np.testing.assert_allclose(torch.gather(Pm, 1, torch.as_tensor(y4).long()).numpy(), (p * 0.99 + (1 - p) * 0.01 / 3).numpy(), rtol=0, atol=1e-14)


def test_python_surface_without_a_device():
    import dgps_with_iwvi.likelihoods as alias
    from dgps_with_iwvi_amd import _abi, likelihoods
    from dgps_with_iwvi_amd.models import DGP_VI
    assert alias.MultiClass is likelihoods.MultiClass and alias.RobustMax is likelihoods.RobustMax
    lik = likelihoods.MultiClass(5)
    for meth in ("logp", "variational_expectations", "predict_mean_and_var", "predict_density", "lik_desc", "check_targets"):
        assert callable(getattr(lik, meth)), meth
    d = lik.lik_desc()
    assert (d.type, d.param[1], d.param0_dev) == (_abi.LIK_MULTICLASS, 5.0, None) and abs(d.param[0] - 1e-3) < 1e-10
    assert _abi.LIK_MULTICLASS == 3
    assert lik.grad_name is None and lik.trained_scalar() is None and (lik.num_classes, lik.epsilon) == (5, 1e-3)
    d = likelihoods.MultiClass(3, invlink=likelihoods.RobustMax(3, 0.05)).lik_desc()
    assert abs(d.param[0] - 0.05) < 1e-8 and d.param[1] == 3.0
    with pytest.raises(NotImplementedError, match="softmax"):
        likelihoods.MultiClass(3, invlink="softmax")
    with pytest.raises(ValueError):
        likelihoods.MultiClass(3, invlink=likelihoods.RobustMax(4))
    for bad in (1, 33, 2.5):
        with pytest.raises(ValueError):
            likelihoods.MultiClass(bad)
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            likelihoods.RobustMax(3, bad)
    # targets: one column of integral labels in [0, C)
    lik.check_targets(np.array([[0.0], [4.0], [2.0]]))
    lik.check_targets(torch.tensor([[1.0], [3.0]]))
    for bad in (np.zeros((3, 5)), np.zeros(3), np.array([[5.0]]), np.array([[-1.0]]), np.array([[1.5]]), np.array([[float("nan")]])):
        with pytest.raises(ValueError, match="MultiClass"):
            lik.check_targets(bad)
    with pytest.raises(ValueError, match="MultiClass"):           # the models check at construction, before anything touches a device
        DGP_VI(np.zeros((2, 2)), np.array([[0.0], [7.0]]), [], lik)
    with pytest.raises(ValueError, match="5 outputs"):
        DGP_VI(np.zeros((2, 2)), np.array([[0.0], [1.0]]), [], lik)
    assert likelihoods.target_dim(lik, 5) == 1 and likelihoods.output_dim(lik, 1) == 5
    for other in (likelihoods.Gaussian(0.1), likelihoods.Bernoulli(), likelihoods.StudentT(), object()):
        assert likelihoods.target_dim(other, 3) == 3 and likelihoods.output_dim(other, 3) == 3
    assert not likelihoods.is_gaussian(lik)
    with pytest.raises(_abi.IwviError, match="no CPU fallback"):  # the arithmetic exists as HIP kernels only
        lik.logp(torch.zeros(3, 5), torch.zeros(3, 1))


def test_final_layer_width_is_checked_at_construction():
    from dgps_with_iwvi_amd import likelihoods, synthetic
    spec = MR.make_spec(3, B=7, K=2, lv=False)
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="4 outputs"):
        synthetic.build_model(spec, dev, likelihood=likelihoods.MultiClass(4))


def test_checkpoint_state_round_trip():
    from dgps_with_iwvi_amd import build_models, likelihoods
    lik = likelihoods.MultiClass(7, invlink=likelihoods.RobustMax(7, 0.02))
    st = build_models.likelihood_state(lik)
    assert str(st["likelihood.type"]) == "MultiClass" and st["likelihood.params"].tolist() == [7.0, 0.02]
    fresh = likelihoods.MultiClass(7)
    build_models.load_likelihood_state(fresh, st)
    assert (fresh.num_classes, fresh.epsilon) == (7, 0.02) and abs(fresh.lik_desc().param[0] - 0.02) < 1e-8
    with pytest.raises(ValueError, match="MultiClass"):
        build_models.load_likelihood_state(likelihoods.Bernoulli(), st)
    with pytest.raises(ValueError, match="MultiClass"):
        build_models.load_likelihood_state(fresh, build_models.likelihood_state(likelihoods.Gaussian(0.1)))
    with pytest.raises(ValueError, match="classes"):
        build_models.load_likelihood_state(likelihoods.MultiClass(6), st)


def test_header_names_the_type():
    text = open(os.path.join(ROOT, "include", "iwvi_hip.h")).read()
    assert "IWVI_LIK_MULTICLASS = 3" in text and "#define IWVI_ABI_VERSION 19" in text
    assert "ONE column of class labels" in text


def _lib():
    from dgps_with_iwvi_amd import _abi
    path = os.path.join(ROOT, "dgps_with_iwvi_amd", "csrc", "libiwvi_hip.so")
    if not os.path.exists(path):
        pytest.skip("libiwvi_hip.so is not built")
    return _abi, _abi.lib()


def _desc(_abi, eps, C):
    d = _abi.LikDesc()
    d.type, d.param[0], d.param[1] = _abi.LIK_MULTICLASS, eps, C
    return d


def test_refused_descriptors_and_shapes_return_before_any_launch():
    _abi, lib = _lib()
    p = ctypes.c_void_p(16)                                      # never dereferenced: every call below is refused on its arguments
    E = _abi.ERR_ARG
    entries = {
        "iwvi_lik_var_exp": lambda d, Dy=3: lib.iwvi_lik_var_exp(d, p, p, p, 4, Dy, 1, 4, p, None),
        "iwvi_lik_predict_density": lambda d, Dy=3: lib.iwvi_lik_predict_density(d, p, p, p, 4, Dy, 1, 4, p, None),
        "iwvi_lik_predict_mean_and_var": lambda d, Dy=3: lib.iwvi_lik_predict_mean_and_var(d, p, p, 4 * Dy, p, p, None),
        "iwvi_lik_elbo_reduce": lambda d, Dy=3: lib.iwvi_lik_elbo_reduce(d, p, p, p, 4, 2, Dy, 2, 1, None, None, 0, None, None, 0, 1.0, 2, 0,
                                                                         None, p, p, p, None),
        "iwvi_lik_elbo_backward": lambda d, Dy=3: lib.iwvi_lik_elbo_backward(d, p, p, p, Dy, None, None, 0, 4, 2, 1.0, 0, p, p, p, None, None, 0,
                                                                             None, 2, p, p, None),
    }
    bad = [(0.0, 3.0), (1.0, 3.0), (-0.1, 3.0), (float("nan"), 3.0), (1e-3, 1.0), (1e-3, 2.5), (1e-3, 33.0), (1e-3, float("nan"))]
    for name, call in entries.items():
        for eps, C in bad:
            assert call(_desc(_abi, eps, C)) == E, (name, eps, C)
            msg = lib.iwvi_last_error()
            assert name.encode() in msg and b"MultiClass" in msg, (name, msg)   # the text names the entry
    good = _desc(_abi, 1e-3, 3.0)
    for name, call in entries.items():
        if name == "iwvi_lik_predict_mean_and_var":
            continue
        assert call(good, Dy=4) == E, name                       # Dy must be the number of classes
        assert b"Dy = 3" in lib.iwvi_last_error()
    assert lib.iwvi_lik_predict_mean_and_var(good, p, p, 10, p, p, None) == E      # n = T C
    assert b"T x 3" in lib.iwvi_last_error()
    assert lib.iwvi_lik_var_exp(good, p, p, p, 0, 3, 1, 1, p, None) == 0           # T = 0: nothing to do, nothing launched
    assert lib.iwvi_lik_predict_mean_and_var(good, p, p, 0, p, p, None) == 0
