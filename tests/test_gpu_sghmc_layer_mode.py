"""``q_sqrt = None`` on ``layers.GPLayer`` (the SGHMC mode's layer, reference build_models.py:252-257): per-layer moments and the VI bound
against the float64 oracle's conditional called with ``q_sqrt=None`` plus the restatement's negative log prior (a test-side subclass of the
oracle's layer: oracle/ itself does not know the mode), ``propagate``'s regulariser, and ``backward.iw_elbo_and_gradients``.

Tolerances: those of tests/test_gpu_parity.py for the same family of shapes (mean rtol 2e-3 + atol 1e-3, variance rtol 2e-3 + atol 1e-4,
bound 1e-4 relative); the gradient against central differences of the device bound as in
tests/test_gpu_backward.py::test_full_size_gradient_agrees_with_central_differences_of_the_forward (2 % + the forward's noise / eps)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sghmc_reference as sr   # noqa: E402
from oracle import iwvi_oracle as O   # noqa: E402
from oracle.from_spec import build_oracle   # noqa: E402

pytestmark = pytest.mark.gpu

MEAN_TOL = dict(rtol=2e-3, atol=1e-3)
VAR_TOL = dict(rtol=2e-3, atol=1e-4)
ELBO_RTOL = 1e-4
CASES = [(L, M, S) for L in (1, 2) for M in (16, 33) for S in (1, 3)]
B = 9


class _PriorGPLayer(O.GPLayer):
    """The oracle's layer in the SGHMC mode: the conditional without q_sqrt, the negative log prior of q_mu in place of the KL."""

    def propagate(self, F, full_cov=False, z=None, **kwargs):
        samples, mean, cov = O.multisample_sample_conditional(F, self.Z, self.kern, self.q_mu, full_cov=full_cov, q_sqrt=None, white=True,
                                                              z=z, jitter=self.jitter)
        mf = self.mean_function(F)
        return samples + mf, mean + mf, cov, sr.neg_log_prior(self.q_mu)


def _build(dev, L, M, S, seed=7):
    from dgps_with_iwvi_amd import synthetic
    from dgps_with_iwvi_amd.models import DGP_VI
    spec = synthetic.make_spec(L=L, M=M, B=B, K=S, seed=seed + 10 * L + M)
    model = synthetic.build_model(spec, dev, cls=DGP_VI, num_samples=S)
    for layer in model.layers:
        layer.q_sqrt = None
    om = build_oracle(spec, iw=False, num_samples=S)
    for layer in om.layers:
        layer.__class__ = _PriorGPLayer
    zs = [np.asarray(z, np.float32).transpose(1, 0, 2).reshape(S * B, -1).astype(np.float64) for z in synthetic.make_noise(spec, seed=3)]
    zd = [torch.as_tensor(z, dtype=torch.float32, device=dev) for z in zs]
    return spec, model, om, zs, zd


@pytest.fixture(scope="module")
def built(gpu_device):
    cache = {}

    def get(L, M, S):
        if (L, M, S) not in cache:
            cache[(L, M, S)] = _build(gpu_device, L, M, S)
        return cache[(L, M, S)]
    return get


def test_q_sqrt_is_assignable_and_reads_back_none(gpu_device):
    from dgps_with_iwvi_amd import synthetic
    model = synthetic.build_model(synthetic.make_spec(L=2, M=16, B=B, K=1, seed=1), gpu_device)
    layer = model.layers[0]
    assert layer.q_sqrt is not None
    layer.q_sqrt = None
    assert layer.q_sqrt is None
    op = layer.q_sqrt_operand()
    assert tuple(op.shape) == (layer.num_outputs, 16, 16) and float(op.abs().max()) == 0.0
    assert layer.q_sqrt_operand().data_ptr() == op.data_ptr()     # one operand, owned by the layer


@pytest.mark.parametrize("L,M,S", CASES)
def test_moments_and_bound_match_the_oracle(built, L, M, S):
    spec, model, om, zs, zd = built(L, M, S)
    Xt = np.tile(spec["X"][:B], [S, 1])
    _, means_o, covs_o, kls_o, _ = om.propagate(Xt, zs=zs)
    _, means, covs, kls, _ = model.propagate(torch.as_tensor(Xt, dtype=torch.float32, device=model.X.device), zs=zd)
    for i in range(L):
        np.testing.assert_allclose(means[i].cpu().numpy(), means_o[i], **MEAN_TOL)
        np.testing.assert_allclose(covs[i].cpu().numpy(), covs_o[i], **VAR_TOL)
        kl = float(kls[i].item())
        assert np.isfinite(kl)
        prior = sr.neg_log_prior(spec["layers"][i]["q_mu"])
        assert abs(kl - prior) <= 1e-12 * prior, (i, kl, prior)
        assert abs(float(model.layers[i].kl.item()) - prior) <= 1e-12 * prior
    ref = om.build_likelihood(zs)
    got = model.compute_log_likelihood(zd)
    print("L=%d M=%d S=%d bound device %.8g oracle %.8g rel %.2e" % (L, M, S, got, ref, abs(got - ref) / abs(ref)))
    assert np.isfinite(got) and abs(got - ref) <= ELBO_RTOL * abs(ref), (got, ref)


@pytest.mark.parametrize("L,M,S", CASES)
def test_q_mu_gradients_against_central_differences_of_the_device_bound(built, L, M, S):
    from dgps_with_iwvi_amd import backward
    spec, model, om, zs, zd = built(L, M, S)
    elbo0, grads = backward.iw_elbo_and_gradients(model, zd)
    f0 = model.compute_log_likelihood(zd)
    assert np.isfinite(float(elbo0)) and abs(float(elbo0) - f0) <= 1e-5 * abs(f0), (float(elbo0), f0)
    assert not any(k.endswith("q_sqrt") for k in grads), sorted(grads)
    assert all(("l%d.q_mu" % i) in grads for i in range(L))
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert "l0.q_sqrt" not in dict(backward.parameter_list(model))
    gen = torch.Generator(device="cpu").manual_seed(5)
    noise = 2e-6 * abs(f0)
    for i in range(L):
        p = model.layers[i].q_mu
        g = grads["l%d.q_mu" % i].reshape(p.shape).double()
        for _ in range(3):
            d = torch.randn(p.shape, generator=gen).to(p.device)
            d = d / d.norm()
            gd = float((g * d.double()).sum())
            eps = min(0.02, 100.0 * noise / max(abs(gd), 1e-30))
            with torch.no_grad():
                p.add_(eps * d); fp = model.compute_log_likelihood(zd)
                p.add_(-2 * eps * d); fm = model.compute_log_likelihood(zd)
                p.add_(eps * d)
            fd = (fp - fm) / (2 * eps)
            print("L=%d M=%d S=%d l%d.q_mu: g.d %.6g central difference %.6g (eps %.3g)" % (L, M, S, i, gd, fd, eps))
            assert abs(fd - gd) <= 0.02 * abs(gd) + noise / eps, (i, fd, gd, eps)


def test_checkpoint_round_trips_the_mode(gpu_device, tmp_path):
    from dgps_with_iwvi_amd import build_models as bm, synthetic
    from dgps_with_iwvi_amd.models import DGP_VI
    spec = synthetic.make_spec(L=2, M=16, B=B, K=1, seed=2)
    a = synthetic.build_model(spec, gpu_device, cls=DGP_VI, num_samples=1)
    for layer in a.layers:
        layer.q_sqrt = None
    path = str(tmp_path / "sghmc_mode.npz")
    bm.save_checkpoint(a, path)
    b = synthetic.build_model(spec, gpu_device, cls=DGP_VI, num_samples=1)       # the same data, other parameters, the usual mode
    for layer in b.layers:
        layer.q_mu.add_(1.0)
    assert all(layer.q_sqrt is not None for layer in b.layers)
    bm.load_checkpoint(b, path)
    assert all(layer.q_sqrt is None for layer in b.layers)
    for la, lb in zip(a.layers, b.layers):
        assert torch.equal(la.q_mu, lb.q_mu)
    zd = [torch.as_tensor(np.asarray(z, np.float32).reshape(B, -1), device=gpu_device) for z in synthetic.make_noise(spec, seed=3, K=1)]
    assert a.compute_log_likelihood(zd) == b.compute_log_likelihood(zd)
