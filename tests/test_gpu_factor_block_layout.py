"""The block layout of the factorisation (csrc/precompute_dev.h: chol_blocks on 16x16 blocks with padded rows), pinned at the small shapes at
which a layout or a hand-off between the diagonal pass and the block rows below can go wrong: 1, 2, 3, 4, 5 and 8 blocks per side (windows
of 0, 1 and 2 block rows, rows beyond the window), a padded last block (M = 24, 80), and M = 144 for the route whose factor lives in the L2
workspace, not in LDS.  Criteria and tolerances of the residual test are those of
tests/test_gpu_parity.py::test_precompute_factorisation."""
import numpy as np
import pytest
import torch

from oracle import iwvi_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(M, D, R) for M in (16, 24, 32, 48, 64, 80, 128, 144) for D in (1, 8) for R in (1, 5)]


def _t(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)


def _inputs(M, D, R):
    rng = np.random.default_rng(M + D)
    Z = rng.standard_normal((M, D)).astype(np.float32)
    ls = ((0.7 + rng.random(D)) * np.sqrt(D)).astype(np.float32)
    q_mu = rng.standard_normal((M, R)).astype(np.float32)
    q_sqrt = (rng.standard_normal((R, M, M)) * 0.2 + np.eye(M)).astype(np.float32)
    return Z, ls, q_mu, q_sqrt


@pytest.mark.parametrize("M,D,R", SHAPES)
def test_factorisation_residuals(gpu_device, M, D, R):
    from dgps_with_iwvi_amd import kernels, settings
    from dgps_with_iwvi_amd.temp_workaround import GpState, precompute_states
    Z, ls, q_mu, q_sqrt = _inputs(M, D, R)
    k = kernels.RBF(D, variance=1.3, lengthscales=ls).to(gpu_device)
    st = GpState(M, R, gpu_device)
    precompute_states([st.desc(_t(Z, gpu_device), k, _t(q_mu, gpu_device), _t(q_sqrt, gpu_device), settings.jitter_level)])
    torch.cuda.synchronize()
    # the Gram the device factorises: of the float32-rounded, centred scaled inputs (test_precompute_factorisation)
    Zs32 = (Z.astype(np.float64) / ls.astype(np.float64)).astype(np.float32)
    zc = Zs32.astype(np.float64).mean(0).astype(np.float32)
    Zs = (Zs32 - zc).astype(np.float32).astype(np.float64)
    Kuu = O.RBF(D, variance=float(np.float32(1.3)), lengthscales=1.0).K(Zs) + 1e-6 * np.eye(M)
    Lm, Linv = st.Lm.double().cpu().numpy(), st.Linv.double().cpu().numpy()
    assert np.all(np.triu(Lm, 1) == 0) and np.all(np.triu(Linv, 1) == 0)
    np.testing.assert_allclose(Lm @ Lm.T, Kuu, rtol=0, atol=1e-12)
    np.testing.assert_allclose(Lm, np.linalg.cholesky(Kuu), rtol=0, atol=1e-6)
    np.testing.assert_allclose(Linv @ Lm, np.eye(M), atol=1e-7)
    np.testing.assert_allclose(float(st.kl.item()), O.gauss_kl(q_mu, q_sqrt), rtol=1e-6)


@pytest.mark.parametrize("M,D,R", SHAPES)
def test_no_uninitialised_tail(gpu_device, M, D, R):
    """The same inputs through a layer whose flags ask for every region of the factorisation's LDS carve (IWVI_GP_WANT_DENSE: the diagonal
    inverses and the inversion's scratch) and through one that asks for none: byte-equal state buffers, outside the dense outputs only the
    first writes (and, M > 128, the L2 workspace the dense inversion overwrites in place).  Both buffers are poisoned first, so that a tail
    one route leaves unwritten is a difference, not two equal leftovers."""
    from dgps_with_iwvi_amd import _abi, kernels, settings
    from dgps_with_iwvi_amd.temp_workaround import GpState, precompute_states
    Z, ls, q_mu, q_sqrt = _inputs(M, D, R)
    k = kernels.RBF(D, variance=1.3, lengthscales=ls).to(gpu_device)
    ops = (_t(Z, gpu_device), k, _t(q_mu, gpu_device), _t(q_sqrt, gpu_device), settings.jitter_level)
    bufs = []
    for flags in (0, _abi.GP_WANT_DENSE):
        st = GpState(M, R, gpu_device)
        st.buf.fill_(0xA5)
        d = st.desc(*ops)
        d.flags = flags
        precompute_states([d])
        torch.cuda.synchronize()
        bufs.append((st, st.buf.cpu().numpy().copy()))
    (st, plain), (_, dense) = bufs
    lo = st.offsets["LsP"]                                      # (Lm and Linv come first in the state buffer)
    assert lo > st.offsets["Linv"] > st.offsets["Lm"] == 0
    nbk = st.Mp // 16
    ws0 = (st.offsets["kl"] + 8 * _abi.MAX_R + 255) // 256 * 256
    ws1 = ws0 + 8 * 16 * 17 * (nbk * (nbk + 1) // 2 + nbk + (nbk * nbk + 3) // 4)
    assert ws1 <= plain.size
    if M > 128:
        np.testing.assert_array_equal(plain[lo:ws0], dense[lo:ws0])
        np.testing.assert_array_equal(plain[ws1:], dense[ws1:])
    else:
        np.testing.assert_array_equal(plain[lo:], dense[lo:])
        assert np.all(plain[ws0:ws1] == 0xA5)                   # the factor stayed in LDS: nothing leaves as blocks
    assert np.all(plain[:lo] == 0xA5) and not np.all(dense[:lo] == 0xA5)


def test_model_evaluation_is_reproducible(gpu_device):
    """Two-layer M = 32 model, B = 64, K = 4: two evaluations from the same noise counter give the same bits."""
    from dgps_with_iwvi_amd import settings, synthetic
    spec = synthetic.make_spec(L=2, M=32, B=64, K=4, with_lv=False, seed=5)
    settings.set_seed(11)
    model = synthetic.build_model(spec, gpu_device)
    got = []
    for _ in range(2):
        model._words().zero_()
        elbo, logp, _ = model._elbo_parts(None)
        torch.cuda.synchronize()
        got.append((elbo.detach().cpu().numpy().copy(), logp.detach().cpu().numpy().copy()))
    assert np.isfinite(got[0][0]).all() and np.isfinite(got[0][1]).all() and got[0][1].shape == (64,)
    assert got[0][0].tobytes() == got[1][0].tobytes()
    assert got[0][1].tobytes() == got[1][1].tobytes()
