"""``iwvi_unwhiten`` called directly (white=False, temp_workaround.py:63-65): f_w = Lm^-1 f and q_sqrt_w[r] = Lm^-1 tril(q_sqrt[r]) are
float64 sums rounded to float32 once, so they are checked to the float32 ulp against the same products formed in NumPy float64 from the
device's own dense Lm^-1 (read out of the state as tests/test_gpu_parity.py::test_precompute_factorisation reads it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _state_with_dense_inverse(dev, M, R, seed):
    """A state precomputed with IWVI_GP_WANT_DENSE on some well-spread inducing inputs -> (GpState, Linv [M, M] float64 NumPy)."""
    from dgps_with_iwvi_amd import _abi, kernels, settings
    from dgps_with_iwvi_amd.temp_workaround import GpState, precompute_states
    rng = np.random.default_rng(seed)
    D = 4
    Z = torch.as_tensor(rng.standard_normal((M, D)).astype(np.float32), device=dev)
    kern = kernels.RBF(D, variance=1.3, lengthscales=np.full(D, 1.5, np.float32)).to(dev)
    q_mu = torch.zeros(M, R, device=dev)
    q_sqrt = torch.eye(M, device=dev).repeat(R, 1, 1).contiguous()
    st = GpState(M, R, dev)
    d = st.desc(Z, kern, q_mu, q_sqrt, settings.jitter_level)
    d.flags |= _abi.GP_WANT_DENSE
    precompute_states([d])
    torch.cuda.synchronize()
    Linv = st.view("Linv", torch.float64, st.Mp * st.Mp).view(st.Mp, st.Mp)[:M, :M].cpu().numpy().copy()
    assert np.all(np.triu(Linv, 1) == 0) and np.all(np.diagonal(Linv) > 0)
    return st, Linv


def _within_one_ulp(got, ref64):
    """got: float32 values (as float64); ref64: the float64 value.  One float32 spacing at the reference's magnitude."""
    return np.abs(got - ref64) <= np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("M,R", [(1, 1), (1, 17), (15, 3), (16, 17), (17, 3), (40, 17), (100, 3), (512, 1), (512, 3)])
def test_unwhiten_to_the_ulp(gpu_device, M, R):
    """Every element of f_w and q_sqrt_w is written (the outputs start as NaN), the strict upper triangle of q_sqrt_w is exactly 0 -- the
    input's upper triangle is non-zero and must be ignored --, everything else is within one float32 ulp of the float64 product.  M on
    both sides of the 16-wide tile, R = 17 puts the columns of f across a tile edge -- and at M <= 16 beyond the
    column tiles a q_sqrt batch needs (the launch was once sized by M alone: column 16 of f_w stayed unwritten at M = 16, R = 17)."""
    from dgps_with_iwvi_amd import _abi
    st, Linv = _state_with_dense_inverse(gpu_device, M, R, 1000 * M + R)
    rng = np.random.default_rng(M + R)
    f = rng.standard_normal((M, R)).astype(np.float32)
    q = (0.3 * rng.standard_normal((R, M, M)) + np.eye(M)).astype(np.float32)               # full: upper triangle ~ 0.3
    fd, qd = torch.as_tensor(f, device=gpu_device), torch.as_tensor(q, device=gpu_device)
    f_w = torch.full((M, R), NAN, device=gpu_device)
    q_w = torch.full((R, M, M), NAN, device=gpu_device)
    _abi.check(_abi.lib().iwvi_unwhiten(_abi.ptr(st.buf), M, R, _abi.ptr(fd), _abi.ptr(qd), _abi.ptr(f_w), _abi.ptr(q_w), _abi.stream_ptr()))
    torch.cuda.synchronize()
    f_w, q_w = f_w.double().cpu().numpy(), q_w.double().cpu().numpy()
    assert not np.isnan(f_w).any() and not np.isnan(q_w).any()
    iu = np.triu_indices(M, 1)
    assert np.all(q_w[:, iu[0], iu[1]] == 0)
    ok_f = _within_one_ulp(f_w, Linv @ f.astype(np.float64))
    assert ok_f.all(), np.argwhere(~ok_f)[:5]
    ref_q = np.tril(Linv @ np.tril(q.astype(np.float64)))                                   # [R, M, M]; lower triangular by construction
    ok_q = _within_one_ulp(q_w, ref_q)
    assert ok_q.all(), np.argwhere(~ok_q)[:5]
    assert np.abs(np.diagonal(q_w, axis1=1, axis2=2)).min() > 0                             # and it is not trivially zero

    # q_sqrt == NULL: only f_w is written, the same values
    f_w2 = torch.full((M, R), NAN, device=gpu_device)
    _abi.check(_abi.lib().iwvi_unwhiten(_abi.ptr(st.buf), M, R, _abi.ptr(fd), None, _abi.ptr(f_w2), None, _abi.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(f_w2.double().cpu().numpy(), f_w)


def test_unwhiten_arguments(gpu_device):
    from dgps_with_iwvi_amd import _abi
    lib = _abi.lib()
    M, R = 8, 2
    st, _ = _state_with_dense_inverse(gpu_device, M, R, 3)
    f, q = torch.zeros(M, R, device=gpu_device), torch.zeros(R, M, M, device=gpu_device)
    f_w, q_w = torch.full((M, R), NAN, device=gpu_device), torch.full((R, M, M), NAN, device=gpu_device)
    a = [_abi.ptr(f), _abi.ptr(q), _abi.ptr(f_w), _abi.ptr(q_w), _abi.stream_ptr()]
    for m, r in ((0, R), (513, R), (-1, R), (M, 0), (M, 33)):
        assert lib.iwvi_unwhiten(_abi.ptr(st.buf), m, r, *a) == _abi.ERR_ARG, (m, r)
    assert lib.iwvi_unwhiten(None, M, R, *a) == _abi.ERR_ARG
    assert lib.iwvi_unwhiten(_abi.ptr(st.buf), M, R, None, _abi.ptr(q), _abi.ptr(f_w), _abi.ptr(q_w), _abi.stream_ptr()) == _abi.ERR_ARG
    assert lib.iwvi_unwhiten(_abi.ptr(st.buf), M, R, _abi.ptr(f), _abi.ptr(q), _abi.ptr(f_w), None, _abi.stream_ptr()) == _abi.ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(f_w).all()) and bool(torch.isnan(q_w).all())                    # a refused call writes nothing
