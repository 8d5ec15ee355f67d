"""``iwvi_gp_layer_fullcov_ex`` called directly after a precompute through ``GpState`` (the way temp_workaround._factorise sets it up), at
the edges of k_fullcov's 32-row strips, with both kernels, S > 1 and R > 1, and BOTH templates chosen by the layer flag rather than by
the input dimension.  Workspace and outputs start as 0xFF bytes (NaN), so an element that is read or returned without having been
written shows.

White box: ``a`` [T, Mp] and ``u`` [R, T, Mp] are read back from the workspace and the covariance is re-formed from those very values
in float64, which isolates k_fullcov from the forward's own error.  That layout is csrc/gp_layer.hip's (a first, then u), NOT a promise
of include/iwvi_hip.h ("scratch"): a change of the layout has to change this test knowingly.  The inverse lengthscales are the state's
constant block (iwvi_gp_state_offsets: cst), the float32 numbers the kernel itself reads."""
import numpy as np
import pytest
import torch

from oracle import iwvi_oracle as O

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
VARIANCE = 1.1
VARIANCE32 = float(np.float32(VARIANCE))          # what crosses the C-ABI
# N, S, R, M, D, kernel: every N in {1, 31, 32, 33, 65, 300}, (S, R) in {(1, 1), (3, 2)}, M in {24 (Mp = 32), 64}, D in {1, 3, 8} and both
# kernels appear; the list runs with each template
SHAPES = [(1, 1, 1, 24, 1, "rbf"), (31, 3, 2, 64, 3, "matern"), (32, 3, 2, 24, 8, "rbf"), (33, 1, 1, 64, 8, "matern"),
          (33, 3, 2, 64, 1, "rbf"), (65, 3, 2, 24, 3, "rbf"), (300, 1, 1, 64, 1, "matern")]
_CACHE = {}


def _inputs(N, S, R, M, D, kern):
    """Inducing inputs on a jittered grid one lengthscale apart for D <= 3 (K_uu stays well-conditioned, so the float32 template is
    accurate there too), Gaussian for D = 8; test inputs inside the same region."""
    rng = np.random.default_rng(N * 1000 + M + D)
    if D <= 3:
        side = int(np.ceil(M ** (1.0 / D) - 1e-9))
        grid = np.stack(np.meshgrid(*[np.arange(side)] * D, indexing="ij"), -1).reshape(-1, D)[:M]
        ls = np.full(D, 0.9, np.float32)
        Z = ((grid - (side - 1) / 2.0) * 0.9 + 0.05 * rng.standard_normal((M, D))).astype(np.float32)
        X = (rng.uniform(-0.5, 0.5, (S, N, D)) * side * 0.9).astype(np.float32)
    else:
        ls = ((0.8 + 0.4 * rng.random(D)) * np.sqrt(D)).astype(np.float32)
        Z = rng.standard_normal((M, D)).astype(np.float32)
        X = rng.standard_normal((S, N, D)).astype(np.float32)
    q_mu = rng.standard_normal((M, R)).astype(np.float32)
    q_sqrt = (np.tril(rng.standard_normal((R, M, M))) * 0.1 / np.sqrt(M) + 0.5 * np.eye(M)).astype(np.float32)
    return Z, ls, X, q_mu, q_sqrt


def _oracle(shape):
    """The float64 conditional, computed once per shape and shared by the two templates."""
    if shape not in _CACHE:
        N, S, R, M, D, kern = shape
        Z, ls, X, q_mu, q_sqrt = _inputs(*shape)
        ko = (O.Matern52 if kern == "matern" else O.RBF)(D, float(np.float32(VARIANCE)), ls)
        _, m, cov = O.independent_multisample_sample_conditional(X, Z, ko, q_mu, q_sqrt=q_sqrt, white=True, full_cov=True)
        m.setflags(write=False)
        cov.setflags(write=False)
        _CACHE[shape] = (m, cov)
    return _CACHE[shape]


def _kernel_value(r2, kern):
    if kern == "matern":
        r = np.sqrt(r2 + 1e-12)
        return VARIANCE32 * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * np.exp(-np.sqrt(5.0) * r)
    return VARIANCE32 * np.exp(-0.5 * r2)


@pytest.mark.parametrize("f64", [False, True], ids=["f32_template", "f64_template"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-S%d-R%d-M%d-D%d-%s" % s)
def test_fullcov_direct(gpu_device, shape, f64):
    """Observed on an MI355X, max |cov - white-box reference| / bound: float32 template <= 0.12, float64 template <= 0.50."""
    from dgps_with_iwvi_amd import _abi, kernels, settings
    from dgps_with_iwvi_amd.temp_workaround import GpState, precompute_states
    N, S, R, M, D, kern = shape
    dev = gpu_device
    Z, ls, X, q_mu, q_sqrt = _inputs(*shape)
    T, Mp = S * N, (M + 15) // 16 * 16
    k = (kernels.Matern52 if kern == "matern" else kernels.RBF)(D, variance=VARIANCE, lengthscales=ls).to(dev)
    Zd, qmd, qsd, Xd = (torch.as_tensor(a, device=dev) for a in (Z, q_mu, q_sqrt, X))
    st = GpState(M, R, dev)
    d = st.desc(Zd, k, qmd, qsd, settings.jitter_level)
    if f64:
        d.flags |= _abi.GP_F64_STAGE1
    precompute_states([d])
    flags = _abi.LAYER_F64_STAGE1 if f64 else 0
    lib = _abi.lib()
    nws = lib.iwvi_gp_fullcov_ws_bytes(T, M, R)
    assert nws == 4 * T * Mp * (R + 1)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=dev)
    mean = torch.full((S * N * R * 4,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32).view(S, N, R)
    cov = torch.full((S * R * N * N * 4,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32).view(S, R, N, N)
    assert bool(torch.isnan(cov).all()) and bool(torch.isnan(ws.view(torch.float32)).all())
    _abi.check(lib.iwvi_gp_layer_fullcov_ex(_abi.ptr(st.buf), M, D, R, k.kern_type, k.variance, _abi.ptr(Xd), S, N,
                                            _abi.MF_ZERO, None, None, _abi.ptr(mean), _abi.ptr(cov), _abi.ptr(ws), flags, _abi.stream_ptr()))
    var = torch.full((T, R), float("nan"), device=dev)               # the marginal-variance route on the same state, same flags
    _abi.check(lib.iwvi_gp_layer_forward_ex(_abi.ptr(st.buf), M, D, R, R, k.kern_type, k.variance, _abi.ptr(Xd), None, None,
                                            _abi.MF_ZERO, None, None, None, None, _abi.ptr(var), T, 1, flags, _abi.stream_ptr()))
    torch.cuda.synchronize()
    assert bool(_abi.lib().iwvi_debug_last_forward_variant() >> 12 & 1) == f64      # the template asked for is the one that ran
    cov_t = cov
    cov, mean = cov.double().cpu().numpy(), mean.double().cpu().numpy()
    assert not np.isnan(cov).any() and not np.isnan(mean).any()
    assert torch.equal(cov_t, cov_t.transpose(2, 3))                                # bitwise symmetric

    # ---- white box: the workspace as csrc/gp_layer.hip lays it out ----
    wsf = ws.view(torch.float32)
    a = wsf[:T * Mp].view(T, Mp).double().cpu().numpy()
    u = wsf[T * Mp:].view(R, T, Mp).double().cpu().numpy()
    assert not np.isnan(a).any() and not np.isnan(u).any()                          # k_fullcov reads all of it: all of it must be written
    assert np.all(a[:, M:] == 0) and np.all(u[:, :, M:] == 0)                       # pad columns M .. Mp enter the dot products
    invls = st.view("cst", torch.float32, 64)[:D].double().cpu().numpy()
    np.testing.assert_allclose(invls, 1.0 / ls.astype(np.float64), rtol=4 * U32)      # a float32 reciprocal, at most an ulp off
    a3, u4 = a.reshape(S, N, Mp), u.reshape(R, S, N, Mp)
    worst = 0.0
    for s in range(S):
        diff = (X[s].astype(np.float64)[:, None, :] - X[s].astype(np.float64)[None, :, :]) * invls
        r2 = (diff ** 2).sum(-1)
        kv = _kernel_value(r2, kern)
        aa, abs_aa = a3[s] @ a3[s].T, np.abs(a3[s]) @ np.abs(a3[s]).T
        for r in range(R):
            uu, abs_uu = u4[r, s] @ u4[r, s].T, np.abs(u4[r, s]) @ np.abs(u4[r, s]).T
            ref = kv - aa + uu
            if f64:       # differenced and summed in float64, rounded once; one ulp of the float32 inverse lengthscale is in r2 on both sides
                bound = 2 * U32 * (np.abs(ref) + kv * (1.0 + r2))
            else:         # sequential fma dots of length Mp, the fast exponential, float32 r2
                bound = (Mp + 8) * U32 * (kv * (2.0 + r2) + abs_aa + abs_uu)
            err = np.abs(cov[s, r] - ref)
            assert np.all(err <= bound), (s, r, float((err / bound).max()), np.argwhere(err > bound)[:3])
            worst = max(worst, float((err / bound).max()))
    print("fullcov %s %s: max |cov - white-box reference| / bound = %.3g" % (shape, "f64" if f64 else "f32", worst))

    # ---- end to end against the float64 oracle, and the diagonal against the marginal-variance route ----
    mo, covo = _oracle(shape)
    np.testing.assert_allclose(mean, mo, rtol=2e-3, atol=1e-3)
    np.testing.assert_allclose(cov, covo, rtol=2e-3, atol=1e-4)
    diag = np.diagonal(cov, axis1=-2, axis2=-1).transpose(0, 2, 1).reshape(T, R)
    np.testing.assert_allclose(diag, var.double().cpu().numpy(), rtol=1e-4, atol=2e-5)
