"""Bernoulli (probit) and Student-t likelihoods on the GPU against the float64 restatement (tests/lik_restatement.py, pinned by
tests/test_likelihoods_host.py), with injected noise.  Tolerances: the Gaussian tests' own for the same shapes (the layers are the same
kernels; tests/test_gpu_parity.py: bound 1e-4 relative; tests/test_gpu_lean_variant.py: per-point rtol 2e-4 + atol 2e-2;
tests/test_gpu_backward.py: gradients 5e-3 of each array's max-norm), and for the elementwise callables 4x the error recorded in
DESIGN.md section 6."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import lik_restatement as R   # noqa: E402

pytestmark = pytest.mark.gpu

ELBO_RTOL = 1e-4
# DESIGN.md section 6 records the maximum absolute error of the float32 callables over the grid of the host test (mu in [-3, 3],
# v in [1e-4, 4]) against the float64 restatement on the same float32 moments; asserted at 4x the record
ELEMENTWISE_RECORD = {"bernoulli": 1.503e-6, "student_t": 1.291e-6}


def _t(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)


def _liks(name):
    from dgps_with_iwvi_amd import likelihoods
    if name == "bernoulli":
        return likelihoods.Bernoulli(), R.Bernoulli()
    return likelihoods.StudentT(scale=0.7, df=4.0), R.StudentT(scale=0.7, df=4.0)


def _spec(name, L=2, M=32, B=12, K=4, lv=True, Dy=1, seed=3, **kw):
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=L, M=M, B=B, K=K, with_lv=lv, Dy=Dy, seed=seed, distinct_y=Dy > 1, **kw)
    if name == "bernoulli":
        spec["Y"] = (spec["Y"] > 0).astype(np.float64)            # two classes
    return spec


def _close(name, got, ref, rtol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-12)
    err = np.abs(got - ref).max()
    print("  %-12s max err %.3e of scale %.3e (%.2e relative)" % (name, err, scale, err / scale))
    assert err <= rtol * scale, "%s: max err %.3e vs scale %.3e" % (name, err, scale)


# ---- test 3: the elementwise callables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bernoulli", "student_t"])
def test_elementwise_callables_match_the_restatement(gpu_device, name):
    lik, ref = _liks(name)
    MU, V = R.moment_grid()
    ys = (0.0, 1.0) if name == "bernoulli" else (-1.5, 0.3, 2.5)
    mu32, v32 = MU.astype(np.float32), V.astype(np.float32)
    worst = 0.0
    for y in ys:
        Y = np.full_like(mu32, y)
        m, v, yy = (_t(a.reshape(-1, 1), gpu_device) for a in (mu32, v32, Y))
        m64, v64, y64 = mu32.astype(np.float64), v32.astype(np.float64), Y.astype(np.float64)
        pm, pv = lik.predict_mean_and_var(m, v)
        rm, rv = ref.predict_mean_and_var(m64, v64)
        pairs = [("var_exp", lik.variational_expectations(m, v, yy), ref.variational_expectations(m64, v64, y64)),
                 ("logp", lik.logp(m, yy), ref.logp(m64, y64)),
                 ("predict_density", lik.predict_density(m, v, yy), ref.predict_density(m64, v64, y64)),
                 ("predict_mean", pm, rm), ("predict_var", pv, rv)]
        for what, got, want in pairs:
            err = float(np.abs(got.cpu().numpy().reshape(-1).astype(np.float64) - want.numpy().reshape(-1)).max())
            print("%s y=%g %-16s max abs err %.3e" % (name, y, what, err))
            worst = max(worst, err)
    print("%s: worst %.3e (record %.3e)" % (name, worst, ELEMENTWISE_RECORD[name]))
    assert worst <= 4 * ELEMENTWISE_RECORD[name], worst


def test_bernoulli_predict_y_is_a_probability(gpu_device):
    """predict_y in (0, 1), equal to inv_probit(mu / sqrt(1 + v)) of predict_f at the same draw; the row tiling of the callables."""
    from dgps_with_iwvi_amd import synthetic, _abi
    spec = _spec("bernoulli", B=20, K=3)
    lik, ref = _liks("bernoulli")
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    X = spec["X"][:20]
    zs = [torch.zeros(20, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1], device=gpu_device) for l in spec["layers"]]
    m, v = model.predict_f(X, zs=zs)
    p, pv = model.predict_y(X, zs=zs)
    p64 = ref.predict_mean_and_var(m.cpu().double().numpy(), v.cpu().double().numpy())[0].numpy()
    assert float(p.min()) > 0.0 and float(p.max()) < 1.0
    np.testing.assert_allclose(p.cpu().numpy(), p64, rtol=0, atol=4 * ELEMENTWISE_RECORD["bernoulli"])
    np.testing.assert_allclose(pv.cpu().numpy(), p64 - p64 ** 2, rtol=0, atol=4 * ELEMENTWISE_RECORD["bernoulli"])
    # row_div / row_mod: 4 samples per data row read Y[t // 4]
    Fm, Fv = _t(np.linspace(-2, 2, 24).reshape(24, 1), gpu_device), _t(np.full((24, 1), 0.3), gpu_device)
    Y6 = _t((np.arange(6) % 2).reshape(6, 1), gpu_device)
    out = torch.empty_like(Fm)
    _abi.check(_abi.lib().iwvi_lik_var_exp(lik.lik_desc(), _abi.ptr(Fm), _abi.ptr(Fv), _abi.ptr(Y6), 24, 1, 4, 6, _abi.ptr(out), _abi.stream_ptr()))
    assert torch.equal(out, lik.variational_expectations(Fm, Fv, Y6.repeat_interleave(4, 0)))


# ---- tests 4 and 5: bound, per-point log p, gradients ------------------------------------------------------------------------------
def _vi_noise(zs, B, K):
    """[B, K, dim] (the restatement's layout) -> [S*N, dim], S-major (models.py:50)."""
    return [np.ascontiguousarray(np.asarray(z).transpose(1, 0, 2).reshape(K * B, -1)) for z in zs]


@pytest.mark.parametrize("name", ["bernoulli", "student_t"])
@pytest.mark.parametrize("iw", [True, False], ids=["iwvi", "vi"])
@pytest.mark.parametrize("lv", [True, False], ids=["lv", "nolv"])
@pytest.mark.parametrize("Dy,K", [(1, 1), (1, 20), (3, 20), (3, 1)])
def test_bound_logp_and_gradients_match_the_restatement(gpu_device, name, iw, lv, Dy, K):
    from dgps_with_iwvi_amd import synthetic, backward
    from dgps_with_iwvi_amd.models import DGP_IWVI, DGP_VI
    spec = _spec(name, B=12, K=K, lv=lv, Dy=Dy, seed=7 + K + Dy)
    zs = synthetic.make_noise(spec, seed=2)
    lik, ref = _liks(name)
    val, logp, gref = R.bound_and_gradients(spec, ref, zs, mode_vi=not iw)
    model = synthetic.build_model(spec, gpu_device, cls=DGP_IWVI if iw else DGP_VI, likelihood=lik)
    zd = [_t(z, gpu_device) for z in (zs if iw else _vi_noise(zs, 12, K))]
    got = model.compute_log_likelihood(zd)
    print("%s iw=%s lv=%s Dy=%d K=%d: bound %.6f vs %.6f (%.2e relative)" % (name, iw, lv, Dy, K, got, val, abs(got - val) / abs(val)))
    assert abs(got - val) <= ELBO_RTOL * abs(val), (got, val)
    if iw:
        lp = model.E_log_p_Y(zd).cpu().numpy()
        print("  per-point log p: max abs err %.3e" % np.abs(lp - logp).max())
        np.testing.assert_allclose(lp, logp, rtol=2e-4, atol=2e-2)
        ms, _ = model.lse_partials(zd)                           # the K-shard exchange unit carries the same numbers
        np.testing.assert_allclose((ms[:, 0] + torch.log(ms[:, 1])).cpu().numpy() - math.log(K), lp, rtol=1e-5, atol=1e-5)
    elbo, grads = backward.iw_elbo_and_gradients(model, zd)
    assert abs(float(elbo) - val) <= 2e-4 * abs(val), (float(elbo), val)
    assert sorted(grads) == sorted(gref), (sorted(grads), sorted(gref))
    for k, v in grads.items():
        _close(k, v.detach().cpu().numpy().reshape(gref[k].shape), gref[k], rtol=5e-3)


@pytest.mark.parametrize("name", ["bernoulli", "student_t"])
def test_full_headline_shape_matches_the_restatement(gpu_device, name):
    """BASELINE configs[2] (L=2, M=128, K=20, B=1024, latent-variable layer), Y thresholded to {0, 1} for the Bernoulli: bound and
    per-point log p at the tolerance the Gaussian test of that shape uses (tests/test_gpu_lean_variant.py)."""
    from dgps_with_iwvi_amd import synthetic
    spec = _spec(name, L=2, M=128, B=1024, K=20, lv=True, seed=0, n_data=65536)
    zs = synthetic.make_noise(spec, seed=1)
    lik, ref = _liks(name)
    m = R.LikDGP(spec, ref)
    with torch.no_grad():
        val, logp = float(m.elbo_tensor(zs)), m.per_point(zs).numpy()
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    zd = [_t(z, gpu_device) for z in zs]
    got = model.compute_log_likelihood(zd)
    lp = model.E_log_p_Y(zd).cpu().numpy()
    print("%s full shape: bound %.4f vs %.4f (%.2e relative); log p max abs err %.3e" % (name, got, val, abs(got - val) / abs(val), np.abs(lp - logp).max()))
    assert abs(got - val) <= ELBO_RTOL * abs(val), (got, val)
    np.testing.assert_allclose(lp, logp, rtol=2e-4, atol=2e-2)


@pytest.mark.parametrize("name", ["bernoulli", "student_t"])
def test_gradient_agrees_with_central_differences_of_the_forward(gpu_device, name):
    """One finite-difference spot check per likelihood (the pattern of tests/test_gpu_backward.py): directional derivatives of the HIP
    adjoint against central differences of the HIP bound on the same injected noise; for the Student-t also d / d scale."""
    from dgps_with_iwvi_amd import synthetic, backward
    spec = _spec(name, L=2, M=64, B=64, K=8, lv=True, seed=13)
    lik, _ = _liks(name)
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    zs = [_t(z, gpu_device) for z in synthetic.make_noise(spec, seed=1)]
    elbo0, grads = backward.iw_elbo_and_gradients(model, zs)
    f0 = model.compute_log_likelihood(zs)
    assert abs(float(elbo0) - f0) <= 1e-5 * abs(f0)
    gen = torch.Generator(device="cpu").manual_seed(5)
    params = dict(backward.parameter_list(model))
    noise = 2e-6 * abs(f0)
    for pname in ("l2.q_mu", "l1.Z", "l0.encW0", "l2.ls"):
        p, g = params[pname], grads[pname].reshape(params[pname].shape).double()
        d = torch.randn(p.shape, generator=gen).to(gpu_device)
        d = d / d.norm()
        gd = float((g * d.double()).sum())
        eps = min(0.02, 100.0 * noise / max(abs(gd), 1e-30))
        with torch.no_grad():
            p.add_(eps * d); fp = model.compute_log_likelihood(zs)
            p.add_(-2 * eps * d); fm = model.compute_log_likelihood(zs)
            p.add_(eps * d)
        fd = (fp - fm) / (2 * eps)
        print("%s %s: fd %.6e adjoint %.6e eps %.3g" % (name, pname, fd, gd, eps))
        assert abs(fd - gd) <= 0.02 * abs(gd) + noise / eps, (pname, fd, gd, eps)
    if name == "student_t":
        gd, s0 = float(grads["lik_scale"]), lik.scale
        eps = min(0.02, 100.0 * noise / max(abs(gd), 1e-30))
        lik.scale = s0 + eps; fp = model.compute_log_likelihood(zs)
        lik.scale = s0 - eps; fm = model.compute_log_likelihood(zs)
        lik.scale = s0
        fd = (fp - fm) / (2 * eps)
        print("student_t lik_scale: fd %.6e adjoint %.6e eps %.3g" % (fd, gd, eps))
        assert abs(fd - gd) <= 0.02 * abs(gd) + noise / eps, (fd, gd, eps)
    else:
        assert "lik_scale" not in grads and "lik_var" not in grads


# ---- test 6: the Gaussian is untouched ---------------------------------------------------------------------------------------------
class _Calls:
    """Counts the calls of the named entry points of the loaded library while active (the Python side looks them up on the handle)."""

    def __init__(self, *names):
        self.names, self.n = names, {k: 0 for k in names}

    def __enter__(self):
        from dgps_with_iwvi_amd import _abi
        self.lib = _abi.lib()
        self.orig = {k: getattr(self.lib, k) for k in self.names}
        for k in self.names:
            def wrap(*a, _k=k):
                self.n[_k] += 1
                return self.orig[_k](*a)
            setattr(self.lib, k, wrap)
        return self.n

    def __exit__(self, *exc):
        for k, f in self.orig.items():
            setattr(self.lib, k, f)


_TAILS = ("iwvi_dgp_forward", "iwvi_iw_elbo_reduce_dev", "iwvi_iw_elbo_backward_dev", "iwvi_lik_elbo_reduce", "iwvi_lik_elbo_backward")


def test_gaussian_model_takes_the_fused_tail_and_heads_at_the_headline_shape(gpu_device):
    """configs[2] (L=2, M=128, K=20, B=1024, latent-variable layer), where the routes differ observably: the bound-only launch reports
    LEAN mode 1 (bits 10-11 of iwvi_debug_last_forward_variant), a launch with per-layer outputs mode 2.  A Gaussian model: one
    iwvi_dgp_forward per evaluation in mode 1 and no separate reduction; value + gradient: one launch in mode 2 whose own tail leaves the
    heads -- iwvi_iw_elbo_backward_dev is NOT called (it is with fuse_heads=False, and the two routes agree); never an iwvi_lik_* call.
    The same model with a Bernoulli likelihood takes the other route, so every one of these observables can tell them apart."""
    from dgps_with_iwvi_amd import synthetic, backward, _abi, likelihoods
    spec = synthetic.make_spec(L=2, M=128, B=1024, K=20, with_lv=True, seed=0, n_data=65536)
    model = synthetic.build_model(spec, gpu_device)
    variant = lambda: int(_abi.lib().iwvi_debug_last_forward_variant())
    lean = lambda: (variant() >> 10) & 3

    def rewind(m):                                               # the compiled-in-shapes variants draw their noise on the device: the same
        m._words()[1] = 0                                        # counter gives every evaluation below the same draws

    with _Calls(*_TAILS) as n:
        rewind(model); e1 = model.compute_log_likelihood()
        assert lean() == 1, hex(variant())
        rewind(model); lp1 = model.E_log_p_Y()
        assert lean() == 1, hex(variant())
        rewind(model); ms, _ = model.lse_partials()
        assert lean() == 1, hex(variant())
    assert n == dict(iwvi_dgp_forward=3, iwvi_iw_elbo_reduce_dev=0, iwvi_iw_elbo_backward_dev=0, iwvi_lik_elbo_reduce=0, iwvi_lik_elbo_backward=0), n
    with _Calls(*_TAILS) as n:
        rewind(model); elbo_f, g_f = backward.iw_elbo_and_gradients(model)
        assert lean() == 2, hex(variant())
    assert n == dict(iwvi_dgp_forward=1, iwvi_iw_elbo_reduce_dev=0, iwvi_iw_elbo_backward_dev=0, iwvi_lik_elbo_reduce=0, iwvi_lik_elbo_backward=0), n
    with _Calls(*_TAILS) as n:
        rewind(model); elbo_u, g_u = backward.iw_elbo_and_gradients(model, fuse_heads=False)
    assert n == dict(iwvi_dgp_forward=1, iwvi_iw_elbo_reduce_dev=0, iwvi_iw_elbo_backward_dev=1, iwvi_lik_elbo_reduce=0, iwvi_lik_elbo_backward=0), n
    assert abs(float(elbo_f) - e1) <= 1e-5 * abs(e1) and abs(float(elbo_u) - e1) <= 1e-5 * abs(e1)
    assert sorted(g_f) == sorted(g_u) and "lik_var" in g_f
    for k in g_f:
        _close(k, g_f[k].cpu().numpy(), g_u[k].cpu().numpy().reshape(g_f[k].shape), rtol=5e-3)
    # deterministic kernels: the same evaluation twice gives the same bits
    rewind(model); e2 = model.compute_log_likelihood()
    rewind(model); lp2 = model.E_log_p_Y()
    assert e1 == e2 and torch.equal(lp1, lp2)
    np.testing.assert_allclose((ms[:, 0] + torch.log(ms[:, 1])).cpu().numpy() - math.log(20), lp1.cpu().numpy(), rtol=1e-5, atol=1e-5)
    rewind(model); elbo_2, g_2 = backward.iw_elbo_and_gradients(model)
    assert torch.equal(elbo_f, elbo_2) and all(torch.equal(g_f[k], g_2[k]) for k in g_f)
    # the other route, same shape: the observables above do differ
    sp = dict(spec, Y=(spec["Y"] > 0).astype(np.float64))
    other = synthetic.build_model(sp, gpu_device, likelihood=likelihoods.Bernoulli())
    with _Calls(*_TAILS) as n:
        other.compute_log_likelihood()
        assert lean() != 1, hex(variant())
        backward.iw_elbo_and_gradients(other)
    assert n == dict(iwvi_dgp_forward=2, iwvi_iw_elbo_reduce_dev=0, iwvi_iw_elbo_backward_dev=0, iwvi_lik_elbo_reduce=1, iwvi_lik_elbo_backward=1), n


def test_generic_tail_fed_a_gaussian_agrees_with_the_fused_one(gpu_device):
    """The new kernels fed type = Gaussian -- the closed form integrated by the 20-point rule, which is exact for a quadratic -- against the
    Gaussian tail and heads, within the Gaussian tests' tolerance: a cross-check of the quadrature machinery."""
    import ctypes
    from dgps_with_iwvi_amd import synthetic, _abi
    spec = synthetic.make_spec(L=2, M=32, B=16, K=4, with_lv=True, seed=3)
    zs = synthetic.make_noise(spec, seed=4)
    model = synthetic.build_model(spec, gpu_device)
    zd = [_t(z, gpu_device) for z in zs]
    e1 = model.compute_log_likelihood(zd)
    lp1 = model.E_log_p_Y(zd)
    # the generic tail on the same final moments
    B, K = 16, 4
    fmean, fvar, local_kls, global_kls, _, _, _ = model._forward_iw(zd)
    T = B * K
    fm, fv = fmean.reshape(T, -1).contiguous(), fvar.reshape(T, -1).contiguous()
    kls = [k.reshape(T, -1).contiguous() for k in local_kls]
    kl_dims = (ctypes.c_int32 * len(kls))(*[k.shape[1] for k in kls])
    glob = [g.reshape(-1) for g in global_kls]
    glob_n = (ctypes.c_int32 * len(glob))(*[g.numel() for g in glob])
    logp = torch.empty(B, device=gpu_device)
    elbo = torch.empty(1, dtype=torch.float64, device=gpu_device)
    ticket = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    scale = float(model.num_data) / B
    d = model.likelihood.lik_desc()
    _abi.check(_abi.lib().iwvi_lik_elbo_reduce(d, _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(model.Y), B, K, 1, K, 1, _abi.ptr_array(kls), kl_dims, len(kls),
                                               _abi.ptr_array(glob), glob_n, len(glob), scale, K, 0, None, _abi.ptr(logp), _abi.ptr(elbo),
                                               _abi.ptr(ticket), _abi.stream_ptr()))
    assert abs(float(elbo) - e1) <= ELBO_RTOL * abs(e1), (float(elbo), e1)
    np.testing.assert_allclose(logp.cpu().numpy(), lp1.cpu().numpy(), rtol=2e-4, atol=2e-2)
    assert int(ticket) == 0                                      # re-armed by the last workgroup
    w, dm, dv = torch.empty(T, device=gpu_device), torch.empty(T, 1, device=gpu_device), torch.empty(T, 1, device=gpu_device)
    sums = torch.empty(3, dtype=torch.float64, device=gpu_device)
    ws = torch.empty(2 * B, dtype=torch.float64, device=gpu_device)
    _abi.check(_abi.lib().iwvi_lik_elbo_backward(d, _abi.ptr(fm), _abi.ptr(fv), _abi.ptr(model.Y), 1, _abi.ptr_array(kls), kl_dims, len(kls), B, K,
                                                 scale, 0, _abi.ptr(w), _abi.ptr(dm), _abi.ptr(dv), _abi.ptr_array(glob), glob_n, len(glob),
                                                 None, K, _abi.ptr(sums), _abi.ptr(ws), _abi.stream_ptr()))
    w2, dm2, dv2 = torch.empty_like(w), torch.empty_like(dm), torch.empty_like(dv)
    sums2 = torch.empty_like(sums)
    _abi.check(_abi.lib().iwvi_iw_elbo_backward(_abi.ptr(fm), _abi.ptr(fv), _abi.ptr(model.Y), 1, _abi.ptr_array(kls), kl_dims, len(kls), B, K,
                                                model.likelihood.variance, scale, 0, _abi.ptr(w2), _abi.ptr(dm2), _abi.ptr(dv2),
                                                _abi.ptr_array(glob), glob_n, len(glob), None, K, _abi.ptr(sums2), _abi.ptr(ws), _abi.stream_ptr()))
    for what, a, b in (("w", w, w2), ("d_mean", dm, dm2), ("d_var", dv, dv2), ("sums", sums, sums2)):
        _close(what, a.cpu().numpy(), b.cpu().numpy(), rtol=5e-3)


def test_gaussian_only_routes_refuse_other_likelihoods(gpu_device):
    from dgps_with_iwvi_amd import synthetic, evaluation
    spec = _spec("bernoulli", B=16, K=3)
    lik, ref = _liks("bernoulli")
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    X, Y = spec["X"][:16], spec["Y"][:16]
    with pytest.raises(NotImplementedError, match="predict_y_samples"):
        model.predict_y_samples_fused(X, 8)
    with pytest.raises(NotImplementedError, match="predict_y_samples"):
        evaluation.evaluate(model, X, Y, num_predict_samples=8, on_device=True)
    with pytest.raises(NotImplementedError, match="iwvi_lik_elbo_reduce"):
        model._fused_forward(48, 3, 16, (48,), elbo=dict(B=16, K=3, stride_b=3, stride_k=1, mode_vi=False))
    ys = model.predict_y_samples(X, 5)                           # the layer-by-layer alternative works
    assert tuple(ys.shape) == (5, 16, 1) and bool(torch.isfinite(ys).all())


@pytest.mark.parametrize("name", ["bernoulli", "student_t"])
def test_predict_log_density_matches_the_restatement(gpu_device, name):
    """logsumexp_s sum_d predict_density(m_s, v_s, Y) - log S over the draws of predict_f_multisample (same injected noise)."""
    from dgps_with_iwvi_amd import synthetic
    spec = _spec(name, B=10, K=3, lv=True, Dy=3, seed=9)
    lik, ref = _liks(name)
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    S, N = 6, 10
    rng = np.random.default_rng(3)
    X, Y = spec["X"][:N], spec["Y"][:N]
    zs = [_t(rng.standard_normal((S, N, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1])), gpu_device) for l in spec["layers"]]
    got = model.predict_log_density(X, Y, S, zs=zs).cpu().numpy()
    m, v = model.predict_f_multisample(X, S, zs=zs)
    lp = ref.predict_density(m.cpu().double().numpy(), v.cpu().double().numpy(), np.broadcast_to(Y, (S, N, 3)).copy()).sum(-1)
    want = (torch.logsumexp(lp, 0) - math.log(S)).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=3 * 4 * ELEMENTWISE_RECORD[name] + 1e-5 * np.abs(want).max())


# ---- test 7: training ---------------------------------------------------------------------------------------------------------------
# The float64 restatement trained for 200 steps by oracle/optim_oracle.py on the same problem with the same injected noise, on the CPU.
# To regenerate the constants below:
#   python -c "import sys; sys.path.insert(0, 'tests'); import lik_restatement as R; print(R.oracle_training_record())"
# Bound seen by the Adam op: -2014.5727734096397 at step 1, mean of steps 191-200 -493.9825, mean of steps 141-150 -502.4900; training
# accuracy 0.96875 (62 of 64) against a majority-class rate of 0.578125 (37 of 64); 6 of the 64 points have a float64 predictive
# probability within 0.1 of 1/2.
# The device trajectory is float32 (Adam normalises gradient entries that are rounding noise, so it drifts from the float64 one), hence
#   * its late bound (mean of steps 191-200) must lie within what the float64 loop itself gains over its last 50 steps (8.51) of the
#     float64 value: a device optimiser may lag or lead the restatement by at most a quarter of the run;
#   * its accuracy may lose only the points the restatement itself decides narrowly (those 6): floor 56 of 64.
ORACLE_FIRST, ORACLE_LATE, ORACLE_LATE_50_EARLIER = -2014.5727734096397, -493.9825146042158, -502.49003922278445
ORACLE_ACCURACY, MAJORITY, ORACLE_NARROW_POINTS = 0.96875, 0.578125, 6
BOUND_BAND = ORACLE_LATE - ORACLE_LATE_50_EARLIER
ACCURACY_FLOOR = ORACLE_ACCURACY - ORACLE_NARROW_POINTS / 64.0


def _two_class_model(dev, likelihood=None):
    from dgps_with_iwvi_amd import synthetic, likelihoods
    spec, noise = R.two_class_problem()
    return spec, noise, synthetic.build_model(spec, dev, likelihood=likelihood or likelihoods.Bernoulli())


def test_training_raises_the_bound_and_classifies(gpu_device):
    from dgps_with_iwvi_amd.training import Trainer
    spec, noise, model = _two_class_model(gpu_device)
    assert max(spec["Y"][:64].mean(), 1 - spec["Y"][:64].mean()) == MAJORITY
    tr = Trainer(model, lr=5e-3, gamma=1e-2)
    assert "lik_var" not in [n for n, _, _ in tr._entries]       # the Bernoulli contributes no Adam scalar
    vals = []
    for s in range(200):
        vals.append(float(tr.step([_t(z, gpu_device) for z in noise(2 * s)], [_t(z, gpu_device) for z in noise(2 * s + 1)])))
    zs0 = [torch.zeros(64, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1], device=gpu_device) for l in spec["layers"]]
    p = model.predict_y(spec["X"][:64], zs=zs0)[0].cpu().numpy()
    acc = float(((p > 0.5) == (spec["Y"][:64] == 1)).mean())
    late = float(np.mean(vals[-10:]))
    print("bound %.4f -> late mean %.4f (restatement: %.4f -> %.4f, band %.2f); accuracy %.4f (restatement %.4f, floor %.4f)"
          % (vals[0], late, ORACLE_FIRST, ORACLE_LATE, BOUND_BAND, acc, ORACLE_ACCURACY, ACCURACY_FLOOR))
    assert abs(vals[0] - ORACLE_FIRST) <= 3e-4 * abs(ORACLE_FIRST)   # the first step sees the restatement's bound
    assert abs(late - ORACLE_LATE) <= BOUND_BAND, (late, ORACLE_LATE, BOUND_BAND)
    assert acc >= ACCURACY_FLOOR > MAJORITY, (acc, ACCURACY_FLOOR)


@pytest.mark.parametrize("name", ["bernoulli", "student_t"])
def test_graph_step_equals_eager_step_and_resume_is_exact(gpu_device, name, tmp_path):
    """Trainer(use_graph=True) captures a step with the three-launch evaluation into a hipGraph: parameters bit-identical to the eager
    trainer's after 6 steps; 3 steps, checkpoint, restore into a fresh model + trainer, 3 more == 6 uninterrupted, bit for bit.  The
    Student-t's scale is an Adam scalar on the device and moves."""
    from dgps_with_iwvi_amd import build_models, settings, likelihoods
    from dgps_with_iwvi_amd.training import Trainer

    def fresh(use_graph):
        settings.set_seed(3)
        lik = likelihoods.Bernoulli() if name == "bernoulli" else likelihoods.StudentT(scale=0.7, df=4.0)
        _, _, model = _two_class_model(gpu_device, lik)
        return model, Trainer(model, use_graph=use_graph, check_finite=False)

    out = []
    for use_graph in (False, True):
        model, tr = fresh(use_graph)
        vals = [float(tr.step()) for _ in range(6)]
        out.append((vals, [p.clone() for _, p, _ in tr._entries], model.layers[-1].q_sqrt.clone(), model, tr))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    for pa, pb in zip(out[0][1], out[1][1]):
        assert torch.equal(pa, pb)
    assert torch.equal(out[0][2], out[1][2])
    names = [n for n, _, _ in out[0][4]._entries]
    if name == "student_t":
        assert "lik_scale" in names and out[0][3].likelihood.scale == out[1][3].likelihood.scale != 0.7
    else:
        assert "lik_scale" not in names and "lik_var" not in names
    b, tb = fresh(False)
    for _ in range(3):
        tb.step()
    path = str(tmp_path / "ckpt_lik.npz")
    build_models.save_checkpoint(b, path, tb)
    c, tc = fresh(False)
    tc.step()                                                    # disturb the fresh state: everything must come from the file
    build_models.load_checkpoint(c, path, tc)
    for _ in range(3):
        tc.step()
    for (n, pa, _), (_, pc, _) in zip(out[0][4]._entries, tc._entries):
        assert torch.equal(pa, pc), n
    assert torch.equal(out[0][3].layers[-1].q_sqrt, c.layers[-1].q_sqrt) and torch.equal(out[0][3].layers[-1].q_mu, c.layers[-1].q_mu)
    if name == "student_t":
        assert out[0][3].likelihood.scale == c.likelihood.scale


def test_k_sharded_training_refuses_other_likelihoods(gpu_device):
    from dgps_with_iwvi_amd.training import Trainer
    _, _, model = _two_class_model(gpu_device)
    with pytest.raises(NotImplementedError, match="K-sharded"):
        Trainer(model, shard="k")
