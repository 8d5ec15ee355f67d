"""MultiClass (robust-max) on the GPU against the float64 restatement (tests/multiclass_restatement.py, pinned by
tests/test_multiclass_host.py), with injected noise.

Tolerances: 4x the error recorded in DESIGN.md section 6 (the project's margin for box-to-box and seed variation), per method for the
elementwise callables (maximum absolute error) and per quantity / gradient array for the bound (relative to the reference array's
max-norm).  The records are measured against the float64 restatement, never against the kernels themselves."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import multiclass_restatement as MR   # noqa: E402

pytestmark = pytest.mark.gpu

# ---- maximum absolute error of the float32 callables over moment_grid(C), C in {2, 3, 10, 32}, every label
ELEMENTWISE_RECORD = {"var_exp": 1.444e-5, "logp": 9.858e-7, "predict_density": 1.321e-5, "predict_mean": 1.433e-6, "predict_var": 1.422e-6}
# ---- the same section: maximum over the cases of BOUND_CASES of |got - ref| / max|ref|; gradient arrays by their kind
BOUND_RECORD = {"bound": 1.966e-7, "logp": 1.424e-6, "elbo_of_gradient_call": 1.934e-7,
                "Z": 9.009e-6, "ls": 1.029e-5, "var": 9.488e-5, "var_final": 1.862e-6, "q_mu": 2.377e-6, "q_sqrt": 3.529e-6, "W": 3.491e-6, "mfA": 2.807e-6,
                "encW": 6.995e-7, "encb": 6.104e-7}
MARGIN = 4.0


def _t(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)


def _lik(C):
    from dgps_with_iwvi_amd import likelihoods
    return likelihoods.MultiClass(C), MR.MultiClass(C)


# ---- the elementwise callables ------------------------------------------------------------------------------------------------------
def elementwise_errors(dev, C):
    """{method: max abs error} over the grid, every label; float32-rounded inputs on both sides."""
    lik, ref = _lik(C)
    MU, V = MR.moment_grid(C)
    mu32, v32 = MU.astype(np.float32), V.astype(np.float32)
    m64, v64 = mu32.astype(np.float64), v32.astype(np.float64)
    m, v = _t(mu32, dev), _t(v32, dev)
    err = {k: 0.0 for k in ELEMENTWISE_RECORD}
    up = lambda k, got, want: err.__setitem__(k, max(err[k], float(np.abs(got.cpu().numpy().astype(np.float64) - want.numpy()).max())))
    pm, pv = lik.predict_mean_and_var(m, v)
    rm, rv = ref.predict_mean_and_var(m64, v64)
    assert tuple(pm.shape) == tuple(pv.shape) == (len(MU), C)
    up("predict_mean", pm, rm)
    up("predict_var", pv, rv)
    for y in range(C):
        Y = np.full((len(MU), 1), float(y))
        yy = _t(Y, dev)
        for k, got, want in (("var_exp", lik.variational_expectations(m, v, yy), ref.variational_expectations(m64, v64, Y)),
                             ("logp", lik.logp(m, yy), ref.logp(m64, Y)),
                             ("predict_density", lik.predict_density(m, v, yy), ref.predict_density(m64, v64, Y))):
            assert tuple(got.shape) == (len(MU), 1), (k, got.shape)
            up(k, got, want)
    return err


@pytest.mark.parametrize("C", [2, 3, 10, 32])
def test_elementwise_callables_match_the_restatement(gpu_device, C):
    err = elementwise_errors(gpu_device, C)
    for k, e in err.items():
        print("C=%d %-16s max abs err %.3e (record %.3e)" % (C, k, e, ELEMENTWISE_RECORD[k]))
    for k, e in err.items():
        assert e <= MARGIN * ELEMENTWISE_RECORD[k], (C, k, e)


def test_logp_ties_and_row_tiling(gpu_device):
    """The first maximum wins; Y row (t / row_div) % row_mod of the entry points; leading batch dimensions of the methods."""
    from dgps_with_iwvi_amd import _abi
    lik, ref = _lik(4)
    F = _t([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0]], gpu_device)
    hit, miss = math.log(1 - 1e-3), math.log(1e-3 / 3)
    np.testing.assert_allclose(lik.logp(F, _t([[1.0], [0.0], [2.0]], gpu_device)).cpu().numpy()[:, 0], [hit] * 3, rtol=1e-6)   # (float32 of a float32 log)
    np.testing.assert_allclose(lik.logp(F, _t([[2.0], [1.0], [3.0]], gpu_device)).cpu().numpy()[:, 0], [miss] * 3, rtol=1e-6)
    rng = np.random.default_rng(5)
    Fm, Fv = _t(rng.uniform(-2, 2, (24, 4)), gpu_device), _t(rng.uniform(0.1, 2.0, (24, 4)), gpu_device)
    Y6 = _t((np.arange(6) % 4).reshape(6, 1), gpu_device)
    out = torch.empty(24, 1, device=gpu_device)
    _abi.check(_abi.lib().iwvi_lik_var_exp(lik.lik_desc(), _abi.ptr(Fm), _abi.ptr(Fv), _abi.ptr(Y6), 24, 4, 4, 6, _abi.ptr(out), _abi.stream_ptr()))
    assert torch.equal(out, lik.variational_expectations(Fm, Fv, Y6.repeat_interleave(4, 0)))
    got = lik.predict_density(Fm.reshape(2, 12, 4), Fv.reshape(2, 12, 4), Y6.repeat_interleave(4, 0).reshape(2, 12, 1))
    assert tuple(got.shape) == (2, 12, 1) and torch.equal(got.reshape(24, 1), lik.predict_density(Fm, Fv, Y6.repeat_interleave(4, 0)))


# ---- bound, per-point log p, lse_partials, gradients --------------------------------------------------------------------------------
def _vi_noise(zs, B, K):
    """[B, K, dim] (the restatement's layout) -> [S*N, dim], S-major (models.py:50)."""
    return [np.ascontiguousarray(np.asarray(z).transpose(1, 0, 2).reshape(K * B, -1)) for z in zs]


def _kind(name, final=None):
    k = name.split(".")[1]
    if k == "var" and name == final:
        return "var_final"
    return "encW" if k.startswith("encW") else "encb" if k.startswith("encb") else k


def bound_errors(dev, C, B, K, lv, iw):
    """{quantity or gradient kind: |got - ref| max / max|ref|} of one case (L = 2, M = 16); also checks names, shapes and lse_partials.
    'var_final', the final layer's kernel variance, is the one exception: the bound does not depend on it but for the jitter on K_uu (the
    arg-max is scale-invariant: multiclass_restatement.bound_and_gradients), its gradient is a sum of cancelling terms, and its error is
    taken relative to the sum of their magnitudes -- relative to its own ~0 value it would measure nothing."""
    from dgps_with_iwvi_amd import synthetic, backward
    from dgps_with_iwvi_amd.models import DGP_IWVI, DGP_VI
    spec = MR.make_spec(C, L=2, M=16, B=B, K=K, lv=lv, seed=7 + K + C + B)
    zs = synthetic.make_noise(spec, seed=2)
    lik, ref = _lik(C)
    val, logp, gref = MR.bound_and_gradients(spec, ref, zs, mode_vi=not iw)
    model = synthetic.build_model(spec, dev, cls=DGP_IWVI if iw else DGP_VI, likelihood=lik)
    zd = [_t(z, dev) for z in (zs if iw else _vi_noise(zs, B, K))]
    err = {"bound": abs(model.compute_log_likelihood(zd) - val) / abs(val)}
    if iw:
        lp = model.E_log_p_Y(zd).cpu().numpy().astype(np.float64)
        err["logp"] = float(np.abs(lp - logp).max() / np.abs(logp).max())
        ms, _ = model.lse_partials(zd)                           # the K-shard exchange unit carries the same numbers
        np.testing.assert_allclose((ms[:, 0] + torch.log(ms[:, 1])).cpu().numpy() - math.log(K), lp, rtol=1e-5, atol=1e-5)
    elbo, grads = backward.iw_elbo_and_gradients(model, zd)
    err["elbo_of_gradient_call"] = abs(float(elbo) - val) / abs(val)
    terms = float(gref.pop("final_var_terms"))
    final = "l%d.var" % (len(spec["layers"]) - 1)
    assert sorted(grads) == sorted(gref), (sorted(grads), sorted(gref))
    for k, g in grads.items():
        got, want = g.detach().cpu().numpy().astype(np.float64).reshape(gref[k].shape), gref[k]
        assert np.isfinite(got).all(), k
        scale = max(np.abs(want).max(), terms) if k == final else np.abs(want).max()
        assert scale > 0.0, k
        kind = _kind(k, final)
        err[kind] = max(err.get(kind, 0.0), float(np.abs(got - want).max() / scale))
    return err


BOUND_CASES = ([(C, B, K, lv, True) for C in (2, 3, 10) for B in (7, 67) for K in (1, 5, 20, 70) for lv in (True, False)]
               + [(3, B, K, lv, False) for B in (7, 67) for K in (1, 5, 20, 70) for lv in (True, False)]
               + [(2, 7, 5, True, False), (10, 7, 5, True, False), (10, 67, 20, False, False)]
               + [(32, 7, 5, True, True), (32, 67, 20, False, False)])


@pytest.mark.parametrize("C,B,K,lv,iw", BOUND_CASES, ids=lambda v: str(v))
def test_bound_logp_and_gradients_match_the_restatement(gpu_device, C, B, K, lv, iw):
    err = bound_errors(gpu_device, C, B, K, lv, iw)
    print("C=%d B=%d K=%d lv=%s iw=%s: " % (C, B, K, lv, iw) + "  ".join("%s %.2e" % kv for kv in sorted(err.items())))
    for k, e in err.items():
        assert e <= MARGIN * BOUND_RECORD[k], (k, e, BOUND_RECORD[k])


def test_gradient_agrees_with_central_differences_of_the_forward(gpu_device):
    """Directional derivatives of the HIP adjoint against central differences of the HIP bound on the same injected noise (the pattern of
    tests/test_gpu_likelihoods.py)."""
    from dgps_with_iwvi_amd import synthetic, backward
    spec = MR.make_spec(3, L=2, M=64, B=64, K=8, lv=True, seed=13)
    lik, _ = _lik(3)
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    zs = [_t(z, gpu_device) for z in synthetic.make_noise(spec, seed=1)]
    elbo0, grads = backward.iw_elbo_and_gradients(model, zs)
    f0 = model.compute_log_likelihood(zs)
    assert abs(float(elbo0) - f0) <= 1e-5 * abs(f0)
    assert "lik_var" not in grads and "lik_scale" not in grads
    gen = torch.Generator(device="cpu").manual_seed(5)
    params = dict(backward.parameter_list(model))
    noise = 2e-6 * abs(f0)
    for pname in ("l2.q_mu", "l2.q_sqrt", "l1.Z", "l0.encW0", "l2.ls"):
        p, g = params[pname], grads[pname].reshape(params[pname].shape).double()
        d = torch.randn(p.shape, generator=gen).to(gpu_device)
        if pname.endswith("q_sqrt"):
            d = torch.tril(d)
        d = d / d.norm()
        gd = float((g * d.double()).sum())
        eps = min(0.02, 100.0 * noise / max(abs(gd), 1e-30))
        with torch.no_grad():
            p.add_(eps * d); fp = model.compute_log_likelihood(zs)
            p.add_(-2 * eps * d); fm = model.compute_log_likelihood(zs)
            p.add_(eps * d)
        fd = (fp - fm) / (2 * eps)
        print("%s: fd %.6e adjoint %.6e eps %.3g" % (pname, fd, gd, eps))
        assert abs(fd - gd) <= 0.02 * abs(gd) + noise / eps, (pname, fd, gd, eps)


# ---- predictions --------------------------------------------------------------------------------------------------------------------
def test_predictions_match_the_restatement(gpu_device):
    """predict_log_density, predict_y and predict_density at N = 9, S = 6 against the restatement on the device's own final moments."""
    from dgps_with_iwvi_amd import synthetic
    C, N, S = 4, 9, 6
    spec = MR.make_spec(C, B=10, K=3, lv=True, seed=9)
    lik, ref = _lik(C)
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    rng = np.random.default_rng(3)
    X, Y = spec["X"][:N], spec["Y"][:N]
    dims = [l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1] for l in spec["layers"]]
    zs = [_t(rng.standard_normal((S, N, d)), gpu_device) for d in dims]
    got = model.predict_log_density(X, Y, S, zs=zs).cpu().numpy()
    m, v = model.predict_f_multisample(X, S, zs=zs)
    lp = ref.predict_density(m.cpu().double().numpy(), v.cpu().double().numpy(), np.broadcast_to(Y, (S, N, 1)).copy()).sum(-1)
    want = (torch.logsumexp(lp, 0) - math.log(S)).numpy()
    assert got.shape == (N,)
    np.testing.assert_allclose(got, want, rtol=0, atol=MARGIN * ELEMENTWISE_RECORD["predict_density"] + 1e-5 * np.abs(want).max())
    with pytest.raises(ValueError, match="Y must be"):
        model.predict_log_density(X, np.zeros((N, C)), S)
    z1 = [_t(rng.standard_normal((N, d)), gpu_device) for d in dims]
    m1, v1 = model.predict_f(X, zs=z1)
    P, PV = model.predict_y(X, zs=z1)
    rP, rV = ref.predict_mean_and_var(m1.cpu().double().numpy(), v1.cpu().double().numpy())
    assert tuple(P.shape) == (N, C) and float(P.min()) > 0.0 and float(P.max()) < 1.0
    np.testing.assert_allclose(P.cpu().numpy(), rP.numpy(), rtol=0, atol=MARGIN * ELEMENTWISE_RECORD["predict_mean"])
    np.testing.assert_allclose(PV.cpu().numpy(), rV.numpy(), rtol=0, atol=MARGIN * ELEMENTWISE_RECORD["predict_var"])
    pd = model.predict_density(X, Y, zs=z1)
    assert tuple(pd.shape) == (N, 1)
    np.testing.assert_allclose(pd.cpu().numpy(), ref.predict_density(m1.cpu().double().numpy(), v1.cpu().double().numpy(), Y).numpy(),
                               rtol=0, atol=MARGIN * ELEMENTWISE_RECORD["predict_density"])
    ys = model.predict_y_samples(X, 5)                           # the reference's literal m + z sqrt(v) on (P, P - P^2)
    assert tuple(ys.shape) == (5, N, C) and bool(torch.isfinite(ys).all())


# ---- training -----------------------------------------------------------------------------------------------------------------------
# The float64 restatement trained for 200 steps by oracle/optim_oracle.py on the same problem with the same injected noise, on the CPU:
#   python -c "import sys; sys.path.insert(0, 'tests'); import multiclass_restatement as MR; print(MR.oracle_training_record())"
# bound seen by the Adam op -1835.558371735588 at step 1, mean of steps 191-200 -256.7941; training accuracy 1.0 (300 of 300) against a
# majority-class rate of 103 / 300.
ORACLE_FIRST, ORACLE_LATE, ORACLE_ACCURACY, MAJORITY = -1835.558371735588, -256.7941000995696, 1.0, 103.0 / 300.0
ACCURACY_MARGIN = (ORACLE_ACCURACY - MAJORITY) - 0.02            # the restatement's own margin over the majority rate, less 0.02


def _three_class_model(dev):
    from dgps_with_iwvi_amd import synthetic, likelihoods
    spec, noise = MR.three_class_problem()
    return spec, noise, synthetic.build_model(spec, dev, likelihood=likelihoods.MultiClass(3))


def test_training_raises_the_bound_and_classifies(gpu_device):
    from dgps_with_iwvi_amd.training import Trainer
    spec, noise, model = _three_class_model(gpu_device)
    n = spec["B"]
    labels = spec["Y"][:n, 0]
    assert max(float((labels == k).mean()) for k in range(3)) == MAJORITY
    tr = Trainer(model, lr=5e-3, gamma=1e-2)
    assert not [e for e, _, _ in tr._entries if e.startswith("lik")]   # MultiClass contributes no Adam scalar
    vals = []
    for s in range(200):
        vals.append(float(tr.step([_t(z, gpu_device) for z in noise(2 * s)], [_t(z, gpu_device) for z in noise(2 * s + 1)])))
    zs0 = [torch.zeros(n, l["latent_dim"] if l["type"] == "lv" else l["q_mu"].shape[1], device=gpu_device) for l in spec["layers"]]
    P = model.predict_y(spec["X"][:n], zs=zs0)[0].cpu().numpy()
    acc = float((P.argmax(1) == labels).mean())
    late = float(np.mean(vals[-10:]))
    print("bound %.4f -> late mean %.4f (restatement: %.4f -> %.4f); accuracy %.4f (restatement %.4f, majority %.4f, margin asked %.4f)"
          % (vals[0], late, ORACLE_FIRST, ORACLE_LATE, acc, ORACLE_ACCURACY, MAJORITY, ACCURACY_MARGIN))
    assert abs(vals[0] - ORACLE_FIRST) <= 3e-4 * abs(ORACLE_FIRST)   # the first step sees the restatement's bound
    assert late > vals[0] and float(np.mean(vals[-10:])) > float(np.mean(vals[:10]))   # the bound rises
    assert ACCURACY_MARGIN > 0 and acc >= MAJORITY + ACCURACY_MARGIN, (acc, MAJORITY, ACCURACY_MARGIN)


def test_graph_step_equals_eager_step_and_resume_is_exact(gpu_device, tmp_path):
    """Trainer(use_graph=True) replays a step with the three-launch evaluation as a hipGraph: parameters bit-identical to the eager
    trainer's after 6 steps; 3 steps, checkpoint, restore into a fresh model + trainer, 3 more == 6 uninterrupted, bit for bit."""
    from dgps_with_iwvi_amd import build_models, settings
    from dgps_with_iwvi_amd.training import Trainer

    def fresh(use_graph):
        settings.set_seed(3)
        _, _, model = _three_class_model(gpu_device)
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
    b, tb = fresh(False)
    for _ in range(3):
        tb.step()
    path = str(tmp_path / "ckpt_mc.npz")
    build_models.save_checkpoint(b, path, tb)
    assert str(np.load(path)["likelihood.type"]) == "MultiClass"
    c, tc = fresh(False)
    tc.step()                                                    # disturb the fresh state: everything must come from the file
    build_models.load_checkpoint(c, path, tc)
    for _ in range(3):
        tc.step()
    for (n, pa, _), (_, pc, _) in zip(out[0][4]._entries, tc._entries):
        assert torch.equal(pa, pc), n
    assert torch.equal(out[0][3].layers[-1].q_sqrt, c.layers[-1].q_sqrt) and torch.equal(out[0][3].layers[-1].q_mu, c.layers[-1].q_mu)


# ---- routes -------------------------------------------------------------------------------------------------------------------------
from test_gpu_likelihoods import _Calls, _TAILS   # noqa: E402  (counts the calls of the library's entry points)


from test_gpu_explink import _backward_call   # noqa: E402  (iwvi_lik_elbo_backward directly)


@pytest.mark.parametrize("K", [3, 70])
def test_heads_of_a_k_shard_against_the_jobs_normaliser(gpu_device, K):
    """iwvi_lik_elbo_backward with lse_global (the K-sharded weights scale exp(L - lse_global), out_sums[0] = sum (lse_global - log K_total))
    at K = 3 and K = 70 -- past the one-sample-per-lane shortcut --, B = 5, C = 3, one regulariser of width 2, scale 2.75, against
    lik_restatement.sharded_heads in float64.  L: the margin on the recorded error of the expectation, the float32 subtractions of the two
    regulariser entries (iw_reduction_reference.tol_logw) and half a spacing of the float32 normaliser; the weights follow tol_w from that.
    A head is a float32 sum over the twenty nodes of products of C - 1 cdfs, an exponential and a quotient -- about three roundings a node:
    64 x 2^-24 of the sample's largest head of that array, on top of the weight's relative error."""
    import iw_reduction_reference as IR
    C, B, scale = 3, 5, 2.75
    lik, ref = _lik(C)
    rng = np.random.default_rng(29 + K)
    mu32 = rng.uniform(-1.5, 1.5, (B, K, C)).astype(np.float32)
    v32 = rng.uniform(0.05, 0.5, (B, K, C)).astype(np.float32)
    kl32 = rng.uniform(0.0, 1.0, (B, K, 2)).astype(np.float32)
    Y = rng.integers(0, C, (B, 1)).astype(np.float64)
    glob = np.array([1.25, 0.5])
    m64, v64, kl64 = (a.astype(np.float64) for a in (mu32, v32, kl32))
    L, lse, wr, dmr, dvr, _, _ = MR.R.sharded_heads(lambda m, v: ref.variational_expectations(m, v, Y[:, None, :])[..., 0], m64, v64, kl64, scale)
    Kt = 2 * K
    fm, fv, kl = (_t(a, gpu_device).reshape(B * K, -1) for a in (mu32, v32, kl32))
    w, dm, dv, sums = _backward_call(gpu_device, lik.lik_desc(), fm, fv, _t(Y, gpu_device), B, K, C, scale=scale, mode_vi=0, kls=[kl],
                                     glob=torch.as_tensor(glob, dtype=torch.float64, device=gpu_device), lse_global=_t(lse, gpu_device), K_total=Kt)
    n64 = lambda t: t.cpu().numpy().astype(np.float64)
    w, dm, dv, sums = n64(w).reshape(B, K), n64(dm).reshape(B, K, C), n64(dv).reshape(B, K, C), sums.cpu().numpy()
    E = L + kl64.sum(-1)
    big = np.maximum.reduce([np.abs(E), kl64[..., 0], np.abs(E - kl64[..., 0]), kl64[..., 1], np.abs(L)])
    tol_L = MARGIN * ELEMENTWISE_RECORD["var_exp"] + IR.tol_logw(big, 2) + 0.5 * IR.spacing32(lse)
    tw = IR.tol_w(wr, scale, tol_L)
    print("multiclass K=%d lse_global: w max err / allowed %.3f" % (K, float((np.abs(w - wr) / tw).max())))
    assert np.isfinite(w).all() and np.all(np.abs(w - wr) <= tw), float((np.abs(w - wr) / tw).max())
    for nm, got, want in (("d_mean", dm, dmr), ("d_var", dv, dvr)):
        tol = np.abs(want) * (tw / wr)[..., None] + 64 * 2.0 ** -24 * np.abs(want).max(-1, keepdims=True)
        print("multiclass K=%d lse_global: %s max err / allowed %.3f" % (K, nm, float((np.abs(got - want) / tol).max())))
        assert np.all(np.abs(got - want) <= tol), (nm, float((np.abs(got - want) / tol).max()))
    want0 = float((lse - math.log(Kt)).sum())
    assert abs(sums[0] - want0) <= float(tol_L.sum()), (sums[0], want0)
    assert sums[1] == 0.0                                        # no trained parameter
    assert abs(sums[2] - (scale * sums[0] - glob.sum())) <= 4 * 2.0 ** -52 * (abs(scale * sums[0]) + glob.sum()), sums


def test_gaussian_keeps_the_fused_tail_and_multiclass_takes_the_three_launch_route(gpu_device):
    """BASELINE configs[2] (L=2, M=128, K=20, B=1024, latent-variable layer): a Gaussian model still evaluates in ONE iwvi_dgp_forward in
    LEAN mode 1 and takes its heads from the launch; a MultiClass model of the same stack (10 classes) calls iwvi_lik_elbo_reduce once per
    evaluation and iwvi_lik_elbo_backward once per value + gradient."""
    from dgps_with_iwvi_amd import synthetic, backward, _abi, likelihoods
    spec = synthetic.make_spec(L=2, M=128, B=1024, K=20, with_lv=True, seed=0, n_data=65536)
    model = synthetic.build_model(spec, gpu_device)
    lean = lambda: (int(_abi.lib().iwvi_debug_last_forward_variant()) >> 10) & 3
    with _Calls(*_TAILS) as n:
        model.compute_log_likelihood()
        assert lean() == 1
        backward.iw_elbo_and_gradients(model)
        assert lean() == 2
    assert n == dict(iwvi_dgp_forward=2, iwvi_iw_elbo_reduce_dev=0, iwvi_iw_elbo_backward_dev=0, iwvi_lik_elbo_reduce=0, iwvi_lik_elbo_backward=0), n
    sp = MR.make_spec(10, L=2, M=128, B=1024, K=20, Dx=8, lv=True, seed=0, n_data=65536)
    other = synthetic.build_model(sp, gpu_device, likelihood=likelihoods.MultiClass(10))
    with _Calls(*_TAILS) as n:
        e = other.compute_log_likelihood()
        assert lean() != 1
    assert n == dict(iwvi_dgp_forward=1, iwvi_iw_elbo_reduce_dev=0, iwvi_iw_elbo_backward_dev=0, iwvi_lik_elbo_reduce=1, iwvi_lik_elbo_backward=0), n
    with _Calls(*_TAILS) as n:
        other._words()[1] = 0
        e1 = other.compute_log_likelihood()
        other._words()[1] = 0
        elbo, _ = backward.iw_elbo_and_gradients(other)
    assert n == dict(iwvi_dgp_forward=2, iwvi_iw_elbo_reduce_dev=0, iwvi_iw_elbo_backward_dev=0, iwvi_lik_elbo_reduce=1, iwvi_lik_elbo_backward=1), n
    assert math.isfinite(e) and abs(float(elbo) - e1) <= 1e-5 * abs(e1)


def test_gaussian_only_routes_refuse_multiclass(gpu_device):
    from dgps_with_iwvi_amd import synthetic, evaluation
    from dgps_with_iwvi_amd.training import Trainer
    spec = MR.make_spec(3, B=16, K=3, lv=True)
    lik, _ = _lik(3)
    model = synthetic.build_model(spec, gpu_device, likelihood=lik)
    X, Y = spec["X"][:16], spec["Y"][:16]
    with pytest.raises(NotImplementedError, match="predict_y_samples"):
        model.predict_y_samples_fused(X, 8)
    with pytest.raises(NotImplementedError, match="predict_y_samples"):
        evaluation.evaluate(model, X, Y, num_predict_samples=8, on_device=True)
    with pytest.raises(NotImplementedError, match="iwvi_lik_elbo_reduce"):
        model._fused_forward(48, 3, 16, (48,), elbo=dict(B=16, K=3, stride_b=3, stride_k=1, mode_vi=False))
    with pytest.raises(NotImplementedError, match="K-sharded"):
        Trainer(model, shard="k")
