"""The encoder-gradient estimators ("iwae" | "dreg" | "stl": k_lv_bwd / the fused prologue of k_enc_bwd, csrc/backward.hip) and the
gradient-moments monitor (k_moments, csrc/moments.hip) on the device, against the float64 references of tests/encoder_gradient_reference.py.

Tolerances: the kernel against its float64 closed form at the ABI level, max error <= 1e-4 x max |reference| (the figure of
test_gpu_backward.py::test_encoder_backward_matches_autodiff for this kernel family; the float32 sensitivity of "dreg" is within a factor 5 of
"iwae"'s); a whole model's encoder gradients against the float64 surrogate, 5e-3 (the figure of test_iw_elbo_gradients_match_oracle: the
cotangents arrive through float32 GP layers); the Welford update is float64 on the device, 1e-12."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_gradient_reference as er   # noqa: E402

pytestmark = pytest.mark.gpu

ESTIMATORS = er.ESTIMATORS


def _close(name, got, ref, rtol):
    """As tests/test_gpu_backward.py::_close: max error against rtol x max |reference|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-12)
    err = np.abs(got - ref).max()
    print("%s: max err %.3e, scale %.3e" % (name, err, scale))
    assert err <= rtol * scale, "%s: max err %.3e vs scale %.3e" % (name, err, scale)


def _dev(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)


def _is_encoder(name):
    return ".enc" in name


class _LvCase:
    """Random operands of the latent-variable adjoint and its encoder at the ABI level."""

    def __init__(self, dev, Lw, B, K, with_dF, seed=None):
        from dgps_with_iwvi_amd import _abi
        rng = np.random.default_rng(Lw * B + K if seed is None else seed)
        f32 = lambda a: np.asarray(a, dtype=np.float32)
        self.Lw, self.B, self.K, self.dev = Lw, B, K, dev
        self.dims = [6, 20, 20, 2 * Lw]
        self.h = dict(XY=f32(rng.standard_normal((B, self.dims[0]))), enc_out=f32(rng.standard_normal((B, 2 * Lw))),
                      eps=f32(rng.standard_normal((B * K, Lw))), w=f32(rng.random(B * K)))
        self.ld, self.col0 = Lw + 4, 3
        self.h["dF"] = f32(rng.standard_normal((B * K, self.ld))) if with_dF else None
        self.Ws = [_dev(rng.standard_normal((a, b)) * (2.0 / (a + b)) ** 0.5, dev) for a, b in zip(self.dims[:-1], self.dims[1:])]
        self.bs = [_dev(rng.standard_normal(b) * 0.1, dev) for b in self.dims[1:]]
        self.d = {k: (None if v is None else _dev(v, dev)) for k, v in self.h.items()}
        self.cd = (ctypes.c_int32 * len(self.dims))(*self.dims)
        self.w_unit = 2.5
        self.ws = torch.empty(_abi.lib().iwvi_encoder_backward_ws_bytes(B, self.cd, len(self.Ws)), dtype=torch.uint8, device=dev)

    def latent(self):
        from dgps_with_iwvi_amd import _abi
        d, Lw = self.d, self.Lw
        return (ctypes.c_void_p(d["enc_out"].data_ptr()), ctypes.c_void_p(d["enc_out"].data_ptr() + 4 * Lw), 2 * Lw, 1, _abi.ptr(d["eps"]),
                _abi.ptr(d["dF"]), self.ld if d["dF"] is not None else 0, self.col0, _abi.ptr(d["w"]), Lw, self.B, self.K, 1)

    def layer_ex(self, est):
        from dgps_with_iwvi_amd import _abi
        out = torch.full((self.B, 2 * self.Lw), float("nan"), dtype=torch.float32, device=self.dev)
        _abi.check(_abi.lib().iwvi_lv_layer_backward_ex(*self.latent(), _abi.LV_GRAD[est], self.w_unit if est != "iwae" else 1.0,
                                                        _abi.ptr(out), _abi.stream_ptr()))
        return out

    def layer_old(self):
        from dgps_with_iwvi_amd import _abi
        out = torch.full((self.B, 2 * self.Lw), float("nan"), dtype=torch.float32, device=self.dev)
        _abi.check(_abi.lib().iwvi_lv_layer_backward(*self.latent(), _abi.ptr(out), _abi.stream_ptr()))
        return out

    def _outs(self):
        return [torch.empty_like(t) for t in self.Ws], [torch.empty_like(t) for t in self.bs]

    def encoder(self, d_enc):
        from dgps_with_iwvi_amd import _abi
        dW, db = self._outs()
        _abi.check(_abi.lib().iwvi_encoder_backward_act(_abi.ptr(self.d["XY"]), self.B, _abi.ptr_array(self.Ws), _abi.ptr_array(self.bs), self.cd,
                                                        len(self.Ws), _abi.ACT_TANH, _abi.ptr(d_enc), _abi.ptr_array(dW), _abi.ptr_array(db),
                                                        self.ws.data_ptr(), _abi.stream_ptr()))
        return dW + db

    def fused(self, est=None):
        from dgps_with_iwvi_amd import _abi
        dW, db = self._outs()
        tail = (_abi.ptr(self.d["XY"]), _abi.ptr_array(self.Ws), _abi.ptr_array(self.bs), self.cd, len(self.Ws), _abi.ACT_TANH,
                _abi.ptr_array(dW), _abi.ptr_array(db), self.ws.data_ptr(), _abi.stream_ptr())
        if est is None:
            _abi.check(_abi.lib().iwvi_lv_encoder_backward(*self.latent(), *tail))
        else:
            _abi.check(_abi.lib().iwvi_lv_encoder_backward_ex(*self.latent(), _abi.LV_GRAD[est], self.w_unit if est != "iwae" else 1.0, *tail))
        return dW + db

    def reference(self, est):
        h, Lw = self.h, self.Lw
        return er.lv_adjoint_reference(h["enc_out"][:, :Lw], h["enc_out"][:, Lw:], h["eps"], h["dF"], self.col0, h["w"], self.K, est,
                                       w_unit=self.w_unit if est != "iwae" else 1.0)


# (a second lane pass and a partial one at K = 70; no cotangent from above; one sample)
@pytest.mark.parametrize("Lw,B,K,with_dF", [(1, 5, 3, True), (2, 7, 70, True), (3, 4, 64, False), (1, 9, 1, True)])
@pytest.mark.parametrize("est", ESTIMATORS)
def test_lv_adjoint_matches_the_float64_closed_form(gpu_device, Lw, B, K, with_dF, est):
    c = _LvCase(gpu_device, Lw, B, K, with_dF)
    got = c.layer_ex(est).cpu().numpy()
    ref = c.reference(est)
    _close("d_enc[%s]" % est, got, ref, rtol=1e-4)
    if est != "iwae":                                            # the estimators are different numbers, not one formula under three names
        assert np.abs(ref - c.reference("iwae")).max() > 1e-2 * np.abs(ref).max()


@pytest.mark.parametrize("B", [5, 130])                          # a ragged last workgroup of ER = 4 rows; more than one workgroup of either kernel
def test_ex_entries_are_bit_identical_where_they_must_be(gpu_device, B):
    c = _LvCase(gpu_device, 2, B, 70, True)
    old = c.layer_old()
    assert torch.equal(c.layer_ex("iwae"), old) and bool(torch.isfinite(old).all())
    assert all(torch.equal(a, b) for a, b in zip(c.fused(None), c.fused("iwae")))
    seen = {}
    for est in ESTIMATORS:
        d_enc = c.layer_ex(est)
        assert torch.equal(d_enc, c.layer_ex(est)), est          # two calls, equal bits
        two = c.encoder(d_enc)
        one = c.fused(est)
        again = c.fused(est)
        torch.cuda.synchronize()
        for a, b, b2 in zip(two, one, again):
            assert float(a.abs().max()) > 0
            assert torch.equal(a, b) and torch.equal(b, b2), est
        seen[est] = d_enc
    assert not torch.equal(seen["dreg"], seen["iwae"]) and not torch.equal(seen["dreg"], seen["stl"])


# -- model level ----------------------------------------------------------------------------------------------------------------------

_MODEL_CASES = [(2, 64, 5, 16, 1), (3, 32, 4, 12, 1), (2, 40, 3, 7, 1), (2, 32, 70, 5, 1), (2, 32, 4, 6, 2)]   # (L, M, K, B, latent_dim)
_REF = {}


def _model_case(L, M, K, B, Lw):
    """spec, noise and every estimator's float64 encoder gradients, computed once."""
    key = (L, M, K, B, Lw)
    if key not in _REF:
        from dgps_with_iwvi_amd import synthetic
        spec = synthetic.make_spec(L=L, M=M, B=B, K=K, with_lv=True, seed=7 * L + K, latent_dim=Lw)
        zs = synthetic.make_noise(spec, seed=2)
        _REF[key] = (spec, zs, {e: er.surrogate_gradients(spec, zs, e) for e in ESTIMATORS})
    return _REF[key]


def _grads(model, zd, **kw):
    from dgps_with_iwvi_amd import backward
    elbo, g = backward.iw_elbo_and_gradients(model, zd, **kw)
    return elbo, g


def _assert_only_the_encoder_moved(elbo, g, elbo0, g0, must_differ=True):
    assert torch.equal(elbo, elbo0)
    assert sorted(g) == sorted(g0)
    for n in g:
        if _is_encoder(n):
            assert bool(torch.isfinite(g[n]).all()), n
            if must_differ:
                assert not torch.equal(g[n], g0[n]), n
        else:
            assert torch.equal(g[n], g0[n]), n


@pytest.mark.parametrize("L,M,K,B,Lw", _MODEL_CASES)
def test_model_encoder_gradients_match_the_float64_surrogate(gpu_device, L, M, K, B, Lw):
    from dgps_with_iwvi_amd import synthetic
    spec, zs, ref = _model_case(L, M, K, B, Lw)
    model = synthetic.build_model(spec, gpu_device)
    zd = [_dev(z, gpu_device) for z in zs]
    elbo0, g0 = _grads(model, zd)                                # the model's default: "iwae"
    for est in ESTIMATORS:
        elbo, g = _grads(model, zd, encoder_gradient=est)
        val, rg = ref[est]
        assert abs(float(elbo) - val) <= 2e-4 * abs(val)
        _assert_only_the_encoder_moved(elbo, g, elbo0, g0, must_differ=est != "iwae")
        for n in rg:
            _close("%s[%s]" % (n, est), g[n].cpu().numpy().reshape(rg[n].shape), rg[n], rtol=5e-3)
        # the model's own setting is what None means; the argument wins over it; wrt="final_q" ignores it
        model.encoder_gradient = est
        _, g2 = _grads(model, zd)
        assert all(torch.equal(g2[n], g[n]) for n in g)
        _, g3 = _grads(model, zd, encoder_gradient="iwae")
        assert all(torch.equal(g3[n], g0[n]) for n in g0)
        eq, gq = _grads(model, zd, wrt="final_q")
        assert torch.equal(eq, elbo0) and all(torch.equal(gq[n], g0[n]) for n in gq)
        model.encoder_gradient = "iwae"
    with pytest.raises(ValueError, match="encoder_gradient"):
        _grads(model, zd, encoder_gradient="nope")
    with pytest.raises(ValueError, match="mode_vi"):
        _grads(model, zd, encoder_gradient="dreg", mode_vi=True)


def test_autograd_function_and_a_vi_model_follow_the_setting(gpu_device):
    from dgps_with_iwvi_amd import backward, synthetic
    from dgps_with_iwvi_amd.models import DGP_VI
    spec, zs, _ = _model_case(2, 32, 4, 6, 2)
    model = synthetic.build_model(spec, gpu_device)
    zd = [_dev(z, gpu_device) for z in zs]
    model.encoder_gradient = "dreg"
    _, ref = _grads(model, zd)
    params = backward.parameter_list(model)
    for _, t in params:
        t.requires_grad_(True)
    backward.IwElbo.apply(model, zd, *[t for _, t in params]).backward()
    for n, t in params:
        assert torch.equal(t.grad, ref[n].reshape(t.shape).to(t.dtype)), n
    vi = synthetic.build_model(spec, gpu_device, cls=DGP_VI, num_samples=4)
    with pytest.raises(ValueError, match="encoder_gradient"):
        vi.encoder_gradient = "dreg"


def test_non_gaussian_likelihood_under_dreg(gpu_device):
    from dgps_with_iwvi_amd import likelihoods, synthetic
    spec, zs, _ = _model_case(2, 32, 4, 6, 2)
    model = synthetic.build_model(spec, gpu_device, likelihood=likelihoods.StudentT(scale=0.7, df=4.0))
    zd = [_dev(z, gpu_device) for z in zs]
    elbo0, g0 = _grads(model, zd)
    elbo, g = _grads(model, zd, encoder_gradient="dreg")
    assert bool(torch.isfinite(elbo)) and "lik_scale" in g
    _assert_only_the_encoder_moved(elbo, g, elbo0, g0)


def test_k_sharded_dreg_shares_add_up_to_the_unsharded_gradient(gpu_device):
    """Shards of 4 + 3 out of K = 7, one after the other on one GPU (as test_k_sharded_gradients_add_up_to_the_unsharded_gradient): w is each
    rank's share against the merged normaliser, so w / w_unit is its share of the normalised weight and the DReG shares simply add."""
    from dgps_with_iwvi_amd import backward, sharding, synthetic
    K, B = 7, 10
    spec = synthetic.make_spec(L=2, M=32, B=B, K=K, with_lv=True, seed=17)
    zs = synthetic.make_noise(spec, seed=18)
    val, ref = er.surrogate_gradients(spec, zs, "dreg")
    shards = [(0, 4), (4, 7)]
    models = [synthetic.build_model(dict(spec, K=hi - lo), gpu_device) for lo, hi in shards]
    for m in models:
        m.encoder_gradient = "dreg"                              # what sharding.k_shard_gradients' evaluation reads
    pairs = []
    for (lo, hi), m in zip(shards, models):
        def record(ms):
            pairs.append(ms.clone())
            return sharding.lse_from_pairs(ms[None])
        backward.iw_elbo_and_gradients(m, [_dev(z[:, lo:hi], gpu_device) for z in zs], exchange=record, K_total=K)
    lse = sharding.lse_from_pairs(torch.stack(pairs))
    total = None
    for (lo, hi), m in zip(shards, models):
        e, g = backward.iw_elbo_and_gradients(m, [_dev(z[:, lo:hi], gpu_device) for z in zs], exchange=lambda ms: lse, K_total=K, kl_weight=0.5)
        assert abs(float(e) - val) <= 2e-4 * abs(val)
        total = g if total is None else {k: total[k] + g[k] for k in g}
    for n in ref:
        _close(n, total[n].cpu().numpy().reshape(ref[n].shape), ref[n], rtol=5e-3)


def test_custom_activation_route_gets_the_estimator(gpu_device):
    """A callable activation: d(encoder output) comes from k_lv_bwd with the estimator, the weights' gradients from torch's vector-Jacobian
    product -- the same numbers as the built-in tanh route (fused) up to the float32 of the two encoder adjoints."""
    from dgps_with_iwvi_amd import synthetic
    from dgps_with_iwvi_amd.layers import Encoder, LatentVariableLayer
    spec, zs, _ = _model_case(2, 32, 4, 6, 2)
    zd = [_dev(z, gpu_device) for z in zs]
    builtin = synthetic.build_model(spec, gpu_device)
    custom = synthetic.build_model(spec, gpu_device)
    lvs = spec["layers"][0]
    enc = Encoder(lvs["latent_dim"], lvs["dims"][0], lvs["dims"][1:-1], activation_func=lambda x: torch.tanh(x))
    enc.Ws, enc.bs = [_dev(w, gpu_device) for w in lvs["enc_W"]], [_dev(b, gpu_device) for b in lvs["enc_b"]]
    custom.layers[0] = LatentVariableLayer(lvs["latent_dim"], encoder=enc)
    assert enc.custom_act is not None
    _, gb = _grads(builtin, zd, encoder_gradient="dreg")
    _, gc = _grads(custom, zd, encoder_gradient="dreg")
    _, gc0 = _grads(custom, zd)
    for n in gb:
        if _is_encoder(n):
            _close(n, gc[n].cpu().numpy(), gb[n].cpu().numpy().reshape(tuple(gc[n].shape)), rtol=1e-4)
            assert not torch.equal(gc[n], gc0[n]), n


# -- Trainer ----------------------------------------------------------------------------------------------------------------------------

def _trainer(dev, est, use_graph, seed=3):
    from dgps_with_iwvi_amd import settings, synthetic
    from dgps_with_iwvi_amd.training import Trainer
    settings.set_seed(seed)
    model = synthetic.build_model(synthetic.make_spec(L=2, M=32, B=64, K=5, with_lv=True, seed=31), dev)
    model.encoder_gradient = est
    return model, Trainer(model, use_graph=use_graph, check_finite=False)


def _state(model, tr):
    return [p.clone() for _, p, _ in tr._entries] + [model.layers[-1].q_mu.clone(), model.layers[-1].q_sqrt.clone()]


def test_trainer_follows_the_setting_in_graph_mode_and_across_a_switch(gpu_device):
    runs = []
    for use_graph in (False, True):
        model, tr = _trainer(gpu_device, "dreg", use_graph)
        vals = [float(tr.step()) for _ in range(3)]
        after3 = _state(model, tr)
        model.encoder_gradient = "iwae"                          # mid-run: the captured graphs hold "dreg" and must go
        vals += [float(tr.step()) for _ in range(2)]
        assert tr._graphs_estimator == "iwae"
        runs.append((vals, after3, _state(model, tr)))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)
    # the switch was no formality: a trainer that stays with "dreg" ends elsewhere
    model, tr = _trainer(gpu_device, "dreg", False)
    for _ in range(5):
        tr.step()
    assert not all(torch.equal(a, b) for a, b in zip(_state(model, tr), runs[0][2]))


def test_trainer_step_moves_only_the_encoder_differently(gpu_device):
    """The natural-gradient op reads the final layer's two gradients alone: its update is the "iwae" trainer's.  The Adam op that follows
    moves the encoder by the estimator's gradient."""
    out = {}
    for est in ("iwae", "dreg"):
        model, tr = _trainer(gpu_device, est, False)
        tr.global_step += 1
        tr.natgrad_op()
        q = (model.layers[-1].q_mu.clone(), model.layers[-1].q_sqrt.clone())
        tr.adam_op()
        out[est] = (q, {n: p.clone() for n, p, _ in tr._entries})
    for a, b in zip(out["iwae"][0], out["dreg"][0]):
        assert torch.equal(a, b)
    # (Adam's first step moves every element by lr x the SIGN of its gradient: a two-element bias can land on the same bits under both
    # estimators, the encoder's weights as a whole cannot)
    enc = [n for n in out["iwae"][1] if _is_encoder(n)]
    assert len(enc) == 6
    flat = {est: torch.cat([out[est][1][n].reshape(-1) for n in enc]) for est in out}
    assert not torch.equal(flat["iwae"], flat["dreg"])
    assert not torch.equal(out["iwae"][1]["l0.encW0"], out["dreg"][1]["l0.encW0"])


# -- the moments monitor ----------------------------------------------------------------------------------------------------------------

_NS = (1, 63, 4097)


class _Mom:
    def __init__(self, dev):
        from dgps_with_iwvi_amd import _abi
        self.x = [torch.zeros(n, dtype=torch.float32, device=dev) for n in _NS]
        self.mean = [torch.zeros(n, dtype=torch.float64, device=dev) for n in _NS]
        self.m2 = [torch.zeros(n, dtype=torch.float64, device=dev) for n in _NS]
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.arr = (_abi.MomentsTensor * len(_NS))()
        for a, x, m, s in zip(self.arr, self.x, self.mean, self.m2):
            a.x, a.mean, a.m2, a.n = x.data_ptr(), m.data_ptr(), s.data_ptr(), x.numel()

    def load(self, data, r):
        for x, d in zip(self.x, data):
            x.copy_(torch.as_tensor(d[r], device=x.device))

    def update(self):
        from dgps_with_iwvi_amd import _abi
        _abi.check(_abi.lib().iwvi_moments_update(self.arr, len(_NS), self.count.data_ptr(), _abi.stream_ptr()))


def _moments_data(R, seed):
    rng = np.random.default_rng(seed)
    return [np.asarray(rng.standard_normal((R, n)) * 3.0 + rng.standard_normal(n) * 10.0, dtype=np.float32) for n in _NS]


@pytest.mark.parametrize("R", [1, 2, 7])
def test_moments_update_is_welford_in_float64(gpu_device, R):
    data = _moments_data(R, R)
    mom = _Mom(gpu_device)
    for r in range(R):
        mom.load(data, r)
        mom.update()
    assert int(mom.count.item()) == R
    for d, mean, m2 in zip(data, mom.mean, mom.m2):
        rm, rm2, _ = er.welford_reference(d)
        _close("mean", mean.cpu().numpy(), rm, rtol=1e-12)
        if R == 1:
            assert not bool(m2.any())                            # exactly zero
            assert np.array_equal(mean.cpu().numpy(), d[0].astype(np.float64))
        else:
            _close("m2", m2.cpu().numpy(), rm2, rtol=1e-12)


def test_moments_update_replays_from_a_captured_graph(gpu_device):
    """One eager update, then ONE captured update replayed five times over data changed in place == six eager updates of the same data, bit
    for bit: the count is read and advanced on the device, so a replay depends on nothing the capture saw."""
    R = 6
    data = _moments_data(R, 11)
    eager = _Mom(gpu_device)
    for r in range(R):
        eager.load(data, r)
        eager.update()
    mom = _Mom(gpu_device)
    mom.load(data, 0)
    mom.update()                                                 # eager: nothing of the first call is once-per-process, but the graph starts at count = 1
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            mom.update()                                         # recorded, not executed
        for r in range(1, R):
            mom.load(data, r)
            g.replay()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(mom.count.item()) == R == int(eager.count.item())
    for a, b in zip(mom.mean + mom.m2, eager.mean + eager.m2):
        assert torch.equal(a, b)


def test_moments_update_refusals(gpu_device):
    from dgps_with_iwvi_amd import _abi
    lib = _abi.lib()
    mom = _Mom(gpu_device)
    cp = mom.count.data_ptr()
    assert lib.iwvi_moments_update(None, 3, cp, None) == -1
    assert lib.iwvi_moments_update(mom.arr, 0, cp, None) == -1
    assert lib.iwvi_moments_update(mom.arr, 3, None, None) == -1
    mom.arr[1].n = -1
    assert lib.iwvi_moments_update(mom.arr, 3, cp, None) == -1
    mom.arr[1].n, mom.arr[2].m2 = 63, None
    assert lib.iwvi_moments_update(mom.arr, 3, cp, None) == -1 and b"iwvi_moments_update" in lib.iwvi_last_error()
    torch.cuda.synchronize()
    assert int(mom.count.item()) == 0 and not any(bool(t.any()) for t in mom.mean + mom.m2)


def test_gradient_moments_average_explicit_evaluations(gpu_device):
    from dgps_with_iwvi_amd import backward, settings, synthetic
    spec = synthetic.make_spec(L=2, M=32, B=6, K=4, with_lv=True, seed=9)
    model = synthetic.build_model(spec, gpu_device)
    zs_list = [[_dev(z, gpu_device) for z in synthetic.make_noise(spec, seed=50 + r)] for r in range(4)]
    for est in ("iwae", "dreg"):
        model.encoder_gradient = est
        mom = backward.gradient_moments(model, 4, zs_list=zs_list)
        each = [backward.iw_elbo_and_gradients(model, zs)[1] for zs in zs_list]
        assert sorted(mom) == sorted(each[0])
        for n, m in mom.items():
            ref = torch.stack([g[n].to(torch.float64).reshape(-1) for g in each])
            assert int(m["count"]) == 4 and m["mean"].dtype == torch.float64 and m["var"].dtype == torch.float64
            assert tuple(m["mean"].shape) == tuple(each[0][n].shape)
            _close(n + " mean", m["mean"].reshape(-1).cpu().numpy(), ref.mean(0).cpu().numpy(), rtol=1e-6)
            _close(n + " var", m["var"].reshape(-1).cpu().numpy(), ref.var(0, unbiased=True).cpu().numpy(), rtol=1e-6)
    # a choice of names, the argument over the model's setting, the summary
    names = ["l0.encW0", "l0.encb2"]
    model.encoder_gradient = "iwae"
    sub = backward.gradient_moments(model, 4, names=names, zs_list=zs_list, encoder_gradient="dreg")
    assert sorted(sub) == sorted(names)
    assert all(torch.equal(sub[n]["mean"], mom[n]["mean"]) and torch.equal(sub[n]["var"], mom[n]["var"]) for n in names)
    snr = backward.snr_summary(sub)
    for n in names:
        mean, var = sub[n]["mean"].reshape(-1), sub[n]["var"].reshape(-1)
        assert snr[n]["norm_snr"] == pytest.approx(float(mean.norm() / var.sum().sqrt()), rel=1e-12)
        assert snr[n]["median_snr"] == pytest.approx(float((mean.abs() / var.sqrt()).median()), rel=1e-12)
        assert snr[n]["norm_snr"] > 0 and np.isfinite(snr[n]["median_snr"])
    with pytest.raises(KeyError):
        backward.gradient_moments(model, 1, names=["no.such"])
    with pytest.raises(ValueError):
        backward.gradient_moments(model, 3, zs_list=zs_list)
    # device noise: the replayed graph accumulates what the eager loop does, bit for bit
    out = []
    for use_graph in (False, True):
        settings.set_seed(7)
        fresh = synthetic.build_model(spec, gpu_device)
        out.append(backward.gradient_moments(fresh, 3, names=names, encoder_gradient="stl", use_graph=use_graph))
    for n in names:
        assert int(out[1][n]["count"]) == 3
        assert torch.equal(out[0][n]["mean"], out[1][n]["mean"]) and torch.equal(out[0][n]["var"], out[1][n]["var"])
        assert bool((out[0][n]["var"] > 0).any())                # fresh noise per repeat
