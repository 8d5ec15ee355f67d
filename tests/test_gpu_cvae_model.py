"""cvae.CVAE / cvae.CVAETrainer on the GPU: the methods against the raw entry points on the same tensors, the training step against the
hand-made sequence (``iwvi_cvae_elbo_and_grad`` then ``iwvi_adam_step_dev``: the wiring -- the Adam kernel has tests of its own), hipGraph
replay against eager across an epoch boundary, the step counter and the staircase, a short training run with both evaluation routes, and the
checkpoint round trip.  A multi-step comparison against a float64 trajectory is deliberately absent: Adam's first steps are +-lr whatever the
gradient's size, so a sign flip on a near-zero gradient would fail it without a fault."""
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_cvae_kernel import DEV, Net, _dev   # noqa: E402

pytestmark = pytest.mark.gpu


def _data(n=300, seed=0):
    """1-D bimodal: y = +-sin x + noise."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-3.0, 3.0, (n, 1))
    y = np.where(rng.rand(n, 1) < 0.5, 1.0, -1.0) * np.sin(x) + 0.1 * rng.randn(n, 1)
    return x.astype(np.float32), y.astype(np.float32)


def _model(configuration="50", batch=64, n=300, use_graph=False, lr=5e-3, init_seed=5):
    from dgps_with_iwvi_amd.build_models import build_cvae_model
    X, Y = _data(n)
    np.random.seed(init_seed)                                        # the initial weights come from the host generator, as in the reference
    ARGS = types.SimpleNamespace(mode="CVAE", configuration=configuration, minibatch_size=batch, lr=lr, use_graph=use_graph)
    return build_cvae_model(ARGS, X, Y, device=DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _all_bits(model, trainer):
    out = [_bits(p) for _, p in model.parameters()] + [_bits(trainer.t_dev), _bits(model.rng_state)]
    for x, m, v in trainer.state:
        out += [_bits(x), _bits(m), _bits(v)]
    return out


def test_methods_equal_the_raw_entry_points():
    m = _model("7")
    eps = _dev(np.random.RandomState(1).randn(64, 1))
    raw = Net.of_model(m).train(m.X, m.Y, eps)
    raw_v = Net.of_model(m).train(m.X, m.Y, eps, grad=False)
    parts = m.compute_log_likelihood(eps, parts=True)
    assert _bits(parts) == raw_v["out"].tobytes() == raw["out"].tobytes()
    assert float(m.compute_log_likelihood(eps)) == raw["out"][0]
    elbo, g = m.elbo_and_gradients(eps)
    assert float(elbo) == raw["out"][0]
    for tag in ("enc", "dec"):
        for i in range(2):
            assert _bits(g["%s_W%d" % (tag, i)]) == raw["%s_dW" % tag][i].tobytes()
            assert _bits(g["%s_b%d" % (tag, i)]) == raw["%s_db" % tag][i].tobytes()
    assert float(g["variance"]) == raw["dvariance"]


def test_trainer_step_is_the_hand_made_sequence():
    from dgps_with_iwvi_amd import _abi
    lib = _abi.lib()
    a, b = _model("7"), _model("7")
    ta = a.trainer()
    # by hand on b: the optimiser's state from the parameters, then per step the gather, value + gradient, one Adam launch
    params = b.parameters()
    state = [tuple(torch.empty_like(p) for _ in range(3)) for _, p in params]
    t_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    grads = {name: torch.zeros_like(p) for name, p in params[:-1]}
    grads["variance"] = torch.zeros(1, dtype=torch.float64, device=DEV)

    def tensors(with_grads):
        arr = (_abi.AdamTensor * len(params))()
        for e, (name, p), (x, m, v) in zip(arr, params, state):
            e.param, e.x, e.m, e.v, e.n = p.data_ptr(), x.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
            e.transform = 1 if name == "variance" else 0
            if with_grads:
                e.grad = grads[name].data_ptr()
                if name == "variance":
                    e.transform |= _abi.ADAM_GRAD_F64
        return arr
    _abi.check(lib.iwvi_adam_step(tensors(False), len(params), 0.0, 0.9, 0.999, 1e-8, 1, 1, 1, None))
    net = Net.of_model(b)
    gd = _abi.CvaeGrads()
    keep = [_abi.ptr_array([grads["%s_%s%d" % (tag, kind, i)] for i in range(2)]) for tag in ("enc", "dec") for kind in ("W", "b")]
    gd.enc_dW, gd.enc_db, gd.dec_dW, gd.dec_db = keep
    gd.dvariance = grads["variance"].data_ptr()
    out = torch.empty(3, dtype=torch.float64, device=DEV)
    rng = np.random.RandomState(2)
    for step in range(3):
        eps = _dev(rng.randn(64, 1))
        elbo = ta.step(eps)
        b.next_minibatch()
        ws = net.workspace(64)
        _abi.check(lib.iwvi_cvae_elbo_and_grad(ctypes.byref(net.d), _abi.ptr(b.X), _abi.ptr(b.Y), 64, _abi.ptr(eps), 0, None, None, _abi.ptr(out),
                                               ctypes.byref(gd), _abi.ptr(ws), None))
        _abi.check(lib.iwvi_adam_step_dev(tensors(True), len(params), 5e-3, 0.9, 0.999, 1e-8, t_dev.data_ptr(), 1, None))
        torch.cuda.synchronize()
        assert float(elbo) == float(out[0])
        for (name, pa), (_, pb) in zip(a.parameters(), params):
            assert _bits(pa) == _bits(pb), (step, name)
        for (xa, ma, va), (xb, mb, vb) in zip(ta.state, state):
            assert _bits(xa) == _bits(xb) and _bits(ma) == _bits(mb) and _bits(va) == _bits(vb)
    assert int(ta.t_dev) == int(t_dev) == 3
    assert a.variance != 0.05 and a.variance == float(a.variance_dev)       # the host copy follows the device scalar


def test_graph_replay_equals_eager_across_an_epoch_boundary():
    eager, graph = _model("50", use_graph=False), _model("50", use_graph=True)
    te, tg = eager.trainer(), graph.trainer()
    assert tg.use_graph and not te.use_graph
    for _ in range(7):                                               # 300 rows, 64 per step: the fifth step starts a new shuffle
        eager.train_op()
        graph.train_op()
    torch.cuda.synchronize()
    assert tg._graph is not None
    assert _all_bits(eager, te) == _all_bits(graph, tg)
    assert int(graph.rng_state[0]) == 7 * 16 and int(graph.rng_state[1]) == 0 and graph.global_step == eager.global_step == 7


def test_global_step_counts_and_the_rate_decays_at_1000():
    a, b = _model("7", lr=5e-3), _model("7", lr=5e-3 * 0.98)
    ta, tb = a.trainer(), b.trainer()
    assert a.global_step == 0 and ta.learning_rate() == 5e-3
    a.global_step = ta.global_step = 998
    eps = _dev(np.random.RandomState(3).randn(64, 1))
    ta.step(eps)
    assert ta.global_step == 999 and ta.learning_rate() == 5e-3
    # step 1000 runs at lr 0.98: it equals the first step of a twin built with that rate (same parameters, same optimiser state)
    c = _model("7", lr=5e-3)
    tc = c.trainer()
    tc.global_step = 999
    tc.step(eps)
    tb.step(eps)
    assert tc.global_step == 1000 and tc.learning_rate() == 5e-3 * 0.98 and tb.learning_rate() == 5e-3 * 0.98
    for (name, pc), (_, pb) in zip(c.parameters(), b.parameters()):
        assert _bits(pc) == _bits(pb), name
    c.init_op()
    assert c.global_step == 0 and tc.global_step == 0


def test_training_run_and_both_evaluation_routes():
    from dgps_with_iwvi_amd import evaluation
    m = _model("50", use_graph=True)
    Xh, Yh = _data(64, seed=9)
    Xs, Ys = _data(100, seed=10)
    eps = _dev(np.random.RandomState(4).randn(64, 1))

    def held_out():
        keep = m.X, m.Y
        m.X, m.Y = _dev(Xh), _dev(Yh)
        try:
            return float(m.compute_log_likelihood(eps))
        finally:
            m.X, m.Y = keep
    before = held_out()
    for _ in range(300):
        m.train_op()
    after = held_out()
    print("held-out bound: %.1f -> %.1f" % (before, after))
    assert math.isfinite(before) and math.isfinite(after) and after > before
    assert m.global_step == 300
    on = evaluation.evaluate(m, Xs, Ys, 200, on_device=True)
    off = evaluation.evaluate(m, Xs, Ys, 200, on_device=False)
    for res in (on, off):
        assert math.isfinite(res["test_loglik"]) and math.isfinite(res["test_rmse"]), res
    assert math.isfinite(on["test_shapiro_W_median"])
    mean, sd = m.predict_y(Xs)
    assert mean.shape == sd.shape == (100, 1) and torch.isfinite(mean).all() and float(sd[0, 0]) == float(m.variance_dev.sqrt())
    smp = m.predict_y_samples(Xs, 3)
    assert smp.shape == (3, 100, 1) and torch.isfinite(smp).all()


def test_checkpoint_round_trip(tmp_path):
    from dgps_with_iwvi_amd.build_models import load_checkpoint, save_checkpoint
    a = _model("7")
    for _ in range(3):
        a.train_op()
    path = str(tmp_path / "cvae.npz")
    save_checkpoint(a, path, a.trainer())
    b = _model("7", init_seed=6)                                     # other initial values
    load_checkpoint(b, path, b.trainer())
    assert b.global_step == 3 == b.trainer().global_step
    assert _all_bits(a, a.trainer()) == _all_bits(b, b.trainer())
    assert _bits(a.X) == _bits(b.X) and _bits(a.Y) == _bits(b.Y)
    a.train_op()
    b.train_op()
    assert _all_bits(a, a.trainer()) == _all_bits(b, b.trainer())   # and the two continue alike: batch order, noise counter, optimiser
