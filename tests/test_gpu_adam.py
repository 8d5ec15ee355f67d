"""k_adam (csrc/backward.hip) behind iwvi_adam_step / iwvi_adam_step_dev against the float64 reference of tests/adam_reference.py, at the
kernel's numerical edges: the 1e-6 floor of the positive transform, both sides of its x > 20 branch, gradients of 1e-7 and 1e6, step
counts of 1000 and 10^6, float64 gradients, the grid-stride loop (more than 262144 elements), a full 48-tensor launch.

The rule (adam_reference): x, m, v within 4 x what a NumPy float32 restatement of the recurrence is off the float64 reference, per family;
|p - p_ref| <= tol_x p_ref + spacing32(p_ref); and nowhere outside positive_floor / driven_down further than rtol = 3e-5 on p.

MEASURED (MI355X; worst over all steps and the 4096 elements of a family; "restatement" = tol / 4):
  family            tol_x    device |dx|            device |dp|/p          after / restatement (x)
                             before     after       before     after
  plain             3.8e-06  1.28e-06   9.17e-07    (p is x)               0.97
  positive_mid      7.8e-06  2.52e-06   2.00e-06    2.51e-06   2.12e-06    1.02
  positive_small    2.0e-05  2.28e-04   5.81e-06    2.07e-04   5.02e-06    1.16
  positive_floor    3.1e-05  1.56e-02   7.44e-06    2.87e-03   6.96e-06    0.96
  driven_down       3.6e-05  1.68e-04   9.10e-06    1.63e-04   8.86e-06    1.01
  driven_up         7.9e-05  4.67e-05   1.91e-05    2.61e-06   8.75e-07    0.97
  tiny_grad         4.4e-06  1.31e-06   1.31e-06    1.33e-06   1.33e-06    1.19
  huge_grad         4.1e-06  1.59e-06   9.92e-07    1.53e-06   1.00e-06    0.97
  late_1000         6.2e-06  1.74e-06   1.52e-06    1.73e-06   1.44e-06    0.98
  late_1000000      6.7e-06  1.59e-06   1.39e-06    1.80e-06   1.42e-06    0.83
"before": the kernel that formed the chain factor as 1 - __expf(-(p - 1e-6)) and iwvi_adam_step's bias correction on the unrounded betas
(the worse of the two entry points); "after": the factor from x, 1 / (1 + __expf(-x)), and both entry points correcting on the float32 betas
the recurrences run on.  Before, positive_floor was 500 x outside the rule on x (1.56e-2; 2.9e-3 relative on p), positive_small 11 x,
driven_down 5 x, and the two entry points were up to 45 x their bound apart (1 - 0.999^t against 1 - float(0.999)^t: 6.7e-6 of lr_t);
after, every family sits at 0.83 ... 1.19 x the NumPy restatement's own error, i.e. at a quarter of the rule, and the entry points within
0.66 x their bound.  m and v: 0.78 ... 1.33 x the restatement's.  Init: |dx0| <= 2.9e-6 (x near 19), 2.1e-6 at the floor.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as ar   # noqa: E402

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 64, 777.25                                       # elements past n in every buffer, and what they hold


class _Tensors:
    """Device buffers (param, grad, x, m, v; each n + PAD long, the tail holding SENTINEL) of a list of adam_reference cases."""

    def __init__(self, dev, cases, g64=None):
        self.dev, self.cases = dev, list(cases)
        self.g64 = [False] * len(self.cases) if g64 is None else list(g64)
        self.n = [c.p0.size for c in self.cases]
        mk = lambda n, dt=torch.float32: torch.full((n + PAD,), SENTINEL, dtype=dt, device=dev)
        self.p, self.x, self.m, self.v = ([mk(n) for n in self.n] for _ in range(4))
        self.g = [mk(n, torch.float64 if d else torch.float32) for n, d in zip(self.n, self.g64)]
        for c, p, n in zip(self.cases, self.p, self.n):
            p[:n] = torch.as_tensor(c.p0.astype(np.float32), device=dev)

    def descriptors(self, grad=True, count=None):
        from dgps_with_iwvi_amd import _abi
        k = len(self.cases)
        arr = (_abi.AdamTensor * (count or k))()
        for j in range(count or k):
            i, a = j % k, arr[j]
            a.param, a.x, a.m, a.v = self.p[i].data_ptr(), self.x[i].data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr()
            a.n, a.transform = self.n[i], self.cases[i].transform | (_abi.ADAM_GRAD_F64 if self.g64[i] else 0)
            if grad:
                a.grad = self.g[i].data_ptr()
        return arr

    def load_grads(self, step, negate=False):
        for c, g, n, d in zip(self.cases, self.g, self.n, self.g64):
            src = (c.grads64 if d else c.grads.astype(np.float32))[step]
            g[:n] = torch.tensor(-src if negate else src, device=self.dev)

    def host(self, lr, t, maximise=0, init=0, arr=None):
        from dgps_with_iwvi_amd import _abi
        rc = _abi.lib().iwvi_adam_step(self.descriptors(grad=not init) if arr is None else arr, len(arr) if arr is not None else len(self.cases),
                                       lr, ar.BETA1, ar.BETA2, ar.EPS, t, maximise, init, _abi.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def device(self, lr, t_dev, maximise=0, arr=None):
        from dgps_with_iwvi_amd import _abi
        rc = _abi.lib().iwvi_adam_step_dev(self.descriptors() if arr is None else arr, len(arr) if arr is not None else len(self.cases),
                                           lr, ar.BETA1, ar.BETA2, ar.EPS, None if t_dev is None else t_dev.data_ptr(), maximise, _abi.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def init(self):
        """init = 1 (no gradient attached), then the carried moments of a late_* case."""
        assert self.host(0.0, 1, init=1) == 0
        for c, m, v, n in zip(self.cases, self.m, self.v, self.n):
            if c.m0 is not None:
                m[:n] = torch.as_tensor(c.m0.astype(np.float32), device=self.dev)
                v[:n] = torch.as_tensor(c.v0.astype(np.float32), device=self.dev)

    def read(self, i=0):
        """(x, m, v, p) of tensor i, float32 NumPy, without the tail."""
        return tuple(b[i][:self.n[i]].cpu().numpy() for b in (self.x, self.m, self.v, self.p))

    def snapshot(self):
        return [b.clone() for bufs in (self.p, self.g, self.x, self.m, self.v) for b in bufs]

    def tails_intact(self):
        return all(bool((b[n:] == SENTINEL).all()) for bufs in (self.p, self.g, self.x, self.m, self.v) for b, n in zip(bufs, self.n))


def _run(dev, case, entry, g64=False, lrs=None, maximise=0, negate=False):
    """All steps of one case through one entry point -> (adam_reference.Run of float32 arrays, final device step count or None)."""
    T = _Tensors(dev, [case], [g64])
    T.init()
    x0 = T.read()[0]
    t_dev = torch.full((1,), case.t0 - 1, dtype=torch.int64, device=dev) if entry == "dev" else None
    out = []
    for s in range(case.steps):
        T.load_grads(s, negate)
        lr = case.lr if lrs is None else lrs[s]
        assert (T.device(lr, t_dev, maximise) if entry == "dev" else T.host(lr, case.t0 + s, maximise)) == 0
        out.append(T.read())
    assert T.tails_intact()
    return ar.Run(x0, *(np.array([o[k] for o in out]) for k in range(4))), (None if t_dev is None else int(t_dev.item()))


_RUNS = {}


def family_run(dev, name, entry, g64=False):
    """Each (family, entry point, gradient type) runs on the device once per session."""
    key = (name, entry, g64)
    if key not in _RUNS:
        _RUNS[key] = _run(dev, ar.family(name), entry, g64)
    return _RUNS[key]


def figures(run, ref, case):
    """Worst |dx|, |dm|, |dv|, relative |dp| over all steps and elements, and each as a multiple of the restatement's (tol / 4)."""
    w = ar.worst(run, ref)
    tol = ar.tol_of(case)
    return w, tuple(4.0 * a / b for a, b in zip(w[:3], tol))


def _assert_rule(run, ref, case, what):
    w, ratio = figures(run, ref, case)
    print("ADAM %-15s %-6s |dx| %.3e  |dm| %.3e  |dv| %.3e  |dp|/p %.3e   x restatement: %.2f %.2f %.2f" % ((case.name, what) + w + ratio))
    tol_x, tol_m, tol_v = ar.tol_of(case)
    assert np.abs(run.x0.astype(np.float64) - ref.x0).max() <= tol_x, (case.name, what, "x0")
    for got, want, tol, field in ((run.x, ref.x, tol_x, "x"), (run.m, ref.m, tol_m, "m"), (run.v, ref.v, tol_v, "v")):
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(np.isfinite(got)) and err.max() <= tol, (case.name, what, field, err.max(), tol, np.unravel_index(err.argmax(), err.shape))
    err_p = np.abs(run.p.astype(np.float64) - ref.p)
    assert np.all(err_p <= ar.p_tol(case, ref.p, tol_x)), (case.name, what, "p", (err_p / np.abs(ref.p)).max())
    ceil = ar.ceiling(case, ref.p)
    if ceil is not None:
        assert np.all(err_p <= ceil), (case.name, what, "ceiling", (err_p / np.abs(ref.p)).max())
    if not case.transform:
        assert np.array_equal(run.p, run.x)


@pytest.mark.parametrize("name", sorted(ar.FAMILIES))
def test_every_family_through_both_entry_points(gpu_device, name):
    """x, m, v and param after every step, iwvi_adam_step (host t) and iwvi_adam_step_dev (int64 device counter starting at t0 - 1, k_inc_i64)."""
    case, ref = ar.family(name), ar.family_reference(name)
    host, _ = family_run(gpu_device, name, "host")
    devr, count = family_run(gpu_device, name, "dev")
    _assert_rule(host, ref, case, "host")
    _assert_rule(devr, ref, case, "dev")
    assert count == case.t0 - 1 + case.steps
    # the two forms against each other: the _dev form rounds lr to float32 BEFORE the bias correction (the kernel argument is a float), the
    # host form rounds lr_t once; both correct on the float32 betas.  One spacing of lr_t, propagated (adam_reference.entry_points_bound)
    bound = ar.entry_points_bound(case, ref)
    dx = np.abs(host.x.astype(np.float64) - devr.x.astype(np.float64))
    print("ADAM %-15s host-dev |dx| %.3e (bound at its worst element %.3e)" % (name, dx.max(), bound.flat[dx.argmax()]))
    assert np.array_equal(host.x0, devr.x0) and np.all(dx <= bound), (name, dx.max(), np.unravel_index((dx - bound).argmax(), dx.shape))
    dp = np.abs(host.p.astype(np.float64) - devr.p.astype(np.float64))
    assert np.all(dp <= (bound * np.abs(ref.p) if case.transform else bound) + ar.spacing32(ref.p))


@pytest.mark.parametrize("name", sorted(ar.FAMILIES))
def test_float64_gradients_equal_their_float32_roundings(gpu_device, name):
    """IWVI_ADAM_GRAD_F64 (the head kernel's float64 sums): the kernel rounds each to float32 and goes on as before -- bit-identical to
    being handed the roundings, in the form Trainer calls."""
    a, ca = family_run(gpu_device, name, "dev", g64=True)
    b, cb = family_run(gpu_device, name, "dev")
    assert ca == cb
    for u, w in zip(a, b):
        assert np.array_equal(u, w)


def test_one_call_mixing_float64_and_float32_gradients(gpu_device):
    cases = [ar.generic_case(1, 300, 7), ar.generic_case(0, 70000, 8), ar.generic_case(1, 1, 9), ar.generic_case(0, 7, 10)]
    flags = [True, False, False, True]
    T = _Tensors(gpu_device, cases, flags)
    T.init()
    t_dev = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    for s in range(3):
        T.load_grads(s)
        assert T.device(0.01, t_dev) == 0
    assert T.tails_intact() and int(t_dev.item()) == 3
    for i, c in enumerate(cases):
        alone, _ = _run(gpu_device, c, "dev", g64=not flags[i])    # each tensor on its own, with the OTHER gradient type
        for got, want in zip(T.read(i), (alone.x[-1], alone.m[-1], alone.v[-1], alone.p[-1])):
            assert np.array_equal(got, want), i


@pytest.mark.parametrize("transform", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 262144, 262145, 524288 + 3])
def test_sizes_and_the_grid_stride_loop(gpu_device, n, transform):
    """One tensor of n elements: one thread, the edges of a workgroup, the last size without the grid-stride loop (1024 workgroups of 256),
    the first with it, and an inner q_sqrt at M = 128, R = 32 plus an odd tail.  Every element against the reference; nothing past n moves
    (_run asserts the sentinels behind all five buffers)."""
    case = ar.generic_case(transform, n, 1000 + transform)
    run, _ = _run(gpu_device, case, "dev")
    _assert_rule(run, ar.reference(case), case, "n=%d" % n)


def test_a_full_launch_of_48_tensors(gpu_device):
    """ADAM_MAX tensors in one launch, short ones sharing a grid sized for the longest (300000 elements: the grid-stride loop)."""
    sizes = [(1, 7, 300, 70000)[i % 4] for i in range(ar.ADAM_MAX)]
    sizes[5] = 300000
    cases = [ar.generic_case(i % 2, n, 2000 + i) for i, n in enumerate(sizes)]
    T = _Tensors(gpu_device, cases)
    T.init()
    t_dev = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    runs = [[] for _ in cases]
    x0 = [T.read(i)[0] for i in range(len(cases))]
    for s in range(3):
        T.load_grads(s)
        assert T.device(0.01, t_dev) == 0
        for i in range(len(cases)):
            runs[i].append(T.read(i))
    assert T.tails_intact() and int(t_dev.item()) == 3
    for i, c in enumerate(cases):
        run = ar.Run(x0[i], *(np.array([o[k] for o in runs[i]]) for k in range(4)))
        _assert_rule(run, ar.reference(c), c, "tensor %d" % i)


def test_maximise_is_the_step_on_the_negated_gradient(gpu_device):
    for name in ("plain", "positive_small"):
        case = ar.family(name, 1000, 5, 3)
        for entry in ("host", "dev"):
            a, _ = _run(gpu_device, case, entry, maximise=1)
            b, _ = _run(gpu_device, case, entry, maximise=0, negate=True)
            for u, w in zip(a, b):
                assert np.array_equal(u, w), (name, entry)
        ref = ar.reference(case, maximise=True)
        _assert_rule(a, ref, case, "maximise")


def _large_positive_case():
    """p0 on both sides of the inverse transform's y > 20 branch (no family starts above 19)."""
    p0 = ar.f32(np.concatenate([np.random.default_rng(4).uniform(15.0, 40.0, 1000), [20.0, 20.000002, 20.000004, 19.999998]]))
    return ar.Case("init_large", 1, p0, np.ones((1, p0.size)), np.ones((1, p0.size)), 0.01, 1, None, None, 1)


@pytest.mark.parametrize("name", sorted(ar.FAMILIES) + ["init_large"])
def test_init_and_a_step_of_zero_rate(gpu_device, name):
    """init = 1: x = transform^-1(param) under the family's rule, m = v = 0, param untouched, no gradient attached.  Then a step with lr = 0:
    x keeps its bits, m and v move as the reference says, and param becomes transform(x): bit for bit the old value where the transform is
    the identity, and for a positive tensor the float32 round trip softplus(log(expm1(p - 1e-6))) + 1e-6 of it -- within the rule of
    param, reproduced bit for bit by a second such step (p is a function of x alone)."""
    from oracle import optim_oracle as oo
    case = _large_positive_case() if name == "init_large" else ar.family(name)
    T = _Tensors(gpu_device, [case])
    before = T.p[0].clone()
    assert T.host(0.0, 1, init=1) == 0                              # (descriptors(grad=False): grad is NULL)
    x, m, v, p = T.read()
    xr = oo.to_unconstrained(case.p0, bool(case.transform))
    # init_large: y = p - 1e-6f, expm1f, logf round to half a spacing of ~x each, and a few units in the last place of expm1f move its
    # logarithm by ~1e-7 absolute: two spacings of x (9.5e-7 at 15)
    tol_x = 2 * ar.spacing32(xr) if name == "init_large" else ar.TOL[name][0]
    err = np.abs(x.astype(np.float64) - xr)
    print("ADAM init %-15s |dx0| %.3e" % (name, err.max()))
    assert np.all(err <= tol_x), (name, err.max())
    assert not m.any() and not v.any() and torch.equal(T.p[0], before) and T.tails_intact()
    if name == "init_large":
        above = case.p0 - 1e-6 > 20.0 + 1e-5
        assert above.sum() > 100 and (~above).sum() > 100
        assert np.array_equal(x[above], (case.p0.astype(np.float32) - np.float32(1e-6))[above])   # the branch: x = y
    if case.m0 is not None:
        return                                                     # (late_*: the same start as positive_mid, moments written by the test)
    T.load_grads(0)
    assert T.host(0.0, case.t0) == 0
    x1, m1, v1, p1 = T.read()
    assert np.array_equal(x1, x)
    ref = ar.reference(case._replace(grads=case.grads[:1], steps=1), lrs=[0.0])
    if name != "init_large":
        assert np.abs(m1 - ref.m[0]).max() <= ar.TOL[name][1] and np.abs(v1 - ref.v[0]).max() <= ar.TOL[name][2]
    else:                                                          # g = 1: m = 0.1 sigmoid(x), v = 0.001 sigmoid(x)^2, sigmoid = 1 to 3e-7
        np.testing.assert_allclose(m1, ref.m[0], rtol=4e-7); np.testing.assert_allclose(v1, ref.v[0], rtol=8e-7)
    if case.transform:
        rel = np.abs(p1.astype(np.float64) - case.p0) / case.p0
        print("ADAM init %-15s round trip of param: %.3e relative, %d of %d elements keep their bits" % (name, rel.max(), (p1 == case.p0.astype(np.float32)).sum(), p1.size))
        assert np.all(np.abs(p1.astype(np.float64) - case.p0) <= ar.p_tol(case, case.p0, np.max(tol_x)))
        assert T.host(0.0, case.t0 + 1) == 0
        assert np.array_equal(T.read()[3], p1) and np.array_equal(T.read()[0], x)
    else:
        assert np.array_equal(p1, case.p0.astype(np.float32))


def test_the_same_inputs_give_the_same_bits(gpu_device):
    for name, entry in (("positive_small", "host"), ("driven_up", "dev")):
        first, _ = family_run(gpu_device, name, entry)
        again, _ = _run(gpu_device, ar.family(name), entry)
        for u, w in zip(first, again):
            assert np.array_equal(u, w), (name, entry)


def test_bad_arguments_are_refused_before_any_launch(gpu_device):
    """Argument checks only: each returns IWVI_ERR_ARG and leaves every buffer as it was."""
    from dgps_with_iwvi_amd import _abi
    T = _Tensors(gpu_device, [ar.generic_case(1, 300, 1), ar.generic_case(0, 7, 2)])
    T.init()
    T.load_grads(0)
    t_dev = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    snap = T.snapshot()

    def edited(**kw):
        arr = T.descriptors()
        for k, val in kw.items():
            setattr(arr[1], k, val)
        return arr

    calls = {
        "49 tensors": lambda: T.host(0.01, 1, arr=T.descriptors(count=ar.ADAM_MAX + 1)),
        "49 tensors, device count": lambda: T.device(0.01, t_dev, arr=T.descriptors(count=ar.ADAM_MAX + 1)),
        "n = 0": lambda: T.host(0.01, 1, arr=edited(n=0)),
        "n = 0, device count": lambda: T.device(0.01, t_dev, arr=edited(n=0)),
        "transform 2": lambda: T.host(0.01, 1, arr=edited(transform=2)),
        "transform 2, device count": lambda: T.device(0.01, t_dev, arr=edited(transform=2 | _abi.ADAM_GRAD_F64)),
        "t = 0 without init": lambda: T.host(0.01, 0),
        "null t_dev": lambda: T.device(0.01, None),
        "null grad without init": lambda: T.host(0.01, 1, arr=T.descriptors(grad=False)),
        "null grad, device count": lambda: T.device(0.01, t_dev, arr=T.descriptors(grad=False)),
    }
    for what, call in calls.items():
        assert call() == _abi.ERR_ARG, what
        assert _abi.lib().iwvi_last_error(), what
        assert all(torch.equal(a, b) for a, b in zip(snap, T.snapshot())) and int(t_dev.item()) == 0, what


def test_a_likelihood_variance_at_the_floor_follows_the_oracle_through_trainer(gpu_device):
    """A one-layer Gaussian model whose likelihood variance is 2e-5, ten ``adam_op`` steps on fixed noise: the trained variance follows
    the float64 trainer (gradient oracle + optimiser oracle) within the positive_floor rule, relative on p."""
    import copy
    from dgps_with_iwvi_amd import synthetic
    from dgps_with_iwvi_amd.training import Trainer
    from test_gpu_training import _OracleTrainer, _t
    spec = synthetic.make_spec(L=1, M=16, B=16, K=2, seed=1)
    spec["lik_var"] = float(np.float32(2e-5))
    model = synthetic.build_model(spec, gpu_device)
    tr = Trainer(model, lr=0.01, gamma=1e-2)
    ot = _OracleTrainer(copy.deepcopy(spec), 0.01, 1e-2)
    zs = synthetic.make_noise(spec, seed=100)
    zs_dev = [_t(z, gpu_device) for z in zs]
    tol_x = ar.TOL["positive_floor"][0]
    seen = []
    for s in range(10):
        tr.adam_op(zs_dev)
        ot.adam_step(zs)
        got, want = float(tr._scalars[-1][0].item()), ot.spec["lik_var"]
        seen.append((got, want, abs(got - want) / want))
    print("ADAM trainer lik_var: " + ", ".join("%.6e/%.6e (%.1e)" % t for t in seen))
    assert abs(seen[-1][1] - spec["lik_var"]) > 0.02 * spec["lik_var"]   # it moved (ten steps of ~0.01 in x, dp/dx ~ p)
    for got, want, _ in seen:
        assert abs(got - want) <= tol_x * want + ar.spacing32(want), seen
    assert model.likelihood.variance == seen[-1][0]
