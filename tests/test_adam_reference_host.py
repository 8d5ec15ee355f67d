"""CPU pins of tests/adam_reference.py: the float64 Adam reference against a per-element loop of the TensorFlow rule, the transform round
trip, the stored tolerances against what the float32 restatement measures, and the discrimination of the rule -- the restatement of
k_adam's former chain factor (1 - exp(-(p - 1e-6)), sigmoid(x) rebuilt from the rounded constrained value) fails the rule that the one
formed from x passes."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as ar   # noqa: E402
from oracle import optim_oracle as oo   # noqa: E402


def _loop_adam(p0, positive, grads, lr, b1, b2, eps, t0=1, m=0.0, v=0.0):
    """tf.train.AdamOptimizer on ONE element, in Python floats, on GPflow's Log1pe variable."""
    x = math.log(math.expm1(p0 - 1e-6)) if positive else p0
    out = []
    for s, g in enumerate(grads):
        t = t0 + s
        if positive:
            g = g / (1.0 + math.exp(-x))                           # d softplus / dx = sigmoid(x)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        x = x - lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (math.sqrt(v) + eps)
        out.append((x, m, v, (math.log1p(math.exp(x)) + 1e-6) if positive else x))
    return out


@pytest.mark.parametrize("name", ["plain", "positive_mid", "positive_floor", "driven_up", "tiny_grad", "late_1000"])
def test_reference_equals_a_per_element_loop_of_the_tensorflow_rule(name):
    c, ref = ar.family(name), ar.family_reference(name)
    for i in (0, 1, 17, 4095):
        loop = _loop_adam(float(c.p0[i]), bool(c.transform), [float(g) for g in c.grads[:, i]], c.lr, ar.B1F, ar.B2F, ar.EPSF, c.t0,
                          0.0 if c.m0 is None else float(c.m0[i]), 0.0 if c.v0 is None else float(c.v0[i]))
        for k, field in enumerate((ref.x, ref.m, ref.v, ref.p)):
            # (the oracle writes the chain factor as 1 - exp(-softplus(x)): the same number to ~1e-9 relative at the floor in float64;
            # m is a sum of terms of both signs, so its share of that is relative to the largest |m| of the run)
            np.testing.assert_allclose(field[:, i], [row[k] for row in loop], rtol=1e-8, atol=1e-8 * np.abs(field[:, i]).max(),
                                       err_msg="%s[%d] field %d" % (name, i, k))


def test_start_step_and_exposed_state_do_not_change_what_the_oracle_computes():
    """Adam(t0=11) with the moments of ten steps continues the uninterrupted run exactly."""
    rng = np.random.default_rng(3)
    p, gs = [rng.uniform(0.1, 2.0, 5), rng.standard_normal(4)], [[rng.standard_normal(5), rng.standard_normal(4)] for _ in range(15)]
    a = oo.Adam(p, [True, False], 0.01)
    for g in gs[:10]:
        mid = a.step(g)
    b = oo.Adam(mid, [True, False], 0.01, t0=11)
    b.x, b.m, b.v = [x.copy() for x in a.x], [m.copy() for m in a.m], [v.copy() for v in a.v]
    for g in gs[10:]:
        pa, pb = a.step(g, lr=0.02), b.step(g, lr=0.02)
    assert a.t == b.t == 15
    for u, w in zip(pa + a.x + a.m + a.v, pb + b.x + b.m + b.v):
        assert np.array_equal(u, w)


def test_transforms_round_trip_in_float64():
    p = np.concatenate([np.exp(np.random.default_rng(0).uniform(math.log(1.2e-6), math.log(40.0), 2000)), [1.0e-6 + 1e-9, 19.9, 20.1, 31.0, 500.0]])
    x = oo.to_unconstrained(p, True)
    # p - 1e-6 is exact to 2^-53 p, so the round trip is good to 2^-52 p / (p - 1e-6) relative on y = p - 1e-6
    np.testing.assert_allclose(oo.to_constrained(x, True) - 1e-6, p - 1e-6, rtol=4e-16 * (p / (p - 1e-6)).max() + 1e-15)
    np.testing.assert_allclose(oo.to_constrained(x, True), p, rtol=1e-14)   # (a rounding of x moves softplus(x) by |x| 2^-53 relative at most, |x| < 21 below the branch)
    q = np.array([-3.0, 0.0, 7.5])
    assert np.array_equal(oo.to_constrained(oo.to_unconstrained(q, False), False), q)
    # and the float32 restatement of the pair agrees with it to float32 rounding of x (both branches of both directions)
    p32 = ar.f32(p[p > 1.1e-6])
    x32 = ar.init_f32(p32, 1).astype(np.float64)
    xr = oo.to_unconstrained(p32, True)
    assert np.all(np.abs(x32 - xr) <= 2 * ar.spacing32(xr) + 2.0 ** -23 * p32 / (p32 - 1e-6))


@pytest.mark.parametrize("name", sorted(ar.FAMILIES))
def test_stored_tolerance_is_four_times_the_restatement_and_under_the_ceiling(name):
    c, ref = ar.family(name), ar.family_reference(name)
    run = ar.restate_f32(c, "from_x")
    ex, em, ev, _ = ar.worst(run, ref)
    for got, tol, what in zip((ex, em, ev), ar.TOL[name], "xmv"):
        assert got <= tol / 4, (name, what, got, tol)              # inside the rule with the whole margin to spare, by construction
        assert tol / 4 <= 1.15 * got, (name, what, got, tol)       # ... and the stored constant is that measurement, not a looser number
    # the _dev form's rate (lr rounded first) stays inside the rule as well
    ex_dev = ar.worst(ar.restate_f32(c, "from_x", ar.lr_t_dev), ref)[0]
    assert ex_dev <= ar.TOL[name][0] / 2, (name, ex_dev)
    # p under the rule, and under the project's rtol = 3e-5 where the ceiling applies
    err_p = np.abs(run.p.astype(np.float64) - ref.p)
    assert np.all(err_p <= ar.p_tol(c, ref.p, ar.TOL[name][0] / 4))
    ceil = ar.ceiling(c, ref.p)
    assert (ceil is None) == (name in ar.LOOSE_FAMILIES)
    if ceil is not None:
        assert np.all(err_p <= ceil), (name, (err_p / np.abs(ref.p)).max())


def test_families_are_what_they_say():
    for name, (transform, rng_p, steps, lr) in ar.FAMILIES.items():
        c = ar.family(name)
        assert c.grads.shape == (steps, ar.N_FAMILY) and c.transform == transform and c.lr == lr
        assert np.array_equal(c.grads, ar.f32(c.grads64)) and np.array_equal(c.p0, ar.f32(c.p0))
        if rng_p is not None and c.m0 is None:
            assert c.p0.min() >= rng_p[0] * (1 - 1e-7) and c.p0.max() <= rng_p[1] * (1 + 1e-7)
            assert c.p0.min() < rng_p[0] * 1.05 and c.p0.max() > rng_p[1] / 1.05       # log-uniform reaches both ends
    x = ar.family_reference("driven_up").x
    up = ar.family_reference("driven_up")
    assert up.x0.max() < 20 < x[-1].max() and x[-1].min() < 20      # some elements cross the softplus branch at 20, some never do
    down = ar.family_reference("driven_down").p[-1]
    assert down.max() < 1e-3 and down.min() < 3e-5                   # ... and driven_down ends below where it started, some of it near the floor
    assert np.abs(ar.family("tiny_grad").grads).max() < 1e-6 and np.abs(ar.family("huge_grad").grads).max() > 3e6
    for name in ("late_1000", "late_1000000"):
        c = ar.family(name)
        assert c.t0 == int(name[5:]) and c.m0 is not None and np.abs(c.m0).max() > 0 and c.v0.min() > 0
    assert float(ar.lr_t_host(0.01, 10 ** 6)) == float(np.float32(0.01))   # the bias correction is gone by then


def test_rule_rejects_the_factor_rebuilt_from_the_constrained_value():
    """Discrimination: the "from_p" restatement is outside tol_x on positive_floor, and on positive_small restricted to p0 <= 3e-5 --
    so a kernel that forms the factor that way fails tests/test_gpu_adam.py (a correctly rounded exp here; __expf can only be worse)."""
    seen = {}
    for name in ("positive_floor", "positive_small", "driven_down"):
        c, ref = ar.family(name), ar.family_reference(name)
        sel = c.p0 <= 3e-5 if name == "positive_small" else np.ones(c.p0.shape, dtype=bool)
        assert sel.sum() >= 500
        tol_x = ar.TOL[name][0]
        err = {f: np.abs(ar.restate_f32(c, f).x.astype(np.float64) - ref.x)[:, sel].max() for f in ("from_x", "from_p")}
        seen[name] = err
        assert err["from_x"] <= tol_x / 4 and err["from_p"] > tol_x, (name, err, tol_x)
    assert seen["positive_floor"]["from_p"] > 100 * ar.TOL["positive_floor"][0], seen   # not a near miss: the factor is noise there
    # and on p, relative: the same verdict through the rule's constrained form
    c, ref = ar.family("positive_floor"), ar.family_reference("positive_floor")
    bad = np.abs(ar.restate_f32(c, "from_p").p.astype(np.float64) - ref.p) > ar.p_tol(c, ref.p, ar.TOL["positive_floor"][0])
    assert bad.any(axis=0).mean() > 0.5                             # most elements, not one outlier


def test_entry_point_rates_are_one_rounding_apart():
    """iwvi_adam_step and iwvi_adam_step_dev form lr_t on the same float32 betas; the only difference is lr rounded to float32 first."""
    for lr in (0.01, 0.05, 5e-3):
        for t in (1, 2, 5, 50, 1000, 10 ** 6):
            a, b = float(ar.lr_t_host(lr, t)), float(ar.lr_t_dev(lr, t))
            assert abs(a - b) <= ar.spacing32(a), (lr, t, a, b)
    # the unrounded betas give another rate altogether while t << 1000 (1 - 0.999^t against 1 - float(0.999)^t)
    assert abs(float(ar.lr_t_host(0.01, 1, ar.BETA1, ar.BETA2)) - float(ar.lr_t_host(0.01, 1))) > 50 * ar.spacing32(float(ar.lr_t_host(0.01, 1)))
