"""Float64 reference, float32 restatement, input families and tolerances for the Adam update kernel (k_adam behind iwvi_adam_step /
iwvi_adam_step_dev, csrc/backward.hip).  TEST INFRASTRUCTURE ONLY: tests/test_adam_reference_host.py pins this module on the CPU,
tests/test_gpu_adam.py compares the kernel with it.

The reference is ``oracle/optim_oracle.Adam`` (NumPy float64), started at a step count ``t0`` and read after every step.  It is given what
the device is given: parameters and gradients rounded to float32 first, and beta1 / beta2 / eps as the float32 numbers the kernel holds
(the kernel's recurrences run on float(beta); a reference on the unrounded 0.999 would differ from ANY float32 Adam by 1.3e-5 in v).

``restate_f32`` is the device recurrence in NumPy float32, operation for operation (the compiler may contract a multiply-add that NumPy
rounds twice: half a spacing, inside the margin below).  Its chain factor through softplus is selectable:
  "from_p":  1 - exp(-(p - 1e-6))      sigmoid(x) rebuilt from the rounded constrained value (the kernel before this module existed)
  "from_x":  1 / (1 + exp(-x))         sigmoid(x) from the unconstrained state

Tolerance rule, stated on the unconstrained state x because an atol on p hides the 1e-6 floor:
  tol_x(family) = 4 x max |x_restatement("from_x") - x_float64| over all steps and elements; m and v likewise;
  |p - p_ref| <= tol_x p_ref + spacing32(p_ref) for positive tensors (|dp/dx| = sigmoid(x) <= p everywhere), and
  |p - p_ref| <= tol_x + spacing32(p_ref) for unconstrained ones (p is x).
The constants (TOL) were computed by ``measure_tol`` at N_FAMILY elements, seed 0, and rounded up to two digits
with 2% to spare for another libm's last bit; the factor 4 is a margin
for the device's __expf / log1pf / logf (a few units in the last place where NumPy's are correctly rounded or nearly so), never fitted to
the kernel.  CEILING_RTOL: no family outside positive_floor / driven_down may be further than the project's rtol = 3e-5 off on p."""
import functools
import math
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import optim_oracle as oo   # noqa: E402

ADAM_MAX = 48                                                    # csrc/backward.hip
MAX_BLOCKS, BLOCK = 1024, 256                                    # the launch: min(1024, ceil(n_max / 256)) x n_tensors workgroups of 256
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8                             # what a caller passes (training.Trainer's defaults)
B1F, B2F, EPSF = (float(np.float32(v)) for v in (BETA1, BETA2, EPS))   # what the kernel holds
N_FAMILY = 4096
CEILING_RTOL, CEILING_ATOL_PLAIN = 3e-5, 3e-6                    # tests/test_gpu_training.py::test_adam_steps_match_oracle
LOOSE_FAMILIES = ("positive_floor", "driven_down")               # exempt from the ceiling (relative on p, spacing32(x) alone is ~1e-6 there)

# family -> (transform, p0 range or None, steps, lr)
FAMILIES = {
    "plain":          (0, None,           20, 0.01),
    "positive_mid":   (1, (1e-2, 3.0),    20, 0.01),
    "positive_small": (1, (1e-5, 1e-3),   20, 0.01),
    "positive_floor": (1, (1.2e-6, 3e-5), 50, 0.01),
    "driven_down":    (1, (1e-3, 1e-2),  200, 0.05),
    "driven_up":      (1, (10.0, 19.0),  100, 0.05),
    "tiny_grad":      (1, (0.1, 1.0),     20, 0.01),
    "huge_grad":      (1, (0.1, 1.0),     20, 0.01),
    "late_1000":      (1, (1e-2, 3.0),    10, 0.01),
    "late_1000000":   (1, (1e-2, 3.0),    10, 0.01),
}
LATE_WARMUP = 50

# family -> (tol_x, tol_m, tol_v): 4 x the "from_x" restatement's worst distance from float64 (measure_tol(); N_FAMILY elements, seed 0)
TOL = {
    "plain":          (3.8e-06, 5.8e-07, 5.4e-08),
    "positive_mid":   (7.8e-06, 4.2e-07, 3.0e-08),
    "positive_small": (2.0e-05, 2.0e-09, 1.8e-13),
    "positive_floor": (3.1e-05, 2.6e-10, 1.3e-15),
    "driven_down":    (3.6e-05, 2.9e-08, 1.3e-11),
    "driven_up":      (7.9e-05, 1.6e-06, 3.4e-07),
    "tiny_grad":      (4.4e-06, 2.6e-14, 1.3e-22),
    "huge_grad":      (4.1e-06, 2.8e-01, 1.4e+04),
    "late_1000":      (6.2e-06, 3.3e-07, 7.7e-08),
    "late_1000000":   (6.7e-06, 3.2e-07, 7.2e-08),
}

Case = namedtuple("Case", "name transform p0 grads grads64 lr t0 m0 v0 steps")
Run = namedtuple("Run", "x0 x m v p")                            # x0 [n]; the rest [steps, n], after each step


def f32(a):
    """Round to float32, return float64."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def spacing32(x):
    """Distance from |x| to the next float32 above it."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def lr_t_host(lr, t, b1=B1F, b2=B2F):
    """The bias-corrected rate of step t as iwvi_adam_step forms it: float64 on the betas the kernel holds, rounded once."""
    return np.float32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def lr_t_dev(lr, t, b1=B1F, b2=B2F):
    """... and as k_adam forms it from the device step count (iwvi_adam_step_dev): lr is rounded to float32 FIRST."""
    return np.float32(float(np.float32(lr)) * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), n))


def _draw_grads(name, rng, steps, n):
    if name == "driven_down":
        return rng.uniform(0.5, 1.5, (steps, n))
    if name == "driven_up":
        return -rng.uniform(0.5, 1.5, (steps, n))
    g = rng.standard_normal((steps, n))
    return 1e-7 * g if name == "tiny_grad" else 1e6 * g if name == "huge_grad" else g


@functools.lru_cache(maxsize=None)
def family(name, n=N_FAMILY, seed=0, steps=None):
    """The seeded inputs of a family: p0 [n] and grads [steps, n] hold float32 values (what the device reads); grads64 are the draws
    before rounding (for IWVI_ADAM_GRAD_F64).  late_*: p0, m0, v0 are the float32 roundings of a float64 warm-up of LATE_WARMUP steps."""
    transform, rng_p, fam_steps, lr = FAMILIES[name]
    steps = steps or fam_steps
    rng = np.random.default_rng([seed, n, sorted(FAMILIES).index(name)])
    p0 = rng.standard_normal(n) if rng_p is None else _log_uniform(rng, rng_p[0], rng_p[1], n)
    p0 = f32(p0)
    t0, m0, v0 = 1, None, None
    if name.startswith("late_"):
        t0 = int(name[5:])
        warm = oo.Adam([p0], [True], lr, B1F, B2F, EPSF)
        for g in f32(rng.standard_normal((LATE_WARMUP, n))):
            p0 = warm.step([g])[0]
        p0, m0, v0 = f32(p0), f32(warm.m[0]), f32(warm.v[0])
    g64 = _draw_grads(name, rng, steps, n)
    for a in (p0, g64, m0, v0):
        if a is not None:
            a.setflags(write=False)
    g = f32(g64); g.setflags(write=False)
    return Case(name, transform, p0, g, g64, lr, t0, m0, v0, steps)


def generic_case(transform, n, seed, steps=3):
    """plain / positive_mid inputs at any length (the size and full-launch tests): same distributions, own seed."""
    return family("positive_mid" if transform else "plain", n, seed, steps)


def tol_of(case):
    return TOL[case.name]


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def reference(case, lrs=None, maximise=False):
    """oracle/optim_oracle.Adam on the case, float64; ``lrs``: a rate per step (default: the family's, every step)."""
    opt = oo.Adam([case.p0], [bool(case.transform)], case.lr, B1F, B2F, EPSF, t0=case.t0)
    if case.m0 is not None:
        opt.m[0], opt.v[0] = case.m0.copy(), case.v0.copy()
    x0 = opt.x[0].copy()
    xs, ms, vs, ps = [], [], [], []
    for s, g in enumerate(case.grads):
        p = opt.step([-g if maximise else g], lr=None if lrs is None else lrs[s])[0]
        xs.append(opt.x[0].copy()); ms.append(opt.m[0].copy()); vs.append(opt.v[0].copy()); ps.append(p.copy())
    return Run(x0, np.array(xs), np.array(ms), np.array(vs), np.array(ps))


@functools.lru_cache(maxsize=None)
def family_reference(name, n=N_FAMILY, seed=0):
    r = reference(family(name, n, seed))
    for a in r:
        a.setflags(write=False)
    return r


# ---- float32 restatement of the device recurrence ------------------------------------------------------------------------------------
_F = np.float32


def init_f32(p, transform):
    """init != 0: x = p, or logf(expm1f(p - 1e-6f)) with y > 20 -> y."""
    p = np.asarray(p, dtype=_F)
    if not transform:
        return p.copy()
    y = (p - _F(1e-6)).astype(_F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return np.where(y > _F(20), y, np.log(np.expm1(np.minimum(y, _F(80))).astype(_F)).astype(_F)).astype(_F)


def softplus_f32(x):
    """(x > 20 ? x : log1pf(expf(x))) + 1e-6f."""
    x = np.asarray(x, dtype=_F)
    with np.errstate(over="ignore"):
        sp = np.where(x > _F(20), x, np.log1p(np.exp(np.minimum(x, _F(80))).astype(_F)).astype(_F)).astype(_F)
    return (sp + _F(1e-6)).astype(_F)


def chain_factor_f32(x, p, factor):
    with np.errstate(over="ignore"):
        if factor == "from_p":
            return (_F(1) - np.exp(-((p - _F(1e-6)).astype(_F))).astype(_F)).astype(_F)
        if factor == "from_x":
            return (_F(1) / (_F(1) + np.exp(-x).astype(_F)).astype(_F)).astype(_F)
    raise ValueError(factor)


def restate_f32(case, factor="from_x", lr_t=lr_t_host, lrs=None):
    """k_adam in NumPy float32 on the case -> Run of float32 arrays."""
    b1, b2, eps = _F(BETA1), _F(BETA2), _F(EPS)
    p = case.p0.astype(_F)
    x = init_f32(p, case.transform)
    x0 = x.copy()
    m = np.zeros_like(x) if case.m0 is None else case.m0.astype(_F)
    v = np.zeros_like(x) if case.v0 is None else case.v0.astype(_F)
    xs, ms, vs, ps = [], [], [], []
    for s, g in enumerate(case.grads.astype(_F)):
        rate = lr_t(case.lr if lrs is None else lrs[s], case.t0 + s)
        if case.transform:
            g = (g * chain_factor_f32(x, p, factor)).astype(_F)
        m = ((b1 * m).astype(_F) + ((_F(1) - b1) * g).astype(_F)).astype(_F)
        v = ((b2 * v).astype(_F) + (((_F(1) - b2) * g).astype(_F) * g).astype(_F)).astype(_F)
        x = (x - ((rate * m).astype(_F) / (np.sqrt(v).astype(_F) + eps).astype(_F)).astype(_F)).astype(_F)
        p = softplus_f32(x) if case.transform else x.copy()
        xs.append(x); ms.append(m); vs.append(v); ps.append(p)
    return Run(x0, np.array(xs), np.array(ms), np.array(vs), np.array(ps))


# ---- tolerances -----------------------------------------------------------------------------------------------------------------------
def worst(run, ref):
    """(max |dx|, max |dm|, max |dv|, max |dp| / p_ref) of a run against the reference, over all steps and elements (x0 included)."""
    dx = max(np.abs(run.x.astype(np.float64) - ref.x).max(), np.abs(run.x0.astype(np.float64) - ref.x0).max())
    return (dx, np.abs(run.m.astype(np.float64) - ref.m).max(), np.abs(run.v.astype(np.float64) - ref.v).max(),
            (np.abs(run.p.astype(np.float64) - ref.p) / np.abs(ref.p)).max())


def measure_tol(name):
    """4 x the "from_x" restatement's worst distance from float64 on x, m, v: what TOL holds (rounded up to two digits, 2% to spare)."""
    return tuple(4.0 * e for e in worst(restate_f32(family(name)), family_reference(name))[:3])


def p_tol(case, p_ref, tol_x):
    """The rule on the constrained value."""
    p_ref = np.asarray(p_ref, dtype=np.float64)
    return (tol_x * np.abs(p_ref) if case.transform else tol_x) + spacing32(p_ref)


def ceiling(case, p_ref):
    """The hard ceiling on |p - p_ref| (None for the two families whose p lives at the floor): rtol = 3e-5, with the project's
    atol = 3e-6 only where p is an unconstrained number that may be 0."""
    if case.name in LOOSE_FAMILIES:
        return None
    return CEILING_RTOL * np.abs(p_ref) + (0.0 if case.transform else CEILING_ATOL_PLAIN)


def entry_points_bound(case, ref):
    """How far the x of iwvi_adam_step and of iwvi_adam_step_dev may be apart after each step [steps, n]: the _dev form rounds lr to
    float32 before the bias correction, so its lr_t is at most one float32 spacing away; propagated: per step two spacings of lr_t times
    the reference's |m / (sqrt v + eps)| (one for the rate itself, one for the roundings of m and v that a moved x flips through the
    chain factor) plus one spacing of x (the subtraction rounds on a different number), accumulated over the steps."""
    per = []
    for s in range(case.steps):
        rate = float(lr_t_host(case.lr, case.t0 + s))
        ratio = np.abs(ref.m[s]) / (np.sqrt(ref.v[s]) + EPSF)
        per.append(2.0 * spacing32(rate) * ratio + spacing32(ref.x[s]))
    return np.cumsum(np.array(per), axis=0)
