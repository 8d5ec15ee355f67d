"""The bound-family kernels through the C-ABI (csrc/bound_family.hip: iwvi_bound_logw_reduce -> k_bound_logw<SEG>, iwvi_bound_elbo_backward ->
k_bound_bwd + k_bound_finish), fed chosen log-weights and compared with the float64 statement of tests/bound_family_reference.py (pinned on
the CPU by tests/test_bound_family_reference_host.py) and with the entries that already exist at the family's two ends.

(K, G): (1,1), (4,2), (6,3), (16,16), (64,2), (65,5), (65,13), (66,2), (130,2), (130,65), (128,4) -- groups narrower than the smallest
segment, a group straddling lane 63/64, groups of 65 -- against B = 5; B in {1, 3, 5, 65, 257} against (6,3) and (130,2); every (tau, beta) of
the reference module on every shape; the families near_equal, dominant, wide, ties_all, ties_two; the rest (layouts, global KL arrays, the
regulariser channel, the device likelihood variance) rotated over the cases.  Tolerances: all from the two reference modules."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bound_family_reference as F   # noqa: E402
import iw_reduction_reference as R   # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ("bk", "kb")
GLOBS = ((0, 1), (1, R.MAX_R), (R.MAX_GLOB, 1))


def _abi():
    from dgps_with_iwvi_amd import _abi
    return _abi


def _f(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _desc(G=1, tau=1.0, beta=0.0):
    d = _abi().BoundDesc()
    d.groups, d.tau, d.beta = G, tau, beta
    return d


def _glob(kls, dev):
    g = [torch.as_tensor(np.ascontiguousarray(k, dtype=np.float64), device=dev) for k in kls]
    return g, _abi().ptr_array(g), (ctypes.c_int32 * max(len(g), 1))(*[k.numel() for k in g])


def _lay(a, layout):
    """[B, K] -> the array as the device reads it, (stride_b, stride_k): contiguous (the IW tiling) or strided (the VI tiling)."""
    B, K = a.shape[:2]
    if layout == "bk":
        return np.ascontiguousarray(a), K, 1
    return np.ascontiguousarray(np.swapaxes(a, 0, 1)), 1, B


def _reduce(dev, L, G=1, tau=1.0, beta=0.0, layout="bk", kls=(), scale=1.0, want=("logp", "ess", "elbo"), what=""):
    """One reduction, run TWICE on the same ticket word: the same bits, the word zero after each.  -> dict of float64 arrays."""
    a = _abi()
    B, K = L.shape
    arr, sb, sk = _lay(L, layout)
    lw = _f(arr, dev)
    g, gp, gn = _glob(kls, dev)
    ticket = torch.zeros(1, dtype=torch.int64, device=dev)
    out = dict(logp=torch.empty(B, device=dev), ess=torch.empty(B, device=dev), elbo=torch.empty(1, dtype=torch.float64, device=dev))
    first = None
    for _ in range(2):
        for t in out.values():
            t.fill_(float("nan"))
        a.check(a.lib().iwvi_bound_logw_reduce(_desc(G, tau, beta), a.ptr(lw), B, K, sb, sk, gp, gn, len(g), scale,
                                               *[a.ptr(out[k]) if k in want else None for k in ("logp", "ess", "elbo")], a.ptr(ticket), a.stream_ptr()))
        assert int(ticket.item()) == 0, "%s: ticket word left at %d" % (what, int(ticket.item()))
        got = {k: out[k].clone() for k in out}
        if first is None:
            first = got
        else:
            for k in want:
                assert torch.equal(got[k], first[k]), "%s: %s not bit-identical on the second call" % (what, k)
    for k in out:
        if k not in want:
            assert bool(torch.isnan(first[k]).all()), "%s: %s written although not asked for" % (what, k)
    return {k: _np(first[k]) for k in want}


def _check(got, ref, tol, what):
    err = np.abs(got - ref)
    i = int(np.argmax(err / tol))
    print("  %s: max err %.3e (worst %d: err %.3e, allowed %.3e)" % (what, err.max(), i, err.reshape(-1)[i], np.reshape(tol, -1)[i]))
    assert np.all(np.isfinite(got)) and np.all(err <= tol), (what, i, float(err.reshape(-1)[i]), float(np.reshape(tol, -1)[i]))


def _check_elbo(elbo, lp_dev, scale, kls, what):
    want = R.bound(lp_dev, scale, kls)
    kl_abs = sum(float(np.abs(k).sum()) for k in kls)
    tol = R.bound_tol(lp_dev, scale) + sum(np.size(k) for k in kls) * 2.0 ** -52 * kl_abs
    assert abs(elbo - want) <= tol, (what, elbo, want, tol)


# ---- iwvi_bound_logw_reduce ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.FAMILIES)
def test_reduce_every_shape_and_every_member(gpu_device, name):
    n = 0
    for B, K, G in F.shape_cases():
        L = R.family(name, B, K, seed=40)
        for tau, beta in F.TAU_BETA:
            kls = R.global_kls(*GLOBS[n % 3], seed=n)
            what = "%s B=%d K=%d G=%d tau=%g beta=%g %s" % (name, B, K, G, tau, beta, LAYOUTS[n % 2])
            got = _reduce(gpu_device, L, G, tau, beta, LAYOUTS[n % 2], kls, 1.0 + n % 7, what=what)
            _check(got["logp"], F.bound_n(L, G, tau, beta), F.tol_bound(L, G, tau, beta), what + " logp")
            _check(got["ess"], F.ess(L), F.tol_ess(L), what + " ess")
            assert np.all(got["ess"] >= 1.0 - F.tol_ess(L)) and np.all(got["ess"] <= K + F.tol_ess(L)), what
            _check_elbo(float(got["elbo"][0]), got["logp"], 1.0 + n % 7, kls, what)
            n += 1
    if name == "ties_all":                                       # every weight equal: K exactly
        assert np.array_equal(got["ess"], np.full(B, float(K)))


def test_reduce_ess_at_its_two_ends(gpu_device):
    for B, K, G in F.shape_cases():
        got = _reduce(gpu_device, R.family("ties_all", B, K, seed=41), G, 0.5, 0.3, want=("ess",))
        assert np.array_equal(got["ess"], np.full(B, float(K))), (B, K)
        if K > 1:
            got = _reduce(gpu_device, R.family("dominant", B, K, seed=41), G, 0.5, 0.3, want=("ess",))
            assert np.all(np.abs(got["ess"] - 1.0) <= 1e-6), (B, K, float(np.abs(got["ess"] - 1.0).max()))


def test_reduce_each_output_null_in_turn(gpu_device):
    """logp, ess and the bound each left out in turn (out_elbo needs out_logp: the workgroups publish through it); what is asked for does not
    depend on what else is."""
    for B, K, G in ((5, 6, 3), (65, 130, 2)):
        L = R.family("near_equal", B, K, seed=42)
        kls = R.global_kls(2, 3, seed=1)
        full = _reduce(gpu_device, L, G, 0.5, 0.3, kls=kls, scale=2.5)
        for want in (("logp", "ess"), ("logp", "elbo"), ("ess",), ("logp",)):
            got = _reduce(gpu_device, L, G, 0.5, 0.3, kls=kls, scale=2.5, want=want, what="want=%s" % (want,))
            for k in want:
                assert np.array_equal(got[k], full[k]), (want, k)


def test_reduce_without_re_zeroing_the_ticket_between_different_calls(gpu_device):
    """One ticket word through calls of different grids (B = 257: five workgroups; B = 3: one) without a host re-zero in between."""
    a = _abi()
    dev = gpu_device
    ticket = torch.zeros(1, dtype=torch.int64, device=dev)
    for B, K, G in ((257, 6, 3), (3, 130, 2), (257, 130, 65), (65, 65, 5)):
        L = R.family("ties_two", B, K, seed=43)
        lw, logp, elbo = _f(L, dev), torch.empty(B, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
        a.check(a.lib().iwvi_bound_logw_reduce(_desc(G, 1.0, 0.0), a.ptr(lw), B, K, K, 1, None, None, 0, 3.0, a.ptr(logp), None, a.ptr(elbo),
                                               a.ptr(ticket), a.stream_ptr()))
        assert int(ticket.item()) == 0
        _check(_np(logp), F.bound_n(L, G), F.tol_bound(L, G), "B=%d K=%d G=%d" % (B, K, G))
        _check_elbo(float(elbo.item()), _np(logp), 3.0, (), "B=%d K=%d" % (B, K))


def _logw_reduce(dev, L, mode_vi):
    a = _abi()
    B, K = L.shape
    lw, logp = _f(L, dev), torch.empty(B, device=dev)
    a.check(a.lib().iwvi_logw_reduce(a.ptr(lw), B, K, K, 1, None, None, 0, 1.0, 0, 1 if mode_vi else 0, None, a.ptr(logp), None, None, a.stream_ptr()))
    return _np(logp)


@pytest.mark.parametrize("name", F.FAMILIES)
def test_reduce_ends_of_the_family_against_the_existing_reduction(gpu_device, name):
    """(1, 1, 0) against iwvi_logw_reduce, beta = 1 against its mode_vi: each within the sum of the two tolerances."""
    for B, K, G in F.shape_cases():
        L = R.family(name, B, K, seed=44)
        what = "%s B=%d K=%d" % (name, B, K)
        got = _reduce(gpu_device, L, want=("logp",))["logp"]
        _check(got, _logw_reduce(gpu_device, L, False), F.tol_bound(L) + R.tol_reduce(L), what + " iwae")
        got = _reduce(gpu_device, L, G, 0.5, 1.0, want=("logp",))["logp"]
        _check(got, _logw_reduce(gpu_device, L, True), F.tol_bound(L, G, 0.5, 1.0) + R.tol_vi(L), what + " beta=1")


@pytest.mark.parametrize("name", F.FAMILIES)
def test_reduce_orderings(gpu_device, name):
    """beta = 1 <= miwae(G) <= iwae per point and the tempered term monotone in tau, up to the tolerances of the two sides."""
    for B, K, G in F.shape_cases():
        L = R.family(name, B, K, seed=45)
        run = lambda G_, tau, beta: (_reduce(gpu_device, L, G_, tau, beta, want=("logp",))["logp"], F.tol_bound(L, G_, tau, beta))
        what = "%s B=%d K=%d G=%d" % (name, B, K, G)
        (el, t0), (mi, t1), (iw, t2) = run(1, 1.0, 1.0), run(G, 1.0, 0.0), run(1, 1.0, 0.0)
        assert np.all(el <= mi + t0 + t1) and np.all(mi <= iw + t1 + t2), what
        prev, tp = el, t0
        for tau in (0.05, 0.5, 1.0):
            cur, tc = run(G, tau, 0.0)
            assert np.all(prev <= cur + tp + tc), (what, tau)
            prev, tp = cur, tc


def _call_refused(call, outs, what):
    a = _abi()
    for t in outs:
        t.fill_(float("nan"))
    rc = call()
    torch.cuda.synchronize()
    assert rc == a.ERR_ARG, (what, rc)
    assert a.lib().iwvi_last_error(), what
    for t in outs:
        assert bool(torch.isnan(t).all()), "%s: an output was written" % what


def test_reduce_refusals_leave_the_outputs_untouched(gpu_device):
    a, dev = _abi(), gpu_device
    B, K = 5, 6
    lw = _f(R.family("near_equal", B, K, seed=46), dev)
    logp, ess, elbo = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int64, device=dev)
    g, gp, gn = _glob(R.global_kls(1, 2), dev)
    bad_n = (ctypes.c_int32 * 1)(R.MAX_R + 1)

    def call(desc=_desc(3, 0.5, 0.3), lw_=lw, B_=B, K_=K, gp_=gp, gn_=gn, ng=1, logp_=logp, ticket_=ticket):
        return lambda: a.lib().iwvi_bound_logw_reduce(desc, a.ptr(lw_), B_, K_, K_, 1, gp_, gn_, ng, 1.0, a.ptr(logp_), a.ptr(ess), a.ptr(elbo),
                                                      a.ptr(ticket_), a.stream_ptr())

    cases = {"null descriptor": call(desc=None), "groups = 0": call(_desc(0)), "groups = -1": call(_desc(-1)), "K % groups": call(_desc(4)),
             "tau = 0": call(_desc(1, 0.0)), "tau < 0": call(_desc(1, -0.5)), "tau > 1": call(_desc(1, 1.0 + 2.0 ** -20)), "tau NaN": call(_desc(1, float("nan"))),
             "beta < 0": call(_desc(1, 1.0, -2.0 ** -20)), "beta > 1": call(_desc(1, 1.0, 1.5)), "beta NaN": call(_desc(1, 1.0, float("nan"))),
             "null input": call(lw_=None), "B = 0": call(B_=0), "K = 0": call(K_=0), "bound without logp": call(logp_=None),
             "bound without a ticket": call(ticket_=None), "too many global arrays": call(ng=R.MAX_GLOB + 1),
             "null global array": call(gp_=None), "bad global count": call(gn_=bad_n)}
    for what, c in cases.items():
        _call_refused(c, (logp, ess, elbo), what)
    assert int(ticket.item()) == 0
    assert call()() == 0                                         # and the good call goes through
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logp).all()) and bool(torch.isfinite(ess).all()) and bool(torch.isfinite(elbo).all())


# ---- iwvi_bound_elbo_backward ----------------------------------------------------------------------------------------------------------
def _moment_inputs(target, Dy, lik_var, rng):
    """fmean, fvar [B, K, Dy] float32-valued and Y [B, Dy] whose Gaussian expectation sums to about ``target`` [B, K] (<= Dy c0)."""
    B, K = target.shape
    c0 = -0.5 * math.log(2 * math.pi) - 0.5 * math.log(lik_var)
    q = (Dy * c0 - target) / Dy
    assert np.all(q >= 0), "target above the Gaussian's maximum"
    split = rng.uniform(0.2, 0.8, (B, K, Dy))
    Y = R.f32(rng.standard_normal((B, Dy)))
    fvar = R.f32(split * q[..., None] * 2 * lik_var)
    e = np.sqrt((1 - split) * q[..., None] * 2 * lik_var) * rng.choice([-1.0, 1.0], (B, K, Dy))
    return R.f32(Y[:, None, :] - e), fvar, Y


def _heads_inputs(name, B, K, n, rng):
    """The family through the moments (odd n, and ``wide``: a small likelihood variance gives the range) or the regulariser channel."""
    Dy = (1, 3)[n % 2]
    lik_var = F.f32v(1e-3 if name == "wide" else 0.4)
    c0 = -0.5 * math.log(2 * math.pi) - 0.5 * math.log(lik_var)
    L = R.family(name, B, K, seed=51)
    if name == "wide" or n % 2:
        if name != "wide":
            L = L - np.maximum(L.max(1, keepdims=True) - Dy * c0 + 0.5, 0.0)
        fm, fv, Y = _moment_inputs(L, Dy, lik_var, rng)
        kls = []
    else:
        Y = R.f32(rng.standard_normal((B, Dy)))
        fm, fv = np.repeat(Y[:, None, :], K, 1), np.zeros((B, K, Dy))
        kls = R.split_regularisers(Dy * c0 - L, (1, R.MAX_KL)[n % 4 // 2], (1, 3)[n % 3 % 2], seed=n)
    Lref, big, n_add = R.gaussian_logw(fm, fv, Y, lik_var, kls)
    return fm, fv, Y, kls, lik_var, Lref, R.tol_logw(big, n_add)


def _backward(dev, fm, fv, Y, lik_var, kls_local, glob, scale, desc=None, lik_var_dev=None, mode_vi=None, null=()):
    """iwvi_bound_elbo_backward (``desc``), or iwvi_iw_elbo_backward_dev (``mode_vi`` given) on the same inputs."""
    a = _abi()
    B, K, Dy = fm.shape
    tm, tv, tY = _f(fm, dev), _f(fv, dev), _f(Y, dev)
    tk = [_f(k, dev) for k in kls_local]
    kd = (ctypes.c_int32 * max(len(tk), 1))(*[k.shape[-1] for k in kls_local])
    g, gp, gn = _glob(glob, dev)
    w = torch.full((B, K), float("nan"), device=dev)
    dm, dv = torch.full((B, K, Dy), float("nan"), device=dev), torch.full((B, K, Dy), float("nan"), device=dev)
    sums = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.empty(2 * B, dtype=torch.float64, device=dev)
    ts = None if lik_var_dev is None else _f([lik_var_dev], dev)
    outs = [None if nm in null else a.ptr(t) for nm, t in (("w", w), ("d_mean", dm), ("d_var", dv))]
    if mode_vi is None:
        a.check(a.lib().iwvi_bound_elbo_backward(desc, a.ptr(tm), a.ptr(tv), a.ptr(tY), Dy, a.ptr_array(tk), kd, len(tk), B, K, lik_var, a.ptr(ts), scale,
                                                 *outs, gp, gn, len(g), a.ptr(sums), a.ptr(ws), a.stream_ptr()))
    else:
        a.check(a.lib().iwvi_iw_elbo_backward_dev(a.ptr(tm), a.ptr(tv), a.ptr(tY), Dy, a.ptr_array(tk), kd, len(tk), B, K, lik_var, a.ptr(ts), scale,
                                                  1 if mode_vi else 0, *outs, gp, gn, len(g), None, K, a.ptr(sums), a.ptr(ws), a.stream_ptr()))
    return w, dm, dv, sums


def _head_tols(Lref, tol_L, fm, fv, Y, lik_var, scale, G, tau, beta):
    """Reference heads and their tolerances: w under the family's weight rule; d_mean, d_var: the same relative error plus four float32
    roundings; the likelihood-variance sum: the weights' errors through its terms (as tests/test_gpu_iw_reduction.py)."""
    wr, dmr, dvr, dlr = F.heads(Lref, fm, fv, Y, lik_var, scale, G, tau, beta)
    tw = F.tol_w(wr, scale, Lref, tau, tol_L)
    rel = tw / np.maximum(wr, 1e-300)
    td = [np.abs(r_) * (rel[..., None] + 4 * 2.0 ** -23) + 1e-30 * np.abs(r_ / np.maximum(wr[..., None], 1e-300)) for r_ in (dmr, dvr)]
    e = Y[:, None, :] - fm
    term = np.abs(-0.5 / lik_var + 0.5 * (e * e + fv) / lik_var ** 2)
    tol_dl = float(((tw[..., None] + 2.0 ** -23 * wr[..., None]) * term).sum()) + 1e-300
    return (wr, dmr, dvr, dlr), (tw, td[0], td[1], tol_dl)


@pytest.mark.parametrize("name", F.FAMILIES)
def test_heads_every_shape_and_every_member(gpu_device, name):
    rng = np.random.default_rng(50)
    n = 0
    for B, K, G in F.shape_cases():
        for tau, beta in F.TAU_BETA if B == 5 else F.TAU_BETA[2::3]:
            fm, fv, Y, kls, lik_var, Lref, tol_L = _heads_inputs(name, B, K, n, rng)
            glob = R.global_kls((0, 1, R.MAX_GLOB_BWD)[n % 3], (1, R.MAX_R)[n % 2], seed=n)
            scale = 1.5 + n % 5
            dev_var = lik_var if n % 2 == 0 else None             # the device scalar wins over the host argument
            host_var = lik_var if dev_var is None else F.f32v(3.0 * lik_var)
            what = "%s B=%d K=%d G=%d tau=%g beta=%g Dy=%d n_kl=%d" % (name, B, K, G, tau, beta, fm.shape[2], len(kls))
            n += 1
            first = None
            for _ in range(2):
                got = _backward(gpu_device, fm, fv, Y, host_var, kls, glob, scale, _desc(G, tau, beta), lik_var_dev=dev_var)
                if first is None:
                    first = got
                else:
                    assert all(torch.equal(x, y) for x, y in zip(got, first)), what + ": not bit-identical on the second call"
            w, dm, dv, sums = (_np(t) for t in first)
            (wr, dmr, dvr, dlr), (tw, tdm, tdv, tol_dl) = _head_tols(Lref, tol_L, fm, fv, Y, lik_var, scale, G, tau, beta)
            _check(w, wr, tw, what + " w")
            assert np.all(np.abs(w.sum(1) - scale) <= K * 2.0 ** -23 * scale), (what, float(np.abs(w.sum(1) - scale).max()))
            _check(dm, dmr, tdm + 1e-300, what + " d_mean")
            _check(dv, dvr, tdv + 1e-300, what + " d_var")
            assert abs(sums[1] - dlr) <= tol_dl, (what, sums[1], dlr, tol_dl)
            lpr = F.bound_n(Lref, G, tau, beta)
            assert abs(sums[0] - lpr.sum()) <= float(np.sum(tol_L + F.tol_bound(Lref, G, tau, beta))), (what, sums[0], lpr.sum())
            want = scale * sums[0] - math.fsum(v for k in glob for v in k)
            assert abs(sums[2] - want) <= 4 * 2.0 ** -52 * (abs(scale * sums[0]) + sum(float(np.abs(k).sum()) for k in glob)), (what, sums[2], want)


@pytest.mark.parametrize("name", F.FAMILIES)
def test_heads_ends_of_the_family_against_the_existing_heads(gpu_device, name):
    """(1, 1, 0) against iwvi_iw_elbo_backward_dev, beta = 1 against its mode_vi: every output within the sum of the two tolerances."""
    rng = np.random.default_rng(52)
    for n, (B, K, G) in enumerate(F.shape_cases()):
        fm, fv, Y, kls, lik_var, Lref, tol_L = _heads_inputs(name, B, K, n, rng)
        glob = R.global_kls(n % 3, 2, seed=n)
        for (G_, tau, beta), mode_vi in (((1, 1.0, 0.0), False), ((G, 0.5, 1.0), True)):
            what = "%s B=%d K=%d %s" % (name, B, K, "beta=1" if mode_vi else "iwae")
            new = [_np(t) for t in _backward(gpu_device, fm, fv, Y, lik_var, kls, glob, 2.5, _desc(G_, tau, beta))]
            old = [_np(t) for t in _backward(gpu_device, fm, fv, Y, lik_var, kls, glob, 2.5, mode_vi=mode_vi)]
            (wr, _, _, _), (tw, tdm, tdv, tol_dl) = _head_tols(Lref, tol_L, fm, fv, Y, lik_var, 2.5, G_, tau, beta)
            tw_old = np.full_like(wr, 2.0 ** -23 * 2.5 / K) if mode_vi else R.tol_w(wr, 2.5, tol_L)
            rel_old = tw_old / np.maximum(wr, 1e-300)
            _check(new[0], old[0], tw + tw_old, what + " w")
            for i, td in ((1, tdm), (2, tdv)):
                _check(new[i], old[i], td + np.abs(old[i]) * (rel_old[..., None] + 4 * 2.0 ** -23) + 1e-300, what + (" d_mean", " d_var")[i - 1])
            assert abs(new[3][1] - old[3][1]) <= 2 * tol_dl, (what, new[3][1], old[3][1])
            tol0 = float(np.sum(2 * tol_L + F.tol_bound(Lref, G_, tau, beta) + (R.tol_vi(Lref) if mode_vi else R.tol_reduce(Lref))))
            assert abs(new[3][0] - old[3][0]) <= tol0, (what, new[3][0], old[3][0], tol0)


def test_heads_each_optional_output_null_in_turn(gpu_device):
    rng = np.random.default_rng(53)
    fm, fv, Y, kls, lik_var, _, _ = _heads_inputs("near_equal", 5, 130, 1, rng)
    full = _backward(gpu_device, fm, fv, Y, lik_var, kls, (), 2.0, _desc(2, 0.5, 0.3))
    for null in ("w", "d_mean", "d_var"):
        got = _backward(gpu_device, fm, fv, Y, lik_var, kls, (), 2.0, _desc(2, 0.5, 0.3), null=(null,))
        for nm, x, y in zip(("w", "d_mean", "d_var", "sums"), got, full):
            if nm == null:
                assert bool(torch.isnan(x).all()), null
            else:
                assert torch.equal(x, y), (null, nm)


def test_heads_refusals_leave_the_outputs_untouched(gpu_device):
    a, dev = _abi(), gpu_device
    B, K, Dy = 5, 6, 2
    rng = np.random.default_rng(54)
    tm, tv, tY = (_f(rng.standard_normal(s), dev) for s in ((B, K, Dy), (B, K, Dy), (B, Dy)))
    tv = tv.abs()
    kl = _f(rng.uniform(0, 1, (B, K, 2)), dev)
    w, dm, dv = torch.empty(B, K, device=dev), torch.empty(B, K, Dy, device=dev), torch.empty(B, K, Dy, device=dev)
    sums, ws = torch.empty(3, dtype=torch.float64, device=dev), torch.empty(2 * B, dtype=torch.float64, device=dev)
    g, gp, gn = _glob(R.global_kls(1, 2), dev)
    klp, kld = a.ptr_array([kl]), (ctypes.c_int32 * 1)(2)
    bad_kld, bad_gn = (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(0)

    def call(desc=_desc(3, 0.5, 0.3), fm_=tm, Dy_=Dy, klp_=klp, kld_=kld, nl=1, B_=B, K_=K, var=0.4, gp_=gp, gn_=gn, ng=1, sums_=sums, ws_=ws):
        return lambda: a.lib().iwvi_bound_elbo_backward(desc, a.ptr(fm_), a.ptr(tv), a.ptr(tY), Dy_, klp_, kld_, nl, B_, K_, var, None, 1.0,
                                                        a.ptr(w), a.ptr(dm), a.ptr(dv), gp_, gn_, ng, a.ptr(sums_), a.ptr(ws_), a.stream_ptr())

    cases = {"null descriptor": call(desc=None), "groups = 0": call(_desc(0)), "K % groups": call(_desc(4)), "tau = 0": call(_desc(1, 0.0)),
             "tau > 1": call(_desc(1, 1.5)), "tau NaN": call(_desc(1, float("nan"))), "beta < 0": call(_desc(1, 1.0, -0.5)),
             "beta > 1": call(_desc(1, 1.0, 1.0 + 2.0 ** -20)), "beta NaN": call(_desc(1, 1.0, float("nan"))),
             "null input": call(fm_=None), "Dy = 0": call(Dy_=0), "B = 0": call(B_=0), "K = 0": call(K_=0), "variance = 0": call(var=0.0),
             "too many regularisers": call(nl=R.MAX_KL + 1), "null regulariser": call(klp_=None), "bad regulariser width": call(kld_=bad_kld),
             "too many global arrays": call(ng=R.MAX_GLOB_BWD + 1), "null global array": call(gp_=None), "bad global count": call(gn_=bad_gn),
             "no sums": call(sums_=None), "no workspace": call(ws_=None)}
    for what, c in cases.items():
        _call_refused(c, (w, dm, dv) + (() if what == "no sums" else (sums,)), what)
    assert call()() == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (w, dm, dv, sums))
