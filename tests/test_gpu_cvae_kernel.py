"""The CVAE kernels (csrc/cvae.hip) through the C-ABI, against the float64 restatement of tests/cvae_restatement.py.

Shapes (hidden widths; Dx, Dy, L; B): the smallest that reach one row, a ragged last tile of eight rows, several workgroups, widths that are
no multiple of 16 and differ between layers, every cap (4 maps, width 128, L = Dy = 8) and L, Dy > 1.  Tolerances: the bound and its two parts
within 1e-5 (|sum log p| + |sum KL|); every gradient tensor max |got - ref| <= 1e-4 max |ref|; sampler outputs 1e-5 in the same max-norm
form.  tests/test_cvae_host.py shows the float32 restatement of the same inputs within a tenth of each.

The sampler's statistical bounds are derived, not tuned: for y = w_z z + w_x . x + b + sqrt(var) eps' with S = 16384 draws per point, the
sample mean is within 5 sigma / sqrt(S), the sample variance within 5 sigma^2 sqrt(2 / (S - 1)), the sample correlation of the z part and
the eps' part within 5 / sqrt(S)."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvae_restatement as cr   # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 8
DEV = "cuda:0"
CASE_IDS = ["%s-%d-%d-%d-B%d" % ("_".join(map(str, s[0])) or "lin", *s[1:]) for s in cr.KERNEL_CASES]


def _padded(shape, dtype=torch.float32):
    """(view of `shape` inside a NaN-filled buffer PAD elements longer at each end, the buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=DEV)
    return buf[PAD:PAD + n].view(*shape), buf


def _margins_are_nan(buf):
    return bool(torch.isnan(buf[:PAD]).all() and torch.isnan(buf[-PAD:]).all())


class Net:
    """A case of cvae_restatement.make_case on the device, with its descriptor."""

    def __init__(self, case, act=0, tensors=None):
        from dgps_with_iwvi_amd import _abi
        self._abi, self.case = _abi, case
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=DEV).contiguous()
        if tensors is None:
            tensors = ([t(a) for a in case[k]] for k in ("Ws", "bs", "Ws_dec", "bs_dec"))
        self.Ws, self.bs, self.Ws_dec, self.bs_dec = tensors
        self.n = len(self.Ws)
        self.enc_dims, self.dec_dims = cr.widths(case["hidden"], case["Dx"], case["Dy"], case["L"])
        self.keep = [_abi.ptr_array(self.Ws), _abi.ptr_array(self.bs), _abi.ptr_array(self.Ws_dec), _abi.ptr_array(self.bs_dec),
                     (ctypes.c_int32 * (self.n + 1))(*self.enc_dims), (ctypes.c_int32 * (self.n + 1))(*self.dec_dims)]
        d = self.d = _abi.CvaeDesc()
        d.enc_W, d.enc_b, d.dec_W, d.dec_b, d.enc_dims, d.dec_dims = self.keep
        d.n_maps, d.Dx, d.Dy, d.L, d.act, d.variance = self.n, case["Dx"], case["Dy"], case["L"], act, float(case["variance"])

    @classmethod
    def of_model(cls, model):
        """The descriptor over a cvae.CVAE's OWN tensors (its variance as the device scalar)."""
        case = {"hidden": model.layers_widths, "Dx": model.X_dim, "Dy": model.Y_dim, "L": model.latent_dim, "variance": np.float32(0.05)}
        net = cls(case, model.activation, (model.Ws, model.bs, model.Ws_dec, model.bs_dec))
        net.d.variance_dev = model.variance_dev.data_ptr()
        return net

    def workspace(self, B):
        nbytes = self._abi.lib().iwvi_cvae_ws_bytes(ctypes.byref(self.d), B)
        assert nbytes > 0 and nbytes % 4 == 0
        return torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)    # the entries need no initial contents

    def train(self, X, Y, eps=None, grad=True, seed=0, rng_state=None, want_eps_out=False):
        """-> dict: out [3] float64, the gradients (grad=True), eps_out; every output sits inside a NaN-filled buffer whose margins are checked."""
        _abi, lib = self._abi, self._abi.lib()
        B, L = X.shape[0], self.case["L"]
        ws = self.workspace(B)
        out, out_buf = _padded((3,), torch.float64)
        bufs = [out_buf]
        res = {}
        eps_out = None
        if want_eps_out:
            eps_out, b = _padded((B, L))
            bufs.append(b)
        args = [ctypes.byref(self.d), _abi.ptr(X), _abi.ptr(Y), B, _abi.ptr(eps), seed, _abi.ptr(rng_state), _abi.ptr(eps_out), _abi.ptr(out)]
        if grad:
            g = {}
            for tag, Ws, bs in (("enc", self.Ws, self.bs), ("dec", self.Ws_dec, self.bs_dec)):
                for kind, ps in (("W", Ws), ("b", bs)):
                    pairs = [_padded(tuple(p.shape)) for p in ps]
                    g[tag + "_d" + kind] = [v for v, _ in pairs]
                    bufs += [b for _, b in pairs]
            dvar, b = _padded((1,), torch.float64)
            bufs.append(b)
            gd = _abi.CvaeGrads()
            keep = [_abi.ptr_array(g[k]) for k in ("enc_dW", "enc_db", "dec_dW", "dec_db")]
            gd.enc_dW, gd.enc_db, gd.dec_dW, gd.dec_db = keep
            gd.dvariance = dvar.data_ptr()
            _abi.check(lib.iwvi_cvae_elbo_and_grad(*args, ctypes.byref(gd), _abi.ptr(ws), None))
            torch.cuda.synchronize()
            res.update({k: [v.cpu().numpy().copy() for v in vs] for k, vs in g.items()})
            res["dvariance"] = float(dvar.cpu()[0])
        else:
            _abi.check(lib.iwvi_cvae_elbo(*args, _abi.ptr(ws), None))
            torch.cuda.synchronize()
        res["out"] = out.cpu().numpy().copy()
        res["eps_out"] = None if eps_out is None else eps_out.cpu().numpy().copy()
        res["margins_ok"] = all(_margins_are_nan(b) for b in bufs)
        return res

    def sample(self, Xs, S, z=None, zy=None, flags=0, seed=0, rng_state=None):
        _abi = self._abi
        N = Xs.shape[0]
        out, buf = _padded((N, S, self.case["Dy"]))
        _abi.check(_abi.lib().iwvi_cvae_predict_samples(ctypes.byref(self.d), _abi.ptr(Xs), N, S, _abi.ptr(z), _abi.ptr(zy), flags, seed,
                                                        _abi.ptr(rng_state), _abi.ptr(out), None))
        torch.cuda.synchronize()
        assert _margins_are_nan(buf)
        return out.cpu().numpy().copy()


def _dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=DEV).contiguous()


@functools.lru_cache(maxsize=None)
def _runs(i):
    """Case i once: the float64 restatement, two gradient calls and one value call on the same inputs."""
    case = cr.make_case(*cr.KERNEL_CASES[i])
    net = Net(case)
    X, Y, eps = _dev(case["X"]), _dev(case["Y"]), _dev(case["eps"])
    return cr.value_and_grads(case), net.train(X, Y, eps), net.train(X, Y, eps), net.train(X, Y, eps, grad=False)


def _check_against(ref, got, what):
    scale = abs(ref["logp"]) + abs(ref["kl"])
    for j, k in enumerate(("elbo", "logp", "kl")):
        err = abs(got["out"][j] - ref[k]) / scale
        print("%s %s: %.3g of |log p| + |KL|" % (what, k, err))
        assert err <= cr.BOUND_RTOL, (what, k, got["out"][j], ref[k], err)
    for kg, kr in (("enc_dW", "dWs"), ("enc_db", "dbs"), ("dec_dW", "dWs_dec"), ("dec_db", "dbs_dec")):
        for l, (a, b) in enumerate(zip(got[kg], ref[kr])):
            err = cr.max_norm_err(a, b)
            print("%s %s[%d]: %.3g of max |ref|" % (what, kg, l, err))
            assert np.isfinite(a).all() and err <= cr.GRAD_RTOL, (what, kg, l, err)
    err = abs(got["dvariance"] - ref["dvariance"]) / abs(ref["dvariance"])
    print("%s dvariance: %.3g" % (what, err))
    assert err <= cr.GRAD_RTOL, (what, got["dvariance"], ref["dvariance"])


@pytest.mark.parametrize("i", range(len(cr.KERNEL_CASES)), ids=CASE_IDS)
def test_bound_and_gradients_against_float64(i):
    ref, g1, _, _ = _runs(i)
    _check_against(ref, g1, CASE_IDS[i])


@pytest.mark.parametrize("i", range(len(cr.KERNEL_CASES)), ids=CASE_IDS)
def test_value_entry_matches_the_gradient_entry_bit_for_bit(i):
    _, g1, _, v = _runs(i)
    assert v["out"].tobytes() == g1["out"].tobytes(), (v["out"], g1["out"])


@pytest.mark.parametrize("i", range(len(cr.KERNEL_CASES)), ids=CASE_IDS)
def test_two_calls_are_bit_identical(i):
    _, g1, g2, _ = _runs(i)
    assert g1["out"].tobytes() == g2["out"].tobytes() and g1["dvariance"] == g2["dvariance"]
    for k in ("enc_dW", "enc_db", "dec_dW", "dec_db"):
        for a, b in zip(g1[k], g2[k]):
            assert a.tobytes() == b.tobytes(), k


@pytest.mark.parametrize("i", range(len(cr.KERNEL_CASES)), ids=CASE_IDS)
def test_outputs_stay_inside_their_buffers(i):
    """Every output was allocated inside a larger NaN-filled tensor and the workspace was NaN-filled before the call."""
    _, g1, g2, v = _runs(i)
    assert g1["margins_ok"] and g2["margins_ok"] and v["margins_ok"]
    assert np.isfinite(g1["out"]).all() and all(np.isfinite(a).all() for k in ("enc_dW", "enc_db", "dec_dW", "dec_db") for a in g1[k])


def test_clip_in_both_directions():
    case = cr.make_case(*cr.CLIP_CASE, clip=True)
    ref = cr.value_and_grads(case)
    L = case["L"]
    below, above = (ref["raw"] < cr.CLIP_LO).any(1), (ref["raw"] > cr.CLIP_HI).any(1)
    assert below.sum() >= 2 and above.sum() >= 1
    net = Net(case)
    X, Y, eps = _dev(case["X"]), _dev(case["Y"]), _dev(case["eps"])
    got = net.train(X, Y, eps)
    assert got["margins_ok"] and np.isfinite(got["out"]).all() and math.isfinite(got["dvariance"])
    _check_against(ref, got, "clip")
    # the raw columns of the last encoder map: the restatement's, and no contribution from the clipped rows -- the same call on the
    # unclipped rows alone gives the same columns (another order of the same sum)
    keep = ~(below | above)
    sub = net.train(_dev(case["X"][keep]), _dev(case["Y"][keep]), _dev(case["eps"][keep]))
    for k, cols in (("enc_dW", lambda a: a[:, L:]), ("enc_db", lambda a: a[L:])):
        full, part, r = cols(got[k][-1]), cols(sub[k][-1]), cols(ref["dWs" if k == "enc_dW" else "dbs"][-1])
        assert cr.max_norm_err(full, r) <= cr.GRAD_RTOL
        assert cr.max_norm_err(part, full) <= cr.GRAD_RTOL, (k, cr.max_norm_err(part, full))


def test_variance_dev_overrides_the_value_field():
    case = cr.make_case([7], 5, 1, 1, 37, seed=3)
    X, Y, eps = _dev(case["X"]), _dev(case["Y"]), _dev(case["eps"])
    plain = Net(case).train(X, Y, eps)
    over = Net(dict(case, variance=np.float32(3.0)))
    var_dev = torch.full((1,), float(case["variance"]), dtype=torch.float32, device=DEV)
    over.d.variance_dev = var_dev.data_ptr()
    got = over.train(X, Y, eps)
    assert got["out"].tobytes() == plain["out"].tobytes() and got["dvariance"] == plain["dvariance"]
    other = Net(dict(case, variance=np.float32(3.0))).train(X, Y, eps)
    assert other["out"][1] != plain["out"][1]


def _fill_normal(n, seed, offset):
    from dgps_with_iwvi_amd import _abi
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    _abi.check(_abi.lib().iwvi_fill_normal(_abi.ptr(out), n, seed, offset, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "value"])
@pytest.mark.parametrize("shape", [([], 5, 1, 1, 37), ([33, 17], 5, 3, 3, 130)], ids=["L1-B37", "L3-B130"])
def test_device_noise_follows_fill_normal_and_advances_the_counter(shape, grad):
    case = cr.make_case(*shape)
    net = Net(case)
    X, Y = _dev(case["X"]), _dev(case["Y"])
    B, L = shape[4], shape[3]
    seed, c0 = 0x1234ABCD5678, 5
    nq = (B * L + 3) // 4
    state = torch.tensor([c0, 0], dtype=torch.int64, device=DEV)
    first = net.train(X, Y, None, grad=grad, seed=seed, rng_state=state, want_eps_out=True)
    assert first["margins_ok"]
    np.testing.assert_array_equal(first["eps_out"].reshape(-1), _fill_normal(B * L, seed, c0))
    assert state.cpu().tolist() == [c0 + nq, 0]
    second = net.train(X, Y, None, grad=grad, seed=seed, rng_state=state, want_eps_out=True)
    np.testing.assert_array_equal(second["eps_out"].reshape(-1), _fill_normal(B * L, seed, c0 + nq))
    assert state.cpu().tolist() == [c0 + 2 * nq, 0]
    # the drawn noise is what the bound was evaluated with
    again = net.train(X, Y, _dev(first["eps_out"]), grad=grad)
    assert again["out"].tobytes() == first["out"].tobytes()


@pytest.mark.parametrize("net_shape", cr.SAMPLER_NETS, ids=lambda s: "_".join(map(str, s[0])) or "lin")
def test_sampler_with_injected_noise(net_shape):
    for N, S in cr.SAMPLER_SHAPES:
        case, Xs, z, zy = cr.sampler_inputs(*net_shape, N, S)
        net = Net(case)
        got = net.sample(_dev(Xs), S, _dev(z.reshape(N * S, -1)), _dev(zy.reshape(N * S, -1)))
        ref = cr.samples(case, Xs, z, zy)                             # [N, S, Dy]: the layout
        assert got.shape == ref.shape == (N, S, net_shape[2])
        err = cr.max_norm_err(got, ref)
        print("sampler %s N=%d S=%d: %.3g" % (net_shape, N, S, err))
        assert err <= cr.SAMPLE_RTOL, (net_shape, N, S, err)
        quiet = net.sample(_dev(Xs), S, _dev(z.reshape(N * S, -1)), None, flags=1)    # no z_y, no counter: the decoder's output alone
        assert cr.max_norm_err(quiet, cr.samples(case, Xs, z, zy, y_noise=False)) <= cr.SAMPLE_RTOL


def test_sampler_with_device_noise_on_the_linear_model():
    N, S, Dx = 4, 16384, 5
    case, Xs, _, _ = cr.sampler_inputs([], Dx, 1, 1, N, 1, seed=7)
    net = Net(case)
    seed, c0 = 99, 1000
    nqz, nqy = (N * S + 3) // 4, (N * S + 3) // 4
    state = torch.tensor([c0, 0], dtype=torch.int64, device=DEV)
    noisy = net.sample(_dev(Xs), S, flags=0, seed=seed, rng_state=state)[:, :, 0].astype(np.float64)
    assert state.cpu().tolist() == [c0 + nqz + nqy, 0]
    state[0] = c0
    quiet = net.sample(_dev(Xs), S, flags=1, seed=seed, rng_state=state)[:, :, 0].astype(np.float64)
    W, b, var = case["Ws_dec"][0].astype(np.float64), case["bs_dec"][0].astype(np.float64), float(case["variance"])
    w_z, w_x = W[0, 0], W[1:, 0]
    mean = Xs.astype(np.float64) @ w_x + b[0]                        # [N]
    sigma2 = w_z * w_z + var
    # the z stream is the documented one: quiet = mean + w_z z with z = iwvi_fill_normal(., N S, seed, c0)
    zs = _fill_normal(N * S, seed, c0).astype(np.float64).reshape(N, S)
    assert np.abs(quiet - (mean[:, None] + w_z * zs)).max() <= 1e-5 * np.abs(quiet).max()
    ey = _fill_normal(N * S, seed, c0 + nqz).astype(np.float64).reshape(N, S)
    assert np.abs((noisy - quiet) - math.sqrt(var) * ey).max() <= 1e-5 * np.abs(noisy).max()
    for n in range(N):
        assert abs(noisy[n].mean() - mean[n]) <= 5.0 * math.sqrt(sigma2 / S), (n, noisy[n].mean(), mean[n])
        assert abs(noisy[n].var(ddof=1) - sigma2) <= 5.0 * sigma2 * math.sqrt(2.0 / (S - 1)), (n, noisy[n].var(ddof=1), sigma2)
        z_part, e_part = quiet[n] - mean[n], noisy[n] - quiet[n]
        assert abs(np.corrcoef(z_part, e_part)[0, 1]) <= 5.0 / math.sqrt(S), n
