"""k_sghmc_step / k_neg_log_prior (csrc/sghmc.hip) alone, against the float64 restatement of tests/sghmc_reference.py.

One call updates tensors of 1, 3, 4, 5, 255, 256, 257 and 1027 elements together: the four-per-counter tail of the Philox layout, the
edges of a 256-thread block (1027 elements = 257 groups of four: a second block) and the per-tensor counter offsets.

The bound on the float64 state.  Each updated quantity is a sum of terms, each term a short chain of float64 operations; an evaluation
with n roundings along its longest chain (the additions included) is within n 2^-53 sum|terms| of the exact value:
  p'     = p - eps^2 Minv grad - mdecay p + sigma n
           Minv: g2 + 1e-16, sqrt, + 1e-16, 1 / x (4); eps^2 (1), eps^2 Minv (1), .. grad (1)                        -> 7 for the second term
           sigma: eps / sqrt(N) (2), squared (1), 2 .. mdecay (1), .. Minv (4 + 1), sqrt (1), .. n (1)               -> 11 for the fourth
           three additions (3)                                                                                       -> N_OPS p = 14
  theta' = theta + p'                                                                                                -> 15
  g'     = (1 - r) g + r grad:  r: xi + 1, 1 / x (2); 1 - r (1); product (1); sum (1)                                -> 5
  g2'    = (1 - r) g2 + r grad^2: as g' and grad^2 (1)                                                               -> 6
  xi'    = 1 + xi (1 - g^2 / (g2 + 1e-16)): g^2, g2 + 1e-16, quotient, 1 - x, xi .., 1 + x                            -> 6
(the terms of xi' are 1, xi and xi g^2 / g2: the error of the quotient enters through the last one).  theta (float32) must be the
float32 rounding of the restatement's theta' or its neighbour.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sghmc_reference as sr   # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 255, 256, 257, 1027)
N_OPS = dict(p=14, theta=15, g=5, g2=6, xi=6)
PAD, SENTINEL = 8, 777.25
EPSILON, MDECAY, NUM_DATA = 0.01, 0.05, 1234.0
KEYS64 = ("xi", "g", "g2", "p", "theta")


def _grads(rng, n, step):
    """d bound / d theta: mixed sign, exact zeros, 1e-6 and 1e+6 among them."""
    g = rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)
    special = np.array([0.0, 1e-6, -1e6, 1e6, -1e-6, 0.0])
    idx = rng.permutation(n)[:min(n, special.size)]
    g[idx] = special[(np.arange(idx.size) + step) % special.size]
    return g.astype(np.float32)


class _Bank:
    """Device buffers of the SIZES tensors, each PAD elements longer than its tensor (the tail holds SENTINEL)."""

    def __init__(self, dev, rng):
        self.dev = dev
        f32 = lambda n: torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device=dev)
        f64 = lambda n: torch.full((n + PAD,), SENTINEL, dtype=torch.float64, device=dev)
        self.theta32, self.grad, self.noise, self.noise_out = ([f32(n) for n in SIZES] for _ in range(4))
        self.s = {k: [f64(n) for n in SIZES] for k in KEYS64}    # "theta" here: the float64 master
        for i, n in enumerate(SIZES):
            th = rng.standard_normal(n).astype(np.float32)
            st = sr.init_state(th)
            self.theta32[i][:n] = torch.as_tensor(th, device=dev)
            for k in KEYS64:
                self.s[k][i][:n] = torch.as_tensor(st[k], device=dev)

    def launch(self, burn_in, inject, rng_state=None, seed=0, want_noise_out=False):
        from dgps_with_iwvi_amd import _abi
        arr = (_abi.SghmcTensor * len(SIZES))()
        for i, n in enumerate(SIZES):
            a = arr[i]
            a.theta, a.grad, a.n = self.theta32[i].data_ptr(), self.grad[i].data_ptr(), n
            a.xi, a.g, a.g2, a.p, a.theta64 = (self.s[k][i].data_ptr() for k in KEYS64)
            a.noise = self.noise[i].data_ptr() if inject else None
            a.noise_out = self.noise_out[i].data_ptr() if want_noise_out else None
        _abi.check(_abi.lib().iwvi_sghmc_step(arr, len(SIZES), EPSILON, MDECAY, NUM_DATA, 1 if burn_in else 0, seed,
                                              None if rng_state is None else rng_state.data_ptr(), _abi.stream_ptr()))
        torch.cuda.synchronize()

    def read(self, i):
        n = SIZES[i]
        return {k: self.s[k][i][:n].cpu().numpy() for k in KEYS64}

    def check_padding(self):
        for i, n in enumerate(SIZES):
            for t in [self.theta32[i], self.noise_out[i]] + [self.s[k][i] for k in KEYS64]:
                assert bool((t[n:] == SENTINEL).all()), "a write past the end of tensor %d" % i


def _assert_step(bank, i, before, grad, noise, burn_in):
    want, mag = sr.step(before, grad, noise, EPSILON, MDECAY, NUM_DATA, burn_in)
    got = bank.read(i)
    n = SIZES[i]
    for k in KEYS64:
        if not burn_in and k in ("xi", "g", "g2"):
            assert (got[k] == before[k]).all(), "the sample op wrote %s" % k
            continue
        err = np.abs(got[k] - want[k])
        tol = N_OPS[k] * sr.U64 * mag[k]
        worst = float((err / tol).max())
        print("tensor n=%d burn_in=%d %s: worst |device - restatement| = %.3g, %.3g of the bound" % (n, burn_in, k, float(err.max()), worst))
        assert (err <= tol).all(), (n, k, worst)
    th32 = bank.theta32[i][:n].cpu().numpy()
    r = want["theta"].astype(np.float32)
    ok = (th32 == r) | (th32 == np.nextafter(r, np.float32(np.inf))) | (th32 == np.nextafter(r, np.float32(-np.inf)))
    assert ok.all(), "theta is not the float32 rounding of theta' (or its neighbour), tensor n=%d" % n
    assert (th32 == got["theta"].astype(np.float32)).all(), "theta is not the float32 rounding of its own master"


@pytest.mark.parametrize("burn_in", [True, False])
def test_injected_noise_five_steps(gpu_device, burn_in):
    rng = np.random.default_rng(11 + burn_in)
    bank = _Bank(gpu_device, rng)
    if not burn_in:                                              # a sample op on a state that two burn-in steps have moved off (1, 1, 1, 0)
        for step in range(2):
            for i, n in enumerate(SIZES):
                bank.grad[i][:n] = torch.as_tensor(_grads(rng, n, step), device=gpu_device)
                bank.noise[i][:n] = torch.as_tensor(rng.standard_normal(n).astype(np.float32), device=gpu_device)
            bank.launch(True, inject=True)
    for step in range(5):
        before, grads, noises = [], [], []
        for i, n in enumerate(SIZES):
            g, z = _grads(rng, n, step), rng.standard_normal(n).astype(np.float32)
            bank.grad[i][:n] = torch.as_tensor(g, device=gpu_device)
            bank.noise[i][:n] = torch.as_tensor(z, device=gpu_device)
            before.append(bank.read(i))                          # the device's own state: errors do not compound
            grads.append(g)
            noises.append(z)
        bank.launch(burn_in, inject=True)
        for i in range(len(SIZES)):
            _assert_step(bank, i, before[i], grads[i], noises[i], burn_in)
    bank.check_padding()


def _fill_normal(dev, n, seed, offset):
    from dgps_with_iwvi_amd import _abi
    out = torch.empty(n, dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().iwvi_fill_normal(_abi.ptr(out), n, seed, offset, _abi.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_in_kernel_noise_is_the_documented_stream(gpu_device):
    """noise_out of tensor i = iwvi_fill_normal(n_i, seed, c + sum_{j < i} ceil(n_j / 4)) bit for bit; the update used exactly that noise;
    the launch advances the counter by sum_j ceil(n_j / 4), so the next launch continues the stream."""
    rng = np.random.default_rng(5)
    bank = _Bank(gpu_device, rng)
    seed, c0 = 0x1234567887654321, 1000
    state = torch.tensor([c0, 0], dtype=torch.int64, device=gpu_device)
    total = sum((n + 3) // 4 for n in SIZES)
    for launch in range(2):
        before, grads = [], []
        for i, n in enumerate(SIZES):
            g = _grads(rng, n, launch)
            bank.grad[i][:n] = torch.as_tensor(g, device=gpu_device)
            before.append(bank.read(i))
            grads.append(g)
        bank.launch(launch == 0, inject=False, rng_state=state, seed=seed, want_noise_out=True)
        off = c0 + launch * total
        for i, n in enumerate(SIZES):
            drawn = bank.noise_out[i][:n].cpu().numpy()
            want = _fill_normal(gpu_device, n, seed, off)
            assert (drawn.view(np.uint32) == want.view(np.uint32)).all(), "tensor %d of launch %d is not the stream at offset %d" % (i, launch, off)
            _assert_step(bank, i, before[i], grads[i], drawn, launch == 0)
            off += (n + 3) // 4
        assert state.cpu().tolist() == [c0 + (launch + 1) * total, 0]
    bank.check_padding()


@pytest.mark.parametrize("M,R", [(3, 2), (33, 5), (512, 32)])
def test_neg_log_prior(gpu_device, M, R):
    """1/2 |q_mu|^2 + 1/2 M R log 2 pi: M R + 2 float64 roundings of non-negative terms (any summation order) -> (M R + 2) 2^-53 relative."""
    from dgps_with_iwvi_amd.temp_workaround import neg_log_prior
    q = np.random.default_rng(M).standard_normal((M, R)).astype(np.float32) * 3
    got = float(neg_log_prior(torch.as_tensor(q, device=gpu_device)).item())
    want = sr.neg_log_prior(q)
    assert abs(got - want) <= (M * R + 2) * sr.U64 * want
