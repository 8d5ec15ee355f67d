"""The stand-alone noise generator of the C-ABI, called directly: ``iwvi_fill_normal`` against the NumPy restatement of its documented
stream (tests/philox_reference.py: Philox4x32-10, counter (offset + i / 4, 0, 0, 0), key = seed, Box-Muller on word pairs (0, 1) and
(2, 3)), and ``iwvi_fill_normal_dev`` -- the same stream with the counter on the device -- bit for bit against ``iwvi_fill_normal`` at the
offsets its counter must have reached."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_reference as pr   # noqa: E402

pytestmark = pytest.mark.gpu

STREAM_ATOL = 1e-4     # tells streams apart (a wrong counter, key, word or pairing moves a draw by O(1)); not a precision statement
SENTINEL = -77.25
GRID_QUADS = pr.FILL_BLOCKS * pr.FILL_THREADS                    # quads one pass of the full grid covers
SEEDS_OFFSETS = [(0, 0), ((0x9E3779B9 << 32) | 0x7F4A7C15, 12345), (5, (3 << 32) + 11), (1, 2 ** 32 - 2)]


def _fill(dev, n, seed, offset, pad=3):
    """iwvi_fill_normal into a buffer with `pad` sentinel elements behind it -> (the n draws, the pad) as device tensors."""
    from dgps_with_iwvi_amd import _abi
    buf = torch.full((n + pad,), SENTINEL, dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().iwvi_fill_normal(_abi.ptr(buf), n, seed, offset, _abi.stream_ptr()))
    return buf[:n], buf[n:]


def _fill_dev(dev, n, seed, state, out=None):
    from dgps_with_iwvi_amd import _abi
    out = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev) if out is None else out
    _abi.check(_abi.lib().iwvi_fill_normal_dev(_abi.ptr(out), n, seed, _abi.ptr(state), _abi.stream_ptr()))
    return out


def _state(dev):
    return torch.zeros(2, dtype=torch.int64, device=dev)        # {counter, ticket}: "zero both once"


@pytest.mark.parametrize("seed,offset", SEEDS_OFFSETS)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_fill_normal_is_the_documented_stream(gpu_device, n, seed, offset):
    """Small sizes, every n % 4, a key with a non-zero high word, offsets that use and that carry into the counter's second word.
    Observed max |device - restatement| on an MI355X: 3.2e-7 (the hardware log2 / sin / cos), against the stream tolerance 1e-4."""
    got, pad = _fill(gpu_device, n, seed, offset)
    ref = pr.fill_normal(n, seed, offset)
    err = np.abs(got.double().cpu().numpy() - ref).max()
    print("fill_normal n=%d seed=%#x offset=%d: max |dev - ref| = %.3g" % (n, seed, offset, err))
    assert err <= STREAM_ATOL
    assert bool((pad == SENTINEL).all())                          # a partial last quad writes n elements, not 4 ceil(n / 4)


def test_fill_normal_past_one_pass_of_the_grid(gpu_device):
    """n = 4 x 256 x 4096 + 7: two quads beyond what 4096 blocks of 256 threads cover in one pass, so the grid-stride loop runs; the
    last quad is partial.  Observed max |device - restatement| on an MI355X: 8.5e-7."""
    n = 4 * GRID_QUADS + 7
    seed, offset = (0xABCDEF01 << 32) | 0x2345, (1 << 32) - GRID_QUADS // 2        # the 2^32 carry falls inside the fill
    got, pad = _fill(gpu_device, n, seed, offset)
    got = got.double().cpu().numpy()
    assert bool((pad == SENTINEL).all())
    ref = pr.fill_normal(n, seed, offset)
    err = np.abs(got - ref)
    print("fill_normal n=%d: max |dev - ref| = %.3g, in the strided tail %.3g" % (n, err.max(), err[4 * GRID_QUADS:].max()))
    assert err.max() <= STREAM_ATOL
    for alt in (((0, 2), (1, 3)),):                              # the tolerance does tell a mis-paired stream apart
        assert np.abs(pr.fill_normal(4096, seed, offset, pairing=alt) - ref[:4096]).max() > 1.0


def test_fill_normal_arguments(gpu_device):
    from dgps_with_iwvi_amd import _abi
    lib = _abi.lib()
    buf = torch.full((8,), SENTINEL, device=gpu_device)
    assert lib.iwvi_fill_normal(_abi.ptr(buf), 0, 1, 0, _abi.stream_ptr()) == 0        # n = 0: nothing to do
    assert lib.iwvi_fill_normal(None, 4, 1, 0, _abi.stream_ptr()) == _abi.ERR_ARG
    assert lib.iwvi_fill_normal_dev(_abi.ptr(buf), 4, 1, None, _abi.stream_ptr()) == _abi.ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


def test_fill_normal_dev_equal_launches_advance_the_counter(gpu_device):
    """(a) three equal launches on one zeroed state: launch i is the stateless fill at offset i ceil(n / 4), bit for bit."""
    n, seed = 4 * 256 * 3 + 2, (7 << 32) | 9                     # 4 blocks, partial last quad
    nq = (n + 3) // 4
    st = _state(gpu_device)
    for i in range(3):
        got = _fill_dev(gpu_device, n, seed, st)
        torch.cuda.synchronize()
        assert st.tolist() == [(i + 1) * nq, 0]                  # the counter moved by ceil(n / 4); the ticket is back at 0
        assert torch.equal(got, _fill(gpu_device, n, seed, i * nq)[0])


def test_fill_normal_dev_replayed_graph_draws_the_next_segment(gpu_device):
    """(b) one launch captured in a graph (a single kernel node) and replayed: every replay is the next segment of the stream."""
    n, seed = 4 * 256 * 5, 31
    nq = n // 4
    st = _state(gpu_device)
    out = torch.full((n,), SENTINEL, dtype=torch.float32, device=gpu_device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _fill_dev(gpu_device, n, seed, st, out=out)
    torch.cuda.synchronize()
    assert st.tolist() == [0, 0]                                 # capturing runs nothing
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert st.tolist() == [(i + 1) * nq, 0]
        assert torch.equal(out, _fill(gpu_device, n, seed, i * nq)[0])


def test_fill_normal_dev_launches_of_different_sizes_share_one_state(gpu_device):
    """(c) 4095 blocks, then 4096, then 1, then 4096 on one state.  Each launch is the stateless fill at the sum of the earlier
    ceil(n / 4), the counter equals that sum and the ticket word is 0 after every launch.  (A ticket that is only ever counted up modulo
    the grid leaves the ticket word at the running block count -- this assertion fails on every run -- and lets an early finisher of the
    4096-block launch advance the counter under the blocks dispatched after it, which then draw the NEXT launch's numbers: the bit-for-bit
    comparison fails whenever that race happens.  On an MI355X the former ticket left the word at 4095, 8191, 8192, 12288; the race
    itself did not show in that run -- it depends on dispatch timing --, so the ticket word and the reading of the code carry the fix.)"""
    seed = (0x51 << 32) | 0xED
    st = _state(gpu_device)
    done, seen = 0, []
    for blocks in (4095, 4096, 1, 4096):
        n = 4 * 256 * blocks
        got = _fill_dev(gpu_device, n, seed, st)
        torch.cuda.synchronize()
        ref = _fill(gpu_device, n, seed, done)[0]
        done += n // 4
        seen.append((blocks, done) + tuple(st.tolist()) + (int((got != ref).sum()),))
    print("fill_normal_dev (blocks, expected counter, counter, ticket, elements that differ):", seen)
    assert all(counter == expected for _, expected, counter, _, _ in seen), seen
    assert all(differ == 0 for *_, differ in seen), seen
    assert all(ticket == 0 for _, _, _, ticket, _ in seen), seen
