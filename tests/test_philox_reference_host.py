"""CPU pins of tests/philox_reference.py: Random123's published known answers for Philox4x32-10, a scalar Python-int loop of the round
function in csrc/iwvi_common.h, the float32 uniform at its edges, and the counter / word layout of a fill."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_reference as pr   # noqa: E402

# Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _philox_scalar(c, k):
    """philox4x32_10 of csrc/iwvi_common.h, line for line, in Python integers."""
    c, (k0, k1) = list(c), k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c)


@pytest.mark.parametrize("counter,key,out", KAT)
def test_known_answers(counter, key, out):
    assert tuple(int(w) for w in pr.philox4x32_10(counter, key)) == out
    assert _philox_scalar(counter, key) == out


def test_vectorised_equals_the_scalar_loop():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, (50, 4), dtype=np.uint64)
    k = rng.integers(0, 2 ** 32, (50, 2), dtype=np.uint64)
    got = pr.philox4x32_10(c, k)
    for i in range(50):
        assert tuple(int(w) for w in got[i]) == _philox_scalar([int(x) for x in c[i]], (int(k[i, 0]), int(k[i, 1])))
    one_key = pr.philox4x32_10(c, k[3])                                    # a key that broadcasts over the counters
    assert tuple(int(w) for w in one_key[7]) == _philox_scalar([int(x) for x in c[7]], (int(k[3, 0]), int(k[3, 1])))


def test_uniform_is_the_float32_expression_at_its_edges():
    w = np.array([0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 1], dtype=np.uint64)
    u = pr.uniform32(w)
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -33) and u[1] == np.float32(1.5 * 2.0 ** -32)
    assert u[3] == np.float32(2.0 ** -8) and u[4] == u[3]                  # beyond 2^24 the conversion rounds (ties to even), + 0.5f is absorbed
    assert u[5] == np.float32(0.5)
    assert u[6] == np.float32(1.0 - 2.0 ** -24) and u[7] == np.float32(1.0) and u[8] == np.float32(1.0)   # float(word) reaches 2^32
    z = pr.box_muller(np.array([[2 ** 32 - 1, 2 ** 32 - 1, 0, 2 ** 30]], dtype=np.uint64))[0]
    r_min = math.sqrt(-2.0 * math.log(float(np.float32(0.99999994))))      # u1 = 1 is clamped below 1: the radius is tiny, not 0 or NaN
    assert z[0] == pytest.approx(r_min, rel=1e-12) and abs(z[1]) < 1e-15   # u2 = 1: a whole revolution
    r_max = math.sqrt(-2.0 * math.log(2.0 ** -33))
    assert abs(z[2]) < 1e-8 and z[3] == pytest.approx(r_max, rel=1e-7)     # float32(2^30 + 0.5) = 2^30: exactly a quarter turn


def test_box_muller_pairs_words_01_and_23():
    w = np.array([[123456789, 2 ** 30, 987654321, 2 ** 31]], dtype=np.uint64)
    z = pr.box_muller(w)[0]
    r01 = math.sqrt(-2.0 * math.log(float(pr.uniform32(w[0, 0:1])[0])))
    r23 = math.sqrt(-2.0 * math.log(float(pr.uniform32(w[0, 2:3])[0])))
    assert math.hypot(z[0], z[1]) == pytest.approx(r01, rel=1e-12) and math.hypot(z[2], z[3]) == pytest.approx(r23, rel=1e-12)
    assert abs(z[0]) < 1e-7 * r01 and z[1] == pytest.approx(r01, rel=1e-9)       # u2 ~ 1/4: (cos, sin) = (0, 1)
    assert z[2] == pytest.approx(-r23, rel=1e-9) and abs(z[3]) < 1e-7 * r23      # u2 ~ 1/2: (-1, 0)
    other = pr.box_muller(w, pairing=((0, 2), (1, 3)))[0]                        # a different pairing is a different stream
    assert np.abs(other - z).max() > 0.1


def test_fill_layout_counter_offset_and_key():
    seed, off = (0xDEADBEEF << 32) | 0x12345678, (7 << 32) - 2
    z = pr.fill_normal(23, seed, off)
    assert z.shape == (23,)
    for i in (0, 5, 11, 22):                                                     # quads 0, 1, 2 and 5: the 2^32 carry sits between quads 1 and 2
        ctr = off + i // 4
        words = _philox_scalar([ctr & 0xFFFFFFFF, ctr >> 32, 0, 0], (0x12345678, 0xDEADBEEF))
        ref = pr.box_muller(np.array([words], dtype=np.uint64))[0]
        assert z[i] == ref[i % 4]
    assert np.array_equal(pr.fill_normal(23, seed, off, first=8), z[8:])         # a tail of the same fill
    assert np.array_equal(pr.fill_normal(8, seed, off + 3), pr.fill_normal(20, seed, off)[12:])   # offset counts quads
    big = pr.fill_normal(200000, 1, 0)                                           # and it is N(0,1)
    assert abs(big.mean()) < 5 / math.sqrt(big.size) and abs(big.var() - 1) < 5 * math.sqrt(2 / big.size)
