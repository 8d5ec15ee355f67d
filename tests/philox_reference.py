"""NumPy restatement of the library's noise streams: the layer stack's (``layer_normal`` below, draw_normal4) and the stand-alone one (``iwvi_fill_normal`` / ``iwvi_fill_normal_dev``, k_fill_normal in
csrc/lv_elbo.hip; philox4x32_10 and box_muller4 in csrc/iwvi_common.h).  TEST INFRASTRUCTURE ONLY:
tests/test_philox_reference_host.py pins this module on the CPU (Random123's known answers), tests/test_gpu_fill_normal.py compares the
kernel with it.

Stream: element i of a fill uses the Philox4x32-10 block of counter (lo32(offset + i // 4), hi32(offset + i // 4), 0, 0) under the key
(lo32(seed), hi32(seed)), word i % 4.  Words (0, 1) of a block give (r cos, r sin), words (2, 3) likewise, with
  u = (float32(word) + 0.5f) * 2^-32    formed in float32 exactly as the kernel forms it (the conversion rounds to 24 bits, the + 0.5f is
                                         absorbed above 2^24, the product by a power of two is exact),
  u1 clamped to [FLT_MIN, 1 - 2^-24] (u2 is not clamped: a full revolution is harmless),
  r = sqrt(-2 ln u1), angle 2 pi u2     in float64 here; the kernel uses the hardware log2 / sqrt / sin / cos (~1e-6 on a draw).
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)            # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                                  # Weyl key increments
MASK32 = np.uint64(0xFFFFFFFF)
FILL_BLOCKS, FILL_THREADS = 4096, 256                            # k_fill_normal's launch: min(4096, ceil(ceil(n / 4) / 256)) x 256


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (anything that broadcasts; values < 2^32) -> [..., 4] uint64 holding the four 32-bit output words."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2                                # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def uniform32(words):
    """The kernel's float32 uniform of a 32-bit word, as float32."""
    u = (words.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    assert u.dtype == np.float32
    return u


def box_muller(words, pairing=((0, 1), (2, 3))):
    """words [..., 4] -> normals [..., 4] float64: the pair (a, b) of `pairing` fills its own two positions with (r cos, r sin)."""
    out = np.empty(words.shape, np.float64)
    for a, b in pairing:
        u1 = np.clip(uniform32(words[..., a]), np.float32(1.1754944e-38), np.float32(0.99999994)).astype(np.float64)
        u2 = uniform32(words[..., b]).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(u1))
        out[..., a], out[..., b] = rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)
    return out


def fill_words(n, seed, offset, first=0):
    """The Philox words behind elements first .. n-1 of a fill: [quads, 4] uint64 starting at the quad of `first`."""
    q0, q1 = first // 4, (n + 3) // 4
    ctr = (np.arange(q0, q1, dtype=np.uint64) + np.uint64(offset % 2 ** 64))          # uint64 wrap-around is the kernel's
    counter = np.stack([ctr & MASK32, ctr >> np.uint64(32), np.zeros_like(ctr), np.zeros_like(ctr)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return philox4x32_10(counter, key)


def fill_normal(n, seed, offset, first=0, pairing=((0, 1), (2, 3))):
    """Elements first .. n-1 (first a multiple of 4) of iwvi_fill_normal(out, n, seed, offset), float64."""
    assert first % 4 == 0
    return box_muller(fill_words(n, seed, offset, first), pairing).reshape(-1)[:n - first]


def layer_normal(seed, step, layer, t, dims, pairing=((0, 1), (2, 3))):
    """The layer stack's own stream (draw_normal4 in csrc/iwvi_common.h): the draws of samples ``t`` (array of row indices) for the ``dims``
    noise components of layer ``layer`` in evaluation ``step`` -> [len(t), dims] float64.  Components 4 q .. 4 q + 3 of sample t come from
    the block of counter (lo32(t), hi32(t), 256 layer + q, lo32(step)) under the key (lo32(seed), hi32(seed) ^ hi32(step)); a last quad
    that ``dims`` does not fill is drawn whole and cut."""
    t = np.asarray(t, dtype=np.uint64).reshape(-1, 1)
    q = np.arange((dims + 3) // 4, dtype=np.uint64).reshape(1, -1)
    one = np.ones((t.shape[0], q.shape[1]), dtype=np.uint64)
    counter = np.stack([(t & MASK32) * one, (t >> np.uint64(32)) * one, (np.uint64(256 * layer) + q) * one,
                        np.uint64(step & 0xFFFFFFFF) * one], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, ((seed >> 32) ^ (step >> 32)) & 0xFFFFFFFF], dtype=np.uint64)
    return box_muller(philox4x32_10(counter, key), pairing).reshape(t.shape[0], -1)[:, :dims]
