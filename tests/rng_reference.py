"""Restatement of the step's random draws (csrc/rng.hip; include/tg_kernels.h "RNG") from their definition alone, vectorised in
NumPy on top of the known-answer scalar block of tests/augment_reference.py.  Shared by tests/test_rng_reference.py (CPU) and
tests/test_gpu_rng.py; it does not import the package.

State = (seed, step), two 64-bit words.  Element e of a flat draw belongs to block i = e // 4 and is word e % 4 (x, y, z, w in this order)
of   philox4x32_10(counter = (lo32(i), hi32(i), stream_id, lo32(step)), key = (lo32(seed), hi32(seed) ^ hi32(step))).
A one-hot row r draws ONE block, counter (r, 0, stream_id, lo32(step)), and takes class (word x * k) >> 32.

u01 maps a word to fp32 exactly as the kernel codes it: ((x >> 8) + 0.5f) * 2^-24, the sum rounded to fp32 (k + 0.5 is not representable
for k >= 2^23: it rounds to the even neighbour), a value in (0, 1]: the one word value x >> 8 == 0xFFFFFF gives exactly 1.0.  The uniform and
keep-mask draws clamp it to 1 - 2^-24, the largest fp32 below 1 (u01(..., clamp=True); clamp=False there restates the kernel as it was before
the clamp); the normal draw takes it unclamped, as it always did.  Every other word is untouched by the clamp.

The four modes on u = u01(word) (clamped for the first two):
  uniform    lo + (hi - lo) * u, each of the three operations rounded to fp32 (the library is built with -ffp-contract=off: the code object
             multiplies, then adds; there is no fused multiply-add in this expression);
  keep-mask  u < keep_prob ? 1 : 0;
  normal     Box-Muller per word pair: (x, y) -> stddev * r * cos(t), stddev * r * sin(t) with r = sqrt(-2 ln u(x)), t = 2 pi u(y); (z, w) the
             same for elements 2 and 3.  Returned in float64 on the same fp32 u (the kernel's fp32 evaluation is held to it pointwise);
  one-hot    see above."""
import numpy as np

import augment_reference as A

_M32 = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)
U_MAX = np.float32(1.0) - np.float32(2.0 ** -24)       # 0x3F7FFFFF
EDGE_WORD = 0xFFFFFF                                   # x >> 8 of the one word value the clamp changes


def philox_blocks(c0, c1, c2, c3, key):
    """Philox4x32-10 on arrays of counter words (scalars broadcast): [len, 4] uint32, columns x, y, z, w."""
    x0, x1, x2, x3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) & _M32 for c in (c0, c1, c2, c3)])
    k0, k1 = int(key[0]) & A.M32, int(key[1]) & A.M32
    m0, m1 = np.uint64(A.PHILOX_M0), np.uint64(A.PHILOX_M1)
    for rnd in range(10):
        if rnd > 0:
            k0, k1 = (k0 + A.PHILOX_W0) & A.M32, (k1 + A.PHILOX_W1) & A.M32
        p0, p1 = m0 * x0, m1 * x2                      # 32 x 32 -> 64 bits: exact in uint64
        x0, x1, x2, x3 = (p1 >> _SH) ^ x1 ^ np.uint64(k0), p1 & _M32, (p0 >> _SH) ^ x3 ^ np.uint64(k1), p0 & _M32
    return np.stack([x0, x1, x2, x3], axis=-1).astype(np.uint32).reshape(-1, 4)


def key_of(seed, step):
    seed, step = seed % (1 << 64), step % (1 << 64)
    return seed & A.M32, (seed >> 32) ^ (step >> 32)


def words(n, seed, step, stream_id, first_block=0):
    """the (n + 3) // 4 blocks of a flat draw of n elements: [blocks, 4] uint32."""
    i = np.arange(first_block, first_block + (n + 3) // 4, dtype=np.uint64)
    return philox_blocks(i & _M32, i >> _SH, stream_id, (step % (1 << 64)) & A.M32, key_of(seed, step))


def u01(x, clamp=True):
    """fp32 value of a 32-bit word, operation by operation as the kernel: (0, 1], or (0, 1) with the clamp of the uniform / keep-mask draws."""
    k = (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32)            # < 2^24: exact
    u = ((k + np.float32(0.5)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    return np.minimum(u, U_MAX) if clamp else u


def _u(n, seed, step, stream_id, clamp):
    return u01(words(n, seed, step, stream_id), clamp).reshape(-1)[:n]


def uniform(n, lo, hi, seed, step, stream_id, clamp=True):
    lo, hi = np.float32(lo), np.float32(hi)
    d = np.float32(hi - lo)
    return (lo + (d * _u(n, seed, step, stream_id, clamp)).astype(np.float32)).astype(np.float32)


def keep_mask(n, keep_prob, seed, step, stream_id, clamp=True):
    return (_u(n, seed, step, stream_id, clamp) < np.float32(keep_prob)).astype(np.float32)


def normal64(n, stddev, seed, step, stream_id, swap_sincos=False, swap_pairs=False):
    """(values, magnitudes) in float64 on the UNCLAMPED u: magnitudes = stddev * r, the radius of each element's pair.  swap_sincos / swap_pairs build the
    wrong references of the negative controls (sine and cosine exchanged; the pairs (x, y) and (z, w) exchanged)."""
    u = u01(words(n, seed, step, stream_id), clamp=False).astype(np.float64)         # (0, 1]: u = 1 gives radius 0
    if swap_pairs:
        u = u[:, [2, 3, 0, 1]]
    a = np.float64(np.float32(stddev))
    r = np.sqrt(-2.0 * np.log(u[:, 0::2]))             # [blocks, 2]: pair 0 = (x, y), pair 1 = (z, w)
    t = 2.0 * np.pi * u[:, 1::2]
    c, s = (np.sin(t), np.cos(t)) if swap_sincos else (np.cos(t), np.sin(t))
    v = np.stack([a * r[:, 0] * c[:, 0], a * r[:, 0] * s[:, 0], a * r[:, 1] * c[:, 1], a * r[:, 1] * s[:, 1]], axis=-1)
    mag = np.stack([a * r[:, 0], a * r[:, 0], a * r[:, 1], a * r[:, 1]], axis=-1)
    return v.reshape(-1)[:n], mag.reshape(-1)[:n]


def onehot_classes(rows, k, seed, step, stream_id):
    r = np.arange(rows, dtype=np.uint64)
    w0 = philox_blocks(r, 0, stream_id, (step % (1 << 64)) & A.M32, key_of(seed, step))[:, 0].astype(np.uint64)
    return ((w0 * np.uint64(k)) >> _SH).astype(np.int64)


def onehot(rows, k, seed, step, stream_id):
    out = np.zeros((rows, k), np.float32)
    out[np.arange(rows), onehot_classes(rows, k, seed, step, stream_id)] = 1
    return out


def edge_elements(n, seed, step, stream_id):
    """flat element indices < n whose word has x >> 8 == 0xFFFFFF."""
    w = words(n, seed, step, stream_id).reshape(-1)[:n]
    return np.flatnonzero((w >> np.uint32(8)) == EDGE_WORD)
