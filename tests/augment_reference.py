"""Restatement of the training augmentation (config.AUGMENT) from its definition alone, in plain Python integers and NumPy:
Philox4x32-10 as Random123 defines it, one draw per image, an integer shift with reflect padding and an optional horizontal flip, then
the pipeline's float32 scaling float(x) / 255 * scale + shift.  Shared by tests/test_augment_reference.py (CPU) and
tests/test_gpu_augment.py; it does not import the package."""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments

# Random123 known answers: (counter, key) -> output
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """one Philox4x32-10 block on Python integers: ten rounds, the key bumped between rounds."""
    x0, x1, x2, x3 = counter
    k0, k1 = key
    for rnd in range(10):
        if rnd > 0:
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
        hi0, lo0 = divmod(PHILOX_M0 * x0, 1 << 32)
        hi1, lo1 = divmod(PHILOX_M1 * x2, 1 << 32)
        x0, x1, x2, x3 = hi1 ^ x1 ^ k0, lo1, hi0 ^ x3 ^ k1, lo0
    return x0, x1, x2, x3


def draw(i, max_shift, flip, seed, stream_id, count):
    """(dy, dx, flipped) of image i of a batch."""
    seed, count = seed % (1 << 64), count % (1 << 64)
    r = philox4x32_10((i, stream_id, count & M32, count >> 32), (seed & M32, seed >> 32))
    span = 2 * max_shift + 1
    return (r[0] * span >> 32) - max_shift, (r[1] * span >> 32) - max_shift, bool(flip) and (r[2] >> 31) == 1


def refl(p, size):
    """TF 'REFLECT' padding: -1 -> 1, size -> size - 2 (valid for |overhang| <= size - 1)."""
    if p < 0:
        return -p
    if p >= size:
        return 2 * size - 2 - p
    return p


def transform_u8(src, max_shift, flip, seed, stream_id, count):
    """the pixel rearrangement alone: uint8 [n,h,w,c] -> uint8 [n,h,w,c]."""
    n, h, w, _ = src.shape
    assert 0 <= max_shift <= min(h, w) - 1
    out = np.empty_like(src)
    for i in range(n):
        dy, dx, fl = draw(i, max_shift, flip, seed, stream_id, count)
        rows = [refl(y + dy, h) for y in range(h)]
        cols = [refl((w - 1 - x if fl else x) + dx, w) for x in range(w)]
        out[i] = src[i][rows][:, cols]
    return out


def scale_u8(src, scale, shift):
    """the pipeline's float32 expression, one rounding per operation: float(x) / 255 * scale + shift."""
    return src.astype(np.float32) / np.float32(255) * np.float32(scale) + np.float32(shift)


def augment(src, scale, shift, max_shift, flip, seed, stream_id, count):
    """uint8 [n,h,w,c] -> float32 [n,h,w,c]: what tg_u8_augment_f32 writes."""
    return scale_u8(transform_u8(src, max_shift, flip, seed, stream_id, count), scale, shift)
