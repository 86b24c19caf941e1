"""NumPy reference of the nearest-training-image kernels (include/tg_kernels.h: tg_nearest_u8_i32, tg_f32_quantize_u8).

d2 comes from int64 differences, the k best of a row from np.lexsort((idx, d2)) — the smaller distance first, on a tie the lower index —
and the quantiser's fp32 chain is restated operation by operation in float32.  Everything is integer or a fixed fp32 chain: callers
compare with ==."""
import numpy as np

NONE_D2, NONE_IDX = np.int32(2 ** 31 - 1), np.int32(-1)


def d2(q, r):
    """[m, n] int64 squared distances of uint8 rows q [m, d] and r [n, d]."""
    q, r = np.asarray(q, np.uint8).astype(np.int64), np.asarray(r, np.uint8).astype(np.int64)
    out = np.empty((q.shape[0], r.shape[0]), np.int64)
    for i in range(q.shape[0]):
        diff = r - q[i]
        out[i] = (diff * diff).sum(axis=1)
    return out


def select(dist, idx, k):
    """the k lexicographically smallest (dist, idx) pairs of every row -> (d2 int32 [m, k], idx int32 [m, k]); rows with fewer than k
    candidates are filled with (INT32_MAX, -1).  dist, idx: [m, c]."""
    m, c = dist.shape
    out_d = np.full((m, k), NONE_D2, np.int32)
    out_i = np.full((m, k), NONE_IDX, np.int32)
    for i in range(m):
        real = idx[i] >= 0                                             # (sentinels of an earlier selection do not take part)
        dv, iv = dist[i][real], idx[i][real]
        order = np.lexsort((iv, dv))[:k]
        out_d[i, :len(order)], out_i[i, :len(order)] = dv[order], iv[order]
    return out_d, out_i


def nearest(q, r, k, base=0, prev=None):
    """tg_nearest_u8_i32: the k best (d2, base + j) of every query row over the rows of r; prev = (d2, idx) of an earlier call takes
    part (merge)."""
    dist = d2(q, r)
    idx = np.broadcast_to(np.arange(r.shape[0], dtype=np.int64) + base, dist.shape)
    if prev is not None:
        dist = np.concatenate([dist, np.asarray(prev[0], np.int64)], axis=1)
        idx = np.concatenate([idx, np.asarray(prev[1], np.int64)], axis=1)
    return select(dist, idx, k)


def nearest_chunked(q, chunks, k):
    """the same over a reference set handed in as [(base, rows)] chunks, in the order given."""
    prev = None
    for base, rows in chunks:
        prev = nearest(q, rows, k, base, prev)
    return prev


def affine(u, scale, shift):
    """tg_u8_affine_f32: float(u) / 255 * scale + shift, every operation rounded to fp32."""
    x = np.asarray(u, np.uint8).astype(np.float32)
    return x / np.float32(255) * np.float32(scale) + np.float32(shift)


def quantize(x, scale, shift):
    """tg_f32_quantize_u8: inv = 255 / scale in fp32; t = (x - shift) * inv; floor(t + 0.5) clamped to 0..255, NaN -> 0."""
    x = np.asarray(x, np.float32)
    inv = np.float32(255.0) / np.float32(scale)
    with np.errstate(invalid='ignore', over='ignore'):
        t = ((x - np.float32(shift)).astype(np.float32) * inv).astype(np.float32)
        u = np.floor((t + np.float32(0.5)).astype(np.float32))
        u = np.where(u > 0, np.where(u < 255, u, np.float32(255)), np.float32(0))        # a NaN fails u > 0
    return u.astype(np.uint8)


def scalars(nn_d2, d):
    """(mean, min) over the rows of sqrt(d2 of the nearest / d) / 255, in float64."""
    rmse = np.sqrt(np.asarray(nn_d2, np.int64)[:, 0].astype(np.float64) / float(d)) / 255.0
    return float(rmse.mean()), float(rmse.min())
