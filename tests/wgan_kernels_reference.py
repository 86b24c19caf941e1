"""NumPy restatements of the kernels of csrc/wgan_gp.hip (tg_wgan_interp_f32, tg_grad_penalty_f32, tg_grad_penalty_rows_f32, tg_wgan_loss_f32,
tg_wgan_{d,g,c}_head_f32), of tg_g_loss_f32 (csrc/loss.hip) and of tg_slab_reduce_f32 (csrc/prep.hip), with the inputs the tests feed them.
tests/test_gpu_wgan_kernels.py, test_gpu_loss_heads.py and test_gpu_prep.py hold the kernels to these on the GPU; test_wgan_kernels_reference.py
shows on the CPU, on the very same inputs, that an fp32 evaluation in the kernel's order passes every bound and that every negative control
is rejected.  The float64 restatements are evaluated on the same fp32 inputs and return (ref64, mag) or (ref64, sum|terms|) in the
convention of tests/kernel_check.py; every *32 function is the fp32 evaluation in the kernel's order (the library is built with
-ffp-contract=off: a * b + c is two roundings; fp32 division and sqrtf are correctly rounded).

Tolerance class of every output, u = 2^-24, each K a count of roundings read off the kernel's expression:

  interp out        pointwise, K_INTERP = 3: b - a, the product with alpha, the sum; mag = |a| + |alpha| (|a| + |b|).  Padding exactly 0,
                    rows of alpha = 0 the bits of `real`.
  gp columns r      pointwise, K = h + 7 (k_gp_r): the error of s, ds <= (h + 2) u s (the fp32 sum of h squares, each product and each
                    sum rounded, relative error (h + 1) u, halved by the root, plus sqrtf: within (h + 2) u), reaches (s - 1) / s through
                    its derivative 1 / s^2, i.e. (h + 2) u of 1 / s; then s - 1, the division, weight / (n w c), the product of the two
                    and the product with g: 5 roundings.  mag = 2 weight / (n w c) (s + 1) / s |g| bounds both 1 / s and |s - 1| / s.
  gp columns gp     its own derived bound (penalty_bound): sum over the columns of 2 |s - 1| ds + ds^2, ds = (h + 2) u s, times
                    weight / (n w c) — (s - 1)^2 cancels near s = 1, so no relative bound on gp — plus u |gp| for the one rounding of the
                    double sum to the fp32 result.  The squares, the block sums and the scale are double.
  gp rows r         pointwise, K_ROWS_R = 3: the row sum, the root and 2 (s - 1) / s weight / n are double (2^-53: all of it counted as
                    one rounding), the conversion of the coefficient to fp32, the product with g.  mag = 2 weight / n (s + 1) / s |g|.
  gp rows gp        penalty_bound with ds = (f + 2) 2^-53 s, plus u |gp|.
  wasserstein       loss[5] / terms[:3] / the d head's loss: reduction (TOL sum|terms|: the means of |z| that enter each value, weighted as the
                    value weights them); the negative control drops the last row of a group.  dz: pointwise, K_DZ = 2 (the sum or
                    difference of the halved lambdas, the division by the row count), mag the same on absolute values; dfake and the g
                    head's dz = -1 / n: K_DFAKE = 1.  The d head's terms[3] = gp_w / gp_weight: K = 1.  The d head's loss is the fp32 sum of
                    tg_wgan_loss_f32's d_loss and gp_w (both kernels inline the same `wasserstein`; the lambdas reach it as the same fp32
                    values from an argument or from memory), its terms[:3] and dz the same bits.
  g head            loss = -mean z: reduction, control without the last row.
  c head            loss, terms: reduction over the rows' |lse sum y| + sum |y l| (as tests/test_gpu_loss_heads.py::test_softmax_ce), control
                    without the last row of each labelled group.  dl: pointwise, K = ceil(2.4 k) + 9 (k_c_head), a count of 2.37 k + 8:
                    p_j = e_j / se carries the rounding of l_j - m through exp (|d_j| u: the factor 1 + |d_j| of mag) and expf (2); the
                    sum se, relative to se >= 1: 0.37 k from the roundings of its terms' l - m (|d| e^-|d| <= 0.37 each), 2 from their
                    expf, k - 1 sums; 1 / se and the product with it (2); then sum y (k - 1 sums), the product with it, the difference
                    with y, w = l2 / n and the product with w (4).  mag = |w| (p |sum y| (1 + |d|) + |y|).
  g_loss            value: reduction over 0.5 / n (max(z,0) + |z| + log1p(exp(-|z|))), control without the last row.  dz[:, 0] =
                    0.5 / n (sigmoid(z) - 1): pointwise, K_G_LOSS_DZ = 7: expf (2), 1 + e, the reciprocal, the difference with 1, 0.5 / n,
                    the product; mag = 0.5 / n (sigmoid(z) + 1) — at z = 80 the difference cancels to 0 and the bound is u-sized.
  slab reduce       bit-exact against slab_narrow32 / slab_wide32 (fixed-order fp32 sums), and reduction against float64 with the control
                    that drops the last slab.
"""
import numpy as np

import wgan_gp_reference as RC
from kernel_check import TOL, U, seq_sum32

BLK = 256
f4 = np.float32


def f8(a):
    return np.asarray(a, np.float64)


def padded(v, ld):
    """[..., c] values in a [..., ld] array whose padding columns hold NaN."""
    v = np.asarray(v, np.float32)
    out = np.full(v.shape[:-1] + (ld,), np.nan, np.float32)
    out[..., :v.shape[-1]] = v
    return out


def block_sum32(per_thread):
    """tgd::block_sum<4> of 256 per-thread fp32 values (leading axis): xor butterflies 32..1 inside each wave, then the waves in index order."""
    v = np.asarray(per_thread, np.float32).copy()
    idx = np.arange(BLK)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[idx ^ o]).astype(np.float32)
    return seq_sum32([v[64], v[128], v[192]], init=v[0])


def strided32(rows):
    """the per-thread fp32 sums of a `for (r = threadIdx.x; r < n; r += 256) acc += rows[r]` loop: [256, ...] (adding 0.f is exact)."""
    rows = np.asarray(rows, np.float32)
    turns = -(-len(rows) // BLK)
    pad = np.zeros((turns * BLK,) + rows.shape[1:], np.float32)
    pad[:len(rows)] = rows
    return seq_sum32(list(pad.reshape((turns, BLK) + rows.shape[1:])))


# ---------------------------------------------------------------------------------------------------------------- interpolation
INTERP_CASES = [(3, 35, 3, 4, 5, 4), (33, 1024, 3, 3, 5, 32)]        # n, hw, c, ld_r, ld_f, ld_out; the second wraps the 4096 x 256 grid
K_INTERP = 3


def interp_case(case):
    n, hw, c, ld_r, ld_f, ld_out = case
    rng = np.random.default_rng(n * 7 + hw)
    real = padded(rng.uniform(-1, 1, (n * hw, c)), ld_r)
    fake = padded(rng.uniform(-1, 1, (n * hw, c)), ld_f)
    alpha = rng.random(n).astype(np.float32)
    alpha[0], alpha[-1] = 0.0, 1.0
    return real, fake, alpha


def interp(real, fake, alpha, hw, c):
    a, b = f8(real[:, :c]), f8(fake[:, :c])
    al = np.repeat(f8(alpha), hw)[:, None]
    return a + al * (b - a), np.abs(a) + np.abs(al) * (np.abs(a) + np.abs(b))


def interp32(real, fake, alpha, hw, c):
    a, b = real[:, :c], fake[:, :c]
    return (a + (np.repeat(alpha, hw)[:, None] * (b - a).astype(f4)).astype(f4)).astype(f4)


# ---------------------------------------------------------------------------------------------------------------- the penalty
def penalty_bound(s, ds, scale, gp):
    """the error of gp = scale sum (s - 1)^2 from an error ds of every s, plus the rounding of the result to fp32."""
    return scale * np.sum(2 * np.abs(s - 1) * ds + ds * ds) + U * abs(gp)


GP_CASES = [(3, 5, 7, 3, 32, 8), (5, 32, 32, 3, 3, 3), (1, 1, 1, 1, 1, 1)]          # n, h, w, c, ld_g, ld_r
GP_WEIGHT = 10.0


def k_gp_r(h):
    return h + 7


def gp_case(case):
    """gx [n, h, w, ld_g] with NaN padding; column scales 0.01 .. 0.5, the last y four times larger (the control drops it); column
    (image 0, x 0, channel 0) all zero where there is more than one column."""
    n, h, w, c, ld_g, ld_r = case
    rng = np.random.default_rng(n + h)
    v = rng.standard_normal((n, h, w, c)) * rng.uniform(0.01, 0.5, (n, 1, w, c))
    v[:, -1] *= 4
    if n * w * c > 1:
        v[0, :, 0, 0] = 0.0
    return padded(v, ld_g)


def gp_columns(g, c, weight, drop_last=False):
    """(r, mag of r, gp, bound of gp, s) over axis 1 (H) of g [n, h, w, >= c]; drop_last: s without the column's last y (the control)."""
    g64 = f8(g[..., :c])
    n, h, w, _ = g64.shape
    cnt = n * w * c
    s = np.sqrt((g64[:, :h - 1 if drop_last else h] ** 2).sum(axis=1, keepdims=True))
    gp = weight * np.sum((s - 1.0) ** 2) / cnt
    with np.errstate(divide='ignore', invalid='ignore'):
        r = weight * 2.0 * (s - 1.0) / s * g64 / cnt
        mag = weight * 2.0 * (s + 1.0) / s * np.abs(g64) / cnt
    return r, mag, gp, penalty_bound(s, (h + 2) * U * s, weight / cnt, gp), s


def gp_columns32(g, c, weight):
    g = np.asarray(g[..., :c], np.float32)
    n, h, w, _ = g.shape
    ss = seq_sum32([(g[:, y] * g[:, y]).astype(f4) for y in range(h)])
    s = np.sqrt(ss).astype(f4)
    with np.errstate(divide='ignore', invalid='ignore'):
        coef = ((f4(2) * (s - f4(1))).astype(f4) / s).astype(f4) * (f4(weight) / f4(n * w * c))
        r = (coef.astype(f4)[:, None] * g).astype(f4)
    gp = f4(np.sum((f8(s) - 1.0) ** 2) * (float(f4(weight)) / (n * w * c)))
    return r, gp


# n, f, ld_g, ld_r: one row; f = 1; the scalar path (f, ld_g or ld_r no multiple of 4); rows longer than the registers hold (scalar 1024
# floats, float4 4096 floats)
ROWS_CASES = [(1, 784, 800, 800), (5, 1, 1, 32), (6, 37, 40, 37), (3, 1500, 1501, 1504), (2, 4400, 4400, 4416)]
ROWS_MISALIGNED = (3, 784, 800, 800)           # f % 4 == 0, but gx or r one float off a 16-byte boundary: the scalar path
K_ROWS_R = 3


def rows_vec(case, aligned=True):
    """the vector width tg_grad_penalty_rows_f32 takes."""
    n, f, ld_g, ld_r = case
    return 4 if aligned and f % 4 == 0 and ld_g % 4 == 0 and ld_r % 4 == 0 else 1


def rows_case(case):
    """gx [n, ld_g] with NaN padding; row norms 0.2 .. 3 plus four large last elements (the control drops the last vector); row 1 all
    zero where there are three rows or more."""
    n, f, ld_g, ld_r = case
    rng = np.random.default_rng(n + f)
    v = rng.standard_normal((n, f)) * rng.uniform(0.2, 3.0, (n, 1)) / np.sqrt(f)
    tail = min(4, f)
    v[:, f - tail:] = rng.uniform(0.25, 0.5, (n, tail)) * np.where(rng.random((n, tail)) < 0.5, -1, 1)
    if n >= 3:
        v[1] = 0.0
    return padded(v, ld_g)


def gp_rows(g, f, weight, drop=0):
    """(r, mag of r, gp, bound of gp, s) over the feature axis of g [n, >= f]; drop: s without the row's last `drop` elements."""
    g64 = f8(g[:, :f])
    n = len(g64)
    s = np.sqrt((g64[:, :f - drop] ** 2).sum(axis=1, keepdims=True))
    gp = weight * np.sum((s - 1.0) ** 2) / n
    with np.errstate(divide='ignore', invalid='ignore'):
        r = weight * 2.0 * (s - 1.0) / s * g64 / n
        mag = weight * 2.0 * (s + 1.0) / s * np.abs(g64) / n
    return r, mag, gp, penalty_bound(s, (f + 2) * 2.0 ** -53 * s, weight / n, gp), s


def gp_rows32(g, f, weight, vec):
    """double sums in the kernel's order (per thread: its vectors in stride order, the float4 lanes x, y, z, w; then the butterflies and the
    waves), the coefficient rounded to fp32, fp32 products."""
    g = np.asarray(g[:, :f], np.float32)
    n = len(g)
    fv = f // vec
    turns = -(-fv // BLK)
    sq = np.zeros((n, turns * BLK, vec))
    sq[:, :fv] = (f8(g) ** 2).reshape(n, fv, vec)
    lane = sq[..., 0]
    for j in range(1, vec):
        lane = lane + sq[..., j]
    per = np.zeros((n, BLK))
    for t in range(turns):
        per = per + lane[:, t * BLK:(t + 1) * BLK]
    idx = np.arange(BLK)
    for o in (32, 16, 8, 4, 2, 1):
        per = per + per[:, idx ^ o]
    ss = (per[:, 0] + per[:, 64]) + (per[:, 128] + per[:, 192])
    s = np.sqrt(ss)
    with np.errstate(divide='ignore', invalid='ignore'):
        coef = (2.0 * (s - 1.0) / s * (float(f4(weight)) / n)).astype(f4)
        r = (g * coef[:, None]).astype(f4)
    return r, f4(np.sum((s - 1.0) ** 2) * (float(f4(weight)) / n))


# ---------------------------------------------------------------------------------------------------------------- the Wasserstein heads
WGAN_LOSS_CASES = [(1, 1, 1, 1, 1, 1), (3, 5, 2, 3, 32, 8), (257, 300, 1, 2, 33, 5)]     # n_real, n_fake, n_unl, ld, ld_d, ld_df
D_HEAD_CASES = [(1, 1, 1, 1, 1), (3, 5, 7, 3, 32), (20, 100, 80, 1, 32), (257, 300, 1, 2, 33)]   # n_real, n_fake, n_unl, ld, ld_d
G_HEAD_CASES = [(1, 1, 1), (7, 3, 32), (300, 1, 33)]                                      # n, ld, ld_d
LAMBDAS = np.array([0.3, 0.7], np.float32)
K_DZ, K_DFAKE = 2, 1
# the values each group's rows enter: indices into (d_loss, g_loss, wd1, wd2, wd3)
WD_GROUP_VALUES = ([0, 2, 3], [0, 1, 2, 4], [3, 4])


def wd_case(groups, ld):
    """logits [sum(groups), ld], column 0 standard normal, NaN padding; the last row of every group of two rows or more is +-3 (the
    controls drop it)."""
    rng = np.random.default_rng(sum(groups) + 3 * groups[1])
    v = rng.standard_normal(sum(groups))
    for end, rows, big in zip(np.cumsum(groups), groups, (3.0, -3.0, 3.0)):
        if rows > 1:
            v[end - 1] = big
    return padded(v[:, None], ld)


def wasserstein(z, groups, lam, drop=None):
    """wgan_gp_reference.wgan_loss_head on column 0 of z: (values[5], sum|terms|[5], dz, mag of dz, dfake); drop: the group that loses
    its last row (the control)."""
    l1, l2 = float(f4(lam[0])), float(f4(lam[1]))
    ends = np.cumsum(groups)
    parts = [f8(z[e - r:e, 0]) for e, r in zip(ends, groups)]
    if drop is not None:
        parts[drop] = parts[drop][:-1]
    vals, g, gfake = RC.wgan_loss_head(parts[0], parts[1], parts[2], l1, l2)
    ar, af, au = (np.abs(p).mean() for p in parts)
    s1, s2, s3 = 0.5 * (ar + af), 0.5 * (ar + au), 0.5 * (au + af)
    sabs = np.array([s1 + abs(l1) * s2 + abs(l2) * s3, af, s1, s2, s3])
    gmag = np.concatenate([np.full(len(parts[0]), (0.5 + 0.5 * abs(l1)) / len(parts[0])), np.full(len(parts[1]), (0.5 + 0.5 * abs(l2)) / len(parts[1])),
                           np.full(len(parts[2]), (0.5 * abs(l1) + 0.5 * abs(l2)) / len(parts[2]))])
    return np.array(vals), sabs, g, gmag, gfake


def wasserstein32(z, groups, lam):
    """the fp32 (d_loss, g_loss, wd1, wd2, wd3), dz and dfake of `wasserstein` / wgan_loss in the kernel's order."""
    l1, l2 = f4(lam[0]), f4(lam[1])
    nr, nf, nu = (f4(g) for g in groups)
    v = np.asarray(z[:, 0], np.float32)
    which = np.repeat([0, 1, 2], groups)
    m = [block_sum32(strided32(np.where(which == g, v, f4(0)))) / f4(groups[g]) for g in range(3)]
    wd1, wd2, wd3 = f4(0.5) * (m[0] - m[1]), f4(0.5) * (m[0] - m[2]), f4(0.5) * (m[2] - m[1])
    d_loss = -((wd1 + l1 * wd2) + l2 * wd3)
    w = [(f4(-0.5) - f4(0.5) * l1) / nr, (f4(0.5) + f4(0.5) * l2) / nf, (f4(0.5) * l1 - f4(0.5) * l2) / nu]
    dz = np.repeat(np.array(w, np.float32), groups)
    return np.array([d_loss, -m[1], wd1, wd2, wd3], np.float32), dz, np.full(groups[1], f4(-1) / nf, np.float32)


def g_head_case(n, ld):
    v = np.random.default_rng(n).standard_normal(n)
    if n > 1:
        v[-1] = 3.0
    return padded(v[:, None], ld)


def g_head(z, drop=False):
    """(-mean z, mean |z|, dz = -1/n) on column 0."""
    v = f8(z[:len(z) - 1 if drop else len(z), 0])
    return -v.mean(), np.abs(v).mean(), np.full(len(v), -1.0 / len(v))


def g_head32(z):
    v = np.asarray(z[:, 0], np.float32)
    return -(block_sum32(strided32(v)) / f4(len(v))), np.full(len(v), f4(-1) / f4(len(v)), np.float32)


# n_real, n_zero, n_fake, k, ld, ld_d: the existing tests' rows, and the second-last again without fake rows
C_HEAD_CASES = [(1, 0, 0, 10, 10, 10), (1, 1, 1, 3, 3, 32), (3, 5, 7, 10, 12, 32), (3, 5, 0, 10, 12, 32), (300, 4, 257, 10, 10, 16)]
C_LAMBDAS = np.array([0.3, 0.6], np.float32)


def k_c_head(k):
    return int(np.ceil(2.4 * k)) + 9


def c_head_case(case):
    """(logits [n, ld], y_real [n_real, k], y_fake [n_fake, k]): logits 3 N(0,1) with NaN padding and the n_zero rows NaN throughout
    (the kernel reads neither); labels one-hot, every third row soft with a sum other than 1; the last row of each labelled group of
    two rows or more has its label's logit lowered by 8 (a large term: the controls drop the row)."""
    n_real, n_zero, n_fake, k, ld, ld_d = case
    rng = np.random.default_rng(n_real + 3 * n_fake)
    n = n_real + n_zero + n_fake
    z = padded(3 * rng.standard_normal((n, k)), ld)
    z[n_real:n_real + n_zero] = np.nan
    ys = []
    for rows, off in ((n_real, 0), (n_fake, n_real + n_zero)):
        lab = rng.integers(0, k, rows)
        y = np.eye(k, dtype=np.float32)[lab]
        y[2::3] = rng.random((len(y[2::3]), k)).astype(np.float32)
        if rows > 1:
            y[-1] = np.eye(k, dtype=np.float32)[lab[-1]]
            z[off + rows - 1, lab[-1]] -= 8.0
        ys.append(y)
    return z, ys[0], ys[1]


def ce_rows(l, y):
    """per row: CE = lse sum y - y . l, its magnitude, the gradient p sum y - y and the magnitude that carries p's condition."""
    l, y = f8(l), f8(y)
    m = l.max(axis=1, keepdims=True)
    e = np.exp(l - m)
    se = e.sum(axis=1, keepdims=True)
    lse, ysum = (m + np.log(se))[:, 0], y.sum(axis=1)
    p = e / se
    return (lse * ysum - (y * l).sum(axis=1), np.abs(lse * ysum) + np.abs(y * l).sum(axis=1), p * ysum[:, None] - y,
            p * np.abs(ysum)[:, None] * (1 + np.abs(l - m)) + np.abs(y))


def c_head(z, y_real, y_fake, case, lam, drop=None):
    """((loss, t_real, t_fake), their sum|terms|, dl [n, k], mag of dl); drop: 0 / 1 = the real / fake group loses its last row in the
    values (the control)."""
    n_real, n_zero, n_fake, k, ld, ld_d = case
    l2 = float(f4(lam[1])) if n_fake else 0.0
    dl, mag = np.zeros((len(z), k)), np.zeros((len(z), k))
    t, ts = [0.0, 0.0], [0.0, 0.0]
    for i, (rows, off, y, w) in enumerate(((n_real, 0, y_real, 1.0), (n_fake, n_real + n_zero, y_fake, l2))):
        if rows == 0:
            continue
        ce, cmag, g, gmag = ce_rows(z[off:off + rows, :k], y)
        keep = rows - 1 if drop == i else rows
        t[i], ts[i] = ce[:keep].sum() / keep, cmag[:keep].sum() / keep
        dl[off:off + rows], mag[off:off + rows] = w * g / rows, abs(w) * gmag / rows
    return np.array([t[0] + l2 * t[1], t[0], t[1]]), np.array([ts[0] + abs(l2) * ts[1], ts[0], ts[1]]), dl, mag


def c_head32(z, y_real, y_fake, case, lam):
    """fp32 in the kernel's order: the class loop of one thread per row, rows strided over the threads, block sums."""
    n_real, n_zero, n_fake, k, ld, ld_d = case
    l2 = f4(lam[1]) if n_fake else f4(0)
    dl = np.zeros((len(z), k), np.float32)
    t = [f4(0), f4(0)]
    for i, (rows, off, y, w) in enumerate(((n_real, 0, y_real, f4(1)), (n_fake, n_real + n_zero, y_fake, l2))):
        if rows == 0:
            continue
        l, y = np.asarray(z[off:off + rows, :k], np.float32), np.asarray(y, np.float32)
        w = w / f4(rows)
        m = l.max(axis=1)
        e = [np.exp((l[:, j] - m).astype(f4)).astype(f4) for j in range(k)]
        se, ysum = seq_sum32(e), seq_sum32([y[:, j] for j in range(k)])
        yl = seq_sum32([(y[:, j] * l[:, j]).astype(f4) for j in range(k)])
        lse, inv = (m + np.log(se).astype(f4)).astype(f4), (f4(1) / se).astype(f4)
        ce = ((lse * ysum).astype(f4) - yl).astype(f4)
        for j in range(k):
            dl[off:off + rows, j] = w * (((e[j] * inv).astype(f4) * ysum).astype(f4) - y[:, j]).astype(f4)
        t[i] = block_sum32(strided32(ce)) / f4(rows)
    return np.array([t[0] + l2 * t[1], t[0], t[1]], np.float32), dl


# ---------------------------------------------------------------------------------------------------------------- g_loss
G_LOSS_CASES = [(1, 1, 1), (100, 1, 32), (700, 3, 4)]          # n, ld, ld_d; 700 rows: three turns of the 256-thread row loop
K_G_LOSS_DZ = 7


def g_loss_case(case):
    """logits as tests/test_gpu_loss_heads.py::test_d_loss_terms: N(0, 30) clipped to +-80, exact +-80 entries, NaN padding, and a last row of
    -3 (BCE(z, 1) is large there: the control drops it)."""
    n, ld, ld_d = case
    rng = np.random.default_rng(70 + n)
    v = np.clip(rng.standard_normal(n) * 30, -80, 80)
    v[::17], v[::13] = 80.0, -80.0
    if n > 1:
        v[-1] = -3.0
    return padded(v[:, None], ld)


def g_loss(z, drop=False):
    """0.5 mean BCE(z, 1) over column 0: (value, sum|terms|, dz, mag of dz); drop: the sum without the last row (still / n)."""
    v = f8(z[:, 0])
    n = len(v)
    soft = np.log1p(np.exp(-np.abs(v)))
    terms, mag = 0.5 / n * (np.maximum(v, 0) - v + soft), 0.5 / n * (np.maximum(v, 0) + np.abs(v) + soft)
    sig = 1.0 / (1.0 + np.exp(-v))
    keep = n - 1 if drop else n
    return terms[:keep].sum(), mag.sum(), 0.5 / n * (sig - 1.0), 0.5 / n * (sig + 1.0)


def g_loss32(z):
    v = np.asarray(z[:, 0], np.float32)
    w = f4(0.5) / f4(len(v))
    bce = ((np.maximum(v, f4(0)) - v).astype(f4) + np.log1p(np.exp(-np.abs(v)).astype(f4)).astype(f4)).astype(f4)
    with np.errstate(over='ignore'):
        sig = (f4(1) / (f4(1) + np.exp(-v).astype(f4)).astype(f4)).astype(f4)
    return block_sum32(strided32((w * bce).astype(f4))), (w * (sig - f4(1)).astype(f4)).astype(f4)


# ---------------------------------------------------------------------------------------------------------------- slab reduce
# n_split, t, c_pad, n_pad, c, n
SLAB_WIDE = [(512, 1, 32, 128, 27, 128), (40, 1, 32, 32, 5, 7), (33, 1, 32, 32, 5, 7),       # 33: per = 5, the ranges of lane groups 7 is empty
             (32, 1, 256, 256, 256, 256)]                                                   # total = 65536: the last size on the wide path
SLAB_NARROW = [(31, 1, 32, 32, 5, 7), (32, 1, 264, 256, 257, 256),                          # at the switch: 31 slabs; total = 65792
               (3, 25, 64, 32, 42, 3), (1, 9, 32, 32, 32, 32),
               (2, 9, 384, 320, 381, 307)]                                                  # total = 1 052 703 > 4096 x 256: the grid-stride wrap
SLAB_CASES = SLAB_WIDE + SLAB_NARROW


def slab_path(case):
    """the kernel tg_slab_reduce_f32 launches."""
    n_split, t, c_pad, n_pad, c, n = case
    return 'wide' if n_split >= 32 and t * c * n <= 65536 else 'narrow'


def slab_case(case):
    """slabs [n_split, t, c_pad, n_pad] of N(0,1), the last slab pushed 4 away from zero (the control drops it), NaN where c >= c_dim or
    n >= n_dim."""
    n_split, t, c_pad, n_pad, c, n = case
    rng = np.random.default_rng(n_split + c_pad)
    slab = rng.standard_normal((n_split, t, c_pad, n_pad)).astype(np.float32)
    slab[-1] += np.where(slab[-1] >= 0, 4, -4).astype(np.float32)
    slab[:, :, c:, :] = np.nan
    slab[:, :, :, n:] = np.nan
    return slab


def slab64(slab, c, n, drop_last=False):
    """(sum over the slabs, sum of their magnitudes) [t, c, n]; drop_last: without the last slab."""
    v = f8(slab[:len(slab) - 1 if drop_last else len(slab), :, :c, :n])
    return v.sum(axis=0), np.abs(f8(slab[:, :, :c, :n])).sum(axis=0)


def slab_narrow32(slab, c, n):
    """slab_reduce: slabs 0 .. n_split - 1 in order."""
    return seq_sum32([s[:, :c, :n] for s in slab])


def slab_wide_parts(slab, c, n):
    """slab_reduce_wide's 8 partial sums: contiguous ranges of ceil(n_split / 8) slabs, each summed in order from 0.f (an empty range stays
    0.f)."""
    n_split = len(slab)
    per = (n_split + 7) // 8
    parts = []
    for g in range(8):
        rng_ = [s[:, :c, :n] for s in slab[g * per:min(n_split, (g + 1) * per)]]
        parts.append(seq_sum32(rng_) if rng_ else np.zeros(slab.shape[1:2] + (c, n), np.float32))
    return parts


def slab_wide32(slab, c, n, order=range(8)):
    """slab_reduce_wide: the 8 partial sums added in index order starting from range 0 (order: another order, for the controls)."""
    parts = [slab_wide_parts(slab, c, n)[g] for g in order]
    return seq_sum32(parts[1:], init=parts[0])


def slab32(case, slab):
    n_split, t, c_pad, n_pad, c, n = case
    return (slab_wide32 if slab_path(case) == 'wide' else slab_narrow32)(slab, c, n)


def as_terms(bound):
    """a derived absolute bound (the penalty value's) as the sum|terms| that kernel_check.close / rejected multiply by TOL."""
    return bound / TOL
