"""float64 NumPy restatement of tg_poly3_sums_f32 (include/tg_kernels.h, csrc/kernel_distance.hip) and of the unbiased kernel distance
built on it (tg.metrics.kid_from_sums / kernel_distance), with the tolerance the GPU tests hold the kernel to.

  poly3_sums(a, b, seg_a, seg_b, exclude_diag)   out[s] = sum over i in A_s, j in B_s of (<a_i, b_j> / c + 1)^3
  kid_from_sums(sxx, syy, sxy, m, n)             sxx / (m (m - 1)) + syy / (n (n - 1)) - 2 sxy / (m n), NaN where m < 2 or n < 2
  sum_bound(...)                                 per segment, with u = 2^-53, G = a b^T, A = |a| |b|^T, K = (G / c + 1)^3, P pairs:
        tol_s = 2 sum_ij u [3 (|G_ij| / c + 1)^2 A_ij + 4 |K_ij|]  +  P u sum_ij |K_ij|
     The first term is the first-order effect on K of a c-term fp64 dot product (|error| <= c u A, dK/dG = 3 t^2 / c) and of the cube's own
     roundings (the division, the + 1 and the two multiplies: 4 u |K|), doubled to cover the higher orders; the second is the worst case
     of adding P numbers in any order.  Nothing in it is measured: it holds for any correct implementation, whatever its order — and
     a dot product chained in fp32 falls outside it (tests/test_kernel_distance_reference.py).
Imports no torch and opens no device."""
import numpy as np

U64 = 2.0 ** -53

# (m, n, c, ld) of the kernel tests: ragged differently in rows and columns; one tile, several tiles, a channel tail, several chunks
SHAPES = ((1, 1, 1, 1), (5, 7, 3, 8), (65, 33, 5, 8), (257, 130, 33, 40), (64, 64, 128, 128), (1000, 777, 192, 200))


def features(rng, rows, c):
    """[rows, c] float32 rows shaped like a pooled post-ReLU feature with some spread around zero: max(0.7 N(0,1) + 0.4, 0) + 0.2 N(0,1)."""
    return (np.maximum(0.7 * rng.standard_normal((rows, c)) + 0.4, 0.0) + 0.2 * rng.standard_normal((rows, c))).astype(np.float32)


_INPUTS = {}


def inputs(shape):
    """(a [m, c], b [n, c]) of one of SHAPES: made once from a fixed seed, shared by the tests and read-only.  These are the inputs
    for which the fp32-chained control is asserted to miss the bound (test_kernel_distance_reference.py)."""
    if shape not in _INPUTS:
        m, n, c, _ = shape
        rng = np.random.default_rng(1)
        a, b = features(rng, m, c), features(rng, n, c)
        a.setflags(write=False), b.setflags(write=False)
        _INPUTS[shape] = (a, b)
    return _INPUTS[shape]


def padded(x, ld, fill=np.nan):
    """[rows, ld] float32: x in columns 0..c-1, `fill` in the padding columns the kernel must never read."""
    out = np.full((x.shape[0], ld), fill, np.float32)
    out[:, :x.shape[1]] = x
    return out


def _segments(seg_a, seg_b):
    sa, sb = np.asarray(seg_a, np.int64).reshape(-1), np.asarray(seg_b, np.int64).reshape(-1)
    assert sa.shape == sb.shape and sa.shape[0] >= 2 and (np.diff(sa) >= 0).all() and (np.diff(sb) >= 0).all()
    return sa, sb


def _kept(rows, cols, exclude_diag):
    """the pairs of a segment that enter its sum: all of them, or all but i == j (local indices)."""
    keep = np.ones((rows, cols), bool)
    if exclude_diag:
        d = np.arange(min(rows, cols))
        keep[d, d] = False
    return keep


def gram(a, b, dtype=np.float64):
    """a b^T accumulated in `dtype` (every fp32 x fp32 product is exact in float64 and wider)."""
    return np.asarray(a, dtype) @ np.asarray(b, dtype).T


def gram_f32_chain(a, b):
    """a b^T as an fp32 fma chain over ascending channels — what a kernel on the fp32 MFMA would accumulate — returned as float64."""
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((a32.shape[0], b32.shape[0]), np.float32)
    for ch in range(a32.shape[1]):
        acc = (acc.astype(np.float64) + np.outer(a32[:, ch].astype(np.float64), b32[:, ch].astype(np.float64))).astype(np.float32)
    return acc.astype(np.float64)


def poly3_sums(a, b, seg_a, seg_b, exclude_diag=False, gram_fn=gram):
    """float64 [nseg]; a, b: [., c] arrays (the logical columns only).  gram_fn: how the dot products are taken (controls)."""
    sa, sb = _segments(seg_a, seg_b)
    c = np.asarray(a).shape[1]
    out = np.zeros(sa.shape[0] - 1, np.float64)
    for s in range(out.shape[0]):
        A, B = a[sa[s]:sa[s + 1]], b[sb[s]:sb[s + 1]]
        if A.shape[0] == 0 or B.shape[0] == 0:
            continue
        G = gram_fn(A, B)
        t = G / float(c) + 1.0
        out[s] = float(((t * t) * t)[_kept(A.shape[0], B.shape[0], exclude_diag)].sum())
    return out


def poly3_sums_longdouble(a, b, seg_a, seg_b, exclude_diag=False):
    """the same sums with every operation in np.longdouble, returned as longdouble [nseg]."""
    sa, sb = _segments(seg_a, seg_b)
    c = np.longdouble(np.asarray(a).shape[1])
    out = np.zeros(sa.shape[0] - 1, np.longdouble)
    for s in range(out.shape[0]):
        A, B = np.asarray(a[sa[s]:sa[s + 1]], np.longdouble), np.asarray(b[sb[s]:sb[s + 1]], np.longdouble)
        if A.shape[0] == 0 or B.shape[0] == 0:
            continue
        G = (A[:, None, :] * B[None, :, :]).sum(axis=2)
        t = G / c + np.longdouble(1)
        out[s] = ((t * t) * t)[_kept(A.shape[0], B.shape[0], exclude_diag)].sum()
    return out


def sum_bound(a, b, seg_a, seg_b, exclude_diag=False):
    """float64 [nseg]: tol_s of the module docstring."""
    sa, sb = _segments(seg_a, seg_b)
    c = float(np.asarray(a).shape[1])
    out = np.zeros(sa.shape[0] - 1, np.float64)
    for s in range(out.shape[0]):
        A, B = np.asarray(a[sa[s]:sa[s + 1]], np.float64), np.asarray(b[sb[s]:sb[s + 1]], np.float64)
        if A.shape[0] == 0 or B.shape[0] == 0:
            continue
        keep = _kept(A.shape[0], B.shape[0], exclude_diag)
        G, Ab = A @ B.T, np.abs(A) @ np.abs(B).T
        K = np.abs((G / c + 1.0) ** 3)
        first = (U64 * (3.0 * (np.abs(G) / c + 1.0) ** 2 * Ab + 4.0 * K))[keep].sum()
        out[s] = 2.0 * first + float(keep.sum()) * U64 * K[keep].sum()
    return out


def kid_from_sums(sxx, syy, sxy, m, n):
    sxx, syy, sxy = (np.asarray(v, np.float64) for v in (sxx, syy, sxy))
    m, n = np.asarray(m, np.float64), np.asarray(n, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        val = sxx / (m * (m - 1.0)) + syy / (n * (n - 1.0)) - 2.0 * sxy / (m * n)
    return np.where((m >= 2) & (n >= 2), val, np.nan)


def kid_bound(tol_xx, tol_yy, tol_xy, m, n):
    """the bounds of the three sums propagated through kid_from_sums (its own few roundings are far below them)."""
    m, n = np.asarray(m, np.float64), np.asarray(n, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.asarray(tol_xx) / (m * (m - 1.0)) + np.asarray(tol_yy) / (n * (n - 1.0)) + 2.0 * np.asarray(tol_xy) / (m * n)


def class_segments(labels, num_classes):
    """(order: the rows in class order, stable; offsets [K + 1]) of host labels."""
    lab = np.asarray(labels, np.int64).reshape(-1)
    return np.argsort(lab, kind='stable'), np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=int(num_classes)))]).astype(np.int64)


def kernel_distance(real, fake, labels_real=None, labels_fake=None, num_classes=None, with_bound=False):
    """tg.metrics.kernel_distance on host rows -> its dict; with_bound: (dict, dict of the tolerances of 'kernel_distance' and
    'kernel_distance_per_class')."""
    real, fake = np.asarray(real, np.float32), np.asarray(fake, np.float32)
    m, n = real.shape[0], fake.shape[0]

    def three(r, f, sr, sf):
        sums = [poly3_sums(r, r, sr, sr, True), poly3_sums(f, f, sf, sf, True), poly3_sums(r, f, sr, sf, False)]
        tols = [sum_bound(r, r, sr, sr, True), sum_bound(f, f, sf, sf, True), sum_bound(r, f, sr, sf, False)]
        cm, cn = np.diff(sr), np.diff(sf)
        return kid_from_sums(sums[0], sums[1], sums[2], cm, cn), kid_bound(tols[0], tols[1], tols[2], cm, cn)

    val, tol = three(real, fake, [0, m], [0, n])
    out, bound = dict(kernel_distance=float(val[0])), dict(kernel_distance=float(tol[0]))
    if labels_real is not None:
        (o_r, s_r), (o_f, s_f) = class_segments(labels_real, num_classes), class_segments(labels_fake, num_classes)
        per, ptol = three(real[o_r], fake[o_f], s_r, s_f)
        has = ~np.isnan(per)
        k = int(np.argmax(np.where(has, per, -np.inf))) if has.any() else -1
        out.update(kernel_distance_per_class=per, kernel_distance_worst=float(per[k]) if k >= 0 else float('nan'), kernel_distance_worst_class=k)
        bound['kernel_distance_per_class'] = ptol
    return (out, bound) if with_bound else out
