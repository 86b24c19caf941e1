"""NumPy restatement of the k-nearest-neighbour manifold metrics: the fp32 distance chain of include/tg_kernels.h
(tg_knn_self_f32, tg_manifold_query_f32), a float64 distance, and the radii, query outputs and the four metrics — precision and recall
(Kynkäänniemi et al. 2019), density and coverage (Naeem et al. 2020) — computed from either.

The chain:  acc = 0; for ch = 0 .. c-1: d = a[ch] - b[ch]; p = d * d; acc = acc + p,  every operation rounded to fp32.  NumPy's float32
subtract, multiply and add are each correctly rounded and never fused, so a loop over channels on float32 arrays IS the chain, bit for
bit.  Its terms are non-negative: with u = 2^-24, d carries (1 + u), p = d * d (1 + u)^3 in all, and the c - 1 additions at most
(1 + u)^(c-1) more — within BOUND(c) = (c + 3) u of the exact value, relative."""
import numpy as np

U = 2.0 ** -24
KEYS = ('precision', 'recall', 'density', 'coverage')


def bound(c):
    """relative error bound of the fp32 chain over c channels."""
    return (c + 3) * U


def d2_chain32(a, b):
    """[m, n] float32: the chain between every row of a [m, c] and every row of b [n, c], channel after channel."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for ch in range(a.shape[1]):
        d = a[:, ch, None] - b[None, :, ch]
        p = d * d
        acc = acc + p
        assert d.dtype == p.dtype == acc.dtype == np.float32
    return acc


def d2_f64(a, b):
    """[m, n] float64 squared distances, difference form, accumulated in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float64)
    for ch in range(a.shape[1]):
        d = a[:, ch, None] - b[None, :, ch]
        acc += d * d
    return acc


def d2_gram32(a, b):
    """[m, n] float32: |a|^2 + |b|^2 - 2 a.b with every intermediate in fp32 — the form a GEMM would compute (negative control)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    aa, bb = (a * a).sum(axis=1, dtype=np.float32), (b * b).sum(axis=1, dtype=np.float32)
    return (aa[:, None] + bb[None, :]) - np.float32(2) * (a @ b.T)


def to_bf16(x):
    """float32 -> nearest-even bf16, returned as float32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def within_bound(d, d64, c):
    """every entry of d within BOUND(c) of d64, relative."""
    return bool((np.abs(np.asarray(d, np.float64) - d64) <= bound(c) * d64).all())


def features(n, c, ld, seed, offset=0.75):
    """[n, ld] float32: normal values with a non-zero mean in columns 0..c-1, NaN in the padding columns (a single read of one would
    poison an output)."""
    rng = np.random.default_rng(seed)
    f = np.full((n, ld), np.nan, np.float32)
    f[:, :c] = (rng.standard_normal((n, c)) * 1.5 + offset).astype(np.float32)
    return f


def knn_self(x, k, dist=d2_chain32):
    """[n, k]: the k smallest dist(x_i, x_j) over j != i, ascending.  The row itself is left out by index: a duplicate contributes 0."""
    d = np.array(dist(x, x))
    d[np.arange(d.shape[0]), np.arange(d.shape[0])] = np.inf
    return np.sort(d, axis=1)[:, :k]


def radii(x, k, dist=d2_chain32):
    """[n]: the squared distance of every row to its k-th nearest other row."""
    return knn_self(x, k, dist)[:, k - 1]


def query(q, r, r2=None, dist=d2_chain32):
    """(count [m] int32 or None, nn_d2 [m], nn_idx [m] int32) of every row of q against the rows of r: how many r_j have
    dist(q_i, r_j) <= r2[j], the smallest distance, and the lowest j attaining it."""
    d = dist(q, r)
    idx = np.argmin(d, axis=1).astype(np.int32)                 # the first occurrence
    count = None if r2 is None else (d <= np.asarray(r2)[None, :]).sum(axis=1).astype(np.int32)
    return count, d[np.arange(d.shape[0]), idx], idx


def from_counts(k, n_real, n_fake, count_fr, count_rf, nn_rf, r2_real):
    """the four numbers from the query outputs (fake -> real counts, real -> fake counts and nearest distances) in float64."""
    return dict(precision=float(np.mean(np.asarray(count_fr) > 0)),
                recall=float(np.mean(np.asarray(count_rf) > 0)),
                density=float(np.asarray(count_fr, np.float64).sum() / (float(k) * n_fake)),
                coverage=float(np.mean(np.asarray(nn_rf) <= np.asarray(r2_real))))


def metrics(real, fake, k, dist=d2_chain32):
    """{precision, recall, density, coverage} of fake [n_fake, c] against real [n_real, c]; all NaN with fewer than k + 1 rows on a side."""
    real, fake = np.asarray(real), np.asarray(fake)
    if real.shape[0] < k + 1 or fake.shape[0] < k + 1:
        return dict.fromkeys(KEYS, float('nan'))
    r2_real, r2_fake = radii(real, k, dist), radii(fake, k, dist)
    count_fr, _, _ = query(fake, real, r2_real, dist)
    count_rf, nn_rf, _ = query(real, fake, r2_fake, dist)
    return from_counts(k, real.shape[0], fake.shape[0], count_fr, count_rf, nn_rf, r2_real)
