"""NumPy float64 restatement of the generated-sample metrics: what tg_feature_moments_f32 accumulates, the covariance
tg.metrics.mean_cov makes of it, and the Fréchet distance by a route that shares no step with tg.metrics.frechet_distance (the
eigenvalues of the unsymmetric product C1 C2 instead of eigh of S C2 S)."""
import numpy as np

TOL_MOMENTS = 1e-12        # |got - ref| <= TOL_MOMENTS * sum |terms|: the only rounding is n - 1 fp64 additions of exact products, so the
                           # error is at most n 2^-53 of that sum, and n <= 4096 < 1e-12 * 2^53 = 9007 in every test
TOL_FD = 1e-6              # |got - ref| <= TOL_FD * (tr C1 + tr C2 + |m1 - m2|^2): the square root of a near-zero eigenvalue turns 1e-16 of
                           # relative noise into 1e-8


def moments64(f, c=None):
    """(sum [c], gram [c, c], sum |f| [c], sum |f_a||f_b| [c, c]) of the first c columns of f in float64."""
    x = np.asarray(f, np.float64)[:, :c]
    a = np.abs(x)
    return x.sum(axis=0), x.T @ x, a.sum(axis=0), a.T @ a


def mean_cov64(f):
    """(n, mean, np.cov) of the rows of f in float64."""
    x = np.asarray(f, np.float64)
    return x.shape[0], x.mean(axis=0), np.atleast_2d(np.cov(x, rowvar=False))


def frechet_eigvals(m1, C1, m2, C2):
    """|m1 - m2|^2 + tr C1 + tr C2 - 2 sum_i sqrt(max(Re lambda_i(C1 C2), 0))."""
    m1, m2, C1, C2 = (np.asarray(v, np.float64) for v in (m1, m2, C1, C2))
    lam = np.linalg.eigvals(C1 @ C2)
    d = m1 - m2
    return float(d @ d + np.trace(C1) + np.trace(C2) - 2.0 * np.sqrt(np.maximum(lam.real, 0.0)).sum())


def fd_scale(m1, C1, m2, C2):
    d = np.asarray(m1, np.float64) - np.asarray(m2, np.float64)
    return float(np.trace(C1) + np.trace(C2) + d @ d)


def to_bf16(x):
    """fp32 values rounded to bf16 (round to nearest even), as fp32: the negative control of the moments' bound."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)
