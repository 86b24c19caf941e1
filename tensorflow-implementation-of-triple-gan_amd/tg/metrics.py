"""Generated-sample metrics on classifier features (Train.sample_metrics): the host side of tg_feature_moments_f32
(include/tg_kernels.h, csrc/moments.hip) and the Fréchet distance between two Gaussians in NumPy float64.

The device adds up a feature matrix's column sums and Gram matrix in fp64, batch after batch; the host turns them into a mean and a
covariance once, at the end, and takes the distance — c x c eigenproblems, no scipy.  Importable without a device: torch and the HIP
library are touched only by FeatureMoments."""
import numpy as np

from . import lib

MAX_FEATURES = 512          # tg_feature_moments_f32 accepts 1 <= c <= 512


def mean_cov(n, total, gram):
    """(mean, cov) of n rows from their column sums and Gram matrix: cov = (gram - n mu mu^T) / (n - 1), symmetrised.  NaN for n < 2."""
    total, gram = np.asarray(total, np.float64), np.asarray(gram, np.float64)
    c = total.shape[0]
    if n < 2:
        return np.full(c, np.nan), np.full((c, c), np.nan)
    mu = total / n
    cov = (gram - n * np.outer(mu, mu)) / (n - 1)
    return mu, 0.5 * (cov + cov.T)


def _sqrtm_psd(a):
    """the symmetric square root of a symmetric matrix, negative eigenvalues (rounding of a rank-deficient covariance) clipped to 0."""
    w, v = np.linalg.eigh(0.5 * (a + a.T))
    return (v * np.sqrt(np.maximum(w, 0.0))) @ v.T


def frechet_distance(m1, C1, m2, C2):
    """|m1 - m2|^2 + tr C1 + tr C2 - 2 tr sqrt(C1 C2) between N(m1, C1) and N(m2, C2).  tr sqrt(C1 C2) = sum_i sqrt(max(lambda_i, 0)) over
    the eigenvalues of S C2 S, S the symmetric square root of C1: a symmetric positive semi-definite matrix with the spectrum of C1 C2,
    so eigh applies and nothing complex appears.  NaN in, NaN out."""
    m1, m2 = np.asarray(m1, np.float64), np.asarray(m2, np.float64)
    C1, C2 = np.asarray(C1, np.float64), np.asarray(C2, np.float64)
    if not (np.all(np.isfinite(m1)) and np.all(np.isfinite(m2)) and np.all(np.isfinite(C1)) and np.all(np.isfinite(C2))):
        return float('nan')
    s = _sqrtm_psd(C1)
    m = s @ C2 @ s
    lam = np.linalg.eigvalsh(0.5 * (m + m.T))
    d = m1 - m2
    return float(d @ d + np.trace(C1) + np.trace(C2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


class FeatureMoments(object):
    """streaming first and second moments of [n, c] fp32 feature batches on `device`: add() is one tg_feature_moments_f32 call into fp64
    device accumulators, result() one device->host copy.  The workspace grows to the largest batch seen and belongs to this object."""

    def __init__(self, c, device):
        import torch
        if not 1 <= int(c) <= MAX_FEATURES:
            raise ValueError("FeatureMoments: c must be in 1..%d, got %r" % (MAX_FEATURES, c))
        self.c, self.device, self.n = int(c), device, 0
        self.acc = torch.zeros(self.c + self.c * self.c, dtype=torch.float64, device=device)      # [sum | gram]: one copy to the host
        self.workspace = None

    def reset(self):
        self.n = 0
        self.acc.zero_()
        return self

    def add(self, act, stream=None):
        """act: an Act whose logical shape is [n, c] (h = w = 1), channel stride ld >= c; counts n."""
        import torch
        if act.h != 1 or act.w != 1 or act.c != self.c or act.dtype != 'f32':
            raise lib.TgError("FeatureMoments.add: an fp32 [n, %d] feature is needed, got [%d, %d, %d, %d] %s" % (self.c, act.n, act.h, act.w, act.c, act.dtype))
        need = lib.call('tg_feature_moments_workspace_bytes', act.n, self.c)
        if self.workspace is None or self.workspace.numel() * 8 < need:
            self.workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        if stream is None:
            stream = lib.cur_stream()
        lib.call('tg_feature_moments_f32', act.ptr, act.ld, act.n, self.c, lib.ptr(self.acc[:self.c]), lib.ptr(self.acc[self.c:]),
                 lib.ptr(self.workspace), self.workspace.numel() * 8, stream)
        self.n += act.n
        return self

    def sums(self):
        """(n, column sums [c], Gram matrix [c, c]) as float64 host arrays (synchronises)."""
        host = self.acc.cpu().numpy()
        return self.n, host[:self.c].copy(), host[self.c:].reshape(self.c, self.c).copy()

    def result(self):
        """(n, mean, cov) — mean_cov of what has been added."""
        n, total, gram = self.sums()
        return (n,) + mean_cov(n, total, gram)
