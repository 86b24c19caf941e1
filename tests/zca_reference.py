"""Float64 restatement of the ZCA fit, computed directly from the images as the classifier sees them (x/255*2-1,
Input_Pipeline/cifar10Dataset.py:60): mean over the images, the biased covariance of the centred images, eigh, eigenvalues clipped at 0,
mat = U diag((s + eps)^-1/2) U^T.  Shared by tests/test_zca_fit.py and tests/test_gpu_zca_fit.py."""
import numpy as np


def scaled(images_u8):
    """uint8 [n, ...] -> float64 [n, d] in [-1, 1], NHWC flatten order."""
    x = np.asarray(images_u8, np.uint8).reshape(len(images_u8), -1).astype(np.float64)
    return x / 255 * 2 - 1


def covariance(images_u8):
    x = scaled(images_u8)
    xc = x - x.mean(0)
    return xc.T @ xc / x.shape[0]


def zca(images_u8, eps=1e-5):
    """(mean [d], mat [d, d], cov [d, d], s [d]) in float64; s are the clipped eigenvalues of cov."""
    x = scaled(images_u8)
    mean = x.mean(0)
    xc = x - mean
    cov = xc.T @ xc / x.shape[0]
    s, u = np.linalg.eigh(cov)
    s = np.maximum(s, 0.0)
    mat = (u * (s + eps) ** -0.5) @ u.T
    return mean, mat, cov, s


def int_moments(images_u8, rows=8192):
    """(n, S', G') of x' = x - 128 in exact integer arithmetic: float64 BLAS over integer values whose every partial sum is an integer
    below 2^53, accumulated chunk by chunk into int64."""
    x = np.asarray(images_u8, np.uint8).reshape(len(images_u8), -1)
    n, d = x.shape
    g = np.zeros((d, d), np.int64)
    s = np.zeros(d, np.int64)
    for a in range(0, n, rows):
        xp = x[a:a + rows].astype(np.float64) - 128.0
        g += (xp.T @ xp).astype(np.int64)
        s += xp.sum(0).astype(np.int64)
    return n, s, g


def whitening_eigenvalues(s, eps=1e-5):
    """the eigenvalues of mat · cov · mat, ascending: s / (s + eps)."""
    return np.sort(s / (s + eps))
