"""Generated-sample metrics on classifier features (Train.sample_metrics): the host side of tg_feature_moments_f32
(include/tg_kernels.h, csrc/moments.hip) and the Fréchet distance between two Gaussians in NumPy float64; the host side of
tg_knn_self_f32 / tg_manifold_query_f32 (csrc/knn.hip) and the k-nearest-neighbour precision, recall, density and coverage.  And the
classifier's own evaluation report (Train.evaluate_report): the host side of tg_eval_report_f32 (csrc/evalreport.hip) —
ClassifierReport — and the algebra on its counts, report_from_counts.  And the nearest training images of generated samples in pixel
space (Train.nearest_training): PixelBank and nearest_pixels, the host side of tg_nearest_u8_i32 / tg_f32_quantize_u8
(csrc/nearest.hip).  And the unbiased kernel distance of generated samples, whole-set and per class (Train.sample_kernel_distance,
DESIGN §9.14): poly3_sums, the host side of tg_poly3_sums_f32 (csrc/kernel_distance.hip), kid_from_sums and kernel_distance.

The device adds up a feature matrix's column sums and Gram matrix in fp64, batch after batch; the host turns them into a mean and a
covariance once, at the end, and takes the distance — c x c eigenproblems, no scipy.  Importable without a device: torch and the HIP
library are touched only by FeatureMoments, FeatureBank, manifold_metrics, poly3_sums, kernel_distance, ClassifierReport, PixelBank and nearest_pixels."""
import numpy as np

from . import lib

MAX_FEATURES = 512          # tg_feature_moments_f32, tg_knn_self_f32, tg_manifold_query_f32 and tg_poly3_sums_f32 accept 1 <= c <= 512
MAX_K = 16                  # tg_knn_self_f32 accepts 1 <= k <= 16
MANIFOLD_KEYS = ('precision', 'recall', 'density', 'coverage')


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


def check_k(k, what='k'):
    """the k of the k-nearest-neighbour radii: an int in 1..MAX_K (what tg_knn_self_f32 accepts), not a bool -> int.  ValueError
    otherwise, naming `what`.  The one check of it: options.check_sample_manifold_k, Train.sample_manifold_metrics and
    manifold_metrics all come here."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise ValueError("%s must be an integer in 1..%d, got %r" % (what, MAX_K, k))
    return int(k)


class FeatureBank(object):
    """the [n, c] fp32 feature rows of a pass, dense on `device`, for the k-nearest-neighbour kernels: add() is one tg_copy2d_f32 launch
    behind the rows already there.  The buffer grows by re-allocation (doubling), which a hipGraph capture or a launch-plan recording
    must not see: add() refuses to run inside one."""

    def __init__(self, c, device):
        if not 1 <= int(c) <= MAX_FEATURES:
            raise ValueError("FeatureBank: c must be in 1..%d, got %r" % (MAX_FEATURES, c))
        self.c, self.device, self.n = int(c), device, 0
        self.buf = None

    def reset(self):
        self.n = 0
        return self

    def _reserve(self, rows):
        import torch
        have = 0 if self.buf is None else self.buf.numel() // self.c
        if rows <= have:
            return
        grown = torch.empty(max(rows, 2 * have, 256) * self.c, dtype=torch.float32, device=self.device)
        if self.n:
            grown[:self.n * self.c].copy_(self.buf[:self.n * self.c])
        self.buf = grown

    def add(self, act, stream=None):
        """act: an Act whose logical shape is [n, c] (h = w = 1), channel stride ld >= c; its padding columns are not copied."""
        import torch
        if act.h != 1 or act.w != 1 or act.c != self.c or act.dtype != 'f32':
            raise lib.TgError("FeatureBank.add: an fp32 [n, %d] feature is needed, got [%d, %d, %d, %d] %s" % (self.c, act.n, act.h, act.w, act.c, act.dtype))
        if lib._recorder is not None or torch.cuda.is_current_stream_capturing():
            raise lib.TgError("FeatureBank.add: called inside a hipGraph capture / launch-plan recording; the bank re-allocates as it grows")
        if act.n == 0:
            return self
        self._reserve(self.n + act.n)
        if stream is None:
            stream = lib.cur_stream()
        lib.call('tg_copy2d_f32', act.ptr, act.ld, lib.ptr(self.buf[self.n * self.c:]), self.c, act.n, self.c, stream)
        self.n += act.n
        return self

    def rows(self):
        """the [n, c] device tensor of what has been added (a view of the buffer)."""
        import torch
        if self.buf is None:
            return torch.empty((0, self.c), dtype=torch.float32, device=self.device)
        return self.buf[:self.n * self.c].view(self.n, self.c)

    def numpy(self):
        """the rows as a host [n, c] float32 array (synchronises)."""
        return self.rows().cpu().numpy().copy()


def knn_self(x, k, stream=None):
    """x: [n, c] dense fp32 device tensor -> [n, k] device tensor of tg_knn_self_f32: every row's k smallest squared distances to the
    other rows, ascending."""
    import torch
    n, c = x.shape
    need = lib.call('tg_knn_self_workspace_bytes', n, k)
    work = torch.empty(max((need + 3) // 4, 4), dtype=torch.float32, device=x.device)
    out = torch.empty((n, k), dtype=torch.float32, device=x.device)
    lib.call('tg_knn_self_f32', lib.ptr(x), c, n, c, k, lib.ptr(out), lib.ptr(work), work.numel() * 4, lib.cur_stream() if stream is None else stream)
    return out


def manifold_query(q, r, r2=None, stream=None):
    """q [m, c], r [n, c] dense fp32 device tensors, r2 [n] or None -> (count int32 [m] or None, nn_d2 [m], nn_idx int32 [m]) device
    tensors of tg_manifold_query_f32."""
    import torch
    (m, c), n = q.shape, r.shape[0]
    need = lib.call('tg_manifold_query_workspace_bytes', m, n)
    work = torch.empty(max((need + 3) // 4, 4), dtype=torch.float32, device=q.device)
    count = None if r2 is None else torch.empty(m, dtype=torch.int32, device=q.device)
    nn_d2 = torch.empty(m, dtype=torch.float32, device=q.device)
    nn_idx = torch.empty(m, dtype=torch.int32, device=q.device)
    lib.call('tg_manifold_query_f32', lib.ptr(q), c, m, lib.ptr(r), c, n, c, lib.ptr(r2), lib.ptr(count), lib.ptr(nn_d2), lib.ptr(nn_idx),
             lib.ptr(work), work.numel() * 4, lib.cur_stream() if stream is None else stream)
    return count, nn_d2, nn_idx


def manifold_from_counts(k, n_fake, count_fr, count_rf, nn_rf, r2_real):
    """{precision, recall, density, coverage} from the query outputs, reduced in float64 on the host: count_fr [n_fake] the reals whose
    ball holds fake i, count_rf [n_real] the fakes whose ball holds real j, nn_rf [n_real] real j's squared distance to its nearest fake,
    r2_real [n_real] the reals' squared radii."""
    count_fr, count_rf = np.asarray(count_fr), np.asarray(count_rf)
    return dict(precision=float(np.mean(count_fr > 0)), recall=float(np.mean(count_rf > 0)),
                density=float(count_fr.astype(np.float64).sum() / (float(k) * n_fake)),
                coverage=float(np.mean(np.asarray(nn_rf) <= np.asarray(r2_real))))


def manifold_metrics(real_bank, fake_bank, k, stream=None):
    """k-nearest-neighbour precision and recall (Kynkäänniemi et al. 2019) and density and coverage (Naeem et al. 2020) of the fake
    bank's rows against the real bank's.  A row's ball has the squared radius of its k-th nearest other row of its own
    side (tg_knn_self_f32, twice); fake -> real and real -> fake queries (tg_manifold_query_f32, twice) count the balls a row falls in:
      precision  the share of fakes inside some real ball          recall    the share of reals inside some fake ball
      density    the real balls a fake falls in, over k, averaged   coverage  the share of reals whose nearest fake is inside their own ball
    Every distance is the fp32 chain of include/tg_kernels.h, so the four numbers are reproducible exactly.  All NaN when either side
    has fewer than k + 1 rows (no launch).  stream: the stream the four launches go to — the current torch stream (the default), or one
    ordered with it: the buffers are allocated and the results copied back on the current torch stream.  Synchronises."""
    k = check_k(k, 'manifold_metrics: k')
    if real_bank.c != fake_bank.c:
        raise ValueError("manifold_metrics: the banks hold features of different widths (%d, %d)" % (real_bank.c, fake_bank.c))
    if real_bank.n < k + 1 or fake_bank.n < k + 1:
        return dict.fromkeys(MANIFOLD_KEYS, float('nan'))
    real, fake = real_bank.rows(), fake_bank.rows()
    r2_real = knn_self(real, k, stream)[:, k - 1].contiguous()
    r2_fake = knn_self(fake, k, stream)[:, k - 1].contiguous()
    count_fr, _, _ = manifold_query(fake, real, r2_real, stream)
    count_rf, nn_rf, _ = manifold_query(real, fake, r2_fake, stream)
    return manifold_from_counts(k, fake_bank.n, count_fr.cpu().numpy(), count_rf.cpu().numpy(), nn_rf.cpu().numpy(), r2_real.cpu().numpy())


# ---- the unbiased kernel distance of generated samples, whole-set and per class (Train.sample_kernel_distance) -----------
KERNEL_DISTANCE_KEYS = ('kernel_distance', 'kernel_distance_per_class', 'kernel_distance_worst', 'kernel_distance_worst_class')
MAX_SEGMENTS = 1024         # tg_poly3_sums_f32 accepts 1 <= nseg <= 1024


def poly3_sums(a, b, seg_a, seg_b, exclude_diag, stream=None):
    """a [., c], b [., c] dense fp32 device tensors; seg_a, seg_b: nseg + 1 non-decreasing row offsets each (host) -> float64 NumPy
    [nseg] of tg_poly3_sums_f32: out[s] = the sum over rows i of a in [seg_a[s], seg_a[s+1]) and j of b in [seg_b[s], seg_b[s+1]) of
    (<a_i, b_j> / c + 1)^3 in fp64, with exclude_diag without the pairs i - seg_a[s] == j - seg_b[s].  The offsets must lie inside
    the tensors (ValueError otherwise).  An eager launch sequence: refused inside a hipGraph capture / launch-plan recording.
    Synchronises."""
    import ctypes as C
    import torch
    if lib._recorder is not None or torch.cuda.is_current_stream_capturing():
        raise lib.TgError("poly3_sums: called inside a hipGraph capture / launch-plan recording; the segment map is copied from the host")
    sa, sb = np.asarray(seg_a, np.int64).reshape(-1), np.asarray(seg_b, np.int64).reshape(-1)
    nseg = sa.shape[0] - 1
    if sb.shape[0] != sa.shape[0] or not 1 <= nseg <= MAX_SEGMENTS:
        raise ValueError("poly3_sums: seg_a and seg_b must hold nseg + 1 offsets each, 1 <= nseg <= %d (got %d and %d entries)"
                         % (MAX_SEGMENTS, sa.shape[0], sb.shape[0]))
    for what, t, seg in (('a', a, sa), ('b', b, sb)):
        if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("poly3_sums: %s must be a contiguous [n, c] float32 tensor, got %s %s" % (what, tuple(t.shape), t.dtype))
        if seg[0] < 0 or seg[-1] > t.shape[0] or (np.diff(seg) < 0).any():
            raise ValueError("poly3_sums: seg_%s must be non-decreasing offsets inside the %d rows of %s, got %r" % (what, t.shape[0], what, seg.tolist()))
    c = int(a.shape[1])
    if int(b.shape[1]) != c or not 1 <= c <= MAX_FEATURES:
        raise ValueError("poly3_sums: a and b must share a width in 1..%d, got %d and %d" % (MAX_FEATURES, c, int(b.shape[1])))
    ca, cb = (C.c_int32 * (nseg + 1))(*sa.tolist()), (C.c_int32 * (nseg + 1))(*sb.tolist())
    need = lib.call('tg_poly3_sums_workspace_bytes', ca, cb, nseg)
    work = torch.empty(max((need + 7) // 8, 2), dtype=torch.float64, device=a.device)
    out = torch.empty(nseg, dtype=torch.float64, device=a.device)
    # a tensor without rows has no storage to point at; the kernel never follows the pointer of a side whose segments are all empty
    pa, pb = (lib.ptr(t if t.shape[0] else work) for t in (a, b))
    lib.call('tg_poly3_sums_f32', pa, c, pb, c, c, ca, cb, nseg, int(bool(exclude_diag)), lib.ptr(out), lib.ptr(work), work.numel() * 8,
             lib.cur_stream() if stream is None else stream)
    return out.cpu().numpy()


def kid_from_sums(sxx, syy, sxy, m, n):
    """the unbiased estimator of MMD^2 from the kernel sums, elementwise in float64:
        sxx / (m (m - 1)) + syy / (n (n - 1)) - 2 sxy / (m n)
    sxx, syy: the sums over the ordered pairs i != j of one side (m rows, n rows), sxy: the sum over all m n cross pairs.  NaN where
    m < 2 or n < 2.  No device work."""
    sxx, syy, sxy = (np.asarray(v, np.float64) for v in (sxx, syy, sxy))
    m, n = np.asarray(m, np.float64), np.asarray(n, np.float64)
    ok = (m >= 2) & (n >= 2)
    ms, ns = np.where(ok, m, 2.0), np.where(ok, n, 2.0)
    val = sxx / (ms * (ms - 1.0)) + syy / (ns * (ns - 1.0)) - 2.0 * sxy / (ms * ns)
    return np.where(ok, val, np.nan)


def class_order(labels, num_classes):
    """host labels [n] -> (order int64 [n]: the rows in class order, a stable sort; offsets int64 [K + 1] of the classes in it).
    ValueError for a label outside 0..K-1."""
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    K = int(num_classes)
    if lab.size and (lab.min() < 0 or lab.max() >= K):
        raise ValueError("kernel_distance: labels must lie in 0..%d, got %d..%d" % (K - 1, lab.min(), lab.max()))
    return np.argsort(lab, kind='stable'), np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=K))]).astype(np.int64)


def worst_of(per_class):
    """(the largest non-NaN entry, the lowest index attaining it) of a per-class array; (NaN, -1) when every entry is NaN."""
    v = np.asarray(per_class, np.float64)
    if not (~np.isnan(v)).any():
        return float('nan'), -1
    k = int(np.argmax(np.where(np.isnan(v), -np.inf, v)))
    return float(v[k]), k


def kernel_distance(real_bank, fake_bank, labels_real=None, labels_fake=None, num_classes=None, stream=None):
    """The unbiased cubic-kernel MMD^2 ("Kernel Inception Distance", Binkowski et al. 2018) between the rows of two FeatureBanks
     -> dict(kernel_distance=...): kid_from_sums of three one-segment tg_poly3_sums_f32 calls — real x real and
    fake x fake without their diagonals, real x fake — on the banks as they are, so the number is the same bits whether or not labels
    are given.  NaN (no launch) with fewer than two rows on either side.
    labels_real, labels_fake (host integer arrays, one label per bank row) and num_classes = K add
      kernel_distance_per_class    float64 [K]: the same estimator between the rows of each class, from three K-segment calls on the
                                   rows gathered into class order (a stable sort of the labels and index_select on the bank: buffer
                                   plumbing, no arithmetic); NaN where a class has fewer than two rows on either side
      kernel_distance_worst        its largest non-NaN entry (NaN if there is none)
      kernel_distance_worst_class  the lowest index attaining it (-1 if there is none)
    Unbiased at any sample count — which is what keeps it meaningful per class — and therefore possibly negative.  stream: as
    manifold_metrics.  Synchronises."""
    import torch
    if real_bank.c != fake_bank.c:
        raise ValueError("kernel_distance: the banks hold features of different widths (%d, %d)" % (real_bank.c, fake_bank.c))
    if (labels_real is None) != (labels_fake is None):
        raise ValueError("kernel_distance: give the labels of both sides or of neither")
    real, fake = real_bank.rows(), fake_bank.rows()
    m, n = int(real.shape[0]), int(fake.shape[0])
    out = dict(kernel_distance=float('nan'))
    if m >= 2 and n >= 2:
        sxx = poly3_sums(real, real, [0, m], [0, m], True, stream)
        syy = poly3_sums(fake, fake, [0, n], [0, n], True, stream)
        sxy = poly3_sums(real, fake, [0, m], [0, n], False, stream)
        out['kernel_distance'] = float(kid_from_sums(sxx, syy, sxy, m, n)[0])
    if labels_real is None:
        return out
    if num_classes is None or not 1 <= int(num_classes) <= MAX_SEGMENTS:
        raise ValueError("kernel_distance: with labels, num_classes must be in 1..%d, got %r" % (MAX_SEGMENTS, num_classes))
    K = int(num_classes)
    if np.size(labels_real) != m or np.size(labels_fake) != n:
        raise ValueError("kernel_distance: %d / %d labels for %d / %d rows" % (np.size(labels_real), np.size(labels_fake), m, n))
    (ord_r, off_r), (ord_f, off_f) = class_order(labels_real, K), class_order(labels_fake, K)
    cm, cn = np.diff(off_r), np.diff(off_f)
    per = np.full(K, np.nan)
    if m and n and ((cm >= 2) & (cn >= 2)).any():
        rs = real.index_select(0, torch.from_numpy(ord_r).to(real.device))
        fs = fake.index_select(0, torch.from_numpy(ord_f).to(fake.device))
        per = kid_from_sums(poly3_sums(rs, rs, off_r, off_r, True, stream), poly3_sums(fs, fs, off_f, off_f, True, stream),
                            poly3_sums(rs, fs, off_r, off_f, False, stream), cm, cn)
    worst, which = worst_of(per)
    out.update(kernel_distance_per_class=per, kernel_distance_worst=worst, kernel_distance_worst_class=which)
    return out


# ---- the nearest training images of generated samples, in pixel space (Train.nearest_training) ----------------------------
MAX_PIXELS = 16384          # tg_nearest_u8_i32 accepts 1 <= d <= 16 384 (255^2 d stays below 2^31)
PIXEL_STAGE = 16384         # rows per pinned staging copy of PixelBank.add_u8


class PixelBank(object):
    """growing [n, d] uint8 image rows, dense on `device`, for tg_nearest_u8_i32: add_u8() copies host bytes through pinned staging,
    add_act() quantises an fp32 image batch back to the input pipeline's bytes (tg_f32_quantize_u8).  The buffer grows by
    re-allocation (doubling), which a hipGraph capture or a launch-plan recording must not see: both refuse to run inside one."""

    def __init__(self, d, device):
        if not 1 <= int(d) <= MAX_PIXELS:
            raise ValueError("PixelBank: d must be in 1..%d, got %r" % (MAX_PIXELS, d))
        self.d, self.device, self.n = int(d), device, 0
        self.buf = None

    def reset(self):
        self.n = 0
        return self

    def _reserve(self, rows):
        import torch
        if lib._recorder is not None or torch.cuda.is_current_stream_capturing():
            raise lib.TgError("PixelBank: called inside a hipGraph capture / launch-plan recording; the bank re-allocates as it grows")
        have = 0 if self.buf is None else self.buf.numel() // self.d
        if rows <= have:
            return
        grown = torch.empty(max(rows, 2 * have, 64) * self.d, dtype=torch.uint8, device=self.device)
        if self.n:
            grown[:self.n * self.d].copy_(self.buf[:self.n * self.d])
        self.buf = grown

    def add_u8(self, rows):
        """rows: a host uint8 array of n * d values (any shape whose rows flatten to d) -> copied behind the rows already there."""
        import torch
        a = np.ascontiguousarray(rows, np.uint8).reshape(-1, self.d)
        self._reserve(self.n + a.shape[0])
        for s in range(0, a.shape[0], PIXEL_STAGE):
            part = a[s:s + PIXEL_STAGE]
            stage = torch.from_numpy(part).pin_memory()
            self.buf[(self.n + s) * self.d:(self.n + s + part.shape[0]) * self.d].copy_(stage.reshape(-1), non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()         # the staging buffers are released with this call
        self.n += a.shape[0]
        return self

    def add_records(self, chunks, n_threads=4):
        """chunks: (tg.io.RecordFile, record indices) pieces, e.g. Input_Pipeline.tfrecordDataset.training_chunks — every piece is
        decoded straight into one pinned staging buffer and copied behind the rows already there -> the records' labels, int32 [n]."""
        import torch
        labels, stage = [], None
        for rec, idx in chunks:
            m = len(idx)
            if int(np.prod(rec.shape)) != self.d:
                raise lib.TgError("PixelBank.add_records: %s holds images of shape %r, the bank rows of %d values" % (rec.path, rec.shape, self.d))
            if stage is None or stage.numel() < m * self.d:
                stage = torch.empty(m * self.d, dtype=torch.uint8).pin_memory()
            lab = np.empty(m, np.int32)
            rec.gather(idx, stage.numpy(), lab, n_threads=n_threads)
            self._reserve(self.n + m)
            self.buf[self.n * self.d:(self.n + m) * self.d].copy_(stage[:m * self.d], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()      # the staging buffer is refilled by the next piece
            self.n += m
            labels.append(lab)
        return np.concatenate(labels) if labels else np.zeros(0, np.int32)

    def add_act(self, act, scale, shift, stream=None):
        """act: an fp32 image Act of h * w * c == d values per row, in the scaling x = u / 255 * scale + shift; padding channels
        (ld > c) are dropped by one tg_copy2d_f32 launch first."""
        import torch
        if act.dtype != 'f32' or act.h * act.w * act.c != self.d:
            raise lib.TgError("PixelBank.add_act: fp32 images of %d values are needed, got [%d, %d, %d, %d] %s"
                              % (self.d, act.n, act.h, act.w, act.c, act.dtype))
        if act.n == 0:
            return self
        self._reserve(self.n + act.n)
        stream = lib.cur_stream() if stream is None else stream
        src = act.ptr
        if act.ld != act.c:
            dense = torch.empty(act.n * self.d, dtype=torch.float32, device=self.device)
            lib.call('tg_copy2d_f32', act.ptr, act.ld, lib.ptr(dense), act.c, act.n * act.h * act.w, act.c, stream)
            src = lib.ptr(dense)
        lib.call('tg_f32_quantize_u8', src, lib.ptr(self.buf[self.n * self.d:]), act.n * self.d, float(scale), float(shift), stream)
        self.n += act.n
        return self

    def rows(self, lo=0, hi=None):
        """the [hi - lo, d] device tensor of rows lo..hi (a view of the buffer; hi None: all that has been added)."""
        import torch
        hi = self.n if hi is None else hi
        if self.buf is None:
            return torch.empty((0, self.d), dtype=torch.uint8, device=self.device)
        return self.buf[lo * self.d:hi * self.d].view(hi - lo, self.d)

    def numpy(self):
        """the rows as a host [n, d] uint8 array (synchronises)."""
        return self.rows().cpu().numpy().copy()


def nearest_pixels(query_bank, ref, k, stream=None):
    """the k nearest rows of a reference set for every row of `query_bank` (PixelBank) -> (d2 int32 [m, k], idx int32 [m, k]) device
    tensors of tg_nearest_u8_i32: exact integer squared distances, the smaller first, on a tie the lower index; (INT32_MAX, -1) where
    the set has fewer than k rows.  ref: a PixelBank (one call), or an iterable of (base, [n, d] uint8 device tensor) chunks — one call
    per chunk, merging from the second on; the answer depends neither on the chunking nor on the order of the chunks."""
    import torch
    k = check_k(k, 'nearest_pixels: k')
    m, d = query_bank.n, query_bank.d
    if m < 1:
        raise ValueError("nearest_pixels: the query bank is empty")
    chunks = [(0, ref.rows())] if isinstance(ref, PixelBank) else ref
    q = query_bank.rows()
    best_d2 = torch.empty((m, k), dtype=torch.int32, device=q.device)
    best_idx = torch.empty((m, k), dtype=torch.int32, device=q.device)
    stream = lib.cur_stream() if stream is None else stream
    work, calls = None, 0
    for base, rows in chunks:
        n = int(rows.shape[0])
        if n == 0:
            continue
        if rows.dtype != torch.uint8 or rows.shape[1] != d or not rows.is_contiguous():
            raise ValueError("nearest_pixels: a chunk must be a contiguous [n, %d] uint8 tensor, got %s %s" % (d, tuple(rows.shape), rows.dtype))
        need = lib.call('tg_nearest_u8_workspace_bytes', m, n, d, k)
        if work is None or work.numel() * 8 < need:
            work = torch.empty(max((need + 7) // 8, 2), dtype=torch.int64, device=q.device)
        lib.call('tg_nearest_u8_i32', lib.ptr(q), m, lib.ptr(rows), n, d, k, int(base), int(calls > 0), lib.ptr(best_d2), lib.ptr(best_idx),
                 lib.ptr(work), work.numel() * 8, stream)
        calls += 1
    if calls == 0:
        raise ValueError("nearest_pixels: the reference set is empty")
    return best_d2, best_idx


def nearest_rmse(nn_d2, d):
    """[m] float64: sqrt(d2 of the nearest row / d) / 255 — the root-mean-square pixel difference in units of the full range."""
    return np.sqrt(np.asarray(nn_d2, np.int64).reshape(len(nn_d2), -1)[:, 0].astype(np.float64) / float(d)) / 255.0


# ---- the per-class evaluation report of the classifier (Train.evaluate_report) ------------------------------------------
MAX_CLASSES = 1024          # tg_eval_report_f32 accepts 2 <= k <= 1024 (Training/options.NUM_CLASSES_RANGE),
MAX_RANKS = 32              # 1 <= nr <= 32 rank-histogram entries
MAX_BINS = 64               # and 1 <= nb <= 64 calibration bins
REPORT_SCALARS = ('n', 'n_nonfinite', 'accuracy', 'top5_accuracy', 'nll', 'brier', 'ece', 'balanced_accuracy', 'macro_f1',
                  'worst_class_recall', 'worst_class', 'predicted_class_entropy')
REPORT_ARRAYS = ('support', 'predicted', 'recall', 'precision', 'f1')


class ClassifierReport(object):
    """streaming counts of [n, k] logit batches against their labels on `device`: add() is one tg_eval_report_f32 call into the device
    accumulators — the int64 confusion matrix [k, k], rank histogram [ranks], calibration bin counts and hits [bins], the non-finite
    row count, and the fp64 confidence sums [bins] and {NLL, Brier} sums — counts() one device->host copy of all of them.  ranks is
    clipped to min(ranks, num_classes).  The workspace grows to the largest batch seen and belongs to this object."""

    def __init__(self, num_classes, device, ranks=16, bins=15):
        import torch
        k = int(num_classes)
        if not 2 <= k <= MAX_CLASSES:
            raise ValueError("ClassifierReport: num_classes must be in 2..%d, got %r" % (MAX_CLASSES, num_classes))
        if not 1 <= int(ranks) <= MAX_RANKS or not 1 <= int(bins) <= MAX_BINS:
            raise ValueError("ClassifierReport: ranks must be in 1..%d and bins in 1..%d, got %r and %r" % (MAX_RANKS, MAX_BINS, ranks, bins))
        self.k, self.device, self.ranks, self.bins, self.n = k, device, min(int(ranks), k), int(bins), 0
        # one buffer of 8-byte words, so that counts() is one copy: int64 [confusion | rank_hist | bin_count | bin_correct | nonfinite],
        # then the same storage read as fp64 [bin_conf | sums]
        sizes = (k * k, self.ranks, self.bins, self.bins, 1, self.bins, 2)
        self._off = tuple(int(v) for v in np.concatenate([[0], np.cumsum(sizes)]))
        self.acc = torch.zeros(self._off[-1], dtype=torch.int64, device=device)
        self.workspace = None

    def reset(self):
        self.n = 0
        self.acc.zero_()
        return self

    def _part(self, i):
        return self.acc[self._off[i]:self._off[i + 1]]

    def add(self, labels, logits, stream=None):
        """labels, logits: Acts whose logical shape is [n, k] (h = w = 1), channel strides >= k; the arg-max of both is taken in the
        kernel, as tg_accuracy_count_f32 takes it."""
        import torch
        for what, a in (('labels', labels), ('logits', logits)):
            if a.h != 1 or a.w != 1 or a.c != self.k or a.dtype != 'f32':
                raise lib.TgError("ClassifierReport.add: fp32 [n, %d] %s are needed, got [%d, %d, %d, %d] %s" % (self.k, what, a.n, a.h, a.w, a.c, a.dtype))
        if labels.n != logits.n:
            raise lib.TgError("ClassifierReport.add: %d label rows for %d logit rows" % (labels.n, logits.n))
        need = lib.call('tg_eval_report_workspace_bytes', logits.n, self.k)
        if self.workspace is None or self.workspace.numel() * 8 < need:
            self.workspace = torch.empty(max((need + 7) // 8, 2), dtype=torch.float64, device=self.device)
        if stream is None:
            stream = lib.cur_stream()
        P = lambda i: lib.ptr(self._part(i))
        lib.call('tg_eval_report_f32', logits.ptr, logits.ld, labels.ptr, labels.ld, logits.n, self.k, self.ranks, self.bins, P(0), P(1), P(2), P(3),
                 P(5), P(6), P(4), lib.ptr(self.workspace), self.workspace.numel() * 8, stream)
        self.n += logits.n
        return self

    def counts(self):
        """{confusion [k, k], rank_hist, bin_count, bin_correct, nonfinite: int64; bin_conf, sums: float64} as host arrays — the
        arguments of report_from_counts (synchronises)."""
        host = self.acc.cpu().numpy()
        part = lambda i: host[self._off[i]:self._off[i + 1]].copy()
        return dict(confusion=part(0).reshape(self.k, self.k), rank_hist=part(1), bin_count=part(2), bin_correct=part(3),
                    bin_conf=part(5).view(np.float64), sums=part(6).view(np.float64), nonfinite=part(4))

    def result(self):
        """report_from_counts of what has been added."""
        return report_from_counts(**self.counts())


def report_from_counts(confusion, rank_hist, bin_count, bin_correct, bin_conf, sums, nonfinite):
    """The classifier's evaluation report from what tg_eval_report_f32 accumulates, in NumPy float64 on the host.
    confusion [K, K] counts rows by (target, prediction), every row of the pass; the other counts cover the rows whose logits are all
    finite.  -> dict:
      n, n_nonfinite            rows counted, and those among them with a non-finite logit
      accuracy                  trace / sum of confusion (0 for an empty pass, as Train.evaluate)
      top5_accuracy             sum(rank_hist[:5]) / n_finite; NaN when K <= 5 or the histogram has no more than 5 entries
      nll, brier                means over the finite rows of -log softmax_t and of sum_j (softmax_j - [j == t])^2
      ece                       sum_b (n_b / n_finite) |acc_b - conf_b| over the equal-width confidence bins (Guo et al. 2017)
      support, predicted        [K] rows per target class, rows per predicted class
      recall, precision, f1     [K]; NaN where the denominator is 0 (recall of an absent class, precision of a never-predicted one)
      balanced_accuracy         mean recall over the classes with support > 0
      macro_f1                  mean F1 over the same classes (a present class that is never predicted has F1 0)
      worst_class_recall, worst_class   the lowest recall among the present classes and the lowest class index attaining it (-1: none)
      predicted_class_entropy   the entropy of predicted / n over log K: 1 for a uniform prediction histogram, 0 for a collapsed one
      reliability               [bins, 3]: count, mean confidence, accuracy per bin (NaN in the last two for an empty bin)
      confusion                 the matrix itself, int64
    Means over an empty set are NaN."""
    conf_m = np.asarray(confusion, np.int64)
    K = conf_m.shape[0]
    if conf_m.ndim != 2 or conf_m.shape[1] != K or K < 2:
        raise ValueError("report_from_counts: confusion must be a square [K, K] matrix with K >= 2, got shape %r" % (conf_m.shape,))
    rank_hist, bin_count, bin_correct = (np.asarray(a, np.int64).reshape(-1) for a in (rank_hist, bin_count, bin_correct))
    bin_conf, sums = np.asarray(bin_conf, np.float64).reshape(-1), np.asarray(sums, np.float64).reshape(-1)
    if not (bin_count.shape == bin_correct.shape == bin_conf.shape) or sums.shape != (2,):
        raise ValueError("report_from_counts: bin_count, bin_correct and bin_conf must have one length and sums two entries")
    n, n_bad = int(conf_m.sum()), int(np.asarray(nonfinite).reshape(-1)[0])
    n_fin = int(rank_hist.sum())
    nan = float('nan')
    with np.errstate(divide='ignore', invalid='ignore'):
        diag = np.diag(conf_m).astype(np.float64)
        support, predicted = conf_m.sum(axis=1), conf_m.sum(axis=0)
        recall = np.where(support > 0, diag / support, np.nan)
        precision = np.where(predicted > 0, diag / predicted, np.nan)
        f1 = np.where(support + predicted > 0, 2.0 * diag / (support + predicted), np.nan)
        present = support > 0
        cnt = bin_count.astype(np.float64)
        mean_conf = np.where(bin_count > 0, bin_conf / cnt, np.nan)
        acc_b = np.where(bin_count > 0, bin_correct / cnt, np.nan)
        ece = float(np.sum(np.where(bin_count > 0, cnt / n_fin * np.abs(acc_b - mean_conf), 0.0))) if n_fin > 0 else nan
        q = predicted[predicted > 0] / float(max(n, 1))
    worst = int(np.argmin(np.where(present, recall, np.inf))) if present.any() else -1
    out = dict(n=n, n_nonfinite=n_bad, accuracy=float(np.trace(conf_m)) / max(float(n), 1.0),
               top5_accuracy=float(rank_hist[:5].sum()) / n_fin if K > 5 and rank_hist.shape[0] > 5 and n_fin > 0 else nan,
               nll=float(sums[0]) / n_fin if n_fin > 0 else nan, brier=float(sums[1]) / n_fin if n_fin > 0 else nan, ece=ece,
               balanced_accuracy=float(recall[present].mean()) if present.any() else nan,
               macro_f1=float(f1[present].mean()) if present.any() else nan,
               worst_class_recall=float(recall[worst]) if worst >= 0 else nan, worst_class=worst,
               predicted_class_entropy=float(-(q * np.log(q)).sum() / np.log(K)) if n > 0 else nan)
    out.update(support=support, predicted=predicted, recall=recall, precision=precision, f1=f1,
               reliability=np.stack([cnt, mean_conf, acc_b], axis=1), confusion=conf_m)
    return out
