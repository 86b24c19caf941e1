"""ZCA whitening of the CIFAR classifiers' inputs: where the constants come from, and their application.

`cifar10_ZCA(config).apply(image)` is the reference's class (Model/Good_GAN_cifar10.py:287-299): (flatten(x) - mean) @ mat with the
constants of DATA_DIR/<data>_zca_{mean,mat}.npy.  The reference loads those files but neither it nor its repository holds code that
makes them, so this module also decides every other source of (mean, mat) — config.ZCA:
  None            the files (zca_paths);
  (mean, mat)     arrays handed in, e.g. synthetic_zca's fixed rotation for the entry points without files;
  'fit'           resolve_zca, called by Training/Train_goodGAN.Train.train before the model first whitens: the files when both exist,
                  else cifar10_ZCA.fit over the training split (tg_gram_u8_i64, exact int64 moments; zca_constants on the host) and
                  write_zca_files; with data parallelism rank 0 does that and broadcasts.
Importing this module needs neither torch nor a device (Training/options.check_zca reads ZCA_DATA)."""
import math
import os

import numpy as np

# Regularisation of the whitening, mat = U diag((s + eps)^-1/2) U^T.  [UNVERIFIED] the value of the ZCA class of the improved-GAN /
# Triple-GAN code lineage, recalled from memory: the reference repository holds no fitting code.
ZCA_EPS = 1e-5
ZCA_DATA = ('cifar10', 'cifar100')        # the DATA_NAMEs whose classifier sees ZCA-whitened inputs
ZCA_CHUNK = 16384                         # images per staging buffer of the fit (50 MB of CIFAR bytes)
# n G' - S' S'^T is exact in int64 while n^2 2^14 <= 2^63 - 1 (|x'| <= 128, so |G'| <= n 2^14 and |S'_i S'_j| <= n^2 2^14)
ZCA_N_MAX = math.isqrt((2 ** 63 - 1) >> 14)


def zca_prefix(config):
    """'cifar100' for CIFAR-100 (cifar100_zca_*.npy), else 'cifar10'."""
    return "cifar100" if getattr(config, 'DATA_NAME', None) == "cifar100" else "cifar10"


def zca_paths(config):
    """(mean, mat) file paths the reference loads (Model/Good_GAN_cifar10.py:289-290)."""
    pre = os.path.join(config.DATA_DIR, zca_prefix(config))
    return pre + "_zca_mean.npy", pre + "_zca_mat.npy"


def zca_constants(n, colsum, gram, eps=ZCA_EPS, timings=None):
    """Host derivation (float64, no device) of the ZCA constants from the exact integer moments of n images x (uint8) with x' = x - 128:
    colsum S' = sum x', gram G' = sum x' x'^T.  The images the classifier sees are x/255*2-1 = (2x'+1)/255 (cifar10Dataset.py:60), so
        mean = (2 S'/n + 1) / 255,   cov = 4/255^2 (n G' - S' S'^T) / n^2      (numerator exact in int64 for n <= ZCA_N_MAX)
    and mat = U diag((s + eps)^-1/2) U^T over eigh(cov) with the eigenvalues s clipped at 0 (n < d leaves a null space).
    Returns float64 (mean [d], mat [d, d]) in the flatten order of the images (NHWC)."""
    import time
    n = int(n)
    if not 0 < n <= ZCA_N_MAX:
        raise ValueError("ZCA fit: %d images; the integer derivation is exact for 1..%d" % (n, ZCA_N_MAX))
    s1 = np.asarray(colsum, np.int64).reshape(-1)
    d = s1.size
    g = np.asarray(gram, np.int64).reshape(d, d)
    mean = (2.0 * s1 / n + 1.0) / 255.0
    num = n * g - np.outer(s1, s1)                                   # n^2 cov(x'), exact
    cov = num.astype(np.float64) * (4.0 / (255.0 ** 2)) / (float(n) * float(n))
    t0 = time.perf_counter()
    s, u = np.linalg.eigh(cov)
    t1 = time.perf_counter()
    s = np.maximum(s, 0.0)
    mat = (u * (s + eps) ** -0.5) @ u.T
    mat = 0.5 * (mat + mat.T)                                        # symmetric to the last bit
    if timings is not None:
        timings['eigh'] = timings.get('eigh', 0.0) + (t1 - t0)
        timings['mat'] = timings.get('mat', 0.0) + (time.perf_counter() - t1)
    return mean, mat


def zca_training_files(dataset):
    """The record files of the training split of a TFRecord dataset, each once: input_from_tfrecord_filename() returns the labelled file
    twice ([labelled for D, labelled for C, unlabelled]).  The test split is not opened."""
    from Input_Pipeline.tfrecordDataset import each_once, tfrecordDataset
    from tg import lib
    if not isinstance(dataset, tfrecordDataset) or dataset.UNIT_RANGE:
        raise lib.TgError("ZCA = 'fit' needs a training split of uint8 TFRecords in [-1, 1] scaling (a tfrecordDataset such as "
                          "cifar10Dataset); %s has none" % type(dataset).__name__)
    if dataset.subset != 'train':
        raise lib.TgError("ZCA = 'fit' reads the training split only, got subset %r" % (dataset.subset,))
    return each_once(dataset.input_from_tfrecord_filename())


def zca_training_chunks(dataset, rows=ZCA_CHUNK):
    """(RecordFile, record indices) pieces of at most `rows` records that cover every training record exactly once: the pieces and the
    order of Input_Pipeline.tfrecordDataset.training_chunks (record_chunks), behind this module's own checks and errors."""
    from Input_Pipeline.tfrecordDataset import record_chunks
    for piece in record_chunks(zca_training_files(dataset), rows):
        yield piece


def write_zca_files(config, mean, mat):
    """Write (mean, mat) as float32 to zca_paths(config), each atomically (temporary file in the same directory, then os.replace); the
    mat file last, so a reader that finds both finds complete ones.  lib.TgError naming the path if it cannot be written."""
    import tempfile
    from tg import lib
    for path, arr in zip(zca_paths(config), (mean, mat)):
        tmp = None
        try:
            fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path) or '.', prefix='.' + os.path.basename(path), suffix='.tmp')
            with os.fdopen(fd, 'wb') as f:
                np.save(f, np.asarray(arr, np.float32))
            os.replace(tmp, path)
            tmp = None
        except OSError as e:
            raise lib.TgError("ZCA = 'fit': cannot write %s (%s)" % (path, e))
        finally:
            if tmp is not None and os.path.exists(tmp):
                os.remove(tmp)


class cifar10_ZCA():
    """Model/Good_GAN_cifar10.py:287-299: (flatten(x) - mean) @ mat.  Constants come from DATA_DIR/cifar10_zca_{mean,mat}.npy as in the
    reference; when the files are absent (they are not part of the reference repository) `config.ZCA` may
    supply (mean, mat) arrays, e.g. the synthetic orthogonal matrix of SURVEY §8d (synthetic_zca), or the ones
    cifar10_ZCA.fit computes (config.ZCA = 'fit', resolved by resolve_zca for Training/Train_goodGAN.Train.train)."""

    @staticmethod
    def fit(dataset, eps=ZCA_EPS, chunk=ZCA_CHUNK, timings=None):
        """ZCA constants of the training split of `dataset` (a tfrecordDataset, subset 'train') -> float32 (mean [d], mat [d, d]).
        Every training record is decoded once into pinned uint8 staging (two buffers: decoding chunk k+1 overlaps the copy and the
        Gram launch of chunk k, the event discipline of tfrecordDataset._to_device), copied to the device and accumulated by
        tg_gram_u8_i64 into exact int64 (S', G'); those come back once and zca_constants derives the constants on the host.
        timings: a dict to receive the wall seconds of each phase (decode, h2d, gram, d2h, eigh, mat); with it every device phase is
        synchronised on its own, so the phases are measured one after the other instead of overlapped."""
        import time
        import torch
        from tg import lib
        from tg.runtime import ctx
        cx = ctx()
        files = [r for r in zca_training_files(dataset) if len(r)]
        shapes = {r.shape for r in files}
        if len(shapes) != 1:
            raise lib.TgError("ZCA = 'fit': the training files hold images of shapes %s (one shape needed, none if empty)" % sorted(shapes))
        d = int(np.prod(shapes.pop()))
        stream = torch.cuda.current_stream(cx.device)
        T = timings

        def tick(key, t0, sync=False):
            if T is None:
                return
            if sync:
                torch.cuda.synchronize(cx.device)
            T[key] = T.get(key, 0.0) + time.perf_counter() - t0

        staging = [torch.empty(chunk * d, dtype=torch.uint8).pin_memory() for _ in range(2)]
        labels = np.empty(chunk, np.int32)
        dev = [torch.empty(chunk * d, dtype=torch.uint8, device=cx.device) for _ in range(2)]
        gram = torch.zeros(d * d, dtype=torch.int64, device=cx.device)
        colsum = torch.zeros(d, dtype=torch.int64, device=cx.device)
        events, n = [None, None], 0
        for k, (rec, idx) in enumerate(zca_training_chunks(dataset, chunk)):
            s, m = k & 1, len(idx)
            if events[s] is not None:                    # the copy out of this staging buffer (two chunks ago) has run
                events[s].synchronize()
            t0 = time.perf_counter()
            rec.gather(idx, staging[s].numpy(), labels, n_threads=4)
            tick('decode', t0)
            t0 = time.perf_counter()
            dev[s][:m * d].copy_(staging[s][:m * d], non_blocking=True)
            events[s] = torch.cuda.Event()
            events[s].record(stream)
            tick('h2d', t0, sync=True)
            t0 = time.perf_counter()
            lib.call('tg_gram_u8_i64', lib.ptr(dev[s]), m, d, lib.ptr(gram), lib.ptr(colsum), cx.stream)
            tick('gram', t0, sync=True)
            n += m
        t0 = time.perf_counter()
        g, s1 = gram.cpu().numpy(), colsum.cpu().numpy()
        tick('d2h', t0)
        mean, mat = zca_constants(n, s1, g, eps, timings)
        return mean.astype(np.float32), mat.astype(np.float32)

    def __init__(self, config):
        from tg.runtime import ctx
        cx = ctx()
        zc = getattr(config, 'ZCA', None)
        if isinstance(zc, str):
            from tg import lib
            raise lib.TgError("config.ZCA = %r is resolved by Train.train (Training/Train_goodGAN.py) before the model whitens" % (zc,))
        if zc is None:
            m_path, mat_path = zca_paths(config)                     # cifar100_zca_*.npy for CIFAR-100
            m = np.load(m_path)
            mat = np.load(mat_path)
        else:
            m, mat = zc
        m = np.asarray(m, np.float32).reshape(-1)
        mat = np.asarray(mat, np.float32)
        import torch
        self.dim = mat.shape[0]
        # (x - mean) @ mat = x @ mat + (-mean @ mat): weights as Wt[n][k] for the MFMA kernel, bias folded
        self.wt = torch.from_numpy(np.ascontiguousarray(mat.T)).to(cx.device).reshape(-1)
        self.bias = torch.from_numpy((-(m.astype(np.float64) @ mat.astype(np.float64))).astype(np.float32)).to(cx.device)

    def apply(self, image):
        """image: Act [N,32,32,3] (ld 3) -> Act of the same shape; forward only (no gradient ever flows through ZCA)."""
        from tg import geom, lib
        from tg.runtime import ctx
        cx = ctx()
        assert image.ld == image.c and image.h * image.w * image.c == self.dim
        out = cx.new_act(image.n, image.h, image.w, image.c, image.c)
        splits = 4 if self.dim % 128 == 0 and image.n <= 1024 else 1
        if splits > 1:
            # few rows, long reduction (3072): four K-ranges as sub-problems of one launch, then one add-up pass
            part = cx.scratch('zcap', image.n * splits * self.dim)
            dds = lib.desc_array(geom.dense_fwd_splitk(image.n, self.dim, self.dim, splits))
            lib.call('tg_igemm_multi_f32', dds, len(dds), image.ptr, lib.ptr(self.wt), None, lib.ptr(part), None, 0, cx.stream)
            lib.call('tg_splitk_reduce_f32', lib.ptr(part), lib.ptr(self.bias), out.ptr, self.dim, image.n, splits, self.dim, cx.stream)
        else:
            d = geom.dense_fwd(image.n, self.dim, self.dim)
            lib.call('tg_igemm_f32', d, image.ptr, lib.ptr(self.wt), lib.ptr(self.bias), out.ptr, None, 0, cx.stream)
        return out


def resolve_zca(config, dataset_train, rank, device):
    """config.ZCA = 'fit' -> ((mean, mat) float32 arrays, source), before the model first whitens.  Rank 0 loads
    DATA_DIR/<data>_zca_{mean,mat}.npy when both exist (the reference's path, no refit: source 'files'), else fits them from the
    training split (cifar10_ZCA.fit) and writes them ('fit'); with data parallelism the other ranks receive rank 0's constants
    (tg.dist.broadcast_: 'broadcast'), so every replica holds the same bits and there is exactly one writer."""
    import torch
    from tg import dist as tgdist
    from tg import lib
    d = int(np.prod(config.IMAGE_DIM))
    mean = mat = source = None
    if rank == 0:
        m_path, mat_path = zca_paths(config)
        if os.path.exists(m_path) and os.path.exists(mat_path):
            mean, mat = np.load(m_path), np.load(mat_path)
            source = 'files'
        else:
            ddir = os.path.dirname(m_path) or '.'
            if not os.access(ddir, os.W_OK):
                raise lib.TgError("ZCA = 'fit': %s is not writable (the fitted constants go to %s)" % (ddir, m_path))
            mean, mat = cifar10_ZCA.fit(dataset_train)
            write_zca_files(config, mean, mat)
            source = 'fit'
        mean = np.asarray(mean, np.float32).reshape(-1)
        mat = np.asarray(mat, np.float32)
        if mean.shape != (d,) or mat.shape != (d, d):
            raise lib.TgError("ZCA constants of shapes %s / %s do not match images of %d values" % (mean.shape, mat.shape, d))
    if tgdist.active():
        flat = torch.empty(d + d * d, dtype=torch.float32, device=device)
        if rank == 0:
            flat.copy_(torch.from_numpy(np.concatenate([mean, mat.reshape(-1)])))
        tgdist.broadcast_(flat)
        if rank != 0:
            host = flat.cpu().numpy()
            mean, mat = host[:d].copy(), host[d:].reshape(d, d).copy()
            source = 'broadcast'
    return (mean, mat), source


def synthetic_zca(tmp_config):
    """the ZCA-whitened (CIFAR) experiments without whitening constants — config.ZCA is None and DATA_DIR holds no <data>_zca_mat.npy —
    whiten with a fixed random rotation and a zero mean."""
    if tmp_config.DATA_NAME in ZCA_DATA and tmp_config.ZCA is None and not os.path.exists(os.path.join(tmp_config.DATA_DIR, tmp_config.DATA_NAME + "_zca_mat.npy")):
        d = int(np.prod(tmp_config.IMAGE_DIM))
        q, _ = np.linalg.qr(np.random.default_rng(4321).standard_normal((d, d)))
        tmp_config.ZCA = (np.zeros(d, np.float32), q.astype(np.float32))
