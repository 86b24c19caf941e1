"""config.ZCA = 'fit' without a GPU: the host derivation of the ZCA constants from exact integer moments against a float64
restatement on the [-1, 1] images, the whitening property, the rank-deficient case, which records the fit reads, the atomic file write,
and the validation of the key."""
import os

import numpy as np
import pytest

import zca_reference as R


def _images(rng, n, d):
    return rng.integers(0, 256, (n, d), dtype=np.uint8)


def test_host_derivation_matches_the_float64_restatement():
    from Model.zca import ZCA_EPS, zca_constants
    assert ZCA_EPS == 1e-5
    x = _images(np.random.default_rng(0), 500, 48)
    mean, mat = zca_constants(*R.int_moments(x))
    mean_r, mat_r, _, _ = R.zca(x, ZCA_EPS)
    assert mean.dtype == mat.dtype == np.float64 and mean.shape == (48,) and mat.shape == (48, 48)
    np.testing.assert_allclose(mean, mean_r, rtol=0, atol=1e-14)
    assert np.linalg.norm(mat - mat_r) <= 1e-10 * np.linalg.norm(mat_r)


@pytest.mark.parametrize("n, d", [(500, 48), (20, 48)])
def test_whitening_property(n, d):
    """mat is symmetric and mat · cov · mat has the eigenvalues s / (s + eps); (20, 48) is the rank-deficient case n < d, where the
    clipping at 0 keeps the constants finite."""
    from Model.zca import zca_constants
    x = _images(np.random.default_rng(n), n, d)
    mean, mat = zca_constants(*R.int_moments(x))
    assert np.isfinite(mean).all() and np.isfinite(mat).all()
    assert np.array_equal(mat, mat.T)
    cov = R.covariance(x)
    s = np.maximum(np.linalg.eigvalsh(cov), 0.0)
    got = np.linalg.eigvalsh(mat @ cov @ mat)
    np.testing.assert_allclose(got, R.whitening_eigenvalues(s), rtol=0, atol=1e-9)
    if n < d:
        assert (R.whitening_eigenvalues(s)[:d - n + 1] < 1e-9).all()         # the null space stays null
        np.testing.assert_allclose(np.sort(got)[-(n - 1):], 1.0, atol=1e-3)


def test_derivation_rejects_counts_outside_the_exact_range():
    from Model.zca import ZCA_N_MAX, zca_constants
    assert ZCA_N_MAX ** 2 << 14 <= 2 ** 63 - 1 < (ZCA_N_MAX + 1) ** 2 << 14
    for n in (0, ZCA_N_MAX + 1):
        with pytest.raises(ValueError, match="exact"):
            zca_constants(n, np.zeros(3, np.int64), np.zeros((3, 3), np.int64))


def _write_cifar10_files(root, n_lab, n_unl, n_test, seed=0):
    """CIFAR-10-named TFRecords under root/Tfrecord -> (training images in file order, test path)."""
    from tg import io as tgio
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    os.makedirs(os.path.join(root, 'Tfrecord'))
    rng = np.random.default_rng(seed)
    tr = cifar10Dataset(root, None, n_lab, 'train')
    te = cifar10Dataset(root, None, n_lab, 'test')
    out = []
    for name, n in zip(tr.get_filenames() + te.get_filenames(), (n_lab, n_unl, n_test)):
        img = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
        tgio.write_tfrecord(name, img, rng.integers(0, 10, n))
        out.append(img)
    return np.concatenate(out[:2]), te.get_filenames()[0]


def test_the_fit_reads_every_training_record_once_and_never_the_test_split(tmp_path, monkeypatch):
    from tg import io as tgio
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    from Model.zca import zca_training_chunks, zca_training_files
    train, test_path = _write_cifar10_files(str(tmp_path), 40, 90, 30)
    opened = []
    real = tgio.RecordFile

    class Spy(real):
        def __init__(self, path):
            opened.append(os.path.abspath(str(path)))
            super(Spy, self).__init__(path)
    monkeypatch.setattr(tgio, 'RecordFile', Spy)
    ds = cifar10Dataset(str(tmp_path), None, 40, 'train')
    assert len(ds.input_from_tfrecord_filename()) == 3                 # the labelled file is listed twice ...
    assert [len(r) for r in zca_training_files(ds)] == [40, 90]         # ... and counted once
    got, sizes = [], []
    for rec, idx in zca_training_chunks(ds, rows=16):
        img, _ = rec.gather(idx)
        got.append(img)
        sizes.append(len(idx))
    got = np.concatenate(got)
    assert max(sizes) == 16 and sum(sizes) == 130 == len(train)
    assert got.shape == train.shape and np.array_equal(got, train)     # every record once, in file order
    assert tgio.crc32c(got.tobytes()) == tgio.crc32c(train.tobytes())
    assert os.path.abspath(test_path) not in opened and len(set(opened)) == 2


def test_zca_files_are_written_atomically_or_the_error_names_the_path(tmp_path):
    from tg import lib
    from Model.zca import write_zca_files, zca_paths

    class C(object):
        DATA_NAME, DATA_DIR = 'cifar100', str(tmp_path)
    mean, mat = np.arange(4, dtype=np.float64), np.eye(4) * 0.5
    write_zca_files(C, mean, mat)
    m_path, mat_path = zca_paths(C)
    assert os.path.basename(m_path) == 'cifar100_zca_mean.npy' and os.path.basename(mat_path) == 'cifar100_zca_mat.npy'
    a, b = np.load(m_path), np.load(mat_path)
    assert a.dtype == b.dtype == np.float32 and np.array_equal(a, mean) and np.array_equal(b, mat)
    assert sorted(os.listdir(str(tmp_path))) == ['cifar100_zca_mat.npy', 'cifar100_zca_mean.npy']     # no temporary file left
    blocker = tmp_path / 'not_a_dir'
    blocker.write_text('x')
    C.DATA_DIR = str(blocker)
    with pytest.raises(lib.TgError, match=r"cannot write .*not_a_dir/cifar100_zca_mean\.npy"):
        write_zca_files(C, mean, mat)


class _Flags(object):
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


@pytest.mark.parametrize("entry", ['_main_training_mnist', '_main_training_svhn', '_main_training_stress64'])
def test_fit_on_a_model_without_whitening_raises(entry, monkeypatch, tmp_path):
    from tg import lib
    from Training import Train_goodGAN as TG
    monkeypatch.setattr(TG, "_root_dir", lambda: str(tmp_path))
    with pytest.raises(lib.TgError, match=r"ZCA = 'fit'.*has no ZCA whitening"):
        getattr(TG, entry)(_Flags(zca='fit'), epochs=1)


def test_fit_needs_a_tfrecord_source(monkeypatch, tmp_path):
    from tg import lib
    from Training import Train_goodGAN as TG
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    from Input_Pipeline.cifar100Dataset import cifar100Dataset
    from Input_Pipeline.mnistDataset import mnistDataset
    from Input_Pipeline.syntheticDataset import syntheticDataset
    monkeypatch.setattr(TG, "_root_dir", lambda: str(tmp_path))
    with pytest.raises(lib.TgError, match=r"ZCA = 'fit' needs .*syntheticDataset"):
        TG._main_training_cifar10(_Flags(zca='fit'), epochs=1)          # the default Dataset of the entry points
    with pytest.raises(lib.TgError, match=r"ZCA = 'fit' needs .*syntheticDataset"):
        TG._main_training_cifar100(_Flags(zca='fit'), epochs=1)

    class C(object):
        DATA_NAME, ZCA = 'cifar100', 'fit'
    assert TG.check_zca(C, cifar100Dataset) == 'fit' and TG.check_zca(C, cifar10Dataset) == 'fit' and TG.check_zca(C) == 'fit'
    with pytest.raises(lib.TgError, match="ZCA"):
        TG.check_zca(C, mnistDataset)                                    # x/255 scaling, one channel
    with pytest.raises(lib.TgError, match="ZCA"):
        TG.check_zca(C, syntheticDataset(None, type('c', (), dict(DATA_NAME='cifar100', NUM_CLASSES=100, IMAGE_DIM=[32, 32, 3])),
                                         10, 'train'))


def test_unknown_zca_value_raises_value_error():
    from Training import Train_goodGAN as TG

    class C(object):
        DATA_NAME = 'cifar10'
    for bad in ('Fit', 'zca', ''):
        C.ZCA = bad
        with pytest.raises(ValueError, match="ZCA"):
            TG.check_zca(C)
    for ok in (None, (np.zeros(3), np.eye(3))):
        C.ZCA = ok
        assert TG.check_zca(C) is ok
