"""config.AUGMENT without a GPU: the Philox known answers, the properties of the transform as tests/augment_reference.py
states it, and the host path of the input pipeline (tfrecordDataset._to_host, the per-record parser) against that restatement: per stream
and batch count, per rank, across epochs, never on the test split; syntheticDataset refuses the option."""
import os

import numpy as np
import pytest

import augment_reference as R
from oracle import tfrecord as O


def test_philox_known_answers():
    from Input_Pipeline.tfrecordDataset import philox4x32
    for counter, key, want in R.PHILOX_KAT:
        assert R.philox4x32_10(counter, key) == want
        assert tuple(int(v) for v in philox4x32(counter, key)) == want


def _u8(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def test_no_shift_no_flip_is_the_plain_scaling():
    x = np.arange(256, dtype=np.uint8).repeat(12).reshape(4, 16, 16, 3)
    for scale, shift in ((2.0, -1.0), (1.0, 0.0)):
        got = R.augment(x, scale, shift, 0, 0, 1234, 1, 7)
        want = x.astype(np.float32) / 255 * scale + shift
        np.testing.assert_array_equal(got, want)
        assert got.dtype == np.float32


def test_flipping_twice_without_shift_is_the_identity():
    x = _u8((64, 6, 7, 3))
    once = R.transform_u8(x, 0, 1, 99, 2, 5)
    flipped = [R.draw(i, 0, 1, 99, 2, 5)[2] for i in range(64)]
    assert 16 < sum(flipped) < 48
    for i, f in enumerate(flipped):
        np.testing.assert_array_equal(once[i], x[i][:, ::-1] if f else x[i])
    np.testing.assert_array_equal(R.transform_u8(once, 0, 1, 99, 2, 5), x)


def test_reflect_indices_at_the_edges():
    from Input_Pipeline.tfrecordDataset import augment_indices
    for size in (1, 2, 5, 32):
        assert [R.refl(p, size) for p in range(size)] == list(range(size))
        if size > 1:
            assert R.refl(-1, size) == 1 and R.refl(size, size) == size - 2
            assert R.refl(-(size - 1), size) == size - 1 and R.refl(2 * size - 2, size) == 0
    # S = H - 1 on a 5 x 9 image reaches both far corners; the package's index maps agree with the restatement
    h, w, n = 5, 9, 400
    ys, xs = augment_indices(n, h, w, h - 1, True, 4321, 1, 3)
    assert ys.min() == 0 and ys.max() == h - 1 and xs.min() == 0 and xs.max() == w - 1
    x = _u8((n, h, w, 2))
    np.testing.assert_array_equal(x[np.arange(n)[:, None, None], ys[:, :, None], xs[:, None, :]], R.transform_u8(x, h - 1, 1, 4321, 1, 3))
    dys = {R.draw(i, h - 1, 1, 4321, 1, 3)[0] for i in range(n)}
    assert dys == set(range(-(h - 1), h))


@pytest.mark.parametrize("max_shift", [2, 4])
def test_draws_are_spread_evenly(max_shift):
    n = 20000
    d = np.array([R.draw(i, max_shift, 1, 1234, 3, 11) for i in range(n)], np.int64)
    span = 2 * max_shift + 1
    for col in (0, 1):
        freq = np.bincount(d[:, col] + max_shift, minlength=span) / n
        assert freq.shape == (span,) and np.all(np.abs(freq - 1.0 / span) <= 0.02), freq
    assert abs(d[:, 2].mean() - 0.5) <= 0.02
    assert not any(R.draw(i, max_shift, 0, 1234, 3, 11)[2] for i in range(200))     # no flips where the dataset allows none


def _cfg(**kw):
    from config import Config

    class Cfg(Config):
        DATA_NAME = 'cifar10'
        BATCH_SIZE = BATCH_SIZE_G = 8
        BATCH_SIZE_L_C, BATCH_SIZE_U_C, BATCH_SIZE_L_D, BATCH_SIZE_U_D = 4, 4, 2, 6
        IMAGE_HEIGHT = IMAGE_WIDTH = 32
        CHANNEL = 3
        NUM_CLASSES = 10
        REPEAT = -1
        PIPELINE_DEVICE = False
    c = Cfg()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _dataset_classes():
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    from Input_Pipeline.cifar100Dataset import cifar100Dataset
    from Input_Pipeline.mnistDataset import mnistDataset
    from Input_Pipeline.svhnDataset import svhnDataset
    return cifar10Dataset, cifar100Dataset, svhnDataset, mnistDataset


def test_dataset_settings():
    from config import Config
    assert Config.AUGMENT is False
    cifar10, cifar100, svhn, mnist = _dataset_classes()
    assert [D.AUG_SHIFT for D in (cifar10, cifar100, svhn, mnist)] == [2, 2, 2, 2]
    assert [D.AUG_FLIP for D in (cifar10, cifar100, svhn, mnist)] == [True, True, False, False]


def _scaling(Dataset):
    return (1.0, 0.0) if Dataset.UNIT_RANGE else (2.0, -1.0)


@pytest.mark.parametrize("which, shape", [(0, (6, 32, 32, 3)), (3, (6, 28, 28, 1))])
def test_host_tail_matches_the_restatement(which, shape):
    """cifar10Dataset (flips) and mnistDataset (one channel, no flips): every batch of a stream draws at its own count."""
    Dataset = _dataset_classes()[which]
    scale, shift = _scaling(Dataset)
    x, lab = _u8(shape, which), np.arange(shape[0], dtype=np.int32) % 10
    ds = Dataset('/nonexistent', _cfg(AUGMENT=True), 10, 'train', True)
    for stream_id, count in ((1, 0), (2, 0), (3, 0), (1, 1)):
        aug = ds._aug_draw(stream_id)
        assert aug == (stream_id, count)
        got, y = ds._to_host(x, lab, aug)
        want = R.augment(x, scale, shift, Dataset.AUG_SHIFT, Dataset.AUG_FLIP, ds.seed, *aug)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(y, np.eye(10, dtype=np.float32)[lab])
    # AUGMENT off, or the test split (use_augmentation False): no draw, the plain tail
    for d in (Dataset('/nonexistent', _cfg(), 10, 'train', True), Dataset('/nonexistent', _cfg(AUGMENT=True), 10, 'test', False)):
        assert d._aug_draw(1) is None and d._aug_counts == [0, 0, 0, 0]
        np.testing.assert_array_equal(d._to_host(x, lab)[0], R.scale_u8(x, scale, shift))


def test_consecutive_batches_differ_and_a_new_dataset_reproduces_them():
    cifar10 = _dataset_classes()[0]
    x, lab = _u8((16, 32, 32, 3), 5), np.zeros(16, np.int32)

    def three(ds):
        return [ds._to_host(x, lab, ds._aug_draw(2))[0] for _ in range(3)]
    a = three(cifar10('/nonexistent', _cfg(AUGMENT=True), 10, 'train', True))
    b = three(cifar10('/nonexistent', _cfg(AUGMENT=True), 10, 'train', True))
    for k in range(3):
        np.testing.assert_array_equal(a[k], b[k])
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])


def test_ranks_draw_differently():
    cifar10 = _dataset_classes()[0]
    x, lab = _u8((16, 32, 32, 3), 6), np.zeros(16, np.int32)
    r0 = cifar10('/nonexistent', _cfg(AUGMENT=True), 10, 'train', True)
    r1 = cifar10('/nonexistent', _cfg(AUGMENT=True, RANK=1), 10, 'train', True)
    assert r1.seed != r0.seed
    a, b = r0._to_host(x, lab, r0._aug_draw(1))[0], r1._to_host(x, lab, r1._aug_draw(1))[0]
    np.testing.assert_array_equal(b, R.augment(x, 2.0, -1.0, 2, True, r1.seed, 1, 0))
    assert not np.array_equal(a, b)


def _write_split(root, Dataset, cfg, n_lab, n_unl, n_test, hw, ch):
    os.makedirs(os.path.join(root, 'Tfrecord'))
    rng = np.random.default_rng(1)
    Dataset.TRAIN_SIZE = n_lab + n_unl
    tr = Dataset(root, cfg, n_lab, 'train', True)
    te = Dataset(root, cfg, n_lab, 'test', False)
    for name, n in zip(tr.get_filenames() + te.get_filenames(), (n_lab, n_unl, n_test)):
        O.write_tfrecord(name, rng.integers(0, 256, (n, hw, hw, ch), dtype=np.uint8), rng.integers(0, 10, n))


def _unscale(x, Dataset):
    """the uint8 pixels behind an unaugmented batch (x/255 or x/255*2-1 inverted; exact after rounding)."""
    u = x * 255 if Dataset.UNIT_RANGE else (x + 1) / 2 * 255
    return np.rint(u).astype(np.uint8)


@pytest.mark.parametrize("which, hw, ch", [(0, 32, 3), (3, 28, 1)])
def test_training_streams_on_the_host(tmp_path, which, hw, ch):
    """the three training streams of _next() with AUGMENT on equal the restatement applied to the same records (read through a twin
    Dataset with AUGMENT off: same shuffle), stream ids 1 / 2 / 3 and counts that keep running across init_op_train(); the test split
    and the per-record parser are unaugmented with the option off."""
    Dataset = _dataset_classes()[which]
    scale, shift = _scaling(Dataset)
    train_size = Dataset.TRAIN_SIZE
    dims = dict(IMAGE_HEIGHT=hw, IMAGE_WIDTH=hw, CHANNEL=ch)
    on, off = _cfg(AUGMENT=True, **dims), _cfg(**dims)
    try:
        _write_split(str(tmp_path), Dataset, off, 20, 50, 10, hw, ch)
        pipes = []
        for cfg in (on, off):
            tr, te = Dataset(str(tmp_path), cfg, 20, 'train', True), Dataset(str(tmp_path), cfg, 20, 'test', False)
            init_train, _, nnio = tr.inputpipline_train_val(te)
            pipes.append((tr, init_train, nnio))
        (tr, init_on, nn_on), (_, init_off, nn_off) = pipes
        for epoch in range(2):
            init_on()
            init_off()
            for k in range(3):
                count = 3 * epoch + k
                a, b = nn_on.next(), nn_off.next()
                for key, stream_id in (('x_l_c', 1), ('x_l_d', 2)):
                    raw = _unscale(b[key], Dataset)
                    np.testing.assert_array_equal(b[key], R.scale_u8(raw, scale, shift))
                    np.testing.assert_array_equal(a[key], R.augment(raw, scale, shift, 2, Dataset.AUG_FLIP, tr.seed, stream_id, count))
                    np.testing.assert_array_equal(a['y' + key[1:]], b['y' + key[1:]])
                xa, xb = (np.concatenate([p['x_u_d'], p['x_u_c']]) for p in (a, b))
                np.testing.assert_array_equal(xa, R.augment(_unscale(xb, Dataset), scale, shift, 2, Dataset.AUG_FLIP, tr.seed, 3, count))
                assert not np.array_equal(xa, xb)
        assert tr._aug_counts == [0, 6, 6, 6]
        va, vb = list(nn_on.val_batches()), list(nn_off.val_batches())
        assert len(va) == len(vb) == 2
        for (x0, y0), (x1, y1) in zip(va, vb):
            np.testing.assert_array_equal(x0, x1)
            np.testing.assert_array_equal(y0, y1)
    finally:
        Dataset.TRAIN_SIZE = train_size


def test_per_record_parser_uses_stream_zero(tmp_path):
    cifar10 = _dataset_classes()[0]
    x = _u8((3, 32, 32, 3), 8)
    p = tmp_path / 'r.tfrecords'
    O.write_tfrecord(p, x, [1, 2, 3])
    payloads = O.read_tfrecord(p)
    ds = cifar10('/nonexistent', _cfg(AUGMENT=True), 10, 'train', True)
    for k, pl in enumerate(payloads):
        img, onehot = ds.parser(pl)
        np.testing.assert_array_equal(img, R.augment(x[k:k + 1], 2.0, -1.0, 2, True, ds.seed, 0, k)[0])
        assert onehot.argmax() == k + 1
    plain = cifar10('/nonexistent', _cfg(), 10, 'train', True)
    np.testing.assert_array_equal(plain.parser(payloads[0])[0], R.scale_u8(x[:1], 2.0, -1.0)[0])


class _Flags(object):
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def test_synthetic_dataset_refuses_augment():
    from tg import lib
    from Input_Pipeline.syntheticDataset import syntheticDataset
    from Training.Train_goodGAN import _customize_config
    cfg = _cfg(IMAGE_DIM=[32, 32, 3])
    _customize_config(cfg, _Flags(augment=True))                       # --augment
    assert cfg.AUGMENT is True
    with pytest.raises(lib.TgError, match="AUGMENT needs .*syntheticDataset has no real images"):
        syntheticDataset(None, cfg, 10, 'train', True)
    syntheticDataset(None, cfg, 10, 'test', False)                       # the test split is never augmented
    syntheticDataset(None, _cfg(IMAGE_DIM=[32, 32, 3]), 10, 'train', True)
