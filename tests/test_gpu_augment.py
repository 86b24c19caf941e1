"""config.AUGMENT on the GPU: tg_u8_augment_f32 bit for bit against tests/augment_reference.py over batch sizes, image
shapes, shifts, flips, every uint8 value and counts past 2^32, with a guard behind the output; S = 0 without flip is tg_u8_affine_f32;
bad arguments are refused before any launch; the device tail of the pipeline equals its host tail; Train.train runs from TFRecord files
with the option on, feeds the augmented records and evaluates on unaugmented ones."""
import numpy as np
import pytest

import augment_reference as R
import gpu_common as G
import kernel_check as K
from oracle import tfrecord as O

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32, 3), (28, 28, 1), (64, 64, 3), (5, 9, 3)]
SEED = (1 << 40) + 1234                  # both key words non-zero


def _src(n, h, w, c, seed):
    x = np.random.default_rng(seed).integers(0, 256, (n, h, w, c), dtype=np.uint8)
    flat = x.reshape(-1)
    k = min(256, flat.size)
    flat[:k] = np.arange(k, dtype=np.uint8)[::-1] if seed % 2 else np.arange(k, dtype=np.uint8)
    return x


def _augment(x, scale, shift, max_shift, flip, seed, stream_id, count):
    L = K.lib()
    n, h, w, c = x.shape
    src = K.dev(x, np.uint8)
    out = K.guarded(x.size)
    L.call('tg_u8_augment_f32', K.ptr(src), out.ptr, n, h, w, c, scale, shift, max_shift, flip, seed, stream_id, count, K.st())
    return K.finish(out, x.shape)


def _context():
    """the Context the pipeline's device tail launches on (the current one, or a new one on cuda:0)."""
    from tg import lib, runtime
    try:
        runtime.ctx()
    except lib.TgError:
        runtime.set_context(runtime.Context('cuda:0'))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("max_shift", [0, 1, 2, 4])
def test_kernel_is_bit_identical_to_the_restatement(shape, max_shift):
    h, w, c = shape
    for k, n in enumerate((1, 7, 200)):
        for flip in (0, 1):
            count = (0, 5, (1 << 32) + 3)[k]                    # the count's high word reaches the counter
            stream_id = 1 + (k + flip) % 3
            scale, shift = (1.0, 0.0) if c == 1 else (2.0, -1.0)
            x = _src(n, h, w, c, 17 * k + flip + max_shift)
            got = _augment(x, scale, shift, max_shift, flip, SEED, stream_id, count)
            want = R.augment(x, scale, shift, max_shift, flip, SEED, stream_id, count)
            K.assert_bits(got, want, "n=%d %s S=%d flip=%d count=%d" % (n, shape, max_shift, flip, count))


def test_every_uint8_value_and_the_high_count_word():
    x = np.tile(np.arange(256, dtype=np.uint8), 36).reshape(3, 32, 32, 3)         # every value in every image
    for count in ((1 << 32) + 7, (1 << 33) + 7, 7):
        K.assert_bits(_augment(x, 2.0, -1.0, 2, 1, SEED, 2, count), R.augment(x, 2.0, -1.0, 2, 1, SEED, 2, count), "count=%d" % count)
    # the high count word changes the draws (the transforms above differ from one another)
    a, b = (_augment(x[:1].repeat(64, 0), 2.0, -1.0, 2, 1, SEED, 2, cnt) for cnt in (7, (1 << 32) + 7))
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("shape", SHAPES)
def test_no_shift_no_flip_is_the_affine_tail(shape):
    """against the pipeline's unaugmented device tail, which launches tg_u8_affine_f32 (x/255*2-1 and MNIST's x/255)."""
    import torch
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    from Input_Pipeline.mnistDataset import mnistDataset
    cfg = G.make_config(dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6))
    _context()
    x = _src(7, *shape, seed=3)
    for Dataset, (scale, shift) in ((cifar10Dataset, (2.0, -1.0)), (mnistDataset, (1.0, 0.0))):
        xa, _ = Dataset('/nonexistent', cfg, 10, 'train')._to_device(x, np.zeros(7, np.int32), want_labels=False)
        torch.cuda.synchronize()
        K.assert_bits(_augment(x, scale, shift, 0, 0, SEED, 1, 9), xa.numpy(), "S=0 vs the affine tail")


def test_bad_arguments_are_refused_without_a_launch():
    import torch
    from tg import lib as L
    L.load()
    x = _src(2, 5, 9, 3, seed=1)
    src = K.dev(x, np.uint8)
    out = K.guarded(x.size)
    cases = [((None, out.ptr, 2, 5, 9, 3), 0, "null pointer"), ((K.ptr(src), None, 2, 5, 9, 3), 0, "null pointer"),
             ((K.ptr(src), out.ptr, 0, 5, 9, 3), 0, "bad shape"), ((K.ptr(src), out.ptr, 2, 0, 9, 3), 0, "bad shape"),
             ((K.ptr(src), out.ptr, 2, 5, 0, 3), 0, "bad shape"), ((K.ptr(src), out.ptr, 2, 5, 9, 0), 0, "bad shape"),
             ((K.ptr(src), out.ptr, 2, 5, 9, 3), 5, r"max_shift=5 outside \[0, min\(h,w\)-1 = 4\]"),
             ((K.ptr(src), out.ptr, 2, 5, 9, 3), -1, "max_shift=-1 outside")]
    for head, max_shift, msg in cases:
        with pytest.raises(L.TgError, match="tg_u8_augment_f32 failed.*u8_augment: " + msg):
            L.call('tg_u8_augment_f32', *head, 2.0, -1.0, max_shift, 1, SEED, 1, 0, K.st())
    torch.cuda.synchronize()
    out.check_guard()
    assert np.isnan(out.get()).all()                                 # nothing was launched: the output is still all NaN


def test_device_tail_equals_the_host_tail():
    import torch
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    from Input_Pipeline.mnistDataset import mnistDataset
    cfg = G.make_config(dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6), AUGMENT=True)
    _context()
    lab = np.array([3, 0, 9, 3, 1, 2], np.int32)
    for Dataset, shape in ((cifar10Dataset, (6, 32, 32, 3)), (mnistDataset, (6, 28, 28, 1))):
        ds = Dataset('/nonexistent', cfg, 10, 'train', True)
        u8 = _src(*shape, seed=5)
        for stream_id in (1, 2, 3):
            aug = ds._aug_draw(stream_id)
            xd, yd = ds._to_device(u8, lab, aug=aug)
            xh, yh = ds._to_host(u8, lab, aug)
            torch.cuda.synchronize()
            K.assert_bits(xd.numpy(), xh, "%s stream %d" % (Dataset.__name__, stream_id))
            np.testing.assert_array_equal(yd.numpy(), yh)
        aug = (1, (1 << 32) + 1)
        xd, _ = ds._to_device(u8, lab, aug=aug)
        torch.cuda.synchronize()
        K.assert_bits(xd.numpy(), ds._to_host(u8, lab, aug)[0], "count past 2^32")


def _files(tmp_path, Dataset, cfg, n_lab, n_unl, n_test):
    d = tmp_path / 'Tfrecord'
    d.mkdir()
    rng = np.random.default_rng(0)
    proto = rng.integers(0, 256, (10, 32, 32, 3))
    Dataset.TRAIN_SIZE = n_lab + n_unl
    tr = Dataset(str(tmp_path), cfg, n_lab, 'train', True)
    te = Dataset(str(tmp_path), cfg, n_lab, 'test', False)
    out = []
    for name, n in zip(tr.get_filenames() + te.get_filenames(), (n_lab, n_unl, n_test)):
        lab = rng.integers(0, 10, n)
        img = np.clip(proto[lab] + rng.normal(0, 30, (n, 32, 32, 3)), 0, 255).astype(np.uint8)
        O.write_tfrecord(name, img, lab)
        out.append(img)
    return out


def _rows(x):
    x = np.ascontiguousarray(x).reshape(len(x), -1)
    return sorted(r.tobytes() for r in x)


def test_train_from_tfrecords_with_augmentation(tmp_path, monkeypatch):
    import torch
    from tg import runtime
    from Training.Train_goodGAN import Train
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    sizes = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
    cfg = G.make_config(sizes, DATA_DIR=str(tmp_path), NUM_LABEL=40, TRAIN_SIZE=8 * 6, EPOCHS=2, SAMPLE_DIR=None, USE_HIP_GRAPH=True,
                        REPEAT=-1, AUGMENT=True)
    seen = dict(raw=[], datasets=[], fed=[], val=[])
    finish, feed, evaluate = cifar10Dataset._finish, Train.feed, Train.evaluate

    def spy_finish(self, slot, stream_id, want_labels=True):
        if stream_id == 1 and not seen['raw']:
            seen['raw'].append(slot.images.copy())
            seen['datasets'].append(self)
        return finish(self, slot, stream_id, want_labels)

    def spy_feed(self, batch):
        if not seen['fed']:
            torch.cuda.synchronize()
            seen['fed'].append(batch['x_l_c'].numpy().copy())
        return feed(self, batch)

    def spy_evaluate(self, batches):
        batches = list(batches)
        seen['val'].append(batches)
        return evaluate(self, batches)
    monkeypatch.setattr(cifar10Dataset, '_finish', spy_finish)
    monkeypatch.setattr(Train, 'feed', spy_feed)
    monkeypatch.setattr(Train, 'evaluate', spy_evaluate)
    train_size = cifar10Dataset.TRAIN_SIZE
    try:
        lab_img, _, test_img = _files(tmp_path, cifar10Dataset, cfg, 40, 120, 24)
        runtime.set_context(None)
        torch.cuda.empty_cache()
        tr = Train(cfg, None, None)
        hist = tr.train(cifar10Dataset, Good_GAN_cifar10, None)
    finally:
        cifar10Dataset.TRAIN_SIZE = train_size
    assert len(hist) == 2 and tr.iteration == 2 * 6
    for rec in hist:
        assert all(np.isfinite(rec[k]) for k in ('d_loss', 'g_loss', 'c_loss')) and 0.0 <= rec['val_accuracy'] <= 1.0
    # the first labelled-for-C batch: records of the labelled file, fed augmented at stream 1, count 0
    raw, ds = seen['raw'][0], seen['datasets'][0]
    assert ds.use_augmentation and ds.subset == 'train' and ds._aug_counts[1:] == [12, 12, 12]
    lab_rows = set(_rows(lab_img))
    assert raw.shape == (4, 32, 32, 3) and all(r in lab_rows for r in _rows(raw))
    want = R.augment(raw, 2.0, -1.0, 2, 1, ds.seed, 1, 0)
    K.assert_bits(seen['fed'][0], want, "fed x_l_c")
    assert not np.array_equal(want, R.scale_u8(raw, 2.0, -1.0))
    # both evaluations saw the whole test split, scaled and not augmented
    assert len(seen['val']) == 2
    for batches in seen['val']:
        x = np.concatenate([b[0] for b in batches])
        assert _rows(x) == _rows(R.scale_u8(test_img, 2.0, -1.0))


def test_augment_entry_point_refuses_the_synthetic_dataset(monkeypatch, tmp_path):
    from tg import lib
    from Training import Train_goodGAN as TG

    class Flags(object):
        augment = True
    monkeypatch.setattr(TG, "_root_dir", lambda: str(tmp_path))
    with pytest.raises(lib.TgError, match="AUGMENT needs .*syntheticDataset"):
        TG._main_training_mnist(Flags(), epochs=1)
