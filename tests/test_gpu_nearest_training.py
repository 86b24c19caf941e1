"""The nearest training images of generated samples in the trainer: Train.nearest_training, tg.metrics.PixelBank /
nearest_pixels and config.SAMPLE_NEAREST in the epoch tail — on the MNIST model at the small counts of
tests/test_gpu_manifold_metrics.py (B_G = 8, N = 24, k = 3), against a 96-record training split in two TFRecord files and 64
validation images, and through _main_training_mnist.

Everything is exact: the distances are integers (tests/test_gpu_nearest_kernels.py holds the kernel to tests/nearest_reference.py), the
scalars are reduced in float64 on the host the same way on both sides, so they are compared with ==; the trainer's state is compared
byte for byte."""
import os
import struct

import numpy as np
import pytest

import gpu_common as G
import manifold_reference as MR
import nearest_reference as R
from oracle import step_goodgan as S

pytestmark = pytest.mark.gpu
SIZES = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
N_SAMPLES, N_VAL, VAL_BATCH, K = 24, 64, 32, 3
N_LAB, N_UNL = 40, 56                                                  # the two training files: 96 records
PLANT_VAL, PLANT_TRAIN = 5, 70                                         # training record 70 is an exact copy of validation image 5
D = 28 * 28
_CACHE = {}


def _val_u8():
    if 'val_u8' not in _CACHE:
        _CACHE['val_u8'] = np.random.default_rng(4).integers(0, 256, (N_VAL, 28, 28, 1), dtype=np.uint8)
        _CACHE['val_u8'].setflags(write=False)
    return _CACHE['val_u8']


def _val():
    """the 64 validation images as two batches of (x = u / 255, one-hot y): byte-representable, so quantising returns u."""
    if 'val' not in _CACHE:
        rng = np.random.default_rng(5)
        x = R.affine(_val_u8(), 1.0, 0.0)
        _CACHE['val'] = [(x[i:i + VAL_BATCH], np.eye(10, dtype=np.float32)[rng.integers(0, 10, VAL_BATCH)]) for i in range(0, N_VAL, VAL_BATCH)]
    return _CACHE['val']


def _write_split(root, test_images=None):
    """MNIST-named TFRecords under root/Tfrecord -> (training images [96, 784] uint8 in file order, labels [96])."""
    from tg import io as tgio
    from Input_Pipeline.mnistDataset import mnistDataset
    os.makedirs(os.path.join(root, 'Tfrecord'))
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (N_LAB + N_UNL, 28, 28, 1), dtype=np.uint8)
    lab = rng.integers(0, 10, N_LAB + N_UNL)
    img[PLANT_TRAIN] = _val_u8()[PLANT_VAL]
    names = mnistDataset(root, None, 100, 'train').get_filenames()
    tgio.write_tfrecord(names[0], img[:N_LAB], lab[:N_LAB])
    tgio.write_tfrecord(names[1], img[N_LAB:], lab[N_LAB:])
    if test_images is not None:
        tgio.write_tfrecord(mnistDataset(root, None, 100, 'test').get_filenames()[0], test_images, rng.integers(0, 10, len(test_images)))
    return img.reshape(len(img), -1), lab.astype(np.int32)


def _trained(tmp_path_factory):
    """one eager MNIST trainer after three iterations and the training Dataset, shared by the tests that only read them."""
    from Model.Good_GAN import Good_GAN
    from Input_Pipeline.mnistDataset import mnistDataset
    from tg import runtime
    if 'tr' not in _CACHE:
        import torch
        root = str(tmp_path_factory.mktemp('nearest'))
        _CACHE['train'] = _write_split(root)
        tr = G.fresh_trainer(G.make_config_goodgan('mnist', SIZES, SEED=7), None, Good_GAN)
        tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
        for i in range(3):
            tr.feed(S.synth_batch('mnist', 80 + i, SIZES))
            tr.sample_latent()
            tr.train_iteration()
        torch.cuda.synchronize()
        _CACHE['tr'], _CACHE['ds'] = tr, mnistDataset(root, tr.config, 100, 'train')
    runtime.set_context(_CACHE['tr'].cx)
    return _CACHE['tr'], _CACHE['ds'], _CACHE['train']


def _state(tr):
    import torch
    torch.cuda.synchronize()
    out = {'rng': tr.cx.rng.state.cpu().numpy().copy()}
    for net, st in tr.cx.stores.items():
        for buf in ('p', 'g', 'm', 'v', 's', 'step'):
            out[net + '/' + buf] = getattr(st, buf).detach().cpu().numpy().copy()
        if st.ema is not None:
            out[net + '/ema'] = st.ema.detach().cpu().numpy().copy()
    return out


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_the_pixel_pass_is_the_reference_on_the_same_bytes(tmp_path_factory, monkeypatch):
    from tg import io as tgio
    tr, ds, (train, labels) = _trained(tmp_path_factory)
    before = _state(tr)
    out, (fake, bank) = tr.nearest_training(ds, _val(), N_SAMPLES, K, return_banks=True)
    _same(_state(tr), before)                                          # stores, slots, shadows, running statistics, counters, Philox
    assert set(out) == {'nn_idx', 'nn_d2', 'nn_label', 'val_nn_d2'} | set(tr.NEAREST_KEYS)
    assert bank.n == 96 and tr.nearest_decoded == 96 and bank.numpy().tobytes() == train.tobytes()          # file order, record order
    samples = fake.numpy()
    assert samples.shape == (N_SAMPLES, D) and samples.dtype == np.uint8 and samples.std() > 0
    want_d2, want_idx = R.nearest(samples, train, K)
    assert out['nn_d2'].dtype == out['nn_idx'].dtype == out['nn_label'].dtype == np.int32
    assert (out['nn_d2'] == want_d2).all() and (out['nn_idx'] == want_idx).all() and (out['nn_label'] == labels[want_idx]).all()
    mean, low = R.scalars(want_d2, D)
    agree = float(np.mean(labels[want_idx[:, 0]] == np.arange(N_SAMPLES) % 10))
    v_d2, _ = R.nearest(_val_u8().reshape(N_VAL, -1)[:N_SAMPLES], train, 1)
    print("nearest: %r, reference %r" % ({k: out[k] for k in tr.NEAREST_KEYS}, (mean, low, agree, R.scalars(v_d2, D)[0])))
    assert (out['g_nn_rmse'], out['g_nn_rmse_min'], out['g_nn_class_agreement']) == (mean, low, agree)
    assert out['val_nn_rmse'] == R.scalars(v_d2, D)[0] and (out['val_nn_d2'] == v_d2[:, 0]).all()
    assert out['val_nn_d2'][PLANT_VAL] == 0 and (np.delete(out['val_nn_d2'], PLANT_VAL) > 0).all()          # the planted copy, and only it
    # a second call decodes nothing again, and says the same
    def refuse(*a, **kw):
        raise AssertionError("a training record was decoded again")
    monkeypatch.setattr(tgio.RecordFile, 'gather', refuse)
    again = tr.nearest_training(ds, iter(()), N_SAMPLES, K)            # (the control is cached too: the split is not read)
    assert tr.nearest_decoded == 96 and set(again) == set(out)
    for k in out:
        assert np.array_equal(again[k], out[k]), k
    part = tr.nearest_training(ds, _val(), N_SAMPLES - 3, 1)           # the head of the same samples, another k
    assert (part['nn_idx'] == want_idx[:N_SAMPLES - 3, :1]).all() and (part['nn_d2'] == want_d2[:N_SAMPLES - 3, :1]).all()
    for bad in (0, 17, True, None, 3.0):
        with pytest.raises(ValueError, match="nearest_training: k"):
            tr.nearest_training(ds, _val(), N_SAMPLES, bad)
    with pytest.raises(ValueError, match="space"):
        tr.nearest_training(ds, _val(), N_SAMPLES, K, space='latent')
    _same(_state(tr), before)


def test_the_feature_route_is_the_manifold_reference_on_the_banks(tmp_path_factory):
    tr, ds, _ = _trained(tmp_path_factory)
    before = _state(tr)
    out, (fake, train) = tr.nearest_training(ds, _val(), N_SAMPLES, 1, space='feature', return_banks=True)
    _same(_state(tr), before)
    q, r = fake.numpy(), train.numpy()
    assert q.shape == (N_SAMPLES, train.c) and r.shape == (96, train.c) and np.isfinite(q).all() and np.isfinite(r).all()
    _, nn, idx = MR.query(q, r)
    assert out['nn_idx'].shape == (N_SAMPLES, 1) and (out['nn_idx'][:, 0] == idx).all()
    assert out['nn_d2'][:, 0].tobytes() == np.asarray(nn, np.float32).tobytes()
    with pytest.raises(ValueError, match="k must be 1"):
        tr.nearest_training(ds, _val(), N_SAMPLES, 2, space='feature')


def _run_mnist(root, monkeypatch, **flags):
    from tg import runtime
    from Training import Train_goodGAN as TG
    from Input_Pipeline.mnistDataset import mnistDataset
    runtime.set_context(None)
    monkeypatch.setattr(TG, "_root_dir", lambda: str(root))
    np.random.seed(3)
    F = type('Flags', (object,), dict(dict(train_size=100, seed=1), **flags))              # BATCH_SIZE 100: one iteration per epoch
    return TG._main_training_mnist(F(), Dataset=mnistDataset, epochs=1)


def test_one_epoch_records_the_four_tags_writes_the_grid_and_changes_nothing_else(tmp_path, monkeypatch):
    roots = {}
    for name in ('on', 'off'):
        roots[name] = tmp_path / name
        _write_split(str(roots[name] / 'DataSet' / 'mnist'), _val_u8())
    on = _run_mnist(roots['on'], monkeypatch, sample_metrics=N_SAMPLES, sample_nearest=K)
    off = _run_mnist(roots['off'], monkeypatch, sample_metrics=N_SAMPLES)
    assert len(on) == len(off) == 1
    r_on, r_off = on[0], off[0]
    new = ('g_nn_rmse', 'g_nn_rmse_min', 'g_nn_class_agreement', 'val_nn_rmse')
    assert set(r_on) == set(r_off) | set(new) and not set(new) & set(r_off) and list(r_on)[-4:] == list(new)
    for k in r_off:
        if k != 'images_per_sec':                                      # (a wall-clock rate)
            assert r_on[k] == r_off[k], k
    assert np.isfinite([r_on[k] for k in new]).all() and 0.0 < r_on['g_nn_rmse_min'] <= r_on['g_nn_rmse'] < 1.0
    assert 0.0 <= r_on['g_nn_class_agreement'] <= 1.0 and 0.0 < r_on['val_nn_rmse'] < 1.0
    sample_dir = lambda root: os.path.join(str(root), 'Training', 'mnist_good_GAN_100')
    png = open(os.path.join(sample_dir(roots['on']), 'nearest_0001.png'), 'rb').read()
    assert png[:8] == b'\x89PNG\r\n\x1a\n' and png[12:16] == b'IHDR'
    assert struct.unpack('>II', png[16:24]) == ((1 + K) * 28, min(16, N_SAMPLES) * 28)     # the sample and its k nearest per row
    assert not [f for f in os.listdir(sample_dir(roots['off'])) if f.startswith('nearest')]
