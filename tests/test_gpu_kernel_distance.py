"""The unbiased kernel distance in the trainer: Train.sample_kernel_distance, tg.metrics.kernel_distance and
config.SAMPLE_KID in the epoch tail — on the MNIST model at the small counts of tests/test_gpu_manifold_metrics.py, and through
_main_training_mnist.

The distances are held to tests/kernel_distance_reference.py evaluated on the banked features with the same labels, within the bounds
of the three kernel sums (sum_bound) propagated through kid_from_sums; the five sample_metrics values and the trainer's state are
compared exactly."""
import os

import numpy as np
import pytest

import gpu_common as G
import kernel_distance_reference as R
from oracle import step_goodgan as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
N_SAMPLES, N_VAL, VAL_BATCH, NUM_CLASSES = 24, 64, 32, 10
OLD = {'val_accuracy', 'g_class_accuracy', 'frechet_distance', 'n_real', 'n_fake'}
PER_CLASS = ('kernel_distance_per_class', 'kernel_distance_worst', 'kernel_distance_worst_class')
_CACHE = {}


def _feeds():
    if 'feeds' not in _CACHE:
        _CACHE['feeds'] = [S.synth_batch('mnist', 80 + i, SIZES) for i in range(3)]
    return _CACHE['feeds']


def _val(drop=None):
    """the 64-image validation set as two batches of (x, one-hot y), made once, never written to; drop: the same images with every
    label of class `drop` moved to the next class (a class absent on the real side)."""
    if 'val' not in _CACHE:
        rng = np.random.default_rng(4)
        _CACHE['val'] = [(rng.uniform(0.0, 1.0, (VAL_BATCH, 28, 28, 1)).astype(np.float32), rng.integers(0, NUM_CLASSES, VAL_BATCH))
                         for _ in range(N_VAL // VAL_BATCH)]
    eye = np.eye(NUM_CLASSES, dtype=np.float32)
    return [(x, eye[np.where(lab == drop, (lab + 1) % NUM_CLASSES, lab)]) for x, lab in _CACHE['val']]


def _labels(val):
    return np.concatenate([np.argmax(y, axis=1) for _, y in val])


def _trained():
    """one eager trainer after three iterations, shared by the tests (each leaves it as it found it)."""
    import torch
    from tg import runtime
    from Model.Good_GAN import Good_GAN
    if 'tr' not in _CACHE:
        tr = G.fresh_trainer(G.make_config_goodgan('mnist', SIZES, SEED=7), None, Good_GAN)
        tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
        for feed in _feeds():
            tr.feed(feed)
            tr.sample_latent()
            tr.train_iteration()
        torch.cuda.synchronize()
        _CACHE['tr'] = tr
    runtime.set_context(_CACHE['tr'].cx)
    return _CACHE['tr']


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


def _same_result(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k], np.float64).tobytes() == np.asarray(b[k], np.float64).tobytes(), k


def _hold(got, real, fake, lab_real, lab_fake):
    """got's distances against the reference on the host rows, within the propagated bounds; NaN exactly where the reference has it."""
    want, tol = R.kernel_distance(real, fake, lab_real, lab_fake, NUM_CLASSES, with_bound=True)
    err = abs(got['kernel_distance'] - want['kernel_distance'])
    print("kernel_distance %.17g reference %.17g error %.3g bound %.3g" % (got['kernel_distance'], want['kernel_distance'], err,
                                                                          tol['kernel_distance']))
    assert err <= tol['kernel_distance']
    per, wper, tper = got['kernel_distance_per_class'], want['kernel_distance_per_class'], tol['kernel_distance_per_class']
    assert per.dtype == np.float64 and per.shape == (NUM_CLASSES,) and (np.isnan(per) == np.isnan(wper)).all()
    has = ~np.isnan(wper)
    print("per class %r\nreference %r\nbound     %r" % (per, wper, tper))
    assert (np.abs(per - wper)[has] <= tper[has]).all()
    if has.any():
        k = got['kernel_distance_worst_class']
        assert has[k] and got['kernel_distance_worst'] == per[k] == np.nanmax(per) and k == int(np.flatnonzero(per == np.nanmax(per))[0])
    else:
        assert np.isnan(got['kernel_distance_worst']) and got['kernel_distance_worst_class'] == -1
    return want


def test_the_pass_adds_the_distances_of_the_reference_on_the_banked_features_and_leaves_no_trace():
    from tg import metrics as M
    tr = _trained()
    val = _val()
    before = _state(tr)
    old = tr.sample_metrics(val, N_SAMPLES)
    assert set(old) == OLD
    got, (bank_real, bank_fake) = tr.sample_kernel_distance(val, N_SAMPLES, per_class=True, return_banks=True)
    _same(_state(tr), before)                                          # weights, shadows, slots, running state, steps, Philox state
    assert set(got) == OLD | set(M.KERNEL_DISTANCE_KEYS) and set(M.KERNEL_DISTANCE_KEYS) == {'kernel_distance'} | set(PER_CLASS)
    _same_result({k: got[k] for k in OLD}, old)                        # the five old values are sample_metrics's, bit for bit
    real, fake = bank_real.numpy(), bank_fake.numpy()
    assert real.shape == (N_VAL, bank_real.c) and fake.shape == (N_SAMPLES, bank_real.c) and np.isfinite(real).all() and np.isfinite(fake).all()
    lab_real, lab_fake = _labels(val), np.arange(N_SAMPLES) % NUM_CLASSES
    _hold(got, real, fake, lab_real, lab_fake)
    again = tr.sample_kernel_distance(val, N_SAMPLES, per_class=True)
    _same_result(again, got)                                           # a second call: the same bits
    whole = tr.sample_kernel_distance(val, N_SAMPLES)                  # without labels: the whole-set number alone, the same bits
    assert set(whole) == OLD | {'kernel_distance'}
    _same_result(whole, {k: got[k] for k in whole})
    _same_result(M.kernel_distance(bank_real, bank_fake, lab_real, lab_fake, NUM_CLASSES), {k: got[k] for k in M.KERNEL_DISTANCE_KEYS})
    _same(_state(tr), before)


def test_a_class_absent_on_one_side_is_nan_and_skipped_by_the_worst():
    tr = _trained()
    before = _state(tr)
    full = _labels(_val())
    drop = int(np.argmax(np.bincount(full, minlength=NUM_CLASSES)))
    val = _val(drop=drop)
    got, (bank_real, bank_fake) = tr.sample_kernel_distance(val, N_SAMPLES, per_class=True, return_banks=True)
    per = got['kernel_distance_per_class']
    assert np.isnan(per[drop]) and got['kernel_distance_worst_class'] != drop and np.isfinite(got['kernel_distance_worst'])
    want = _hold(got, bank_real.numpy(), bank_fake.numpy(), _labels(val), np.arange(N_SAMPLES) % NUM_CLASSES)
    assert np.isnan(want['kernel_distance_per_class'][drop])
    # one generated row per class: every class has fewer than two rows on that side
    few = tr.sample_kernel_distance(val, NUM_CLASSES, per_class=True)
    assert np.isnan(few['kernel_distance_per_class']).all() and np.isnan(few['kernel_distance_worst']) and few['kernel_distance_worst_class'] == -1
    assert np.isfinite(few['kernel_distance'])
    _same(_state(tr), before)


def test_non_finite_moments_give_nan_without_calling_the_kernel(monkeypatch):
    from tg import metrics as M
    tr = _trained()
    before = _state(tr)
    val = [(x.copy(), y) for x, y in _val()]
    val[1][0][5, 3, 3, 0] = np.inf                                     # one pixel: the moment sums of the real side are no longer finite

    def refuse(*a, **kw):
        raise AssertionError("the kernel distance was computed")
    monkeypatch.setattr(M, 'kernel_distance', refuse)
    monkeypatch.setattr(M, 'poly3_sums', refuse)
    got = tr.sample_kernel_distance(val, N_SAMPLES, per_class=True)
    assert set(got) == OLD | set(M.KERNEL_DISTANCE_KEYS) and np.isnan(got['kernel_distance']) and np.isnan(got['kernel_distance_worst'])
    assert np.isnan(got['kernel_distance_per_class']).all() and got['kernel_distance_per_class'].shape == (NUM_CLASSES,)
    assert got['kernel_distance_worst_class'] == -1
    _same(_state(tr), before)


def _run_mnist(root, monkeypatch, **flags):
    from tg import runtime
    from Training import Train_goodGAN as TG
    runtime.set_context(None)
    monkeypatch.setattr(TG, "_root_dir", lambda: str(root))
    np.random.seed(3)                                                                   # Train.train draws sample_z from NumPy's global generator
    F = type('Flags', (object,), dict(dict(train_size=2 * 100, seed=1), **flags))      # BATCH_SIZE 100: two iterations per epoch
    return TG._main_training_mnist(F(), epochs=1)


def test_the_setting_adds_its_two_records_and_the_file_and_changes_nothing_else(tmp_path, monkeypatch):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import read_events as RE
    on_root, off_root = tmp_path / 'on', tmp_path / 'off'
    on = _run_mnist(on_root, monkeypatch, sample_metrics=64, sample_kid='per_class')
    off = _run_mnist(off_root, monkeypatch, sample_metrics=64)
    new, old = ('kernel_distance', 'kernel_distance_worst'), ('g_class_accuracy', 'frechet_distance')
    assert len(on) == len(off) == 1
    r_on, r_off = on[0], off[0]
    assert set(r_on) == set(r_off) | set(new) and not set(new) & set(r_off)
    assert list(r_on)[-2:] == list(new)
    for k in r_off:
        if k != 'images_per_sec':                                                       # (a wall-clock rate)
            assert r_on[k] == r_off[k], k
    assert np.isfinite([r_on[k] for k in new]).all()

    def val_dir(root):
        rd = os.path.join(str(root), 'Training', 'Log_mnist', 'val')
        return os.path.join(rd, os.listdir(rd)[0])

    def val_events(rd):
        files = [f for f in os.listdir(rd) if f.startswith('events.out.tfevents.')]
        assert len(files) == 1
        return RE.read_events(os.path.join(rd, files[0]))[1:], open(os.path.join(rd, 'history.csv')).read().splitlines()

    (ev_on, csv_on), (ev_off, csv_off) = val_events(val_dir(on_root)), val_events(val_dir(off_root))
    assert len(ev_on) == len(ev_off) == 1
    assert csv_off[0] == 'step,val_accuracy,' + ','.join(old) and csv_on[0] == csv_off[0] + ',' + ','.join(new)
    e_on, e_off = ev_on[0], ev_off[0]
    assert set(e_off['scalars']) == {'val_accuracy'} | set(old) and set(e_on['scalars']) == set(e_off['scalars']) | set(new)
    for k in e_off['scalars']:
        assert e_on['scalars'][k] == e_off['scalars'][k], k
    for k in new:
        assert e_on['scalars'][k] == np.float32(r_on[k]), k
    name = 'kid_per_class_%04d.npy' % r_on['epoch']
    per = np.load(os.path.join(val_dir(on_root), name))
    assert per.dtype == np.float64 and per.shape == (NUM_CLASSES,) and np.nanmax(per) == r_on['kernel_distance_worst']
    assert not [f for f in os.listdir(val_dir(off_root)) if f.startswith('kid_per_class')]      # with the setting off, nothing is added


def test_the_setting_without_sample_metrics_is_refused(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="SAMPLE_KID"):
        _run_mnist(tmp_path, monkeypatch, sample_kid=True)
