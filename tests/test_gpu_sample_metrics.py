"""The averaged classifier and the generated-sample metrics in the trainer: Train.evaluate(ema=True), the CIFAR
classifier's `getter`, Train.sample_metrics and the two settings in the epoch tail — on the CIFAR-10 model (ZCA, weight norm and
mean-only BN are where reading the shadows can go wrong) at the small sizes of tests/test_gpu_wn_init_step.py, and through
_main_training_mnist.

What is exact and why: an evaluation with the shadows runs the kernels of a raw evaluation on other operand bits at the same offsets
of another buffer, so it must equal, bit for bit, a raw evaluation after the shadows were copied over the weights by hand; accuracies
are counts, compared with NumPy's arg-max of logits fetched in a separate pass (the input noise is a function of the Philox state,
which no pass here advances).  The Fréchet distance is held to TOL_FD = 1e-6 of scale = tr C1 + tr C2 + |dm|^2 (tests/
sample_metrics_reference.py) where the covariances have full rank — a 2-channel slice of the real features, n >= 2c — and only to
finite and >= -TOL_FD * scale on the 128 channels, where 24 samples leave the covariance rank-deficient."""
import os

import numpy as np
import pytest

import gpu_common as G
import sample_metrics_reference as R
from oracle import step_cifar10 as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
N_SAMPLES, N_VAL, VAL_BATCH = 24, 64, 32
_CACHE = {}


def _feeds():
    if 'feeds' not in _CACHE:
        _CACHE['feeds'] = [S.synth_batch(80 + i, dict(S.SIZES, **SIZES)) for i in range(4)]
    return _CACHE['feeds']


def _val():
    """the 64-image validation set as two batches of (x, one-hot y); made once, never written to."""
    if 'val' not in _CACHE:
        rng = np.random.default_rng(4)
        out = []
        for _ in range(N_VAL // VAL_BATCH):
            x = rng.uniform(-1.0, 1.0, (VAL_BATCH, 32, 32, 3)).astype(np.float32)
            y = np.eye(10, dtype=np.float32)[rng.integers(0, 10, VAL_BATCH)]
            out.append((x, y))
        _CACHE['val'] = out
    return _CACHE['val']


def _iterate(tr, which):
    import torch
    for i in which:
        tr.feed(_feeds()[i])
        tr.sample_latent()
        tr.train_iteration()
    torch.cuda.synchronize()


def _new(iterations=3, **over):
    tr = G.fresh_trainer(G.make_config(SIZES, SEED=7, **over), S.init_params(0))
    tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
    _iterate(tr, range(iterations))
    return tr


def _trained():
    """one eager trainer after three iterations, shared by the tests that only read it (each leaves it as it found it)."""
    from tg import runtime
    if 'tr' not in _CACHE:
        _CACHE['tr'] = _new()
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


def _classify(tr, x, getter=None, generated_from=None):
    """(logits, feature) host arrays of classifier(x, False) as evaluate runs it; generated_from=(z, y): x = good_sampler(z, y)."""
    cx, m = tr.cx, tr.model
    with cx.phase_scope('test_fetch', record=False):
        if generated_from is not None:
            xa = m.as_image(m.good_sampler(cx.from_numpy(generated_from[0]), cx.from_numpy(generated_from[1])))
        else:
            xa = m.as_image(cx.from_numpy(x))
        xa = m.zca().apply(xa)
        with cx.rng_scoped('val/C'):
            logits, fm = m.classifier(xa, False, getter=getter)
        return logits.numpy().copy(), fm.numpy().copy()


def _accuracy(logit_batches, label_batches):
    hit = sum(int((np.argmax(l, axis=1) == np.argmax(y, axis=1)).sum()) for l, y in zip(logit_batches, label_batches))
    return hit / float(sum(len(y) for y in label_batches))


def test_ema_evaluation_is_the_raw_evaluation_of_hand_copied_shadows_and_leaves_no_trace():
    tr = _trained()
    st = tr.cx.stores['classifier']
    val = _val()
    before = _state(tr)
    assert not np.array_equal(before['classifier/ema'], before['classifier/p'])          # three C-updates moved the weights off their shadows
    acc_ema = tr.evaluate(val, ema=True)
    _same(_state(tr), before)
    assert tr.cx.prep_cache is None and not st.read_ema
    shadow = [_classify(tr, x, getter=True) for x, _ in val]
    raw = [_classify(tr, x) for x, _ in val]
    _same(_state(tr), before)
    acc_raw = tr.evaluate(val)
    # by hand: the shadows over the weights, a raw evaluation, the weights back
    kept = st.p.clone()
    st.p.copy_(st.ema)
    acc_hand = tr.evaluate(val)
    hand = [_classify(tr, x) for x, _ in val]
    st.p.copy_(kept)
    _same(_state(tr), before)
    print("accuracy: raw %.4f, shadows %.4f, by hand %.4f" % (acc_raw, acc_ema, acc_hand))
    assert acc_ema == acc_hand == _accuracy([l for l, _ in shadow], [y for _, y in val])
    assert acc_raw == _accuracy([l for l, _ in raw], [y for _, y in val])
    for (l_s, f_s), (l_h, f_h), (l_r, f_r) in zip(shadow, hand, raw):
        assert l_s.tobytes() == l_h.tobytes() and f_s.tobytes() == f_h.tobytes()       # the getter reads exactly the shadows
        assert not np.array_equal(l_s, l_r)                                             # ... which are not the weights
    # pop_mean is read from the store as it is: moving it moves the averaged evaluation too
    nm = 'classifier/conv1_1/meanOnlyBatchNormalization/pop_mean'
    pop = st.get(nm).copy()
    st.set(nm, pop + 0.5)
    moved, _ = _classify(tr, val[0][0], getter=True)
    st.set(nm, pop)
    assert not np.array_equal(moved, shadow[0][0])
    _same(_state(tr), before)


def test_the_shadows_are_refused_inside_the_step_and_for_a_network_without_them():
    from tg import lib
    tr = _trained()
    with pytest.raises(lib.TgError, match="no EMA shadows"):
        with tr.cx.reading_shadows('discriminator'):
            pass
    tr.cx.prep_cache = {}
    try:
        with pytest.raises(lib.TgError, match="inside a training iteration"):
            tr.evaluate(_val(), ema=True)
    finally:
        tr.cx.prep_cache = None
    assert not tr.cx.stores['classifier'].read_ema


@pytest.mark.parametrize("mode", ["eager", "plan"])
def test_a_twin_that_never_evaluated_is_bit_identical_after_the_next_iteration(mode):
    """the plan is recorded in the second iteration and replayed from the third: the passes run while it holds its buffers' addresses."""
    over = dict(EXEC_MODE='plan', USE_HIP_GRAPH=None) if mode == 'plan' else {}
    a = _new(**over)
    acc = a.evaluate(_val(), ema=True)
    m = a.sample_metrics(_val(), N_SAMPLES, ema=True)
    assert m['val_accuracy'] == acc
    _iterate(a, [3])
    got = _state(a)
    b = _new(**over)
    _iterate(b, [3])
    _same(got, _state(b))
    if mode == 'plan':
        assert all(p is not None for p in a.executor.replay['full'].plans)              # the fourth iteration did replay plans


def test_sample_metrics_against_numpy_on_separately_fetched_logits_and_features():
    from tg import metrics as M
    from tg.runtime import Act
    tr = _trained()
    val = _val()
    before = _state(tr)
    np_state = np.random.get_state()[1].copy()
    m = tr.sample_metrics(val, N_SAMPLES)
    _same(_state(tr), before)                                                           # stores (running statistics included) and Philox state
    assert (np.random.get_state()[1] == np_state).all()                                 # NumPy's global generator was not drawn from
    assert tr.sample_metrics(val, N_SAMPLES) == m                                       # the same latents, the same numbers
    assert set(m) == {'val_accuracy', 'g_class_accuracy', 'frechet_distance', 'n_real', 'n_fake'}
    assert (m['n_real'], m['n_fake']) == (N_VAL, N_SAMPLES)
    # separately: the same passes, logits and features fetched to the host
    B = SIZES['B_G']
    z, y = tr._sample_latents(N_SAMPLES // B)
    assert z.shape == (N_SAMPLES, 100) and (np.argmax(y, axis=1) == np.arange(N_SAMPLES) % 10).all() and np.abs(z).max() < 1.0
    real = [_classify(tr, x) for x, _ in val]
    fake = [_classify(tr, None, generated_from=(z[k:k + B], y[k:k + B])) for k in range(0, N_SAMPLES, B)]
    assert m['val_accuracy'] == _accuracy([l for l, _ in real], [yb for _, yb in val]) == tr.evaluate(val)
    assert m['g_class_accuracy'] == _accuracy([l for l, _ in fake], [y[k:k + B] for k in range(0, N_SAMPLES, B)])
    f_real, f_fake = np.concatenate([f for _, f in real]), np.concatenate([f for _, f in fake])
    assert f_real.shape == (N_VAL, 128) and f_fake.shape == (N_SAMPLES, 128)
    # full rank: a 2-channel slice (n >= 2c on both sides) through the device moments, against np.cov and the eigvals route
    dev = {}
    for key, f in (('real', f_real), ('fake', f_fake)):
        act = tr.cx.from_numpy(f)
        dev[key] = M.FeatureMoments(2, tr.cx.device).add(Act(act.t, act.n, 1, 1, 2, act.ld)).result()
    (n1, m1, C1), (n2, m2, C2) = R.mean_cov64(f_real[:, :2]), R.mean_cov64(f_fake[:, :2])
    assert (dev['real'][0], dev['fake'][0]) == (n1, n2) == (N_VAL, N_SAMPLES)
    scale2 = R.fd_scale(m1, C1, m2, C2)
    got2, want2 = M.frechet_distance(*(dev['real'][1:] + dev['fake'][1:])), R.frechet_eigvals(m1, C1, m2, C2)
    print("2 channels: distance %.9g, reference %.9g, scale %.3g" % (got2, want2, scale2))
    assert abs(got2 - want2) <= R.TOL_FD * scale2
    # 128 channels, 24 samples: rank-deficient — finite, not negative beyond the noise, and the number the same features give again
    (_, mr, Cr), (_, mf, Cf) = R.mean_cov64(f_real), R.mean_cov64(f_fake)
    scale = R.fd_scale(mr, Cr, mf, Cf)
    print("128 channels: distance %.9g, scale %.3g" % (m['frechet_distance'], scale))
    assert np.isfinite(m['frechet_distance']) and m['frechet_distance'] >= -R.TOL_FD * scale
    again = {}
    for key, f in (('real', f_real), ('fake', f_fake)):
        again[key] = M.FeatureMoments(128, tr.cx.device).add(tr.cx.from_numpy(f)).result()
    assert abs(M.frechet_distance(*(again['real'][1:] + again['fake'][1:])) - m['frechet_distance']) <= R.TOL_FD * scale
    for s_b, kept in ((tr.cx.stores[net].s, before[net + '/s']) for net in tr.cx.stores):   # the fetches above ran the sampler: put `s` back
        s_b.copy_(s_b.new_tensor(kept))
    _same(_state(tr), before)
    # a count that is no multiple of the batch: the last batch is generated whole, its first rows are scored
    part = tr.sample_metrics(val, N_SAMPLES - 3)
    assert part['n_fake'] == N_SAMPLES - 3 and part['val_accuracy'] == m['val_accuracy']
    assert part['g_class_accuracy'] == _accuracy([np.concatenate([l for l, _ in fake])[:N_SAMPLES - 3]], [y[:N_SAMPLES - 3]])
    with pytest.raises(ValueError, match="n_samples"):
        tr.sample_metrics(val, 0)
    _same(_state(tr), before)


def _run_mnist(root, monkeypatch, **flags):
    from tg import runtime
    from Training import Train_goodGAN as TG
    runtime.set_context(None)
    monkeypatch.setattr(TG, "_root_dir", lambda: str(root))
    np.random.seed(3)                                                                   # Train.train draws sample_z from NumPy's global generator
    F = type('Flags', (object,), dict(dict(train_size=2 * 100, seed=1), **flags))      # BATCH_SIZE 100: two iterations per epoch
    return TG._main_training_mnist(F(), epochs=2)


def test_the_settings_add_their_records_and_change_nothing_else(tmp_path, monkeypatch, capsys):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import read_events as RE
    on_root, off_root = tmp_path / 'on', tmp_path / 'off'
    on = _run_mnist(on_root, monkeypatch, eval_ema=True, sample_metrics=64)
    lines_on = [l for l in capsys.readouterr().out.splitlines() if l.startswith('epoch ')]
    off = _run_mnist(off_root, monkeypatch)
    lines_off = [l for l in capsys.readouterr().out.splitlines() if l.startswith('epoch ')]
    new = ('val_accuracy_ema', 'g_class_accuracy', 'frechet_distance')
    assert len(on) == len(off) == 2
    for r_on, r_off in zip(on, off):
        assert set(r_on) == set(r_off) | set(new) and not set(new) & set(r_off)
        for k in r_off:
            if k != 'images_per_sec':                                                   # (a wall-clock rate)
                assert r_on[k] == r_off[k], k
        assert np.isfinite([r_on[k] for k in new]).all()
        assert 0.0 <= r_on['val_accuracy_ema'] <= 1.0 and 0.0 <= r_on['g_class_accuracy'] <= 1.0
    for l_on, l_off in zip(lines_on, lines_off):                                         # the printed line: today's, then the new values
        head = l_off[:l_off.index(' img/s')].rsplit(' ', 1)[0]
        assert l_on.startswith(head) and all(' %s ' % k in l_on for k in new) and not any(k in l_off for k in new)

    def val_events(root):
        rd = os.path.join(str(root), 'Training', 'Log_mnist', 'val')
        rd = os.path.join(rd, os.listdir(rd)[0])
        files = [f for f in os.listdir(rd) if f.startswith('events.out.tfevents.')]
        assert len(files) == 1
        return RE.read_events(os.path.join(rd, files[0]))[1:], open(os.path.join(rd, 'history.csv')).read().splitlines()

    ev_on, csv_on = val_events(on_root)
    ev_off, csv_off = val_events(off_root)
    assert len(ev_on) == len(ev_off) == 2
    assert csv_off[0] == 'step,val_accuracy' and csv_on[0] == 'step,val_accuracy,' + ','.join(new)
    for e_on, e_off, r_on in zip(ev_on, ev_off, on):
        assert set(e_off['scalars']) == {'val_accuracy'} and set(e_on['scalars']) == {'val_accuracy'} | set(new)
        assert e_on['step'] == e_off['step'] == r_on['epoch']
        for k in ('val_accuracy',) + new:
            assert e_on['scalars'][k] == np.float32(r_on[k]), k
