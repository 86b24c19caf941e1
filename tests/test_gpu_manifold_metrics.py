"""The k-nearest-neighbour manifold metrics in the trainer: Train.sample_manifold_metrics, tg.metrics.FeatureBank /
manifold_metrics and config.SAMPLE_MANIFOLD_K in the epoch tail — on the MNIST model at the small counts of
tests/test_gpu_sample_metrics.py, and through _main_training_mnist.

Everything is exact: the kernels compute a fixed fp32 chain that tests/manifold_reference.py restates (tests/
test_gpu_manifold_kernels.py holds them to it bit for bit), the four numbers are ratios of counts reduced in float64 on the host the
same way on both sides, so they are compared with ==; the trainer's state is compared byte for byte."""
import os

import numpy as np
import pytest

import gpu_common as G
import manifold_reference as R
from oracle import step_goodgan as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
N_SAMPLES, N_VAL, VAL_BATCH, K = 24, 64, 32, 3
OLD = {'val_accuracy', 'g_class_accuracy', 'frechet_distance', 'n_real', 'n_fake'}
_CACHE = {}


def _feeds():
    if 'feeds' not in _CACHE:
        _CACHE['feeds'] = [S.synth_batch('mnist', 80 + i, SIZES) for i in range(4)]
    return _CACHE['feeds']


def _val():
    """the 64-image validation set as two batches of (x, one-hot y); made once, never written to."""
    if 'val' not in _CACHE:
        rng = np.random.default_rng(4)
        _CACHE['val'] = [(rng.uniform(0.0, 1.0, (VAL_BATCH, 28, 28, 1)).astype(np.float32),
                          np.eye(10, dtype=np.float32)[rng.integers(0, 10, VAL_BATCH)]) for _ in range(N_VAL // VAL_BATCH)]
    return _CACHE['val']


def _iterate(tr, which):
    import torch
    for i in which:
        tr.feed(_feeds()[i])
        tr.sample_latent()
        tr.train_iteration()
    torch.cuda.synchronize()


def _new(iterations=3, **over):
    from Model.Good_GAN import Good_GAN
    tr = G.fresh_trainer(G.make_config_goodgan('mnist', SIZES, SEED=7, **over), None, Good_GAN)
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


def test_the_manifold_pass_adds_four_numbers_that_are_the_reference_on_the_banked_features():
    from tg import metrics as M
    tr = _trained()
    val = _val()
    before = _state(tr)
    old = tr.sample_metrics(val, N_SAMPLES)
    assert set(old) == OLD
    m, (bank_real, bank_fake) = tr.sample_manifold_metrics(val, N_SAMPLES, K, return_banks=True)
    _same(_state(tr), before)                                          # stores, running statistics, step counters and the Philox state
    assert set(m) == OLD | set(R.KEYS)
    assert {k: m[k] for k in OLD} == old                               # the five old values are those of sample_metrics
    assert tr.sample_manifold_metrics(val, N_SAMPLES, manifold_k=K) == m                # the same latents, the same numbers
    real, fake = bank_real.numpy(), bank_fake.numpy()
    assert real.shape == (N_VAL, bank_real.c) and fake.shape == (N_SAMPLES, bank_real.c) and real.dtype == np.float32
    assert np.isfinite(real).all() and np.isfinite(fake).all() and (m['n_real'], m['n_fake']) == (N_VAL, N_SAMPLES)
    want = R.metrics(real, fake, K)
    print("manifold metrics %r, reference %r" % ({k: m[k] for k in R.KEYS}, want))
    assert {k: m[k] for k in R.KEYS} == want
    assert all(0.0 <= m[k] <= 1.0 for k in ('precision', 'recall', 'coverage')) and m['density'] >= 0.0
    radii_real = M.knn_self(bank_real.rows(), K).cpu().numpy()
    assert radii_real.tobytes() == R.knn_self(real, K).tobytes()
    assert M.manifold_metrics(bank_real, bank_fake, K) == want         # the banks alone give the numbers again
    # another k: other radii, again the reference's numbers
    m1 = tr.sample_manifold_metrics(val, N_SAMPLES, 1)
    assert {k: m1[k] for k in R.KEYS} == R.metrics(real, fake, 1) and {k: m1[k] for k in OLD} == old
    # a cut at N - 3 samples: the last batch is generated whole and its first rows banked; the real side does not move
    part, (p_real, p_fake) = tr.sample_manifold_metrics(val, N_SAMPLES - 3, K, return_banks=True)
    assert part['n_fake'] == p_fake.n == N_SAMPLES - 3 and p_real.n == N_VAL
    assert p_fake.numpy().tobytes() == fake[:N_SAMPLES - 3].tobytes() and p_real.numpy().tobytes() == real.tobytes()
    assert M.knn_self(p_real.rows(), K).cpu().numpy().tobytes() == radii_real.tobytes()
    assert {k: part[k] for k in R.KEYS} == R.metrics(real, fake[:N_SAMPLES - 3], K)
    # fewer than k + 1 generated rows: NaN, and the rest of the result as it is
    few = tr.sample_manifold_metrics(val, K, K)
    assert all(np.isnan(few[k]) for k in R.KEYS) and few['n_fake'] == K and few['val_accuracy'] == old['val_accuracy']
    for bad in (0, 17, True, -1, None, 3.0):
        with pytest.raises(ValueError, match="manifold_k"):
            tr.sample_manifold_metrics(val, N_SAMPLES, bad)
    _same(_state(tr), before)


def test_non_finite_moments_give_nan_without_calling_the_kernels(monkeypatch):
    from tg import metrics as M
    tr = _trained()
    before = _state(tr)
    val = [(x.copy(), y) for x, y in _val()]
    val[1][0][5, 3, 3, 0] = np.inf                                     # one pixel: the moment sums of the real side are no longer finite

    def refuse(*a, **kw):
        raise AssertionError("manifold_metrics was called")
    monkeypatch.setattr(M, 'manifold_metrics', refuse)
    m = tr.sample_manifold_metrics(val, N_SAMPLES, K)
    assert set(m) == OLD | set(R.KEYS) and all(np.isnan(m[k]) for k in R.KEYS) and np.isnan(m['frechet_distance'])
    _same(_state(tr), before)


def test_the_bank_grows_and_refuses_a_recording():
    import torch
    from tg import lib, metrics as M, plan
    tr = _trained()
    cx = tr.cx
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((700, 5)).astype(np.float32)
    bank = M.FeatureBank(5, cx.device)
    for lo, hi in ((0, 3), (3, 300), (300, 700)):                      # past the first allocation of 256 rows, twice
        bank.add(cx.from_numpy(rows[lo:hi], ld=8), cx.stream)
    assert bank.n == 700 and bank.numpy().tobytes() == rows.tobytes()
    assert bank.reset().n == 0 and bank.numpy().shape == (0, 5)
    with pytest.raises(lib.TgError, match=r"fp32 \[n, 5\]"):
        bank.add(cx.from_numpy(rows[:4, :3]), cx.stream)
    torch.cuda.synchronize()
    p = plan.Plan([cx.stream.value])
    with p.recording():
        with pytest.raises(lib.TgError, match="launch-plan recording"):
            bank.add(cx.from_numpy(rows[:4], ld=8), cx.stream)
    assert bank.n == 0


@pytest.mark.parametrize("mode", ["eager", "plan"])
def test_a_twin_that_never_called_it_is_bit_identical_after_the_next_iteration(mode):
    """the plan is recorded in the second iteration and replayed from the third: the pass runs while it holds its buffers' addresses."""
    over = dict(EXEC_MODE='plan', USE_HIP_GRAPH=None) if mode == 'plan' else {}
    a = _new(**over)
    m = a.sample_manifold_metrics(_val(), N_SAMPLES, K)
    assert all(np.isfinite(m[k]) for k in R.KEYS)
    _iterate(a, [3])
    got = _state(a)
    b = _new(**over)
    _iterate(b, [3])
    _same(got, _state(b))
    if mode == 'plan':
        assert all(p is not None for p in a.executor.replay['full'].plans)              # the fourth iteration did replay plans


def _run_mnist(root, monkeypatch, **flags):
    from tg import runtime
    from Training import Train_goodGAN as TG
    runtime.set_context(None)
    monkeypatch.setattr(TG, "_root_dir", lambda: str(root))
    np.random.seed(3)                                                                   # Train.train draws sample_z from NumPy's global generator
    F = type('Flags', (object,), dict(dict(train_size=2 * 100, seed=1), **flags))      # BATCH_SIZE 100: two iterations per epoch
    return TG._main_training_mnist(F(), epochs=2)


def test_the_setting_adds_its_four_records_and_changes_nothing_else(tmp_path, monkeypatch, capsys):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import read_events as RE
    on_root, off_root = tmp_path / 'on', tmp_path / 'off'
    on = _run_mnist(on_root, monkeypatch, sample_metrics=64, sample_manifold_k=K)
    lines_on = [l for l in capsys.readouterr().out.splitlines() if l.startswith('epoch ')]
    off = _run_mnist(off_root, monkeypatch, sample_metrics=64)
    lines_off = [l for l in capsys.readouterr().out.splitlines() if l.startswith('epoch ')]
    new, old = R.KEYS, ('g_class_accuracy', 'frechet_distance')
    assert len(on) == len(off) == 2 and len(lines_on) == len(lines_off) == 2
    for r_on, r_off in zip(on, off):
        assert set(r_on) == set(r_off) | set(new) and not set(new) & set(r_off)
        assert list(r_on)[-4:] == list(new)                                             # after the values of the setting they extend
        for k in r_off:
            if k != 'images_per_sec':                                                   # (a wall-clock rate)
                assert r_on[k] == r_off[k], k
        assert np.isfinite([r_on[k] for k in new]).all()
        assert all(0.0 <= r_on[k] <= 1.0 for k in ('precision', 'recall', 'coverage')) and r_on['density'] >= 0.0
    for l_on, l_off, r_on in zip(lines_on, lines_off, on):                              # the printed line: today's, then the new values
        head, tail = l_off[:l_off.index(' img/s')].rsplit(' ', 1)[0], l_off[l_off.index(' img/s'):]
        assert l_on.startswith(head) and not any(' %s ' % k in l_off for k in new)
        assert l_on[l_on.index(' img/s'):] == tail + "".join(" %s %.4f" % (k, r_on[k]) for k in new)

    def val_events(root):
        rd = os.path.join(str(root), 'Training', 'Log_mnist', 'val')
        rd = os.path.join(rd, os.listdir(rd)[0])
        files = [f for f in os.listdir(rd) if f.startswith('events.out.tfevents.')]
        assert len(files) == 1
        return RE.read_events(os.path.join(rd, files[0]))[1:], open(os.path.join(rd, 'history.csv')).read().splitlines()

    ev_on, csv_on = val_events(on_root)
    ev_off, csv_off = val_events(off_root)
    assert len(ev_on) == len(ev_off) == 2
    assert csv_off[0] == 'step,val_accuracy,' + ','.join(old) and csv_on[0] == csv_off[0] + ',' + ','.join(new)
    for e_on, e_off, r_on in zip(ev_on, ev_off, on):
        assert set(e_off['scalars']) == {'val_accuracy'} | set(old) and set(e_on['scalars']) == set(e_off['scalars']) | set(new)
        assert e_on['step'] == e_off['step'] == r_on['epoch']
        for k in e_off['scalars']:
            assert e_on['scalars'][k] == e_off['scalars'][k], k
        for k in new:
            assert e_on['scalars'][k] == np.float32(r_on[k]), k


def test_the_setting_without_sample_metrics_is_refused(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="SAMPLE_MANIFOLD_K"):
        _run_mnist(tmp_path, monkeypatch, sample_manifold_k=K)
