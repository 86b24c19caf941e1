"""tg_eval_report_f32 (include/tg_kernels.h, csrc/evalreport.hip) against its row-by-row float64 restatement
(tests/eval_report_reference.py), and the report in the trainer: Train.evaluate(report=), evaluate_report, sample_metrics_report
and config.EVAL_REPORT in the epoch tail.

What is exact and why: the five integer outputs are counts decided by fp32 comparisons and by one fp64 bin index, and the inputs are
redrawn on the host until every row's conf * nb lies at least 1e-9 from an integer in the reference — a million times the error either
side can make in conf — so the bin is unambiguous and every count must EQUAL the reference's.  The three fp64 accumulations are held to
the reference's bound (k + n + 64) 2^-52 sum |terms|, derived in the reference's docstring.  Logits are N(0, 3^2); columns k.. of the
logits and of the labels hold NaN (one read of them would turn a row non-finite or move an arg-max); every output and the workspace
sit between guard words that must keep their bits.  In the trainer, accuracies and confusion matrices are counts: compared exactly with
evaluate's own return value and with the reference run on logits fetched in a separate pass (the input noise is a function of the
Philox state, which no pass here advances)."""
import os

import numpy as np
import pytest
import torch

import eval_report_reference as R
import gpu_common as G
from kernel_check import dev, guarded, lib, ptr, st
from oracle import step_cifar10 as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 2, 2), (77, 10, 32), (257, 11, 11), (130, 100, 128), (5, 1024, 1100)]
NR, NB = 16, 15
TG_ERR_INVALID = -1
INT_KEYS = ('confusion', 'rank_hist', 'bin_count', 'bin_correct', 'nonfinite')
F64_KEYS = ('bin_conf', 'sums')
_DATA = {}


class Outputs(object):
    """the seven outputs of a call at (k, nr, nb), each an allocation of its own with guard words in front and behind, zeroed (or filled
    with `poison`, a float pattern, for the refusals)."""
    ORDER = ('confusion', 'rank_hist', 'bin_count', 'bin_correct', 'bin_conf', 'sums', 'nonfinite')          # the C argument order

    def __init__(self, k, nr, nb, poison=None):
        self.k = k
        self.sizes = dict(confusion=k * k, rank_hist=nr, bin_count=nb, bin_correct=nb, bin_conf=nb, sums=2, nonfinite=1)
        fill = lambda n: np.zeros(2 * n, np.float32) if poison is None else np.full(2 * n, poison, np.float32)
        self.g = {key: guarded(2 * n, offset=2, fill=fill(n)) for key, n in self.sizes.items()}

    def args(self, **swap):
        return tuple(swap[key] if key in swap else self.g[key].ptr for key in self.ORDER)

    def get(self):
        """{name: host array} after the guards were checked (synchronises)."""
        out = {}
        for key, g in self.g.items():
            g.check_guard()
            raw = g.get()
            out[key] = raw.view(np.float64) if key in F64_KEYS else raw.view(np.int64)
        out['confusion'] = out['confusion'].reshape(self.k, self.k)
        return out

    def raw_bytes(self):
        return {key: g.get().tobytes() for key, g in self.g.items()}


def workspace(n, k, fill=None):
    need = lib().call('tg_eval_report_workspace_bytes', n, k)
    assert need % 8 == 0
    return guarded(max(need // 4, 4), offset=4, fill=fill), need


def data(n, k, ld):
    """(logits [n, ld], labels [n, ld_y], reference) — N(0, 3^2) logits and one-hot labels in columns 0..k-1, NaN in the padding; rows whose
    conf * NB lies within 1e-9 of an integer in the reference are redrawn, all of them, until none does.  Made once per shape."""
    key = (n, k, ld)
    if key not in _DATA:
        rng = np.random.default_rng(100000 * n + 100 * k + ld)
        ld_y = k if ld == k else k + 3
        logits, labels = np.full((n, ld), np.nan, np.float32), np.full((n, ld_y), np.nan, np.float32)
        logits[:, :k] = (rng.standard_normal((n, k)) * 3).astype(np.float32)
        labels[:, :k] = np.eye(k, dtype=np.float32)[rng.integers(0, k, n)]
        for _ in range(100):
            ref = R.reference(logits, labels, k, NR if NR < k else k, NB)
            close = np.flatnonzero(ref['finite'] & (ref['bin_distance'] < 1e-9))
            if close.size == 0:
                break
            logits[close, :k] = (rng.standard_normal((close.size, k)) * 3).astype(np.float32)
        assert ref['finite'].all() and (ref['bin_distance'] >= 1e-9).all()
        logits.setflags(write=False), labels.setflags(write=False)
        _DATA[key] = (logits, labels, ref)
    return _DATA[key]


def run(logits, labels, k, nr=NR, nb=NB, into=None, dirty=None):
    """one call on host matrices -> the Outputs it accumulated into (guards of the workspace checked)."""
    L = lib()
    n = logits.shape[0]
    nr = min(nr, k)
    out = into if into is not None else Outputs(k, nr, nb)
    gw, need = workspace(n, k, fill=dirty)
    L.call('tg_eval_report_f32', ptr(dev(np.array(logits))), logits.shape[1], ptr(dev(np.array(labels))), labels.shape[1], n, k, nr, nb, *out.args(),
           gw.ptr, need, st())
    gw.check_guard()
    return out


def check(got, ref, what):
    """integers exactly; the fp64 sums within the reference's bound (figures printed first)."""
    for key in INT_KEYS:
        assert got[key].dtype == np.int64 and (got[key] == ref[key]).all(), "%s: %s differs from the reference" % (what, key)
    e_s, e_b = np.abs(got['sums'] - ref['sums']), np.abs(got['bin_conf'] - ref['bin_conf'])
    print("%s: |sums - ref| = %s of bounds %s; worst bin_conf error %.3g of its bound (%d bins in use)" % (
        what, e_s, ref['bound_sums'], (e_b / (ref['bound_bin_conf'] + 1e-300)).max(), int((ref['bin_count'] > 0).sum())))
    assert np.isfinite(got['sums']).all() and np.isfinite(got['bin_conf']).all()
    assert (e_s <= ref['bound_sums']).all() and (e_b <= ref['bound_bin_conf']).all(), what
    assert (got['bin_conf'][ref['bin_count'] == 0] == 0.0).all()


@pytest.mark.parametrize("n,k,ld", SHAPES)
def test_kernel_matches_the_reference(n, k, ld):
    logits, labels, ref = data(n, k, ld)
    got = run(logits, labels, k).get()
    assert got['confusion'].sum() == n == got['rank_hist'].sum() == got['bin_count'].sum() and got['nonfinite'][0] == 0
    check(got, ref, "n %d k %d ld %d" % (n, k, ld))


def special_rows(k):
    """(logits [8, k], targets [8]) of the rows whose outcome the interface spells out — the four finite ones first."""
    hi = (2, 7) if k == 10 else (1, 3)
    rows = np.zeros((8, k), np.float32)
    rows[0] = np.linspace(-2.0, 1.0, k)
    rows[0, list(hi)] = 4.25                                     # the maximum twice, target the second: prediction the first, rank 1
    rows[1] = 0.5                                                # all equal: prediction 0, conf 1 / k
    rows[2] = -100.0
    rows[2, k - 1] = 100.0                                       # saturated, gap 200: conf exactly 1, NLL of the right target 0
    rows[3] = -6000.0
    rows[3, 0], rows[3, 1] = 5000.0, -5000.0                     # the target 1e4 below the maximum: NLL 1e4, no overflow
    rows[4:] = np.linspace(-1.0, 1.0, k)
    rows[4, 0] = np.nan                                          # never left by the scan: prediction 0
    rows[5, k - 2] = np.nan                                      # never moved to: prediction k - 1
    rows[6, 2] = np.inf                                          # prediction 2
    rows[7, k - 1] = -np.inf                                     # prediction k - 2
    targets = np.array([hi[1], k - 1, k - 1, 1, 0, k - 1, 0, k - 2])
    return rows, targets


@pytest.mark.parametrize("k", [10, 4])
def test_ties_saturation_and_non_finite_rows(k):
    L = lib()
    rows, targets = special_rows(k)
    ld = 32
    logits = np.full((8, ld), np.nan, np.float32)
    logits[:, :k] = rows
    labels = np.eye(k, dtype=np.float32)[targets]                # dense: tg_accuracy_count_f32 reads the labels as [n][k]
    nr = min(NR, k)
    ref = R.reference(logits, labels, k, nr, NB)
    # the reference says of each row what the interface promises
    hi = (2, 7) if k == 10 else (1, 3)
    assert (ref['p'] == [hi[0], 0, k - 1, 0, 0, k - 1, 2, k - 2]).all() and (ref['t'] == targets).all()
    assert (ref['finite'] == [True] * 4 + [False] * 4).all() and (ref['rank'][:4] == [1, k - 1, 0, 1]).all()
    assert ref['conf'][1] == 1.0 / k and ref['conf'][2] == 1.0 and ref['bin'][2] == NB - 1 and ref['nll'][2] == 0.0 and ref['nll'][3] == 1e4
    assert ref['bin_distance'][0] >= 1e-9 and ref['bin_distance'][1] >= 0.2            # the all-equal row: 15 / k is no integer; rows 2 and 3: exactly 15
    got = run(logits, labels, k).get()
    check(got, ref, "special rows, k %d" % k)
    assert got['nonfinite'][0] == 4 and got['rank_hist'].sum() == 4 == got['bin_count'].sum() and got['confusion'].sum() == 8
    cnt = guarded(2, fill=np.zeros(2, np.float32))
    L.call('tg_accuracy_count_f32', ptr(dev(logits)), ld, ptr(dev(labels)), 8, k, cnt.ptr, st())
    cnt.check_guard()
    assert tuple(cnt.get()) == (float(np.trace(got['confusion'])), 8.0) and np.trace(got['confusion']) == 4      # rows 2, 4, 5 and 7
    # row by row on the device: what a single row leaves behind
    one = [run(logits[r:r + 1], labels[r:r + 1], k).get() for r in range(8)]
    for r in range(8):
        assert one[r]['confusion'][ref['t'][r], ref['p'][r]] == 1 and one[r]['confusion'].sum() == 1
        assert one[r]['nonfinite'][0] == (r >= 4) and one[r]['rank_hist'].sum() == (r < 4) == one[r]['bin_count'].sum()
        if r >= 4:
            assert (one[r]['sums'] == 0.0).all() and (one[r]['bin_conf'] == 0.0).all() and one[r]['bin_correct'].sum() == 0
    assert one[0]['rank_hist'][1] == 1 and one[0]['bin_correct'].sum() == 0
    assert one[1]['rank_hist'][min(k - 1, nr - 1)] == 1 and one[1]['bin_conf'][int(15.0 / k)] == 1.0 / k
    assert one[2]['bin_count'][NB - 1] == 1 and one[2]['bin_correct'][NB - 1] == 1 and one[2]['bin_conf'][NB - 1] == 1.0
    assert one[2]['sums'][0] == 0.0 and one[2]['rank_hist'][0] == 1
    assert one[3]['sums'][0] == 1e4 and one[3]['bin_conf'][NB - 1] == 1.0 and one[3]['sums'][1] == 2.0


def test_an_all_equal_row_of_two_classes():
    logits, labels = np.full((1, 2), -3.0, np.float32), np.array([[0.0, 1.0]], np.float32)
    got = run(logits, labels, 2).get()
    assert got['confusion'][1, 0] == 1 and got['rank_hist'][1] == 1 and got['bin_count'][7] == 1 and got['bin_conf'][7] == 0.5
    assert abs(got['sums'][0] - np.log(2.0)) <= 4 * R.EPS and got['sums'][1] == 0.5          # (2 ulp for the logarithm on either side)


@pytest.mark.parametrize("n,k,ld", [(257, 11, 11), (130, 100, 128)])
def test_two_calls_on_the_halves_accumulate_to_the_whole(n, k, ld):
    logits, labels, ref = data(n, k, ld)
    h = n // 2 + 1
    into = run(logits[:h], labels[:h], k)
    got = run(logits[h:], labels[h:], k, into=into).get()
    whole = run(logits, labels, k).get()
    for key in INT_KEYS:
        assert (got[key] == whole[key]).all(), key
    check(got, ref, "two halves, n %d k %d" % (n, k))


def test_other_stream_and_dirty_workspace_give_the_same_bytes():
    """the workspace needs no initialisation and no output depends on the stream or on the run."""
    n, k, ld = 130, 100, 128
    logits, labels, _ = data(n, k, ld)
    first = run(logits, labels, k).raw_bytes()
    again = run(logits, labels, k, dirty=np.full(n * 8, 1e30, np.float32)).raw_bytes()
    L = lib()
    out = Outputs(k, NR, NB)
    gw, need = workspace(n, k, fill=np.full(n * 8, -7.0, np.float32))
    dl, dy = dev(np.array(logits)), dev(np.array(labels))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        L.call('tg_eval_report_f32', ptr(dl), ld, ptr(dy), labels.shape[1], n, k, NR, NB, *out.args(), gw.ptr, need, st())
    side.synchronize()
    gw.check_guard()
    out.get()
    other = out.raw_bytes()
    for key in Outputs.ORDER:
        assert first[key] == again[key] == other[key], key


def test_bad_arguments_are_refused_and_no_rows_is_a_no_op():
    L = lib()
    h = L.load()
    k, n, ld = 10, 16, 16
    x = torch.zeros(n * 1100, dtype=torch.float32, device='cuda')
    out = Outputs(k, NR, NB, poison=-3.5)
    before = out.raw_bytes()
    gw, need = workspace(n, k)

    def call(ld=ld, ld_y=ld, n=n, k=k, nr=NR, nb=NB, ws=gw.ptr, nbytes=need, **swap):
        return h.tg_eval_report_f32(ptr(x), ld, ptr(x), ld_y, n, k, nr, nb, *out.args(**swap), ws, nbytes, st())

    refused = [dict(k=1), dict(k=1025, ld=1100, ld_y=1100), dict(ld=k - 1), dict(ld_y=k - 1), dict(nr=0), dict(nr=33), dict(nb=0), dict(nb=65),
               dict(n=-1), dict(confusion=None), dict(sums=None), dict(ws=None), dict(nbytes=need - 1)]
    for bad in refused:
        assert call(**bad) == TG_ERR_INVALID, bad
        assert b"eval_report" in h.tg_last_error_string()
    assert b"workspace" in h.tg_last_error_string()
    torch.cuda.synchronize()
    assert out.raw_bytes() == before                              # nothing was launched: the poison is what it was
    for g in list(out.g.values()) + [gw]:
        g.check_guard()
    L.call('tg_eval_report_f32', None, ld, None, ld, 0, k, NR, NB, None, None, None, None, None, None, None, None, 0, st())
    assert call(n=0) == 0 and out.raw_bytes() == before
    zero = Outputs(k, NR, NB)
    assert h.tg_eval_report_f32(ptr(x), ld, ptr(x), ld, n, k, NR, NB, *zero.args(), gw.ptr, need, st()) == 0     # in range: goes through
    got = zero.get()
    assert got['confusion'][0, 0] == n and got['bin_conf'][1] == n * 0.1 and got['rank_hist'][0] == n


# ---- the trainer: the CIFAR-10 model at the small sizes of tests/test_gpu_sample_metrics.py ------------------------------------------
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
        _CACHE['val'] = [(rng.uniform(-1.0, 1.0, (VAL_BATCH, 32, 32, 3)).astype(np.float32),
                          np.eye(10, dtype=np.float32)[rng.integers(0, 10, VAL_BATCH)]) for _ in range(N_VAL // VAL_BATCH)]
    return _CACHE['val']


def _iterate(tr, which):
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


def _cx_state(cx):
    torch.cuda.synchronize()
    out = {'rng': cx.rng.state.cpu().numpy().copy()}
    for net, store in cx.stores.items():
        for buf in ('p', 'g', 'm', 'v', 's', 'step'):
            out[net + '/' + buf] = getattr(store, buf).detach().cpu().numpy().copy()
        if store.ema is not None:
            out[net + '/ema'] = store.ema.detach().cpu().numpy().copy()
    return out


def _same(a, b):
    assert set(a) == set(b)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


def _logits(tr, x, getter=None):
    """the logits of classifier(x, False) as evaluate runs it, fetched in a pass of their own."""
    cx, m = tr.cx, tr.model
    with cx.phase_scope('test_fetch', record=False):
        xa = m.zca().apply(m.as_image(cx.from_numpy(x)))
        with cx.rng_scoped('val/C'):
            logits, _ = m.classifier(xa, False, getter=getter)
        return logits.numpy().copy()


def test_evaluate_report_is_evaluate_with_the_counts_of_the_same_logits():
    from tg import metrics as M
    tr = _new()
    val = _val()
    before = _cx_state(tr.cx)
    for ema in (False, True):
        acc = tr.evaluate(val, ema=ema)
        rep = tr.evaluate_report(val, ema=ema)
        _same(_cx_state(tr.cx), before)
        assert rep['accuracy'] == acc and rep['n'] == rep['confusion'].sum() == N_VAL and rep['n_nonfinite'] == 0
        fetched = np.concatenate([_logits(tr, x, getter=True if ema else None) for x, _ in val])
        ref = R.reference(fetched, np.concatenate([y for _, y in val]), 10, 10, 15)
        assert (rep['confusion'] == ref['confusion']).all()
        want = M.report_from_counts(**R.counts(ref))
        assert rep['top5_accuracy'] == want['top5_accuracy'] and rep['balanced_accuracy'] == want['balanced_accuracy']
        assert (rep['reliability'][:, 0] == want['reliability'][:, 0]).all()
        assert abs(rep['nll'] - want['nll']) <= ref['bound_sums'][0] / N_VAL and abs(rep['brier'] - want['brier']) <= ref['bound_sums'][1] / N_VAL
        print("ema %s: accuracy %.4f, balanced %.4f, nll %.4f, ece %.4f" % (ema, acc, rep['balanced_accuracy'], rep['nll'], rep['ece']))
    # the report argument of evaluate is the same pass: one accumulator over two calls holds both splits
    both = tr._new_report()
    assert tr.evaluate(val, report=both) == tr.evaluate(val[:1] + val[1:], report=both)
    assert both.n == 2 * N_VAL and both.result()['confusion'].sum() == 2 * N_VAL
    # the generated side: the class asked for is the target, the rows scored are the first n_samples
    m = tr.sample_metrics_report(val, N_SAMPLES - 3, ema=True)
    _same(_cx_state(tr.cx), before)
    assert m['val_report']['accuracy'] == m['val_accuracy'] == tr.evaluate(val, ema=True)
    g = m['g_report']
    assert g['accuracy'] == m['g_class_accuracy'] and g['n'] == N_SAMPLES - 3
    assert (g['support'] == np.bincount(np.arange(N_SAMPLES - 3) % 10, minlength=10)).all()
    assert g['worst_class_recall'] == np.nanmin(g['recall'])
    plain = tr.sample_metrics(val, N_SAMPLES - 3, ema=True)
    assert 'g_report' not in plain and all(plain[key] == m[key] for key in plain)


def test_a_plan_twin_that_never_reported_is_bit_identical_after_the_next_iteration():
    """the plan is recorded in the second iteration and replayed from the third: the eager report passes run while it holds its buffers."""
    over = dict(EXEC_MODE='plan', USE_HIP_GRAPH=None)
    a = _new(**over)
    rep = a.evaluate_report(_val(), ema=True)
    m = a.sample_metrics_report(_val(), N_SAMPLES, ema=True)
    assert m['val_report']['accuracy'] == rep['accuracy'] and (m['val_report']['confusion'] == rep['confusion']).all()
    _iterate(a, [3])
    got = _cx_state(a.cx)
    assert all(p is not None for p in a.executor.replay['full'].plans)
    b = _new(**over)
    _iterate(b, [3])
    _same(got, _cx_state(b.cx))


# ---- config.EVAL_REPORT in the epoch tail, through _main_training_mnist -------------------------------------------------------------
VAL_NEW = ('val_balanced_accuracy', 'val_macro_f1', 'val_nll', 'val_ece', 'val_top5_accuracy')
NEW = VAL_NEW + tuple(t + '_ema' for t in VAL_NEW) + ('g_worst_class_accuracy',)
OLD = ('val_accuracy_ema', 'g_class_accuracy', 'frechet_distance')
_RUNS = {}


def _mnist(key, tmp_path_factory, monkeypatch, capsys, **flags):
    """(records, printed epoch lines, the context's final state, the run's root) of a 2-epoch MNIST run with EVAL_EMA and
    SAMPLE_METRICS = 64; made once per key."""
    if key not in _RUNS:
        from tg import runtime
        from Training import Train_goodGAN as TG
        root = tmp_path_factory.mktemp(key)
        runtime.set_context(None)
        monkeypatch.setattr(TG, "_root_dir", lambda: str(root))
        np.random.seed(3)                                                               # Train.train draws sample_z from NumPy's global generator
        F = type('Flags', (object,), dict(dict(train_size=2 * 100, seed=1, eval_ema=True, sample_metrics=64), **flags))
        capsys.readouterr()
        hist = TG._main_training_mnist(F(), epochs=2)
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('epoch ')]
        _RUNS[key] = (hist, lines, _cx_state(runtime.ctx()), root)
    return _RUNS[key]


def _val_dir(root):
    rd = os.path.join(str(root), 'Training', 'Log_mnist', 'val')
    return os.path.join(rd, os.listdir(rd)[0])


def test_the_setting_adds_its_records_and_changes_nothing_else(tmp_path_factory, monkeypatch, capsys):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import read_events as RE
    off, lines_off, state_off, off_root = _mnist('off', tmp_path_factory, monkeypatch, capsys)
    on, lines_on, state_on, on_root = _mnist('on', tmp_path_factory, monkeypatch, capsys, eval_report=True)
    _same(state_on, state_off)                                   # weights, shadows, optimiser slots, running statistics, Philox state
    assert len(on) == len(off) == 2 and len(lines_on) == len(lines_off) == 2
    for r_on, r_off in zip(on, off):
        assert set(r_on) == set(r_off) | set(NEW) and not set(NEW) & set(r_off)
        assert tuple(r_on)[-len(NEW):] == NEW                    # after the values of the settings they extend
        for key in r_off:
            if key != 'images_per_sec':                          # (a wall-clock rate)
                assert r_on[key] == r_off[key], key
        assert np.isfinite([r_on[key] for key in NEW]).all()
        assert all(0.0 <= r_on[key] <= 1.0 for key in NEW if 'nll' not in key) and r_on['val_nll'] > 0.0
        assert r_on['val_top5_accuracy'] >= r_on['val_accuracy'] and r_on['g_worst_class_accuracy'] <= r_on['g_class_accuracy']
    for l_on, l_off, r_on in zip(lines_on, lines_off, on):       # the printed line: today's, then the new values
        head, tail = l_off[:l_off.index(' img/s')].rsplit(' ', 1)[0], l_off[l_off.index(' img/s'):]
        assert l_on.startswith(head) and not any(' %s ' % key in l_off for key in NEW)
        assert l_on[l_on.index(' img/s'):] == tail + "".join(" %s %.4f" % (key, r_on[key]) for key in NEW)

    def val_events(root):
        rd = _val_dir(root)
        files = [f for f in os.listdir(rd) if f.startswith('events.out.tfevents.')]
        assert len(files) == 1
        return RE.read_events(os.path.join(rd, files[0]))[1:], open(os.path.join(rd, 'history.csv')).read().splitlines()

    ev_on, csv_on = val_events(on_root)
    ev_off, csv_off = val_events(off_root)
    assert len(ev_on) == len(ev_off) == 2
    assert csv_off[0] == 'step,val_accuracy,' + ','.join(OLD) and csv_on[0] == csv_off[0] + ',' + ','.join(NEW)
    for e_on, e_off, r_on in zip(ev_on, ev_off, on):
        assert set(e_off['scalars']) == {'val_accuracy'} | set(OLD) and set(e_on['scalars']) == set(e_off['scalars']) | set(NEW)
        assert e_on['step'] == e_off['step'] == r_on['epoch']
        for key in e_off['scalars']:
            assert e_on['scalars'][key] == e_off['scalars'][key], key
        for key in NEW:
            assert e_on['scalars'][key] == np.float32(r_on[key]), key
    assert not [f for f in os.listdir(_val_dir(off_root)) if f.endswith('.npy')]
    for r_on in on:
        conf = np.load(os.path.join(_val_dir(on_root), 'confusion_%04d.npy' % r_on['epoch']))
        g_conf = np.load(os.path.join(_val_dir(on_root), 'g_confusion_%04d.npy' % r_on['epoch']))
        assert conf.dtype == g_conf.dtype == np.int64 and conf.shape == g_conf.shape == (10, 10)
        assert conf.sum() > 0 and np.trace(conf) / conf.sum() == r_on['val_accuracy']          # the raw weights' pass, the whole split
        assert g_conf.sum() == 64 and np.trace(g_conf) / 64.0 == r_on['g_class_accuracy']
        assert (g_conf.sum(axis=1) == np.bincount(np.arange(64) % 10, minlength=10)).all()
        assert (np.diag(g_conf) / g_conf.sum(axis=1)).min() == r_on['g_worst_class_accuracy']


def test_the_report_beside_a_replayed_plan_changes_nothing(tmp_path_factory, monkeypatch, capsys):
    """EXEC_MODE = 'plan': the step is recorded in the second iteration and replayed from the third, the report passes stay eager."""
    on, _, state_on, _ = _mnist('on', tmp_path_factory, monkeypatch, capsys, eval_report=True)
    plan, _, state_plan, _ = _mnist('plan', tmp_path_factory, monkeypatch, capsys, eval_report=True, exec_mode='plan')
    _same(state_plan, state_on)
    for r_plan, r_on in zip(plan, on):
        assert tuple(r_plan) == tuple(r_on)
        for key in r_on:
            if key != 'images_per_sec':
                assert r_plan[key] == r_on[key], key
