"""The host side of the classifier's evaluation report without a device: tg.metrics.report_from_counts on count sets made by
hand and by the row-by-row reference (tests/eval_report_reference.py), the EVAL_REPORT setting (Training/options.check_eval_report, the
Options record, the entry points' flag), the epoch tail's tags for every combination of the settings, and the C declarations.

Everything here is a ratio of small integers or a hand-computed float64 expression, so the comparisons are exact unless a tolerance is
written beside them."""
import itertools
import os
import types

import numpy as np
import pytest

import eval_report_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEFAULT = dict(NUM_CLASSES=10, BATCH_SIZE=8, BATCH_SIZE_G=8, BATCH_SIZE_L_D=2, BATCH_SIZE_U_D=6)      # what Config declares no usable default for
REPORT_KEYS = ('n', 'n_nonfinite', 'accuracy', 'top5_accuracy', 'nll', 'brier', 'ece', 'balanced_accuracy', 'macro_f1', 'worst_class_recall',
               'worst_class', 'predicted_class_entropy', 'support', 'predicted', 'recall', 'precision', 'f1', 'reliability', 'confusion')


def counts(confusion, ranks=16, bins=15, top=None, bin_rows=(), sums=(0.0, 0.0), nonfinite=0):
    """a count set around a confusion matrix: every row finite (but `nonfinite`), rank 0 for the diagonal and 1 for the rest unless
    `top` gives the histogram; bin_rows: (bin, count, correct, confidence sum)."""
    confusion = np.asarray(confusion, np.int64)
    k = confusion.shape[0]
    nr = min(ranks, k)
    hist = np.zeros(nr, np.int64)
    if top is None:
        hist[0], hist[1] = np.trace(confusion), confusion.sum() - np.trace(confusion) - nonfinite
    else:
        hist[:len(top)] = top
    bc, bk, bf = np.zeros(bins, np.int64), np.zeros(bins, np.int64), np.zeros(bins)
    for b, cnt, ok, conf in bin_rows:
        bc[b], bk[b], bf[b] = cnt, ok, conf
    return dict(confusion=confusion, rank_hist=hist, bin_count=bc, bin_correct=bk, bin_conf=bf, sums=np.asarray(sums, np.float64),
                nonfinite=np.array([nonfinite], np.int64))


def test_a_perfect_classifier():
    from tg import metrics as M
    sup = np.array([3, 1, 4, 1, 5, 9, 2, 6, 5, 3])
    r = M.report_from_counts(**counts(np.diag(sup), bin_rows=[(14, int(sup.sum()), int(sup.sum()), float(sup.sum()))]))
    assert tuple(sorted(r)) == tuple(sorted(REPORT_KEYS)) and set(M.REPORT_SCALARS + M.REPORT_ARRAYS) | {'reliability', 'confusion'} == set(r)
    assert r['n'] == sup.sum() and r['n_nonfinite'] == 0
    assert r['accuracy'] == r['balanced_accuracy'] == r['macro_f1'] == r['top5_accuracy'] == r['worst_class_recall'] == 1.0
    assert r['worst_class'] == 0 and r['ece'] == 0.0 and r['nll'] == 0.0 and r['brier'] == 0.0
    assert (r['support'] == sup).all() and (r['predicted'] == sup).all()
    assert (r['recall'] == 1.0).all() and (r['precision'] == 1.0).all() and (r['f1'] == 1.0).all()
    q = sup / sup.sum()
    assert abs(r['predicted_class_entropy'] - (-(q * np.log(q)).sum() / np.log(10))) <= 1e-15
    assert r['reliability'].shape == (15, 3) and tuple(r['reliability'][14]) == (sup.sum(), 1.0, 1.0) and np.isnan(r['reliability'][:14, 1:]).all()
    assert r['confusion'].dtype == np.int64 and (r['confusion'] == np.diag(sup)).all()


@pytest.mark.parametrize("k", [2, 10, 100])
def test_a_classifier_collapsed_onto_one_class(k):
    from tg import metrics as M
    conf = np.zeros((k, k), np.int64)
    conf[:, 3 % k] = 7                                                  # seven rows of every class, all predicted as one
    r = M.report_from_counts(**counts(conf))
    one = 3 % k
    assert r['accuracy'] == 1.0 / k and r['balanced_accuracy'] == 1.0 / k and r['predicted_class_entropy'] == 0.0
    others = np.arange(k) != one
    assert np.isnan(r['precision'][others]).all() and (r['f1'][others] == 0.0).all() and (r['recall'][others] == 0.0).all()
    assert r['recall'][one] == 1.0 and r['precision'][one] == 1.0 / k and r['f1'][one] == 2.0 * 7 / (7 + 7 * k)
    assert r['macro_f1'] == r['f1'][one] / k                            # the never-predicted classes count, with an F1 of 0
    assert r['worst_class_recall'] == 0.0 and r['worst_class'] == (1 if one == 0 else 0)


def test_an_absent_class_is_left_out_of_the_means():
    from tg import metrics as M
    conf = np.array([[4, 0, 0, 0], [1, 3, 0, 0], [0, 0, 0, 0], [0, 1, 1, 2]])          # class 2: no support, predicted once
    r = M.report_from_counts(**counts(conf))
    assert np.isnan(r['recall'][2]) and r['precision'][2] == 0.0 and r['f1'][2] == 0.0
    assert (r['recall'][[0, 1, 3]] == [1.0, 0.75, 0.5]).all()
    assert r['balanced_accuracy'] == (1.0 + 0.75 + 0.5) / 3
    f1 = [2 * 4 / (4 + 5), 2 * 3 / (4 + 4), 2 * 2 / (4 + 2)]
    assert abs(r['macro_f1'] - sum(f1) / 3) <= 1e-15
    assert r['worst_class'] == 3 and r['worst_class_recall'] == 0.5 and r['accuracy'] == 9 / 12
    never = M.report_from_counts(**counts(np.array([[2, 0, 0], [0, 0, 0], [1, 0, 1]])))   # class 1: absent and never predicted
    assert np.isnan(never['recall'][1]) and np.isnan(never['precision'][1]) and np.isnan(never['f1'][1])
    assert never['balanced_accuracy'] == (1.0 + 0.5) / 2


def test_top5_accuracy_needs_more_than_five_classes_and_ranks():
    from tg import metrics as M
    assert np.isnan(M.report_from_counts(**counts(np.eye(5, dtype=np.int64)))['top5_accuracy'])
    six = np.full((6, 6), 2, np.int64)
    assert np.isnan(M.report_from_counts(**counts(six, ranks=5, top=[12, 20, 20, 10, 10]))['top5_accuracy'])
    r = M.report_from_counts(**counts(six, ranks=6, top=[12, 20, 20, 10, 4, 6]))
    assert r['top5_accuracy'] == 66 / 72 and r['accuracy'] == 12 / 72
    bad = M.report_from_counts(**counts(six, ranks=6, top=[12, 20, 20, 10, 4, 2], nonfinite=4))       # means over the finite rows
    assert bad['top5_accuracy'] == 66 / 68 and bad['n'] == 72 and bad['n_nonfinite'] == 4


def test_ece_by_hand():
    from tg import metrics as M
    # 20 rows: bin 7 holds 10 rows, 4 right, mean confidence 0.5; bin 13 holds 6, 6 right, 0.9; bin 14 holds 4, 3 right, 0.975
    conf = np.array([[13, 7], [0, 0]])
    r = M.report_from_counts(**counts(conf, bin_rows=[(7, 10, 4, 5.0), (13, 6, 6, 5.4), (14, 4, 3, 3.9)], sums=(8.0, 5.0)))
    want = (10 * abs(0.4 - 0.5) + 6 * abs(1.0 - 5.4 / 6) + 4 * abs(0.75 - 3.9 / 4)) / 20
    assert abs(r['ece'] - want) <= 1e-15 and abs(want - 0.125) <= 1e-15
    assert r['nll'] == 0.4 and r['brier'] == 0.25
    assert tuple(r['reliability'][7]) == (10.0, 0.5, 0.4) and r['reliability'][13, 2] == 1.0 and r['reliability'][14, 0] == 4.0


def test_report_of_the_reference_counts():
    """the two halves meet: counts made row by row from logits give a report whose accuracy is trace / sum and the arg-max accuracy."""
    from tg import metrics as M
    rng = np.random.default_rng(5)
    n, k = 200, 7
    logits = (rng.standard_normal((n, k)) * 3).astype(np.float32)
    labels = np.eye(k, dtype=np.float32)[rng.integers(0, k, n)]
    logits[np.arange(n), labels.argmax(1)] += 2.0
    logits[17, 3] = np.nan
    ref = R.reference(logits, labels, k, 7, 15)
    r = M.report_from_counts(**R.counts(ref))
    assert r['n'] == n and r['n_nonfinite'] == 1
    assert r['accuracy'] == np.trace(ref['confusion']) / ref['confusion'].sum() == float((ref['t'] == ref['p']).sum()) / n
    fin = ref['finite']
    assert r['top5_accuracy'] == float((ref['rank'][fin] < 5).sum()) / fin.sum()
    assert abs(r['nll'] - ref['nll'][fin].mean()) <= 1e-12 and abs(r['brier'] - ref['brier'][fin].mean()) <= 1e-12
    assert r['reliability'][:, 0].sum() == fin.sum() and 0.0 <= r['ece'] <= 1.0
    # the probability of the target, two ways: exp(-NLL), and rank 0 exactly where the prediction is the target
    assert ((ref['rank'][fin] == 0) == (ref['t'][fin] == ref['p'][fin])).all()
    sm = np.exp(logits[fin].astype(np.float64) - logits[fin].max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    assert np.abs(np.exp(-ref['nll'][fin]) - sm[np.arange(fin.sum()), ref['t'][fin]]).max() <= 1e-14
    assert np.abs(ref['conf'][fin] - sm.max(1)).max() <= 1e-14
    with pytest.raises(ValueError, match="square"):
        M.report_from_counts(**dict(R.counts(ref), confusion=np.zeros((3, 4), np.int64)))


def test_the_scan_breaks_ties_low_and_never_moves_to_a_nan():
    nan, inf = np.float32('nan'), np.float32('inf')
    f = lambda *v: R.scan_argmax(np.array(v, np.float32))
    assert f(1, 5, 2, 5) == 1 and f(0, 0, 0) == 0 and f(-0.0, 0.0) == 0
    assert f(nan, 9, 9) == 0 and f(1, nan, 3) == 2 and f(3, nan, 1) == 0
    assert f(1, inf, inf) == 1 and f(-inf, -inf) == 0 and f(-inf, nan, -5) == 2


def test_classifier_report_refuses_what_the_kernel_does_not_take():
    from tg import metrics as M
    for bad in (dict(num_classes=1), dict(num_classes=1025), dict(num_classes=10, ranks=0), dict(num_classes=10, ranks=33),
                dict(num_classes=10, bins=0), dict(num_classes=10, bins=65)):
        with pytest.raises(ValueError, match="ClassifierReport"):
            M.ClassifierReport(device='cpu', **bad)
    assert M.ClassifierReport(4, 'cpu').ranks == 4 and M.ClassifierReport(100, 'cpu').ranks == 16 and M.ClassifierReport(100, 'cpu').bins == 15
    empty = M.ClassifierReport(4, 'cpu').result()                       # nothing added: counts() needs no device call
    assert empty['n'] == 0 and empty['accuracy'] == 0.0 and np.isnan(empty['nll']) and empty['confusion'].shape == (4, 4)


def test_check_eval_report_values_and_errors():
    from config import Config
    from Training import options
    assert not hasattr(Config, 'EVAL_REPORT')                           # not declared: the entry configurations are pinned
    ns = types.SimpleNamespace
    assert options.check_eval_report(ns()) is False and options.check_eval_report(ns(EVAL_REPORT=None)) is False
    assert options.check_eval_report(ns(EVAL_REPORT=False)) is False and options.check_eval_report(ns(EVAL_REPORT=0)) is False
    assert options.check_eval_report(ns(EVAL_REPORT=True)) is True and options.check_eval_report(ns(EVAL_REPORT=1)) is True
    assert options.check_eval_report(ns(EVAL_REPORT=np.bool_(True))) is True
    for bad in ('yes', 'True', 2, -1, 0.5, 1.0, (True,), [1]):
        with pytest.raises(ValueError, match="EVAL_REPORT"):
            options.check_eval_report(ns(EVAL_REPORT=bad))


def test_resolve_carries_the_setting_beside_its_fields():
    from config import Config
    from Training import options
    bare = type('Bare', (object,), NO_DEFAULT)()
    full = type('Full', (Config,), NO_DEFAULT)()
    off = options.resolve(bare)
    assert off == options.resolve(full) and off.eval_report is False
    assert 'eval_report' in options.Options.EXTRAS and 'eval_report' not in off._fields and 'eval_report' not in off._asdict()
    bare.EVAL_REPORT = full.EVAL_REPORT = True
    on = options.resolve(bare)
    assert on == options.resolve(full) and on.eval_report is True
    assert tuple(on) == tuple(off) and on._fields == off._fields and on != off and hash(on) != hash(off)
    bare.EVAL_REPORT = 'on'
    with pytest.raises(ValueError, match="EVAL_REPORT"):
        options.resolve(bare)


def test_the_flag_reaches_the_config_an_entry_point_hands_to_train(monkeypatch, tmp_path):
    from Training import Train_goodGAN as TG
    seen = {}

    class Captured(object):
        def __init__(self, config, log_dir, save_dir, **kwargs):
            seen['config'] = config

        def train(self, Dataset, Model, sample_y):
            return None

    monkeypatch.setattr(TG, '_root_dir', lambda: str(tmp_path))
    monkeypatch.setattr(TG, 'Train', Captured)
    TG._main_training_mnist(types.SimpleNamespace(eval_report=True))
    assert seen['config'].EVAL_REPORT is True and not hasattr(seen['config'], 'EVAL_EMA')
    TG._main_training_mnist(types.SimpleNamespace(seed=3))
    assert not hasattr(seen['config'], 'EVAL_REPORT')


def test_the_trainer_surface():
    """the keyword and the methods the GPU tests drive, checked where no GPU is; the two pinned parameter lists are what they were."""
    import inspect
    from Training.Train_goodGAN import Train
    params = lambda f: list(inspect.signature(f).parameters)[1:]
    assert params(Train.evaluate) == ['batches', 'ema', 'report'] and inspect.signature(Train.evaluate).parameters['report'].default is None
    assert params(Train.evaluate_report) == ['batches', 'ema']
    assert params(Train.sample_metrics_report) == ['batches', 'n_samples', 'ema', 'manifold_k']
    assert params(Train.sample_metrics) == ['batches', 'n_samples', 'ema']
    assert params(Train.sample_manifold_metrics) == ['batches', 'n_samples', 'manifold_k', 'ema', 'return_banks']


VAL_TAGS = ('val_balanced_accuracy', 'val_macro_f1', 'val_nll', 'val_ece')


@pytest.mark.parametrize("report,ema,samples,manifold,k", [c for c in itertools.product((False, True), (False, True), (None, 64), (None, 3), (5, 10, 100))
                                                          if c[2] or not c[3]])
def test_tail_metric_tags_for_every_combination(report, ema, samples, manifold, k):
    from Training import options
    from Training.Train_goodGAN import Train
    cfg = types.SimpleNamespace(**dict(NO_DEFAULT, NUM_CLASSES=k, EVAL_REPORT=report, EVAL_EMA=ema, SAMPLE_METRICS=samples, SAMPLE_MANIFOLD_K=manifold))
    tr = Train.__new__(Train)                                           # the method reads the resolved options and nothing else
    tr.options = options.resolve(cfg)
    before = ((('val_accuracy_ema',) if ema else ()) + (('g_class_accuracy', 'frechet_distance') if samples else ())
              + (('precision', 'recall', 'density', 'coverage') if samples and manifold else ()))
    tags = tr._tail_metric_tags()
    if not report:
        assert tags == before
        return
    val = VAL_TAGS + (('val_top5_accuracy',) if k > 5 else ())
    assert tags == before + val + (tuple(t + '_ema' for t in val) if ema else ()) + (('g_worst_class_accuracy',) if samples else ())
    assert len(set(tags)) == len(tags)


def test_header_declares_both_symbols():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_plan_thunks as gen
    from tg import lib, plan
    sigs = lib.parse_header()
    assert 'tg_eval_report_f32' in sigs and 'tg_eval_report_workspace_bytes' in sigs
    assert len(sigs['tg_eval_report_f32'][1]) == 18 and len(sigs['tg_eval_report_workspace_bytes'][1]) == 2
    text = open(os.path.join(ROOT, "include", "tg_kernels.h")).read()
    assert "int64_t tg_eval_report_workspace_bytes(int n, int k);" in text
    params = dict(gen.launches())['tg_eval_report_f32']
    assert len(params) == 17 and plan.signature('tg_eval_report_f32') == 'pipi' + 4 * 'i' + 8 * 'p' + 'i'
    assert 'tg_eval_report_workspace_bytes' not in dict(gen.launches())
    h = lib.load()
    assert h.tg_eval_report_workspace_bytes(4, 1) < 0 and h.tg_eval_report_workspace_bytes(4, 1025) < 0
    assert h.tg_eval_report_workspace_bytes(-1, 10) < 0 and b"eval_report_workspace_bytes" in h.tg_last_error_string()
    assert h.tg_eval_report_workspace_bytes(0, 10) == 0 and lib.call('tg_eval_report_workspace_bytes', 0, 1024) == 0
    assert lib.call('tg_eval_report_workspace_bytes', 257, 10) >= 257 * 3 * 8      # three doubles and a bin per row, at the least
    with pytest.raises(lib.TgError, match="eval_report_workspace_bytes"):
        lib.call('tg_eval_report_workspace_bytes', 4, 1)
