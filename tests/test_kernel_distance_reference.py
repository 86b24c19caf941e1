"""CPU checks of the kernel distance: the float64 reference tests/kernel_distance_reference.py against np.longdouble and
its bound against an fp32-chained control, kid_from_sums by hand and on its NaN rules, the estimator's unbiasedness, and the device-free
plumbing — Training/options.check_sample_kid, the Options record, the epoch tail's tags, the flag, the header and tg/lib.py's lists."""
import itertools
import types

import numpy as np
import pytest

import kernel_distance_reference as R

SMALL = R.SHAPES[:4]


_inputs = R.inputs


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%dx%d_ld%d" % s)
def test_the_reference_agrees_with_longdouble_within_the_bound(shape):
    m, n, c, _ = shape
    a, b = _inputs(shape)
    for sa, sb, diag, x, y in (([0, m], [0, n], False, a, b), ([0, m], [0, m], True, a, a), ([0, m // 3, m // 3, m], [0, n // 2, n // 2, n], False, a, b)):
        ref, wide, tol = R.poly3_sums(x, y, sa, sb, diag), R.poly3_sums_longdouble(x, y, sa, sb, diag), R.sum_bound(x, y, sa, sb, diag)
        err = np.abs(ref.astype(np.longdouble) - wide).astype(np.float64)
        assert (err <= tol).all(), (shape, err, tol)


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[2] >= 3], ids=lambda s: "%dx%dx%d_ld%d" % s)
def test_the_bound_rejects_a_dot_product_chained_in_fp32(shape):
    """The bound is not vacuous: the sums an fp32-MFMA kernel would give (the dot product an fp32 fma chain, everything behind it
    float64) lie outside it at every shape with c >= 3.  The control's error is rounding noise that grows like sqrt(pairs) while the
    bound's summation term grows like pairs^2, so the margin shrinks with the shape: on these inputs the control misses the bound by
    about 1.8e5 x at (5, 7, 3), 1.4e3 x at (65, 33, 5), 105 x at (257, 130, 33), 3.5e3 x at (64, 64, 128) and 3.3 x at (1000, 777, 192)."""
    m, n, c, _ = shape
    a, b = _inputs(shape)
    ref, tol = R.poly3_sums(a, b, [0, m], [0, n]), R.sum_bound(a, b, [0, m], [0, n])
    control = R.poly3_sums(a, b, [0, m], [0, n], gram_fn=R.gram_f32_chain)
    ratio = float(np.abs(control - ref)[0] / tol[0])
    print("fp32-chained control at %r: %.1f x the bound" % (shape, ratio))
    assert ratio > 1.0, (shape, ratio)


def test_segments_the_diagonal_and_padding():
    rng = np.random.default_rng(3)
    a, b = R.features(rng, 9, 4), R.features(rng, 7, 4)
    whole = R.poly3_sums(a, b, [0, 9], [0, 7])
    parts = R.poly3_sums(a, b, [0, 4, 4, 9], [0, 7, 7, 7])
    assert parts[1] == 0.0 and parts[2] == 0.0                         # empty on one side
    t = a.astype(np.float64) @ b.astype(np.float64).T / 4.0 + 1.0
    assert whole[0] == (t * t * t).sum() and parts[0] == (t * t * t)[:4].sum()
    s = a.astype(np.float64) @ a.astype(np.float64).T / 4.0 + 1.0
    k = s * s * s
    np.testing.assert_allclose(R.poly3_sums(a, a, [0, 9], [0, 9], True)[0], k.sum() - np.trace(k), rtol=1e-14)
    # the diagonal is local to the segment: rows 2.. of a against rows 1.. of b
    got = R.poly3_sums(a, b, [2, 9], [1, 7], True)[0]
    kk = (t * t * t)[2:, 1:]
    np.testing.assert_allclose(got, kk.sum() - np.trace(kk), rtol=1e-14)
    p = R.padded(a, 6)
    assert p.shape == (9, 6) and np.isnan(p[:, 4:]).all() and (p[:, :4] == a).all()


def test_kid_from_sums_by_hand_and_its_nan_rules():
    from tg import metrics as M
    # c = 1, x = (1, 2), y = (0, 3): k(u, v) = (u v + 1)^3
    x, y = np.array([[1.0], [2.0]], np.float32), np.array([[0.0], [3.0]], np.float32)
    sxx = R.poly3_sums(x, x, [0, 2], [0, 2], True)[0]
    syy = R.poly3_sums(y, y, [0, 2], [0, 2], True)[0]
    sxy = R.poly3_sums(x, y, [0, 2], [0, 2], False)[0]
    assert (sxx, syy, sxy) == (27.0 + 27.0, 1.0 + 1.0, 1.0 + 64.0 + 1.0 + 343.0)
    want = 54.0 / 2.0 + 2.0 / 2.0 - 2.0 * 409.0 / 4.0
    for f in (R.kid_from_sums, M.kid_from_sums):
        got = f(sxx, syy, sxy, 2, 2)
        assert float(got) == want == -176.5
        v = f(np.array([54.0, 54.0, 54.0, 0.0]), np.array([2.0, 2.0, 2.0, 0.0]), np.array([409.0, 409.0, 409.0, 0.0]),
              np.array([2, 1, 2, 0]), np.array([2, 2, 1, 0]))
        assert v.dtype == np.float64 and v[0] == want and np.isnan(v[1:]).all()
    assert M.worst_of([np.nan, 2.0, 5.0, 5.0, np.nan]) == (5.0, 2) and M.worst_of([-3.0, np.nan]) == (-3.0, 0)
    w, k = M.worst_of([np.nan, np.nan])
    assert np.isnan(w) and k == -1
    order, off = M.class_order([2, 0, 2, 1, 0], 4)
    assert order.tolist() == [1, 4, 3, 0, 2] and off.tolist() == [0, 2, 3, 5, 5]
    with pytest.raises(ValueError, match="labels"):
        M.class_order([0, 4], 4)
    assert M.KERNEL_DISTANCE_KEYS == ('kernel_distance', 'kernel_distance_per_class', 'kernel_distance_worst', 'kernel_distance_worst_class')


def test_the_estimator_is_unbiased_and_the_diagonal_included_one_is_not():
    """200 draws of two samples of 12 rows from ONE distribution: the mean of the unbiased estimate lies within three standard errors
    of 0, the mean of the V-statistic (diagonals included, divided by m^2 and n^2) does not."""
    rng = np.random.default_rng(2024)
    m = n = 12
    c, draws = 8, 200
    unbiased, biased = np.empty(draws), np.empty(draws)
    for d in range(draws):
        x, y = R.features(rng, m, c), R.features(rng, n, c)
        sxy = R.poly3_sums(x, y, [0, m], [0, n])[0]
        unbiased[d] = R.kid_from_sums(R.poly3_sums(x, x, [0, m], [0, m], True)[0], R.poly3_sums(y, y, [0, n], [0, n], True)[0], sxy, m, n)
        biased[d] = (R.poly3_sums(x, x, [0, m], [0, m])[0] / (m * m) + R.poly3_sums(y, y, [0, n], [0, n])[0] / (n * n) - 2.0 * sxy / (m * n))
    se_u, se_b = unbiased.std(ddof=1) / np.sqrt(draws), biased.std(ddof=1) / np.sqrt(draws)
    print("unbiased mean %.4g (standard error %.3g), biased mean %.4g (standard error %.3g)" % (unbiased.mean(), se_u, biased.mean(), se_b))
    assert abs(unbiased.mean()) <= 3.0 * se_u
    assert biased.mean() > 3.0 * se_b


def test_check_sample_kid_values_and_errors():
    from config import Config
    from Training import options
    assert not hasattr(Config, 'SAMPLE_KID')                           # not declared: the entry configurations are pinned
    ns = types.SimpleNamespace
    for off in (ns(), ns(SAMPLE_KID=None), ns(SAMPLE_KID=False), ns(SAMPLE_METRICS=64), ns(SAMPLE_METRICS=64, SAMPLE_KID=False),
                ns(SAMPLE_KID=np.bool_(False))):
        assert options.check_sample_kid(off) is None
    assert options.check_sample_kid(ns(SAMPLE_METRICS=64, SAMPLE_KID=True)) is True
    assert options.check_sample_kid(ns(SAMPLE_METRICS=64, SAMPLE_KID=np.bool_(True))) is True
    assert options.check_sample_kid(ns(SAMPLE_METRICS=64, SAMPLE_KID='per_class')) == 'per_class'
    for bad in (1, 0, 2, 1.0, 'true', 'per-class', 'PER_CLASS', '', ('per_class',), float('nan')):
        with pytest.raises(ValueError, match="SAMPLE_KID"):
            options.check_sample_kid(ns(SAMPLE_METRICS=64, SAMPLE_KID=bad))
    for without in (ns(SAMPLE_KID=True), ns(SAMPLE_METRICS=None, SAMPLE_KID='per_class')):
        with pytest.raises(ValueError, match="needs SAMPLE_METRICS"):
            options.check_sample_kid(without)


def test_resolve_carries_the_setting_and_the_flag_reaches_the_config(monkeypatch, tmp_path):
    from Training import options
    from Training import Train_goodGAN as TG
    extras = options.Options.EXTRAS
    assert extras[-2:] == ('sample_kid', 'sample_nearest') and extras.index('sample_kid') == extras.index('eval_report') + 1
    c = TG.MnistConfig()
    off = options.resolve(c)
    assert off.sample_kid is None and 'sample_kid' not in off._fields and 'sample_kid' not in off._asdict()
    c.SAMPLE_METRICS, c.SAMPLE_KID = 24, 'per_class'
    on = options.resolve(c)
    assert on.sample_kid == 'per_class' and tuple(on) == tuple(off) and on != off and hash(on) != hash(off) and on == options.resolve(c)
    c.SAMPLE_KID = True
    assert options.resolve(c).sample_kid is True and options.resolve(c) != on
    c.SAMPLE_METRICS = None
    with pytest.raises(ValueError, match="SAMPLE_KID"):
        options.resolve(c)
    seen = {}

    class Captured(object):
        def __init__(self, config, log_dir, save_dir, **kwargs):
            seen['config'] = config

        def train(self, Dataset, Model, sample_y):
            return None

    monkeypatch.setattr(TG, '_root_dir', lambda: str(tmp_path))
    monkeypatch.setattr(TG, 'Train', Captured)
    TG._main_training_mnist(types.SimpleNamespace(sample_metrics=24, sample_kid='per_class'))
    assert seen['config'].SAMPLE_METRICS == 24 and seen['config'].SAMPLE_KID == 'per_class'
    TG._main_training_mnist(types.SimpleNamespace(sample_metrics=24, sample_kid=True))
    assert seen['config'].SAMPLE_KID is True
    TG._main_training_mnist(types.SimpleNamespace(sample_metrics=24))                                   # a flag object without the attribute
    assert not hasattr(seen['config'], 'SAMPLE_KID')


def test_the_tail_gains_its_tags_behind_the_report_rows_and_before_the_nearest_ones():
    from Training import options
    from Training.epoch_tail import EpochTail
    from Training.evaluation import Evaluation
    from Training import Train_goodGAN as TG

    class Tail(Evaluation, EpochTail):
        def __init__(self, **settings):
            c = TG.MnistConfig()
            for k, v in settings.items():
                setattr(c, k, v)
            self.options = options.resolve(c)

    nearest = Evaluation.NEAREST_KEYS
    for manifold, ema, report, near in itertools.product((None, 3), (None, True), (None, True), (None, 3)):
        base = dict(SAMPLE_METRICS=24, SAMPLE_MANIFOLD_K=manifold, EVAL_EMA=ema, EVAL_REPORT=report, SAMPLE_NEAREST=near)
        off = Tail(**base)._tail_metric_tags()
        assert Tail(SAMPLE_KID=None, **base)._tail_metric_tags() == off == Tail(SAMPLE_KID=False, **base)._tail_metric_tags()
        assert not [t for t in off if t.startswith('kernel_distance')]
        head, tail = (off[:-len(nearest)], nearest) if near else (off, ())
        assert head + tail == off
        assert Tail(SAMPLE_KID=True, **base)._tail_metric_tags() == head + ('kernel_distance',) + tail
        assert Tail(SAMPLE_KID='per_class', **base)._tail_metric_tags() == head + ('kernel_distance', 'kernel_distance_worst') + tail
    assert Tail()._tail_metric_tags() == ()


def test_the_pass_takes_the_setting_as_one_keyword_only_argument_off_by_default():
    import inspect
    from Training.evaluation import Evaluation
    p = inspect.signature(Evaluation._sample_metrics_pass).parameters
    assert p['kernel_distance'].kind is inspect.Parameter.KEYWORD_ONLY and p['kernel_distance'].default is None
    assert [k for k, v in p.items() if v.kind is inspect.Parameter.KEYWORD_ONLY] == ['kernel_distance']
    assert list(inspect.signature(Evaluation.sample_kernel_distance).parameters) == ['self', 'batches', 'n_samples', 'ema', 'per_class', 'return_banks']


def test_the_header_declares_both_symbols_and_the_query_is_negative_is_error():
    import ctypes as C
    from tg import lib
    sigs = lib.parse_header()
    assert 'tg_poly3_sums_f32' in sigs and 'tg_poly3_sums_workspace_bytes' in sigs
    assert 'tg_poly3_sums_workspace_bytes' in lib._NEGATIVE_IS_ERROR and {'seg_a', 'seg_b'} <= lib.HOST_INT_ARRAYS
    ret, args = sigs['tg_poly3_sums_workspace_bytes']
    assert ret is C.c_int64 and args == [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]
    ret, args = sigs['tg_poly3_sums_f32']
    assert ret is C.c_int and len(args) == 13 and args[5] == args[6] == C.POINTER(C.c_int32) and args[9] is C.c_void_p
    L = lib.load()
    seg = (C.c_int32 * 3)(0, 65, 130)
    small = lib.call('tg_poly3_sums_workspace_bytes', seg, seg, 2)
    assert small > 0 and small % 8 == 0
    with pytest.raises(lib.TgError, match="poly3_sums_workspace_bytes"):
        lib.call('tg_poly3_sums_workspace_bytes', (C.c_int32 * 3)(0, 65, 64), seg, 2)
    assert L.tg_poly3_sums_workspace_bytes(seg, seg, 0) < 0
