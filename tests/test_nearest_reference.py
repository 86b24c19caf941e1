"""The nearest-training-image feature without a device: the C interface of csrc/nearest.hip on the host (declarations,
the workspace and ranges queries, every argument check of tg_nearest_u8_i32 — all answered before any launch), the NumPy reference's own
invariances (tests/nearest_reference.py: chunking, chunk order, planted ties), the quantiser's round trip restated in float32,
Training/options.check_sample_nearest with the `sample_nearest` flag of the entry points, the epoch tail's tags, and the training-chunk
helper of Input_Pipeline/tfrecordDataset.py.  Everything is integer or a fixed fp32 chain: every comparison is ==."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import nearest_reference as R

TG_ERR_INVALID = -1
INT32_MAX = 2 ** 31 - 1


def test_header_declares_the_four_functions_and_the_queries_answer_on_the_host():
    from tg import lib
    sigs = lib.parse_header()
    for name, nargs in (('tg_nearest_u8_workspace_bytes', 4), ('tg_nearest_u8_ranges', 2), ('tg_nearest_u8_i32', 13), ('tg_f32_quantize_u8', 6)):
        assert name in sigs and len(sigs[name][1]) == nargs, name
    assert sigs['tg_nearest_u8_workspace_bytes'][0] is C.c_int64 and sigs['tg_nearest_u8_ranges'][0] is C.c_int
    # one 8-byte key per (range, row, slot)
    assert lib.call('tg_nearest_u8_ranges', 1, 1) == 1 and lib.call('tg_nearest_u8_workspace_bytes', 1, 1, 1, 1) == 8
    for m, n, k in ((64, 300, 3), (1000, 50000, 16), (10000, 50000, 1), (64, 50000, 16)):
        ranges = lib.call('tg_nearest_u8_ranges', m, n)
        assert 1 <= ranges <= -(-n // 64)
        assert lib.call('tg_nearest_u8_workspace_bytes', m, n, 3072, k) == ranges * m * k * 8
    # a function of (m, n) alone; the tests' small n is still cut into several ranges with a ragged last one, and the usual m of
    # 64..1 000 against 50 000 rows gives more workgroups than the device has compute units (256)
    assert lib.call('tg_nearest_u8_ranges', 65, 300) >= 3 and 300 % 64 != 0
    for m in (64, 1000):
        assert -(-m // 64) * lib.call('tg_nearest_u8_ranges', m, 50000) > 256
    for bad in ((0, 5, 3, 1), (5, 0, 3, 1), (5, 5, 0, 1), (5, 5, 16385, 1), (5, 5, 3, 0), (5, 5, 3, 17), (-1, 5, 3, 1)):
        with pytest.raises(lib.TgError, match="nearest_u8_workspace_bytes"):
            lib.call('tg_nearest_u8_workspace_bytes', *bad)
    for bad in ((0, 5), (5, 0), (-3, 5)):
        with pytest.raises(lib.TgError, match="nearest_u8_ranges"):
            lib.call('tg_nearest_u8_ranges', *bad)


def test_every_argument_violation_is_refused_before_any_launch():
    """no device is touched: the pointers are made-up addresses, which a launch would fault on and a refusal never reads."""
    from tg import lib
    h = lib.load()
    P = lambda a: C.c_void_p(a)
    m, n, d, k = 5, 7, 3, 2
    need = lib.call('tg_nearest_u8_workspace_bytes', m, n, d, k)
    names = ('q', 'm', 'r', 'n', 'd', 'k', 'base', 'merge', 'best_d2', 'best_idx', 'ws', 'nbytes')
    good = (P(0x10000), m, P(0x20000), n, d, k, 0, 0, P(0x30000), P(0x40000), P(0x50000), need)
    bad = {
        'm = 0': (dict(m=0), b"m and n must be at least 1"), 'n = 0': (dict(n=0), b"m and n must be at least 1"),
        'd = 0': (dict(d=0), b"d must be in 1..16384"), 'd = 16385': (dict(d=16385), b"d must be in 1..16384"),
        'k = 0': (dict(k=0), b"k must be in 1..16"), 'k = 17': (dict(k=17), b"k must be in 1..16"),
        'base < 0': (dict(base=-1), b"base"), 'base + n > INT32_MAX': (dict(base=INT32_MAX - n + 1), b"base"),
        'null q': (dict(q=None), b"null pointer"), 'null r': (dict(r=None), b"null pointer"),
        'null best_d2': (dict(best_d2=None), b"null pointer"), 'null best_idx': (dict(best_idx=None), b"null pointer"),
        'null workspace': (dict(ws=None), b"null pointer"), 'workspace one byte short': (dict(nbytes=need - 1), b"workspace of"),
    }
    for what, (over, message) in bad.items():
        args = [over.get(nm, v) for nm, v in zip(names, good)]
        assert h.tg_nearest_u8_i32(*(args + [None])) == TG_ERR_INVALID, what
        msg = h.tg_last_error_string()
        assert msg.startswith(b"nearest_u8") and message in msg, (what, msg)
    for over, message in ((dict(n=-1), b"n must not be negative"), (dict(scale=0.0), b"scale"), (dict(scale=float('inf')), b"scale"),
                          (dict(src=None), b"null pointer"), (dict(dst=None), b"null pointer")):
        a = dict(dict(src=P(0x10000), dst=P(0x20000), n=4, scale=2.0, shift=-1.0), **over)
        assert h.tg_f32_quantize_u8(a['src'], a['dst'], a['n'], a['scale'], a['shift'], None) == TG_ERR_INVALID, over
        assert message in h.tg_last_error_string(), (over, h.tg_last_error_string())
    assert h.tg_f32_quantize_u8(None, None, 0, 2.0, -1.0, None) == 0          # n = 0 is a no-op


def _planted(seed, m=9, n=50, d=6):
    rng = np.random.default_rng(seed)
    q, r = rng.integers(0, 256, (m, d), dtype=np.uint8), rng.integers(0, 4, (n, d), dtype=np.uint8)      # few values: ties abound
    r[40] = r[3]                                                       # duplicate rows in different chunks
    r[11] = r[3]
    q[2] = r[3]                                                        # a query equal to a reference row
    q[5:] = rng.integers(0, 4, (m - 5, d), dtype=np.uint8)
    return q, r


@pytest.mark.parametrize("k", [1, 3, 16])
def test_the_reference_is_invariant_to_chunking_and_chunk_order(k):
    q, r = _planted(5)
    whole = R.nearest(q, r, k)
    dist = R.d2(q, r)
    assert dist.dtype == np.int64 and dist[2, 3] == 0 and dist[0, 0] == ((r[0].astype(int) - q[0].astype(int)) ** 2).sum()
    assert tuple(whole[1][2, :min(k, 3)]) == (3, 11, 40)[:min(k, 3)] and (whole[0][2, :min(k, 3)] == 0).all()
    for i in range(q.shape[0]):                                        # the rule itself: lexicographic in (d2, index)
        pairs = sorted(zip(dist[i].tolist(), range(r.shape[0])))[:k]
        assert [p[0] for p in pairs] == whole[0][i].tolist() and [p[1] for p in pairs] == whole[1][i].tolist()
    cuts = [(0, 7), (7, 30), (30, 50)]
    for order in (cuts, cuts[::-1], [cuts[1], cuts[2], cuts[0]]):
        got = R.nearest_chunked(q, [(lo, r[lo:hi]) for lo, hi in order], k)
        assert (got[0] == whole[0]).all() and (got[1] == whole[1]).all(), order
    few = R.nearest(q, r[:k - 1], k) if k > 1 else None                # fewer rows than k: sentinels
    if few is not None:
        assert (few[0][:, k - 1:] == R.NONE_D2).all() and (few[1][:, k - 1:] == R.NONE_IDX).all() and (few[1][:, :k - 1] >= 0).all()
        again = R.nearest_chunked(q, [(0, r[:k - 1]), (k - 1, r[k - 1:])], k)             # ... which a later chunk replaces
        assert (again[0] == whole[0]).all() and (again[1] == whole[1]).all()


@pytest.mark.parametrize("scale,shift", [(2.0, -1.0), (1.0, 0.0)])
def test_the_quantiser_returns_every_byte_of_the_input_pipeline(scale, shift):
    u = np.arange(256, dtype=np.uint8)
    x = R.affine(u, scale, shift)
    assert x.dtype == np.float32 and x[0] == np.float32(shift) and x[255] == np.float32(scale + shift)
    got = R.quantize(x, scale, shift)
    assert got.dtype == np.uint8 and (got == u).all()
    odd = np.array([np.nan, np.inf, -np.inf, shift - 1.0, scale + shift + 1.0], np.float32)
    assert R.quantize(odd, scale, shift).tolist() == [0, 255, 0, 0, 255]
    half = ((np.arange(255) + 0.5) / 255.0 * scale + shift)           # round half up: just below a boundary stays, at or above goes up
    below = R.quantize(np.nextafter(half.astype(np.float32), np.float32(-np.inf)) - np.float32(1e-6), scale, shift)
    assert (below == np.arange(255)).all()


def test_check_sample_nearest_values_and_errors():
    from config import Config
    from Training import options
    from tg import lib
    from Input_Pipeline.mnistDataset import mnistDataset
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    from Input_Pipeline.syntheticDataset import syntheticDataset
    assert not hasattr(Config, 'SAMPLE_NEAREST')                       # not declared: the entry configurations are pinned
    ns = types.SimpleNamespace
    assert options.check_sample_nearest(ns()) is None and options.check_sample_nearest(ns(SAMPLE_NEAREST=None)) is None
    assert options.check_sample_nearest(ns(SAMPLE_METRICS=64)) is None
    for ok in (1, 3, 16, np.int64(5)):
        got = options.check_sample_nearest(ns(SAMPLE_METRICS=64, SAMPLE_NEAREST=ok))
        assert got == int(ok) and type(got) is int
    for bad in (0, 17, -3, True, False, 3.0, '3', (3,), float('nan')):
        with pytest.raises(ValueError, match="SAMPLE_NEAREST"):
            options.check_sample_nearest(ns(SAMPLE_METRICS=64, SAMPLE_NEAREST=bad))
    for without in (ns(SAMPLE_NEAREST=3), ns(SAMPLE_METRICS=None, SAMPLE_NEAREST=3)):
        with pytest.raises(ValueError, match="needs SAMPLE_METRICS"):
            options.check_sample_nearest(without)
    on = ns(SAMPLE_METRICS=64, SAMPLE_NEAREST=3)
    for Dataset in (mnistDataset, cifar10Dataset, mnistDataset('/data', None, 100, 'train')):          # UNIT_RANGE too; class or instance
        assert options.check_sample_nearest(on, Dataset) == 3
    with pytest.raises(lib.TgError, match="SAMPLE_NEAREST needs a training split of uint8 TFRecords.*syntheticDataset"):
        options.check_sample_nearest(on, syntheticDataset)
    assert options.check_sample_nearest(ns(), syntheticDataset) is None                   # off: any Dataset


def test_resolve_carries_the_setting_and_the_flag_reaches_the_config(monkeypatch, tmp_path):
    from Training import options
    from Training import Train_goodGAN as TG
    from tg import lib
    c = TG.MnistConfig()
    off = options.resolve(c)
    assert off.sample_nearest is None and options.Options.EXTRAS[-1] == 'sample_nearest' and 'sample_nearest' not in off._fields
    c.SAMPLE_METRICS, c.SAMPLE_NEAREST = 24, 3
    on = options.resolve(c)
    assert on.sample_nearest == 3 and tuple(on) == tuple(off) and on != off and hash(on) != hash(off) and on == options.resolve(c)
    c.SAMPLE_METRICS = None
    with pytest.raises(ValueError, match="SAMPLE_NEAREST"):
        options.resolve(c)
    seen = {}

    class Captured(object):
        def __init__(self, config, log_dir, save_dir, **kwargs):
            seen['config'] = config

        def train(self, Dataset, Model, sample_y):
            return None

    from Input_Pipeline.mnistDataset import mnistDataset
    monkeypatch.setattr(TG, '_root_dir', lambda: str(tmp_path))
    monkeypatch.setattr(TG, 'Train', Captured)
    TG._main_training_mnist(types.SimpleNamespace(sample_metrics=24, sample_nearest=3), Dataset=mnistDataset)
    assert seen['config'].SAMPLE_METRICS == 24 and seen['config'].SAMPLE_NEAREST == 3
    TG._main_training_mnist(types.SimpleNamespace(sample_metrics=24), Dataset=mnistDataset)             # a flag object without the attribute
    assert not hasattr(seen['config'], 'SAMPLE_NEAREST')
    with pytest.raises(lib.TgError, match="SAMPLE_NEAREST needs a training split"):                     # the default synthetic Dataset
        TG._main_training_mnist(types.SimpleNamespace(sample_metrics=24, sample_nearest=3))
    with pytest.raises(ValueError, match="needs SAMPLE_METRICS"):
        TG._main_training_mnist(types.SimpleNamespace(sample_nearest=3), Dataset=mnistDataset)


def test_the_tail_gains_exactly_the_four_tags_last():
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

    new = ('g_nn_rmse', 'g_nn_rmse_min', 'g_nn_class_agreement', 'val_nn_rmse')
    assert Evaluation.NEAREST_KEYS == new
    for base in (dict(SAMPLE_METRICS=24), dict(SAMPLE_METRICS=24, SAMPLE_MANIFOLD_K=3, EVAL_EMA=True, EVAL_REPORT=True)):
        off = Tail(**base)._tail_metric_tags()
        assert not set(new) & set(off)
        assert Tail(SAMPLE_NEAREST=None, **base)._tail_metric_tags() == off
        assert Tail(SAMPLE_NEAREST=3, **base)._tail_metric_tags() == off + new
    assert Tail()._tail_metric_tags() == ()


def _write_files(Dataset, root, shape, n_lab, n_unl, seed):
    from tg import io as tgio
    os.makedirs(os.path.join(root, 'Tfrecord'))
    rng = np.random.default_rng(seed)
    tr = Dataset(root, None, n_lab, 'train')
    imgs, labs = [], []
    for name, n in zip(tr.get_filenames(), (n_lab, n_unl)):
        img, lab = rng.integers(0, 256, (n,) + shape, dtype=np.uint8), rng.integers(0, 10, n)
        tgio.write_tfrecord(name, img, lab)
        imgs.append(img), labs.append(lab)
    return tr, np.concatenate(imgs), np.concatenate(labs)


def test_the_training_chunks_cover_every_record_once_in_order(tmp_path):
    from tg import lib
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    from Input_Pipeline.mnistDataset import mnistDataset
    from Input_Pipeline.syntheticDataset import syntheticDataset
    from Input_Pipeline.tfrecordDataset import training_chunks, training_files
    from Model.zca import zca_training_chunks
    for Dataset, shape in ((mnistDataset, (28, 28, 1)), (cifar10Dataset, (32, 32, 3))):               # a UNIT_RANGE dataset too
        root = str(tmp_path / Dataset.__name__)
        ds, images, labels = _write_files(Dataset, root, shape, 10, 23, 3)
        assert len(ds.input_from_tfrecord_filename()) == 3 and [len(r) for r in training_files(ds)] == [10, 23]
        got_i, got_l, sizes, files = [], [], [], []
        for rec, idx in training_chunks(ds, rows=8):
            img, lab = rec.gather(idx)
            got_i.append(img), got_l.append(lab), sizes.append(len(idx)), files.append(rec.path)
        assert sizes == [8, 2, 8, 8, 7] and files[0] == files[1] != files[2] == files[4]
        assert np.array_equal(np.concatenate(got_i), images) and np.array_equal(np.concatenate(got_l), labels)
        assert sum(len(idx) for _, idx in training_chunks(ds)) == 33                       # the default piece holds a whole small file
        with pytest.raises(lib.TgError, match="training split only"):
            list(training_chunks(Dataset(root, None, 10, 'test')))
        if Dataset.UNIT_RANGE:                                         # the ZCA fit keeps its own refusal of x / 255 scaling
            with pytest.raises(lib.TgError, match="ZCA = 'fit' needs"):
                list(zca_training_chunks(ds))
        else:
            assert [len(i) for _, i in zca_training_chunks(ds, rows=8)] == sizes
    with pytest.raises(lib.TgError, match="tfrecordDataset"):
        list(training_chunks(syntheticDataset.__new__(syntheticDataset)))
