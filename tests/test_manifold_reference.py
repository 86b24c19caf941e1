"""The k-nearest-neighbour manifold metrics without a device: tests/manifold_reference.py — the fp32 distance chain the
kernels of csrc/knn.hip are held to bit for bit (tests/test_gpu_manifold_kernels.py), and the four metrics on top of it.

Bound: the chain is within (c + 3) 2^-24 of the float64 distance, relative (manifold_reference.bound; its docstring derives it), on
the shapes the GPU tests run.  Two negative controls on the same data show what the bound tells apart: the data rounded to bf16, and
an fp32 Gram-form distance |a|^2 + |b|^2 - 2ab after a shift of +64 — the offset post-ReLU pooled features share, and the reason the
kernel is not a GEMM.  Closed forms: identical sets, disjoint clusters and mode dropping have answers known without computing a
distance.  Settings: Training/options.check_sample_manifold_k."""
import inspect
import os
import types

import numpy as np
import pytest

import manifold_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1, 1, 1, 1), (5, 7, 3, 8, 1), (17, 4, 5, 8, 16), (257, 130, 33, 40, 3), (64, 64, 128, 128, 5), (1000, 777, 128, 160, 3)]
_DATA = {}


def data(n, m, c, ld):
    """(reference rows [n, c], query rows [m, c]) of a GPU test shape, without the padding; made once, never written to."""
    key = (n, m, c, ld)
    if key not in _DATA:
        r, q = R.features(n, c, ld, 100 * n + c)[:, :c], R.features(m, c, ld, 100 * m + c + 7)[:, :c]
        r.setflags(write=False), q.setflags(write=False)
        _DATA[key] = (r, q)
    return _DATA[key]


@pytest.mark.parametrize("n,m,c,ld,k", SHAPES)
def test_the_fp32_chain_is_within_its_bound_of_float64(n, m, c, ld, k):
    r, q = data(n, m, c, ld)
    for a, b in ((q, r), (r, r)):
        d32, d64 = R.d2_chain32(a, b), R.d2_f64(a, b)
        assert d32.dtype == np.float32 and d32.shape == (a.shape[0], b.shape[0])
        rel = np.abs(d32.astype(np.float64) - d64) / np.where(d64 > 0, d64, 1.0)
        print("n %d m %d c %d: worst error %.3f of the bound" % (n, m, c, rel.max() / R.bound(c)))
        assert R.within_bound(d32, d64, c)
    assert (np.diag(R.d2_chain32(r, r)) == 0).all()


@pytest.mark.parametrize("n,m,c,ld,k", SHAPES)
def test_the_bound_rejects_bf16_rounded_data(n, m, c, ld, k):
    r, q = data(n, m, c, ld)
    assert not R.within_bound(R.d2_chain32(R.to_bf16(q), R.to_bf16(r)), R.d2_f64(q, r), c)


@pytest.mark.parametrize("n,m,c,ld,k", SHAPES)
def test_the_bound_rejects_the_gram_form_on_shifted_data(n, m, c, ld, k):
    """the shift is exact in neither form's favour: both see the same shifted fp32 rows, and float64 of those rows is the truth."""
    r, q = data(n, m, c, ld)
    rs, qs = (r + np.float32(64)).astype(np.float32), (q + np.float32(64)).astype(np.float32)
    d64 = R.d2_f64(qs, rs)
    assert R.within_bound(R.d2_chain32(qs, rs), d64, c)               # the difference form does not care about the offset
    assert not R.within_bound(R.d2_gram32(qs, rs), d64, c)


def test_knn_self_leaves_the_row_out_by_index_and_query_takes_the_lowest_index():
    x = np.array([[0.0], [1.0], [1.0], [3.0], [0.0]], np.float32)
    got = R.knn_self(x, 2)
    assert got.tolist() == [[0.0, 1.0], [0.0, 1.0], [0.0, 1.0], [4.0, 4.0], [0.0, 1.0]]      # a duplicate contributes a 0
    assert R.radii(x, 1).tolist() == [0.0, 0.0, 0.0, 4.0, 0.0]
    count, nn, idx = R.query(np.array([[1.0], [2.0], [-5.0]], np.float32), x, R.radii(x, 2))
    assert idx.tolist() == [1, 1, 0] and nn.tolist() == [0.0, 1.0, 25.0] and idx.dtype == np.int32
    assert count.tolist() == [5, 3, 0] and count.dtype == np.int32
    assert R.query(x, x)[0] is None


def _clusters(rng, n, c, centre, spread=0.5):
    return (rng.standard_normal((n, c)) * spread + centre).astype(np.float32)


@pytest.mark.parametrize("dist", [R.d2_chain32, R.d2_f64])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_identical_sets(dist, k):
    x = _clusters(np.random.default_rng(k), 40, 6, 0.0)
    m = R.metrics(x, x.copy(), k, dist)
    assert m['precision'] == m['recall'] == m['coverage'] == 1.0
    assert m['density'] >= 1.0 / k and set(m) == set(R.KEYS)           # every fake sits at least in its own twin's ball


@pytest.mark.parametrize("dist", [R.d2_chain32, R.d2_f64])
@pytest.mark.parametrize("k", [1, 3])
def test_disjoint_clusters(dist, k):
    rng = np.random.default_rng(10 + k)
    real, fake = _clusters(rng, 30, 4, 0.0), _clusters(rng, 25, 4, 1000.0)     # 2 000 apart, a few units across
    assert R.metrics(real, fake, k, dist) == dict.fromkeys(R.KEYS, 0.0)


@pytest.mark.parametrize("dist", [R.d2_chain32, R.d2_f64])
@pytest.mark.parametrize("k", [1, 3])
def test_mode_dropping(dist, k):
    """reals in two clusters A and B, fakes exact copies of A's reals: every fake is on a real (precision 1), and the reals a fake ball
    reaches are exactly A's (recall |A| / n)."""
    rng = np.random.default_rng(20 + k)
    a, b = _clusters(rng, 12, 4, 0.0), _clusters(rng, 28, 4, 1000.0)
    m = R.metrics(np.concatenate([a, b]), a.copy(), k, dist)
    assert m['precision'] == 1.0 and m['recall'] == 12 / 40.0
    assert m['coverage'] == 12 / 40.0                                  # A's reals have a fake at distance 0, B's none within reach


@pytest.mark.parametrize("k", [1, 3, 16])
def test_fewer_than_k_plus_one_rows_is_nan(k):
    rng = np.random.default_rng(3)
    enough, short = _clusters(rng, k + 1, 3, 0.0), _clusters(rng, k, 3, 0.0)
    for real, fake in ((short, enough), (enough, short)):
        m = R.metrics(real, fake, k)
        assert set(m) == set(R.KEYS) and all(np.isnan(v) for v in m.values())
    assert all(np.isfinite(v) for v in R.metrics(enough, enough, k).values())


def test_host_reduction_of_the_package_matches_the_reference():
    """tg.metrics is importable without a device, and its float64 reduction of the query outputs is the reference's."""
    from tg import metrics as M
    assert M.MANIFOLD_KEYS == R.KEYS and M.MAX_K == 16
    rng = np.random.default_rng(5)
    real, fake, k = _clusters(rng, 50, 5, 0.0), _clusters(rng, 37, 5, 0.3), 3
    r2_real, r2_fake = R.radii(real, k), R.radii(fake, k)
    count_fr, _, _ = R.query(fake, real, r2_real)
    count_rf, nn_rf, _ = R.query(real, fake, r2_fake)
    got = M.manifold_from_counts(k, 37, count_fr, count_rf, nn_rf, r2_real)
    assert got == R.metrics(real, fake, k) and 0.0 < got['precision'] <= 1.0
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="1..16"):
            M.manifold_metrics(None, None, bad)
    for bad in (0, 513):
        with pytest.raises(ValueError, match="1..512"):
            M.FeatureBank(bad, 'cpu')
    few = types.SimpleNamespace(c=4, n=3)
    assert all(np.isnan(v) for v in M.manifold_metrics(few, types.SimpleNamespace(c=4, n=100), 3).values())     # no launch, no device


def test_check_sample_manifold_k_values_and_errors():
    from config import Config
    from Training import options
    assert not hasattr(Config, 'SAMPLE_MANIFOLD_K')                    # not declared: the entry configurations are pinned
    ns = types.SimpleNamespace
    assert options.check_sample_manifold_k(ns()) is None and options.check_sample_manifold_k(ns(SAMPLE_MANIFOLD_K=None)) is None
    assert options.check_sample_manifold_k(ns(SAMPLE_METRICS=64)) is None
    for ok in (1, 3, 16, np.int64(5)):
        got = options.check_sample_manifold_k(ns(SAMPLE_METRICS=64, SAMPLE_MANIFOLD_K=ok))
        assert got == int(ok) and type(got) is int
    for bad in (0, 17, -3, True, False, 3.0, '3', (3,), float('nan')):
        with pytest.raises(ValueError, match="SAMPLE_MANIFOLD_K"):
            options.check_sample_manifold_k(ns(SAMPLE_METRICS=64, SAMPLE_MANIFOLD_K=bad))
    with pytest.raises(ValueError, match="needs SAMPLE_METRICS"):
        options.check_sample_manifold_k(ns(SAMPLE_MANIFOLD_K=3))
    with pytest.raises(ValueError, match="needs SAMPLE_METRICS"):
        options.check_sample_manifold_k(ns(SAMPLE_METRICS=None, SAMPLE_MANIFOLD_K=3))


def test_resolve_carries_the_setting_beside_its_fields():
    from Training import options
    from Training.Train_goodGAN import Cifar10Config
    c = Cifar10Config()
    off = options.resolve(c)
    assert off.sample_manifold_k is None and 'sample_manifold_k' in options.Options.EXTRAS and 'sample_manifold_k' not in off._fields
    c.SAMPLE_METRICS, c.SAMPLE_MANIFOLD_K = 500, 3
    on = options.resolve(c)
    assert on.sample_manifold_k == 3 and tuple(on) == tuple(off) and on != off and hash(on) != hash(off) and on == options.resolve(c)
    c.SAMPLE_MANIFOLD_K = None
    assert options.resolve(c) != on
    c.SAMPLE_METRICS, c.SAMPLE_MANIFOLD_K = None, 3
    with pytest.raises(ValueError, match="SAMPLE_MANIFOLD_K"):
        options.resolve(c)


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
    TG._main_training_mnist(types.SimpleNamespace(sample_metrics=64, sample_manifold_k=3))
    assert seen['config'].SAMPLE_METRICS == 64 and seen['config'].SAMPLE_MANIFOLD_K == 3
    TG._main_training_mnist(types.SimpleNamespace(sample_metrics=64))                      # a flag object without the attribute
    assert seen['config'].SAMPLE_METRICS == 64 and not hasattr(seen['config'], 'SAMPLE_MANIFOLD_K')


def test_header_declares_the_kernels_and_their_workspace_queries():
    from tg import lib
    sigs = lib.parse_header()
    for name, nargs in (('tg_knn_self_f32', 9), ('tg_manifold_query_f32', 14), ('tg_knn_self_workspace_bytes', 2),
                        ('tg_manifold_query_workspace_bytes', 2)):
        assert name in sigs and len(sigs[name][1]) == nargs, name
    assert lib.call('tg_knn_self_workspace_bytes', 10000, 3) > 0 and lib.call('tg_manifold_query_workspace_bytes', 10000, 10000) > 0
    assert lib.call('tg_knn_self_workspace_bytes', 2, 1) == 2 * 4 and lib.call('tg_manifold_query_workspace_bytes', 1, 1) == 12
    for bad in ((3, 3), (100, 0), (100, 17)):
        with pytest.raises(lib.TgError, match="knn_self_workspace_bytes"):
            lib.call('tg_knn_self_workspace_bytes', *bad)
    for bad in ((0, 5), (5, 0)):
        with pytest.raises(lib.TgError, match="manifold_query_workspace_bytes"):
            lib.call('tg_manifold_query_workspace_bytes', *bad)


def test_the_trainer_surface_and_the_docs_say_what_the_numbers_are_not():
    from tg import metrics as M
    from Training.Train_goodGAN import Train
    assert list(inspect.signature(Train.sample_manifold_metrics).parameters)[1:] == ['batches', 'n_samples', 'manifold_k', 'ema', 'return_banks']
    assert list(inspect.signature(Train.sample_metrics).parameters)[1:] == ['batches', 'n_samples', 'ema']          # as it was
    assert M.check_k(np.int64(3)) == 3 and type(M.check_k(np.int64(3))) is int and M.check_k(16) == 16
    for bad in (0, 17, True, None, 3.0, '3'):
        with pytest.raises(ValueError, match="manifold_k must be an integer in 1..16"):                               # before anything of the trainer is touched
            Train.sample_manifold_metrics(None, [], 8, bad)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '9.11' in design and 'tg_knn_self_f32' in design and 'tg_manifold_query_f32' in design
    assert 'SAMPLE_MANIFOLD_K' in open(os.path.join(ROOT, 'README.md')).read()
    papers = open(os.path.join(ROOT, 'PAPERS.md')).read()
    assert 'Kynkäänniemi' in papers and 'Naeem' in papers
