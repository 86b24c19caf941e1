"""The host side of the generated-sample metrics without a device: tg.metrics.frechet_distance against closed forms and an
independent route, the covariance from accumulated moments against np.cov, the two settings' checks, and the C declaration.

Tolerance of a distance (tests/sample_metrics_reference.py): TOL_FD = 1e-6 of scale = tr C1 + tr C2 + |m1 - m2|^2 — the square root of
a near-zero eigenvalue turns 1e-16 of noise into 1e-8.  Measured on a CPU: full-rank cases (n, c) = (257, 33) and (1000, 128) stay below
1e-9 of the scale, rank-deficient ones (40, 128) and (2, 5) below 1e-7.  A rank-deficient pair has no independent reference of that
accuracy (the unsymmetric eigvals route carries the same square-root noise), so there only finite and >= -TOL_FD * scale is asserted."""
import os
import types

import numpy as np
import pytest

import sample_metrics_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_RANK = [(257, 33), (1000, 128)]
RANK_DEFICIENT = [(40, 128), (2, 5)]
_STATS = {}


def stats(n, c):
    """two Gaussian fits (n, mean, cov) of n rows of c features, different in mean and scale; made once per shape."""
    if (n, c) not in _STATS:
        rng = np.random.default_rng(100 * n + c)
        mix = rng.standard_normal((c, c)) / np.sqrt(c)
        a = (rng.standard_normal((n, c)) @ mix + 0.5).astype(np.float32)
        b = (1.3 * rng.standard_normal((n, c)) @ mix.T - 0.25).astype(np.float32)
        _STATS[(n, c)] = (R.mean_cov64(a), R.mean_cov64(b), a, b)
    return _STATS[(n, c)]


def rotation(c, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((c, c)))
    return q


@pytest.mark.parametrize("n,c", FULL_RANK + RANK_DEFICIENT)
def test_identical_statistics_give_zero_and_a_mean_shift_its_square(n, c):
    from tg import metrics as M
    (_, m1, C1), _, _, _ = stats(n, c)
    tol = R.TOL_FD * R.fd_scale(m1, C1, m1, C1)
    assert abs(M.frechet_distance(m1, C1, m1, C1)) <= tol
    d = np.linspace(-1.0, 2.0, c)
    assert abs(M.frechet_distance(m1, C1, m1 + d, C1) - d @ d) <= R.TOL_FD * R.fd_scale(m1, C1, m1 + d, C1)


@pytest.mark.parametrize("c", [5, 33, 128])
def test_commuting_covariances_have_a_closed_form(c):
    from tg import metrics as M
    rng = np.random.default_rng(c)
    q = rotation(c, c + 1)
    a, b = rng.uniform(0.1, 4.0, c), rng.uniform(0.1, 4.0, c)
    a[0] = 0.0                                                    # a singular direction is part of the contract (clipped, not NaN)
    C1, C2 = (q * a) @ q.T, (q * b) @ q.T
    m1, m2 = rng.standard_normal(c), rng.standard_normal(c)
    want = ((m1 - m2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert abs(M.frechet_distance(m1, C1, m2, C2) - want) <= R.TOL_FD * R.fd_scale(m1, C1, m2, C2)


@pytest.mark.parametrize("n,c", FULL_RANK)
def test_agrees_with_the_eigenvalues_of_the_product(n, c):
    from tg import metrics as M
    (_, m1, C1), (_, m2, C2), _, _ = stats(n, c)
    got, want, scale = M.frechet_distance(m1, C1, m2, C2), R.frechet_eigvals(m1, C1, m2, C2), R.fd_scale(m1, C1, m2, C2)
    print("(%d, %d): distance %.9g, eigvals route %.9g, difference %.3g of the scale" % (n, c, got, want, abs(got - want) / scale))
    assert abs(got - want) <= R.TOL_FD * scale
    assert got > 0.01 * scale                                     # the two fits do differ: the agreement is not that of two zeros
    assert abs(M.frechet_distance(m2, C2, m1, C1) - got) <= R.TOL_FD * scale          # symmetric in its arguments


@pytest.mark.parametrize("n,c", FULL_RANK)
def test_invariant_under_an_orthogonal_change_of_basis(n, c):
    from tg import metrics as M
    (_, m1, C1), (_, m2, C2), _, _ = stats(n, c)
    q = rotation(c, 7)
    got = M.frechet_distance(q @ m1, q @ C1 @ q.T, q @ m2, q @ C2 @ q.T)
    assert abs(got - M.frechet_distance(m1, C1, m2, C2)) <= R.TOL_FD * R.fd_scale(m1, C1, m2, C2)


@pytest.mark.parametrize("n,c", RANK_DEFICIENT)
def test_rank_deficient_covariances_stay_finite_and_not_negative(n, c):
    from tg import metrics as M
    (_, m1, C1), (_, m2, C2), _, _ = stats(n, c)
    got, scale = M.frechet_distance(m1, C1, m2, C2), R.fd_scale(m1, C1, m2, C2)
    print("(%d, %d): distance %.9g, scale %.3g" % (n, c, got, scale))
    assert np.isfinite(got) and got >= -R.TOL_FD * scale


def test_non_finite_statistics_give_nan():
    from tg import metrics as M
    m, C = np.zeros(3), np.eye(3)
    assert np.isnan(M.frechet_distance(m, C, m, np.full((3, 3), np.nan)))
    assert np.isnan(M.frechet_distance(np.array([0.0, np.inf, 0.0]), C, m, C))


@pytest.mark.parametrize("n,c", FULL_RANK + RANK_DEFICIENT)
def test_covariance_from_moments_is_np_cov(n, c):
    from tg import metrics as M
    (n_a, mean_a, cov_a), _, a, _ = stats(n, c)
    total, gram, _, _ = R.moments64(a)
    mu, cov = M.mean_cov(n, total, gram)
    # gram - n mu mu^T cancels |mu|^2 against the second moment: absolute error ~ 2^-53 n (|gram| / n) per entry, measured against that
    lim = 1e-12 * (np.abs(gram).max() / n + 1.0)
    assert np.abs(mu - mean_a).max() <= 1e-14 * (np.abs(mean_a).max() + 1.0)
    assert np.abs(cov - cov_a).max() <= lim and (cov == cov.T).all()


def test_fewer_than_two_rows_have_no_covariance():
    from tg import metrics as M
    for n in (0, 1):
        mu, cov = M.mean_cov(n, np.ones(4) * n, np.ones((4, 4)) * n)
        assert mu.shape == (4,) and cov.shape == (4, 4) and np.isnan(mu).all() and np.isnan(cov).all()
        assert np.isnan(M.frechet_distance(mu, cov, np.zeros(4), np.eye(4)))


def test_feature_moments_refuses_a_width_the_kernel_does_not_take():
    from tg import metrics as M
    for bad in (0, 513, -1):
        with pytest.raises(ValueError, match="1..512"):
            M.FeatureMoments(bad, 'cpu')


def test_check_eval_ema_values_and_errors():
    from config import Config
    from Training import options
    assert not hasattr(Config, 'EVAL_EMA') and not hasattr(Config, 'SAMPLE_METRICS')   # not declared: the entry configurations are pinned
    ns = types.SimpleNamespace
    assert options.check_eval_ema(ns()) is False and options.check_eval_ema(ns(EVAL_EMA=None)) is False
    assert options.check_eval_ema(ns(EVAL_EMA=False)) is False and options.check_eval_ema(ns(EVAL_EMA=0)) is False
    assert options.check_eval_ema(ns(EVAL_EMA=True)) is True and options.check_eval_ema(ns(EVAL_EMA=1)) is True
    for bad in ('yes', 'True', 2, -1, 0.5, 1.0, (True,), [1]):
        with pytest.raises(ValueError, match="EVAL_EMA"):
            options.check_eval_ema(ns(EVAL_EMA=bad))


def test_check_sample_metrics_values_and_errors():
    from Training import options
    ns = types.SimpleNamespace
    assert options.check_sample_metrics(ns()) is None and options.check_sample_metrics(ns(SAMPLE_METRICS=None)) is None
    assert options.check_sample_metrics(ns(SAMPLE_METRICS=1)) == 1
    got = options.check_sample_metrics(ns(SAMPLE_METRICS=np.int64(10000)))
    assert got == 10000 and type(got) is int
    for bad in (0, -5, True, False, 64.0, '64', (64,), float('nan')):
        with pytest.raises(ValueError, match="SAMPLE_METRICS"):
            options.check_sample_metrics(ns(SAMPLE_METRICS=bad))


def test_resolve_keeps_its_field_list_and_carries_both():
    from Training import options
    from Training.Train_goodGAN import Cifar10Config
    fields = ('mfma_dtype', 'act_dtype', 'num_classes', 'loss', 'optimizers', 'clip_norms', 'momentum', 'seed', 'no_grad_buckets',
              'summary', 'summary_scalar', 'summary_histogram', 'summary_image', 'summary_image_max_outputs')
    c = Cifar10Config()
    off = options.resolve(c)
    assert off._fields == fields and tuple(off._asdict()) == fields and len(tuple(off)) == len(fields)
    assert (off.eval_ema, off.sample_metrics, off.wn_init) == (False, None, None)
    c.EVAL_EMA, c.SAMPLE_METRICS = True, 500
    on = options.resolve(c)
    assert (on.eval_ema, on.sample_metrics) == (True, 500) and on._fields == fields and tuple(on) == tuple(off)
    assert on != off and hash(on) != hash(off) and on == options.resolve(c) and hash(on) == hash(options.resolve(c))
    c.EVAL_EMA = False
    half = options.resolve(c)
    assert half != on and half != off and off == options.resolve(Cifar10Config())
    c.SAMPLE_METRICS = 0
    with pytest.raises(ValueError, match="SAMPLE_METRICS"):
        options.resolve(c)


def test_flags_reach_the_config_an_entry_point_hands_to_train(monkeypatch, tmp_path):
    from Training import Train_goodGAN as TG
    seen = {}

    class Captured(object):
        def __init__(self, config, log_dir, save_dir, **kwargs):
            seen['config'] = config

        def train(self, Dataset, Model, sample_y):
            return None

    monkeypatch.setattr(TG, '_root_dir', lambda: str(tmp_path))
    monkeypatch.setattr(TG, 'Train', Captured)
    TG._main_training_mnist(types.SimpleNamespace(eval_ema=True, sample_metrics=64))
    assert seen['config'].EVAL_EMA is True and seen['config'].SAMPLE_METRICS == 64
    TG._main_training_mnist(types.SimpleNamespace(seed=3))
    assert not hasattr(seen['config'], 'EVAL_EMA') and not hasattr(seen['config'], 'SAMPLE_METRICS')


def test_header_declares_both_symbols():
    from tg import lib
    sigs = lib.parse_header()
    assert 'tg_feature_moments_f32' in sigs and 'tg_feature_moments_workspace_bytes' in sigs
    assert len(sigs['tg_feature_moments_f32'][1]) == 9 and len(sigs['tg_feature_moments_workspace_bytes'][1]) == 2
    text = open(os.path.join(ROOT, "include", "tg_kernels.h")).read()
    assert "int64_t tg_feature_moments_workspace_bytes(int n, int c);" in text
    assert lib.call('tg_feature_moments_workspace_bytes', 0, 128) == 0 and lib.call('tg_feature_moments_workspace_bytes', 1000, 128) > 0


def test_evaluate_and_the_cifar_classifier_take_the_new_arguments():
    """the surface the GPU tests drive, checked where no GPU is: the keyword, the method, and Model/nn.py's ValueError still in place."""
    import inspect
    from Model import nn
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10
    from Training.Train_goodGAN import Train
    assert inspect.signature(Train.evaluate).parameters['ema'].default is False
    assert list(inspect.signature(Train.sample_metrics).parameters)[1:] == ['batches', 'n_samples', 'ema']
    assert 'getter' in inspect.signature(Good_GAN_cifar10.classifier).parameters
    with pytest.raises(ValueError, match="ema"):
        nn._salimans(None, 1, 1, 1, 'SAME', None, 1.0, False, object(), 1e-8)
