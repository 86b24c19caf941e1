"""CPU tests of the WGAN-GP training step: the config switch (Training/Train_goodGAN.check_loss) and the float64 restatement of one
iteration (tests/wgan_gp_step_reference.py), whose three gradients are pinned here by central differences on a few parameters per
network at a tiny batch."""
import copy
import os
import sys
import types

import numpy as np
import pytest

from oracle import nets_goodgan as NG
from oracle import step_cifar10 as SC
from oracle import step_goodgan as SG
import wgan_gp_step_reference as W

TINY = dict(B_G=4, L_C=2, U_C=2, L_D=1, U_D=3)
HYPER = dict(lr=3e-4, cla_lr=3e-3, beta1=0.5, lambda_1=0.3, lambda_2=0.5)


def _cfg(**kw):
    base = dict(LOSS='WGAN_GP', MFMA_DTYPE='f32', ACT_DTYPE='f32', MINIBATCH_DIS=False, BATCH_SIZE_G=100, BATCH_SIZE_L_D=20, BATCH_SIZE_U_D=80)
    base.update(kw)
    return types.SimpleNamespace(**base)


# ------------------------------------------------------------------------------------------------------------- check_loss
def test_config_default_loss_is_gan():
    from config import Config
    from Training.Train_goodGAN import check_loss
    assert Config.LOSS == 'GAN'
    assert check_loss(types.SimpleNamespace()) == 'GAN'
    assert check_loss(_cfg(LOSS='GAN', MFMA_DTYPE='bf16', MINIBATCH_DIS=True, BATCH_SIZE_G=7)) == 'GAN'     # the GAN step is unchanged


def test_check_loss_refuses_unknown_values():
    from Training.Train_goodGAN import check_loss
    for v in ('WGAN', 'wgan_gp', 'gan', None):
        with pytest.raises(ValueError, match='LOSS'):
            check_loss(_cfg(LOSS=v))


@pytest.mark.parametrize('over, key', [(dict(MFMA_DTYPE='bf16'), 'MFMA_DTYPE'),
                                       (dict(MFMA_DTYPE='bf16', ACT_DTYPE='bf16'), 'MFMA_DTYPE'),
                                       (dict(MINIBATCH_DIS=True), 'MINIBATCH_DIS'),
                                       (dict(BATCH_SIZE_U_D=79), 'BATCH_SIZE_L_D'),
                                       (dict(BATCH_SIZE_G=64), 'BATCH_SIZE_G')])
def test_check_loss_refusals_name_the_config_key(over, key):
    from tg import lib
    from Training.Train_goodGAN import check_loss
    with pytest.raises(lib.TgError, match=key):
        check_loss(_cfg(**over))


def test_check_loss_accepts_every_shipped_config():
    """the experiment configs of Training/Train_goodGAN.py and the bench configs (all 20 + 80 = 100, stress64 51 + 205 = 256)."""
    import Training.Train_goodGAN as TG
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    sys.path.insert(0, tools)
    try:
        import bench_config
    finally:
        sys.path.remove(tools)
    from config import Config
    seen = []
    for fn in (TG._main_training_svhn, TG._main_training_cifar10, TG._main_training_mnist, TG._main_training_stress64):
        captured = {}
        orig = TG._run
        TG._run = lambda TempConfig, *a, **k: captured.setdefault('c', TempConfig)
        try:
            fn()
        finally:
            TG._run = orig
        cls = captured['c']
        c = types.SimpleNamespace(**{k: getattr(cls, k) for k in dir(cls) if k.isupper()})
        c.LOSS = 'WGAN_GP'
        assert TG.check_loss(c) == 'WGAN_GP', cls.DATA_NAME
        seen.append(cls.DATA_NAME)
    assert sorted(seen) == ['cifar10', 'mnist', 'stress64', 'svhn']
    for name in bench_config.SHAPES:
        c = bench_config.make_config(name, 'wgan_gp')
        assert isinstance(c, Config) and c.LOSS == 'WGAN_GP'
        if c.MFMA_DTYPE == 'f32':
            assert TG.check_loss(c) == 'WGAN_GP', name
    assert bench_config.make_config('cifar10').LOSS == 'GAN'


def test_loss_flag_reaches_the_config():
    from Training.Train_goodGAN import _customize_config
    from config import Config
    c = Config.__new__(Config)
    _customize_config(c, types.SimpleNamespace(loss='WGAN_GP'))
    assert c.LOSS == 'WGAN_GP'


# ------------------------------------------------------------------------------------------------------------- the restatement
def _f64(d):
    return {k: (_f64(v) if isinstance(v, dict) else np.asarray(v, np.float64)) for k, v in d.items()}


def _setup(data):
    if data == 'cifar10':
        full = dict(SC.SIZES, **TINY)
        P = SC.init_params(0)
        st = SC.new_state(_f64(P))
        batch, rnd = SC.synth_batch(100, full), SC.synth_rnd(200, full)
        zca = tuple(np.asarray(a, np.float64) for a in SC.synth_zca())
    else:
        P = NG.init_params(data, 0)
        st = SG.new_state(_f64(P))
        batch, rnd = SG.synth_batch(data, 100, TINY), SG.synth_rnd(data, 200, TINY)
        zca = None
    rnd = _f64(rnd)
    rnd['D']['GP'] = _f64(W.gp_draws(data, TINY['B_G'], 300))
    return st, _f64(batch), rnd, zca


def _phase(data, key, st, b, rnd, zca):
    if data == 'cifar10':
        return {'D': lambda: W.d_phase_cifar10(st, b, rnd['D'], HYPER, zca), 'G': lambda: W.g_phase_cifar10(st, b, rnd['G'], HYPER),
                'C': lambda: W.c_phase_cifar10(st, b, rnd['C'], HYPER, zca)}[key]()
    return {'D': lambda: W.d_phase_goodgan(st, data, b, rnd['D'], HYPER), 'G': lambda: W.g_phase_goodgan(st, data, b, rnd['G'], HYPER),
            'C': lambda: W.c_phase_goodgan(st, data, b, rnd['C'], HYPER)}[key]()


@pytest.mark.parametrize('data', ['cifar10', 'svhn', 'mnist'])
@pytest.mark.parametrize('key', ['D', 'G', 'C'])
def test_restated_gradients_match_central_differences(data, key):
    st0, b, rnd, zca = _setup(data)
    st = copy.deepcopy(st0)
    _phase(data, key, st, b, rnd, zca)
    grads = st['last_grads'][key]
    # the three variables with the largest gradients, at each one's largest element
    top = sorted(grads, key=lambda k: -np.abs(grads[k]).max())[:3]
    eps = 1e-6
    for k in top:
        i = np.unravel_index(np.argmax(np.abs(grads[k])), grads[k].shape)
        vals = []
        for sgn in (1.0, -1.0):
            s = copy.deepcopy(st0)
            s['P'][k] = s['P'][k].copy()
            s['P'][k][i] += sgn * eps
            vals.append(_phase(data, key, s, b, rnd, zca))
        fd = (vals[0] - vals[1]) / (2 * eps)
        assert abs(fd - grads[k][i]) <= 1e-5 * max(1.0, abs(grads[k][i])), (key, k, i, fd, grads[k][i])


def test_the_penalty_is_in_the_restated_d_loss_and_gradient():
    """the D-update's value and gradient carry 10 gp: without it they differ by the penalty's own (non-zero) contribution."""
    st, b, rnd, zca = _setup('cifar10')
    out = {}
    d = W.d_phase_cifar10(st, b, rnd['D'], HYPER, zca, gp_out=out)
    wd1, wd2, wd3 = out['wd']
    assert abs(d - (-(wd1 + HYPER['lambda_1'] * wd2 + HYPER['lambda_2'] * wd3) + out['gp10'])) < 1e-12
    assert out['gp10'] > 0
    g = st['last_grads']['D']
    for k, v in out['gp_grads'].items():
        assert np.array_equal(g[k], out['head_grads'][k] + v)
        if k.endswith('bias'):
            assert not np.any(v)
