"""CPU checks of the public surface of config.CLIP_NORM: check_clip_norm, the host-side workspace query, the header's five
new symbols, Train_base._train_op_w_grads and the INTEGRATION table."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('tg_grad_norm_workspace_bytes', 'tg_grad_norm_clip_f32', 'tg_adam_clip_f32', 'tg_momentum_clip_f32', 'tg_rmsprop_clip_f32')
STORE_SIZES = dict(good_generator=5129248, discriminator=327520, classifier=3121856)     # tools/bench_optim.py store_sizes()


def _config(**over):
    from config import Config

    class C(Config):
        BATCH_SIZE = 4
        IMAGE_HEIGHT = IMAGE_WIDTH = 32
        CHANNEL = 3
    c = C()
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_check_clip_norm_accepts_and_normalises():
    import numpy as np
    from Training.Train_goodGAN import check_clip_norm
    assert _config().CLIP_NORM is None
    assert check_clip_norm(_config()) == (None, None, None)
    assert check_clip_norm(_config(CLIP_NORM=1.0)) == (1.0, 1.0, 1.0)
    assert check_clip_norm(_config(CLIP_NORM=5)) == (5.0, 5.0, 5.0)
    assert check_clip_norm(_config(CLIP_NORM=np.float32(0.5))) == (0.5, 0.5, 0.5)
    assert check_clip_norm(_config(CLIP_NORM=(1e-3, 1e30, None))) == (1e-3, 1e30, None)
    assert check_clip_norm(_config(CLIP_NORM=[None, None, 2.0])) == (None, None, 2.0)
    assert check_clip_norm(_config(CLIP_NORM=(None, None, None))) == (None, None, None)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float('nan'), float('inf'), (1.0, 2.0), (1.0, 2.0, 3.0, 4.0), (), 'one', (1.0, 'x', None),
                                 (1.0, -2.0, None), (1.0, float('nan'), 1.0), True, {'d': 1.0}])
def test_check_clip_norm_refuses(bad):
    from Training.Train_goodGAN import check_clip_norm
    with pytest.raises(ValueError, match='CLIP_NORM'):
        check_clip_norm(_config(CLIP_NORM=bad))


def test_clip_norm_flag_reaches_the_config():
    """--clip-norm X on an entry point: _customize_config copies an argparse-like object's clip_norm into CLIP_NORM."""
    from Training.Train_goodGAN import _customize_config, check_clip_norm

    class Flags(object):
        clip_norm = 2.5
    c = _config()
    _customize_config(c, Flags())
    assert c.CLIP_NORM == 2.5 and check_clip_norm(c) == (2.5, 2.5, 2.5)


def test_workspace_query_answers_on_the_host():
    from tg import lib
    sizes = [1] + sorted(STORE_SIZES.values()) + [10 ** 7, 10 ** 9]
    got = [lib.call('tg_grad_norm_workspace_bytes', n) for n in sizes]
    assert all(b > 0 and b % 8 == 0 for b in got)
    assert got == sorted(got) and got[0] == 8 and got[-1] == got[-2] <= 8192          # monotone; one double per workgroup, capped grid
    assert lib.call('tg_grad_norm_workspace_bytes', 3) == lib.call('tg_grad_norm_workspace_bytes', 8192) == 8
    assert lib.call('tg_grad_norm_workspace_bytes', 8192 + 4) == 16
    for n in (0, -5):
        with pytest.raises(lib.TgError, match='positive'):
            lib.call('tg_grad_norm_workspace_bytes', n)


def test_header_declares_and_library_exports_the_new_symbols():
    import ctypes as C
    from tg import lib
    sigs = lib.parse_header()
    handle = lib.load()
    for name in NEW_SYMBOLS:
        assert name in sigs and hasattr(handle, name), name
    assert sigs['tg_grad_norm_workspace_bytes'] == (C.c_int64, [C.c_int64])
    assert len(sigs['tg_grad_norm_clip_f32'][1]) == 8
    for kind in ('adam', 'momentum', 'rmsprop'):                      # the arguments of the unclipped entry point plus factor_dev
        a, b = sigs['tg_%s_f32' % kind][1], sigs['tg_%s_clip_f32' % kind][1]
        assert b == a[:-1] + [C.c_void_p] + a[-1:], kind
    from tg import plan
    assert plan.signature('tg_grad_norm_clip_f32') == 'pifpppi' and plan.signature('tg_grad_norm_workspace_bytes') is None
    assert plan.signature('tg_momentum_clip_f32') == plan.signature('tg_momentum_f32') + 'p'


def test_train_op_w_grads_is_on_train_base():
    from Training.train_base import AdamOptimizer, MomentumOptimizer, RMSPropOptimizer, Train_base
    from Training.Train_goodGAN import Train
    sig = inspect.signature(Train_base._train_op_w_grads)
    assert list(sig.parameters) == ['self', 'optimizer', 'store', 'grad_scale', 'clip']
    assert sig.parameters['grad_scale'].default == 1.0 and sig.parameters['clip'].default is None
    assert list(inspect.signature(Train_base._train_op).parameters) == ['self', 'optimizer', 'store', 'grad_scale']
    for cls in (AdamOptimizer, MomentumOptimizer, RMSPropOptimizer):
        p = inspect.signature(cls.apply).parameters
        assert list(p) == ['self', 'store', 'grad_scale', 'factor_dev'] and p['factor_dev'].default is None
    assert all(hasattr(Train, m) for m in ('set_clip_norm', 'grad_norms'))


def test_docs_name_the_entry_points():
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    row = [l for l in text.splitlines() if 'train_base.py:70-73' in l]
    assert len(row) == 1
    for name in NEW_SYMBOLS[1:]:
        assert name in row[0], name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^### 9\.6 ', design, flags=re.M)
    assert 'CLIP_NORM' in open(os.path.join(ROOT, 'README.md')).read()
