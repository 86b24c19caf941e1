"""config.R1_GAMMA without a device: every accepted and refused value of Training/options.check_r1_gamma, the refusals of
LOSS = 'WGAN_GP', bf16 operands and minibatch discrimination, resolve() with and without the key, the setting's absence from
config.Config (the entry configurations' attribute sets stay the recorded ones), and --r1-gamma reaching the config an entry point hands
to Train."""
import json
import types

import numpy as np
import pytest

from test_entry_configs import ENTRIES, GOLDEN, snapshot
from test_wn_init_config import _capture


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def test_accepted_values():
    from config import Config
    from Training import options
    assert not hasattr(Config, 'R1_GAMMA')                   # not declared: the attribute sets of the entry configurations are pinned
    assert options.check_r1_gamma(_ns()) is None                                       # absent
    assert options.check_r1_gamma(_ns(R1_GAMMA=None)) is None
    for v, want in ((10.0, 10.0), (1, 1.0), (np.float32(0.5), 0.5), (np.int64(3), 3.0), (1e-30, 1e-30), (1e30, 1e30)):
        got = options.check_r1_gamma(_ns(R1_GAMMA=v))
        assert got == want and type(got) is float
    # no relation between the batch sizes is needed (WGAN-GP's L_D + U_D == B_G is the interpolation's)
    assert options.check_r1_gamma(_ns(R1_GAMMA=2.0, BATCH_SIZE_L_D=3, BATCH_SIZE_U_D=4, BATCH_SIZE_G=100)) == 2.0
    assert options.check_r1_gamma(_ns(R1_GAMMA=2.0, LOSS='GAN', MFMA_DTYPE='f32', MINIBATCH_DIS=False)) == 2.0


@pytest.mark.parametrize('bad', [0, 0.0, -1.0, -0.0, float('nan'), float('inf'), -float('inf'), True, False, np.bool_(True), '10', (10.0,), [1.0],
                                 np.array([1.0]), 1 + 0j, np.float32('nan')])
def test_refused_values(bad):
    from Training import options
    with pytest.raises(ValueError, match='R1_GAMMA'):
        options.check_r1_gamma(_ns(R1_GAMMA=bad))


def test_refused_combinations():
    from Training import options
    from tg import lib
    with pytest.raises(ValueError, match=r"R1_GAMMA.*WGAN_GP"):
        options.check_r1_gamma(_ns(R1_GAMMA=1.0, LOSS='WGAN_GP', BATCH_SIZE_L_D=2, BATCH_SIZE_U_D=6, BATCH_SIZE_G=8))
    with pytest.raises(lib.TgError, match=r"R1.*MFMA_DTYPE"):
        options.check_r1_gamma(_ns(R1_GAMMA=1.0, MFMA_DTYPE='bf16'))
    with pytest.raises(lib.TgError, match=r"R1.*MINIBATCH_DIS"):
        options.check_r1_gamma(_ns(R1_GAMMA=1.0, MINIBATCH_DIS=True))
    # with the option off none of them is looked at
    assert options.check_r1_gamma(_ns(LOSS='WGAN_GP', MFMA_DTYPE='bf16', MINIBATCH_DIS=True)) is None
    # a bad value is reported before a bad combination
    with pytest.raises(ValueError, match='positive finite'):
        options.check_r1_gamma(_ns(R1_GAMMA=-1.0, LOSS='WGAN_GP'))


def test_resolve_with_and_without_the_key():
    from Training import options
    from Training.Train_goodGAN import Cifar10Config
    c = Cifar10Config()
    off = options.resolve(c)
    assert off.r1_gamma is None and 'r1_gamma' in options.Options.EXTRAS
    assert 'r1_gamma' not in off._fields and 'r1_gamma' not in off._asdict()
    c.R1_GAMMA = 10
    on = options.resolve(c)
    assert on.r1_gamma == 10.0 and tuple(on) == tuple(off) and on != off and hash(on) != hash(off) and on == options.resolve(c)
    c.R1_GAMMA = 1.0
    assert options.resolve(c) != on
    c.R1_GAMMA = None
    assert options.resolve(c) == off == options.resolve(Cifar10Config())
    c.R1_GAMMA, c.LOSS = 1.0, 'WGAN_GP'
    with pytest.raises(ValueError, match='R1_GAMMA'):
        options.resolve(c)
    c.LOSS, c.MFMA_DTYPE = 'GAN', 'bf16'
    from tg import lib
    with pytest.raises(lib.TgError, match='R1'):
        options.resolve(c)


def test_a_bad_gamma_raises_before_any_device_is_touched(monkeypatch):
    import torch
    from tg import dist as tgdist
    from Training.Train_goodGAN import Cifar10Config, Train
    c = Cifar10Config()
    c.R1_GAMMA = 0.0
    monkeypatch.setattr(tgdist, 'init', lambda: pytest.fail("Train initialised the process group before the config was checked"))
    with pytest.raises(ValueError, match='R1_GAMMA'):
        Train(c, None, None)
    assert not torch.cuda.is_initialized()


@pytest.mark.parametrize('entry', ENTRIES)
def test_flag_reaches_the_config_handed_to_train(entry, monkeypatch):
    from Training import options
    c = _capture(entry, monkeypatch, _ns(r1_gamma=10.0))
    assert c.R1_GAMMA == 10.0 and options.resolve(c).r1_gamma == 10.0
    assert sorted(set(snapshot(c)) - {'R1_GAMMA'}) == sorted(json.load(open(GOLDEN))[entry])       # nothing else moved
    assert 'R1_GAMMA' in c.config_str()                                                             # the run comments name it


def test_flags_without_the_flag_leave_the_attribute_absent(monkeypatch):
    from Training import options
    for flags in (None, _ns(), _ns(r1_gamma=None), _ns(epochs=3)):
        c = _capture('cifar10', monkeypatch, flags)
        assert not hasattr(c, 'R1_GAMMA') and options.resolve(c).r1_gamma is None
    with pytest.raises(ValueError, match='R1_GAMMA'):                                  # a refused value travels and is refused where it is read
        options.resolve(_capture('cifar10', monkeypatch, _ns(r1_gamma=-3.0)))


def test_bench_config_tool_takes_the_flag():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    import bench_config
    from Training import options
    c = bench_config.make_config('cifar10', 'gan', r1_gamma=10.0)
    assert c.R1_GAMMA == 10.0 and options.resolve(c).r1_gamma == 10.0
    assert not hasattr(bench_config.make_config('cifar10', 'gan'), 'R1_GAMMA')


def test_docs_name_the_option():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        assert 'R1_GAMMA' in open(os.path.join(root, name)).read(), name
    assert '9.15' in open(os.path.join(root, 'DESIGN.md')).read()
