"""config.WN_INIT without a device: Training/options.check_wn_init, the setting's absence from config.Config (the entry
configurations' attribute sets stay the recorded ones), and --wn-init reaching the config an entry point hands to Train."""
import json
import types

import numpy as np
import pytest

from test_entry_configs import ENTRIES, FAKE_ROOT, GOLDEN, snapshot


def test_check_wn_init_values_and_errors():
    from config import Config
    from Training import options
    assert not hasattr(Config, 'WN_INIT')                    # not declared: the attribute sets of the entry configurations are pinned
    assert options.check_wn_init(types.SimpleNamespace()) is None                      # absent
    assert options.check_wn_init(types.SimpleNamespace(WN_INIT=None)) is None
    assert options.check_wn_init(types.SimpleNamespace(WN_INIT='data')) == 'data'
    for bad in ('Data', 'none', '', True, 1, 0, ('data',), np.array(['data'])):
        with pytest.raises(ValueError, match="WN_INIT"):
            options.check_wn_init(types.SimpleNamespace(WN_INIT=bad))


def test_resolve_carries_it():
    from Training import options
    from Training.Train_goodGAN import Cifar10Config
    c = Cifar10Config()
    assert options.resolve(c).wn_init is None
    c.WN_INIT = 'data'
    assert options.resolve(c).wn_init == 'data'
    on = options.resolve(c)
    c.WN_INIT = None
    off = options.resolve(c)
    # carried beside the record's fields (their list is what it was), and part of what makes two records equal
    assert 'wn_init' not in on._asdict() and tuple(on) == tuple(off) and on != off and off == options.resolve(Cifar10Config())
    c.WN_INIT = 'batch'
    with pytest.raises(ValueError, match="WN_INIT"):
        options.resolve(c)


def _capture(entry, monkeypatch, FLAGS):
    from Training import Train_goodGAN as TG
    seen = {}

    class Captured(object):
        def __init__(self, config, log_dir, save_dir, **kwargs):
            seen['config'] = config

        def train(self, Dataset, Model, sample_y):
            return None

    monkeypatch.setattr(TG, '_root_dir', lambda: FAKE_ROOT)
    monkeypatch.setattr(TG, 'Train', Captured)
    getattr(TG, '_main_training_' + entry)(FLAGS)
    return seen['config']


@pytest.mark.parametrize('entry', ENTRIES)
def test_entry_configs_keep_their_attribute_sets_without_flags(entry, monkeypatch):
    from Training import options
    c = _capture(entry, monkeypatch, None)
    assert sorted(snapshot(c)) == sorted(json.load(open(GOLDEN))[entry])
    assert not hasattr(c, 'WN_INIT') and options.check_wn_init(c) is None


@pytest.mark.parametrize('entry', ENTRIES)
def test_flag_reaches_the_config_handed_to_train(entry, monkeypatch):
    from Training import options
    c = _capture(entry, monkeypatch, types.SimpleNamespace(wn_init='data'))
    assert c.WN_INIT == 'data' and options.resolve(c).wn_init == 'data'
    assert sorted(set(snapshot(c)) - {'WN_INIT'}) == sorted(json.load(open(GOLDEN))[entry])       # nothing else moved


def test_flags_without_the_flag_leave_the_attribute_absent(monkeypatch):
    from Training import options
    for flags in (types.SimpleNamespace(), types.SimpleNamespace(wn_init=None), types.SimpleNamespace(epochs=3)):
        assert not hasattr(_capture('mnist', monkeypatch, flags), 'WN_INIT')
    with pytest.raises(ValueError, match="WN_INIT"):                                   # an unknown value travels and is refused where it is read
        options.resolve(_capture('mnist', monkeypatch, types.SimpleNamespace(wn_init='yes')))
