"""The five experiment configurations of Training/Train_goodGAN.py, attribute for attribute, against tests/golden/entry_configs.json:
what each `_main_training_*` hands to Train — every non-callable, non-dunder attribute dir() lists, arrays as shape / dtype / sha256 —
recorded with `_root_dir` patched to FAKE_ROOT before the configurations became one shared base and five subclasses.  The key sets must
be equal too: an attribute that appears or disappears changes the run comments config_str() writes."""
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'entry_configs.json')
ENTRIES = ('svhn', 'cifar10', 'cifar100', 'mnist', 'stress64')
FAKE_ROOT = '/nonexistent/triple-gan'


def _enc(v):
    if isinstance(v, np.ndarray):
        return dict(shape=list(v.shape), dtype=str(v.dtype), sha256=hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())
    if isinstance(v, (tuple, list)):
        return [_enc(e) for e in v]
    return v


def snapshot(config):
    return {a: _enc(getattr(config, a)) for a in dir(config) if not a.startswith('__') and not callable(getattr(config, a))}


def capture(entry, monkeypatch):
    """the configuration `_main_training_<entry>` builds, as Train receives it (no device: Train is replaced)."""
    from Training import Train_goodGAN as TG

    class Captured(object):
        def __init__(self, config, log_dir, save_dir, **kwargs):
            assert (log_dir, save_dir) == (config.LOG_DIR, config.WEIGHT_DIR)
            self.config = config

        def train(self, Dataset, Model, sample_y):
            return snapshot(self.config)

    monkeypatch.setattr(TG, '_root_dir', lambda: FAKE_ROOT)
    monkeypatch.setattr(TG, 'Train', Captured)
    return getattr(TG, '_main_training_' + entry)()


@pytest.mark.parametrize('entry', ENTRIES)
def test_entry_config_is_the_recorded_one(entry, monkeypatch):
    want = json.load(open(GOLDEN))[entry]
    got = json.loads(json.dumps(capture(entry, monkeypatch)))
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}


def test_the_fixture_holds_the_five_entry_points():
    assert sorted(json.load(open(GOLDEN))) == sorted(ENTRIES)
