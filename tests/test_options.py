"""Training/options.py: config.Config is the one place a default is written, and every device-free check runs before a device exists."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEFAULT = dict(NUM_CLASSES=10, BATCH_SIZE=8, BATCH_SIZE_G=8, BATCH_SIZE_L_D=2, BATCH_SIZE_U_D=6)      # what Config declares no usable default for


def test_a_bare_object_resolves_like_a_config_subclass():
    from config import Config
    from Training.options import cla_lr, opt, resolve
    bare = type('Bare', (object,), NO_DEFAULT)()
    full = type('Full', (Config,), NO_DEFAULT)()
    assert resolve(bare) == resolve(full)
    assert resolve(bare)._asdict() == dict(
        mfma_dtype='f32', act_dtype='f32', num_classes=10, loss='GAN', optimizers=('adam',) * 3, clip_norms=(None,) * 3, momentum=0.9, seed=0,
        no_grad_buckets=False, summary=True, summary_scalar=True, summary_histogram=False, summary_image=False, summary_image_max_outputs=2)
    bare.LOSS = full.LOSS = 'WGAN_GP'
    assert resolve(bare) == resolve(full) and resolve(bare).loss == 'WGAN_GP'
    assert opt(bare, 'EXEC_MODE') == Config.EXEC_MODE and opt(bare, 'USE_HIP_GRAPH') is None
    assert cla_lr(full) == Config.LEARNING_RATE
    full.CLA_LEARNINIG_RATE = 3e-3
    assert cla_lr(full) == 3e-3


def test_a_bad_mfma_dtype_raises_before_any_device_is_touched(monkeypatch):
    import torch
    from tg import dist as tgdist
    from Training.options import resolve
    from Training.Train_goodGAN import Train
    bad = type('Bad', (object,), dict(NO_DEFAULT, MFMA_DTYPE='fp16'))()
    with pytest.raises(ValueError, match=r"MFMA_DTYPE must be 'f32' or 'bf16', got 'fp16'"):
        resolve(bad)
    monkeypatch.setattr(tgdist, 'init', lambda: pytest.fail("Train initialised the process group before the config was checked"))
    with pytest.raises(ValueError, match=r"MFMA_DTYPE must be 'f32' or 'bf16', got 'fp16'"):
        Train(bad, None, None)
    assert not torch.cuda.is_initialized()


def test_the_trainer_restates_no_config_default():
    """no getattr(x, 'UPPER_CASE', default) in Training/Train_goodGAN.py or the three modules that hold the trainer's other parts — but
    for the two optional class attributes of a MODEL, which are no config settings and have no Config default to fall back to."""
    training = os.path.join(ROOT, 'tensorflow-implementation-of-triple-gan_amd', 'Training')
    src = ''.join(open(os.path.join(training, name)).read() for name in ('Train_goodGAN.py', 'evaluation.py', 'epoch_tail.py', 'schedule.py'))
    found = re.findall(r"""getattr\(\s*([^\n]*?)\s*,\s*['"]([A-Z][A-Z0-9_]*)['"]\s*,""", src)
    assert set(found) <= {('m', 'CONSISTENCY'), ('self.model', 'CONSISTENCY'), ('self.model', 'GRAD_BUCKETS')}, found
    assert not re.search(r"""^def check_|^    def check_""", src, flags=re.M)          # the validators live in Training/options.py
