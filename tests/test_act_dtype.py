"""Host-side rules of bf16-stored activations (config.ACT_DTYPE, tg.runtime.Act.dtype) — no GPU needed."""
import types

import numpy as np
import pytest
import torch

from tg import lib, ops
from tg.runtime import Act


def _cfg(**kw):
    return types.SimpleNamespace(**kw)


def test_act_dtype_switch_is_checked_against_the_mfma_operand_type():
    from Training.Train_goodGAN import check_act_dtype
    assert check_act_dtype(_cfg()) == 'f32'
    assert check_act_dtype(_cfg(MFMA_DTYPE='f32', ACT_DTYPE='f32')) == 'f32'
    assert check_act_dtype(_cfg(MFMA_DTYPE='bf16', ACT_DTYPE='bf16')) == 'bf16'
    with pytest.raises(ValueError):
        check_act_dtype(_cfg(MFMA_DTYPE='f32', ACT_DTYPE='bf16'))
    with pytest.raises(ValueError):
        check_act_dtype(_cfg(ACT_DTYPE='bf16'))                      # MFMA_DTYPE defaults to 'f32'
    with pytest.raises(ValueError):
        check_act_dtype(_cfg(MFMA_DTYPE='bf16', ACT_DTYPE='fp16'))


def test_config_default_is_f32():
    from config import Config
    assert Config.ACT_DTYPE == 'f32'


def _act16(n=2, h=4, w=4, c=24, ld=32):
    x = np.zeros((n, h, w, ld), np.float32)
    x[..., :c] = np.arange(n * h * w * c, dtype=np.float32).reshape(n, h, w, c) / 64.0
    return Act(torch.from_numpy(x.reshape(-1)).to(torch.bfloat16), n, h, w, c, ld, dtype='bf16'), x


def test_bf16_act_handle_keeps_the_meaning_of_its_accessors():
    a, x = _act16()
    assert a.dtype == 'bf16' and a.ld == 32 and a.rows == 32
    got = a.numpy()
    assert got.dtype == np.float32 and got.shape == (2, 4, 4, 24)
    np.testing.assert_array_equal(got, torch.from_numpy(x[..., :24].copy()).to(torch.bfloat16).float().numpy())
    v = a.view_rows(1, 2)
    assert v.dtype == 'bf16' and v.n == 1 and v.t.dtype == torch.bfloat16 and v.t.numel() == 4 * 4 * 32
    np.testing.assert_array_equal(v.numpy(), got[1:2])
    assert Act(torch.zeros(8), 1, 1, 1, 8, 8).dtype == 'f32'


def test_act_dtype_must_match_its_storage():
    with pytest.raises(lib.TgError):
        Act(torch.zeros(8), 1, 1, 1, 8, 8, dtype='bf16')
    with pytest.raises(lib.TgError):
        Act(torch.zeros(8, dtype=torch.bfloat16), 1, 1, 1, 8, 8)
    with pytest.raises(lib.TgError):
        Act(torch.zeros(8), 1, 1, 1, 8, 8, dtype='f16')


@pytest.mark.parametrize("op", [lambda a: ops.global_avgpool(a), lambda a: ops.activation(a, 'relu'), lambda a: ops.maxpool2_dropout(a, None, 2.0),
                                lambda a: ops.batch_norm_eval(a, None, None, None, None, 1e-5), lambda a: ops.reshape(a, 2, 1, 1, 4 * 4 * 24),
                                lambda a: ops.concat_batch([a]), lambda a: ops.cond_concat(a, None, 10), lambda a: ops.global_maxpool(a)])
def test_ops_without_a_bf16_reader_refuse_a_bf16_act(op):
    a, _ = _act16()
    with pytest.raises(lib.TgError, match='bf16'):
        op(a)


def test_launch_argument_refuses_a_bf16_tensor():
    with pytest.raises(lib.TgError):
        ops._p(torch.zeros(4, dtype=torch.bfloat16))
    assert ops._p(torch.zeros(4)) is not None


def test_conv_refuses_a_bf16_input_outside_the_bf16_3x3_path(monkeypatch):
    """conv2d reads a bf16-stored input only with bf16 MFMA operands and on the 3x3 / stride-1 / SAME layers the bf16-input kernels serve."""
    a, _ = _act16()
    for mfma, k in (('f32', 3), ('bf16', 1)):
        monkeypatch.setattr(ops, 'ctx', lambda: types.SimpleNamespace(mfma_dtype=mfma))
        with pytest.raises(lib.TgError, match='bf16'):
            ops.conv2d(a, torch.zeros(1), None, 32, k, 1, 'SAME')
