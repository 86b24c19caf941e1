"""The launch behind ops.wn_data_init: tg_wn_init_f32, the data-dependent initialisation of a weight-normalised layer.
It is an eager, one-time launch outside every recorded step - refused inside a hipGraph capture or a launch-plan recording - and lives
here, beside tg/ops.py, whose launches are the ones a step replays."""
from . import lib
from .lib import ACT
from .ops import _call, _p, require_f32
from .runtime import ctx


def data_init(t, g, b, eps, init_scale, act=None, alpha=0.0):
    """see ops.wn_data_init.  t: Act [n,h,w,c] (fp32); g, b: the variables' device tensors of t.c values each (written).  Returns the Act
    act(g*t + b) in t's layout, channel padding zeroed."""
    require_f32(t, 'wn_data_init')
    cx = ctx()
    if cx.capturing or lib._recorder is not None:
        raise lib.TgError("ops.wn_data_init: called inside a hipGraph capture / launch-plan recording; the data-dependent initialisation assigns "
                          "variables once, before the step is recorded")
    if g.numel() != t.c or b.numel() != t.c:
        raise lib.TgError("ops.wn_data_init: g / b hold %d / %d values, the activation has %d channels" % (g.numel(), b.numel(), t.c))
    work = cx.scratch('wni', _call('tg_wn_init_workspace_floats', t.rows, t.c))
    y = cx.new_act(t.n, t.h, t.w, t.c, t.ld)
    _call('tg_wn_init_f32', t.ptr, t.ld, t.rows, t.c, t.ld, float(eps), float(init_scale), ACT[act], float(alpha), _p(work), _p(g), _p(b),
          y.ptr, y.ld, cx.stream)
    return y
