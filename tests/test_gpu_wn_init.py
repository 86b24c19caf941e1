"""tg_wn_init_f32 (csrc/norm.hip), the data-dependent weight-norm initialisation, held to float64 by direct calls, and the
layers that use it (Model/nn.py inside Context.assigning_init, NN_Base._WN_* with init=True) against tests/wn_init_reference.py.

Kernel: outputs are `guarded` (tests/kernel_check.py).  g, b and y are in the POINTWISE class against the float64 rule evaluated on the
same fp32 inputs and the same fp32 (eps, init_scale) arguments, with K from the roundings the kernel is specified to make — K_G = 1,
K_B = 2, K_PRE = 3 on |g||t| + |b|, plus K_ACT of the activation (tests/wn_init_reference.py derives them; the negative control showing
that this bound rejects a one-pass fp32 accumulation runs on the CPU, tests/test_wn_init_reference.py, on the same ill-conditioned
inputs this file feeds the kernel).  Padding columns are exactly +0.0, the guards are intact, two launches agree bit for bit.

Layers: batch 4 on 8x8 maps with odd channel counts; g, b and the output against the float64 restatement at the forward tolerance of
tests/test_gpu_surface.py (1e-4 of the largest value: the fp32 MFMA product in front of the statistics)."""
import numpy as np
import pytest

import gpu_common as G
import wn_init_reference as R
from kernel_check import ACTS, ALPHA, act64, assert_bits, assert_pointwise, bits, dev, finish, guarded, lib, ptr, st

pytestmark = pytest.mark.gpu

ROWS = [1, 2, 63, 64, 65, 1023, 4099]           # one chunk of 256 rows and its edges, several chunks, more chunks than the 8 summing lanes
CS = [1, 3, 10, 33, 64, 130]                    # below / at / above the 64-column workgroup, odd, more than two column blocks


def _run(L, t, rows, c, ld_t, ld_y, eps, scale, act):
    """one call on fresh guarded outputs -> (g, b, y [rows, ld_y])."""
    wsn = L.call('tg_wn_init_workspace_floats', rows, c)
    assert wsn >= 2 * c * ((rows + 255) // 256 + 1)
    ws, g, b, y = guarded(wsn), guarded(c), guarded(c), guarded(rows * ld_y)
    L.call('tg_wn_init_f32', ptr(t), ld_t, rows, c, ld_y, float(eps), float(scale), L.ACT[act], float(ALPHA), ws.ptr, g.ptr, b.ptr, y.ptr,
           ld_y, st())
    ws.check_guard()
    return finish(g), finish(b), finish(y, (rows, ld_y))


def _check(L, t_host, rows, c, ld, eps, scale, act, what):
    x = np.full((rows, ld), np.nan, np.float32)          # whatever lies in the input's padding is never read
    x[:, :c] = t_host
    td = dev(x)
    g, b, y = _run(L, td, rows, c, ld, ld, eps, scale, act)
    e64, s64 = np.float64(np.float32(eps)), np.float64(np.float32(scale))
    m, v, g64, b64 = R.rule(t_host, e64, s64)
    assert_pointwise(g, g64, np.abs(g64), R.K_G, what + ' g')
    assert_pointwise(b, b64, np.abs(m) * np.abs(g64), R.K_B, what + ' b')
    ref = act64(g64 * t_host.astype(np.float64) + b64, act)
    assert_pointwise(y[:, :c], ref, R.y_bound(t_host, g64, b64, ref, act), 1, what + ' y')
    assert (bits(y[:, c:]) == 0).all(), "%s: padding columns not +0.0" % what
    g2, b2, y2 = _run(L, td, rows, c, ld, ld, eps, scale, act)
    assert_bits(g2, g, what + ' g again')
    assert_bits(b2, b, what + ' b again')
    assert_bits(y2, y, what + ' y again')
    return g, b, (m, v, g64, b64)


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_shapes(rows, c):
    L = lib()
    rng = np.random.default_rng(1000 * rows + c)
    t = (rng.standard_normal((rows, c)) * rng.uniform(0.05, 5.0, c) + rng.uniform(-3, 3, c)).astype(np.float32)
    for ld in (c, c + (5 if c % 2 else 6)):               # ld == c, and ld > c with c_zero_to = ld
        _check(L, t, rows, c, ld, 1e-8 if c % 2 else 1e-10, 1.0 if rows % 2 else 0.1, 'lrelu', "rows=%d c=%d ld=%d" % (rows, c, ld))


@pytest.mark.parametrize("eps", [1e-8, 1e-10])
def test_constant_channel(eps):
    """v = 0: g = init_scale / sqrt(eps), the largest gain the rule can assign."""
    L = lib()
    rng = np.random.default_rng(7)
    t = rng.standard_normal((300, 5)).astype(np.float32)
    t[:, 1], t[:, 4] = np.float32(3.25), np.float32(-0.7)
    g, b, (m, v, g64, b64) = _check(L, t, 300, 5, 8, eps, 0.1, 'none', "constant eps=%g" % eps)
    assert v[1] == 0.0 and v[4] == 0.0
    want = np.float32(np.float64(np.float32(0.1)) / np.sqrt(np.float64(np.float32(eps))))
    assert g[1] == want and g[4] == want


@pytest.mark.parametrize("ld", [3, 8])
def test_ill_conditioned_channels(ld):
    """mean 1e3, standard deviation 1e-2: the inputs of the CPU negative control (an fp32 E[x^2] - m^2 lies far outside this bound)."""
    L = lib()
    t = R.ill_conditioned(1023, 3)
    g, b, (m, v, g64, b64) = _check(L, t, 1023, 3, ld, 1e-8, 1.0, 'none', "ill-conditioned ld=%d" % ld)
    assert R.within(g, b, t, 1e-8)
    g1, b1 = R.one_pass_fp32_model(t, 1e-8)
    assert not R.within(g1, b1, t, 1e-8)


@pytest.mark.parametrize("act", ACTS)
def test_each_activation(act):
    L = lib()
    rng = np.random.default_rng(31)
    t = (rng.standard_normal((65, 33)) * 2.0 + rng.uniform(-1, 1, 33)).astype(np.float32)
    t[::9] = t[0]                                                        # repeated rows: exact zeros of g t + b do not occur, ties do
    _check(L, t, 65, 33, 40, 1e-10, 2.5, act, act)


def test_arguments_are_checked():
    L = lib()
    t, o = dev(np.zeros(64, np.float32)), guarded(64)
    for rows, c, czt, ld_t, ld_y in ((0, 4, 4, 4, 4), (4, 0, 4, 4, 4), (4, 5, 5, 4, 8), (4, 4, 3, 4, 4), (4, 4, 9, 4, 8)):
        with pytest.raises(L.TgError, match="wn_init"):
            L.call('tg_wn_init_f32', ptr(t), ld_t, rows, c, czt, 1e-8, 1.0, 0, 0.0, o.ptr, o.ptr, o.ptr, o.ptr, ld_y, st())
    o.check_guard()


# ---------------------------------------------------------------------------------------------------------------- layers

TOL = 1e-4


@pytest.fixture(scope="module")
def plain():
    return G.fresh_trainer(G.make_config(dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)))


def _x(rng, shape):
    return (rng.standard_normal(shape) + 0.5).astype(np.float32)


def _compare(st, scope, y, ref):
    t, g64, b64, y64 = ref
    assert G.rel_err(st.get(scope + '/g'), g64) < TOL, scope
    assert G.rel_err(st.get(scope + '/b'), b64) < TOL, scope
    assert G.rel_err(y, y64) < TOL, scope


NN_LAYERS = {  # name -> (input shape, call, (kind of product, eps as the reference writes it))
    'conv2d_WN': ((4, 8, 8, 5), lambda nn, a, kw: nn.conv2d_WN(a, 33, name='L', use_weight_normalization=True, **kw), ('conv', 1e-8)),
    'conv2d_WN_mobn': ((4, 8, 8, 5), lambda nn, a, kw: nn.conv2d_WN(a, 33, name='L', pad='VALID', use_weight_normalization=True,
                                                                     use_mean_only_batch_normalization=True, **kw), ('conv', 1e-8)),
    'dense_WN': ((4, 1, 1, 37), lambda nn, a, kw: nn.dense_WN(a, 33, name='L', use_weight_normalization=True, **kw), ('dense', 1e-10)),
    'dense_WN_mobn': ((4, 1, 1, 37), lambda nn, a, kw: nn.dense_WN(a, 33, name='L', use_weight_normalization=True,
                                                                   use_mean_only_batch_normalization=True, **kw), ('dense', 1e-10)),
    'NiN_WN': ((4, 8, 8, 7), lambda nn, a, kw: nn.NiN_WN(a, 33, name='L', use_weight_normalization=True, **kw), ('dense', 1e-10)),
    'NiN_WN_mobn': ((4, 8, 8, 7), lambda nn, a, kw: nn.NiN_WN(a, 33, name='L', use_weight_normalization=True,
                                                              use_mean_only_batch_normalization=True, **kw), ('dense', 1e-10)),
    'conv2d': ((4, 8, 8, 5), lambda nn, a, kw: nn.conv2d(a, 33, stride=[2, 2], init_scale=0.7, counters={}, **kw), ('conv', 1e-8)),
    'dense': ((4, 1, 1, 37), lambda nn, a, kw: nn.dense(a, 33, counters={}, train_scale=False, **kw), ('dense', 1e-10)),
    'deconv2d': ((4, 8, 8, 5), lambda nn, a, kw: nn.deconv2d(a, 33, filter_size=[5, 5], stride=[2, 2], counters={}, **kw), ('deconv', 1e-8)),
}
NN_SCOPE = {'NiN_WN': 'L/L', 'NiN_WN_mobn': 'L/L', 'conv2d': 'conv2d_0', 'dense': 'dense_0', 'deconv2d': 'deconv2d_0'}


@pytest.mark.parametrize("layer", sorted(NN_LAYERS))
def test_nn_layers_assign_inside_the_scope_only(plain, layer):
    from Model import nn
    tr, cx = plain, plain.cx
    shape, call, (kind, eps) = NN_LAYERS[layer]
    rng = np.random.default_rng(len(layer))
    x = _x(rng, shape)
    root = 'wn_' + layer
    scope = root + '/' + NN_SCOPE.get(layer, 'L')
    act = tr.model._leaky_relu
    lrelu = lambda v: np.where(v > 0, v, 0.2 * v)
    with cx.phase_scope('wn_' + layer, record=False), cx.variable_scope(root):
        a = cx.from_numpy(x, ld=32 if shape[-1] <= 32 else 64)
        y0 = call(nn, a, dict(init=True, nonlinearity=act)).numpy()                    # outside the scope: the reference's forward-only branch
        st = cx.stores[root]
        assert (st.get(scope + '/g') == 1.0).all() and (st.get(scope + '/b') == 0.0).all()
        pop = [n for n in st.names() if n.endswith('pop_mean')]
        with cx.assigning_init() as done:
            y1 = call(nn, a, dict(init=True, nonlinearity=act)).numpy()
        assert done == [scope]
        assert not cx.assign_init and cx.tape is None
    V = st.get(scope + '/V').astype(np.float64)
    stride = 2 if layer == 'conv2d' else 1
    ref = R.wn_layer(x.reshape(shape if kind != 'dense' or layer.startswith('NiN') else (shape[0], shape[-1])), V, kind, eps,
                     0.7 if layer == 'conv2d' else 1.0, stride, 'VALID' if layer == 'conv2d_WN_mobn' else 'SAME')
    ref = (ref[0], ref[1], ref[2], lrelu(ref[3]))
    _compare(st, scope, y1.reshape(ref[3].shape), ref)
    assert G.rel_err(y0.reshape(ref[3].shape), ref[3]) < TOL                           # both branches return the same value
    for n in pop:
        assert (st.get(n) == 0.0).all(), n                                             # pop_mean is not touched
    with cx.phase_scope('wn_' + layer, record=False), cx.variable_scope(root):        # the next ordinary call evaluates g t + b
        if 'mobn' not in layer:
            y2 = call(nn, cx.from_numpy(x, ld=32 if shape[-1] <= 32 else 64), dict(init=False, nonlinearity=act)).numpy()
            assert G.rel_err(y2.reshape(ref[3].shape), ref[3]) < TOL


BASE_LAYERS = {  # name -> (input shape, V shape, kind, call)
    '_WN_dense': ((4, 1, 1, 37), (37, 33), 'dense', lambda m, a, kw: m._WN_dense(a, 33, 'L', init_scale=0.5, **kw)),
    '_WN_dense_narrow': ((4, 1, 1, 37), (37, 33), 'dense', lambda m, a, kw: m._WN_dense(a, 33, 'L', init_scale=0.5, narrow=True, **kw)),
    '_WN_conv2d': ((4, 8, 8, 5), (3, 3, 5, 33), 'conv', lambda m, a, kw: m._WN_conv2d(a, 33, k_h=3, k_w=3, d_h=2, d_w=2, init_scale=0.5, name='L', **kw)),
    '_WN_deconv2d': ((4, 8, 8, 5), (5, 5, 3, 5), 'deconv', lambda m, a, kw: m._WN_deconv2d(a, 3, k_h=5, k_w=5, init_scale=0.1, name='L', narrow=True, **kw)),
}


@pytest.mark.parametrize("layer", sorted(BASE_LAYERS))
def test_model_base_layers_assign_on_init(plain, layer):
    tr, cx = plain, plain.cx
    shape, vshape, kind, call = BASE_LAYERS[layer]
    rng = np.random.default_rng(len(layer) + 100)
    x = _x(rng, shape)
    root = 'wnb' + layer
    cout = 3 if kind == 'deconv' else 33
    scale = 0.1 if kind == 'deconv' else 0.5
    act = tr.model._tanh if kind == 'deconv' else tr.model._leaky_relu
    f = (lambda v: np.tanh(v)) if kind == 'deconv' else (lambda v: np.where(v > 0, v, 0.2 * v))
    with cx.phase_scope(root, record=False), cx.variable_scope(root):
        with cx.variable_scope('L'):
            cx.get_variable('V', vshape, lambda s: (0.05 * rng.standard_normal(s)).astype(np.float32))
            cx.get_variable('g', (cout,), 1.0)
            cx.get_variable('b', (cout,), 0.0)
        a = cx.from_numpy(x, ld=32 if shape[-1] <= 32 else 64)
        y1 = call(tr.model, a, dict(init=True, activation=act))                        # no scope needed: the assign is on the value path
        if 'narrow' in layer or kind == 'deconv':
            assert y1.ld == y1.c
        y1 = y1.numpy()
        y2 = call(tr.model, cx.from_numpy(x, ld=32 if shape[-1] <= 32 else 64), dict(init=False, activation=act)).numpy()
    st = cx.stores[root]
    ref = R.wn_layer(x.reshape((shape[0], shape[-1])) if kind == 'dense' else x, st.get(root + '/L/V').astype(np.float64), kind, 1e-10, scale,
                     2 if kind == 'conv' else 1)
    ref = (ref[0], ref[1], ref[2], f(ref[3]))
    _compare(st, root + '/L', y1.reshape(ref[3].shape), ref)
    assert G.rel_err(y2.reshape(ref[3].shape), ref[3]) < TOL


def test_refused_inside_a_recording(plain):
    from tg import lib as tglib
    from tg import ops
    cx = plain.cx
    with cx.phase_scope('wn_refuse', record=False):
        t = cx.from_numpy(np.ones((4, 8), np.float32))
        g, b = cx.scratch('g', 8), cx.scratch('b', 8)
        cx.capturing = True
        try:
            with pytest.raises(tglib.TgError, match="capture"):
                ops.wn_data_init(t, g, b, 1e-8, 1.0)
            with pytest.raises(tglib.TgError, match="capture"):
                with cx.assigning_init():
                    pass
        finally:
            cx.capturing = False
        t16 = cx.new_act(4, 1, 1, 8, 8, dtype='bf16')
        with pytest.raises(tglib.TgError, match="bf16"):
            ops.wn_data_init(t16, g, b, 1e-8, 1.0)
