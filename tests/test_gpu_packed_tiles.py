"""The K-packed MFMA kernels (csrc/packed_conv.hip: 3x3 conv of <= 16 input channels, forward and filter gradient; csrc/narrow.hip: input
and filter gradient of the 5x5 / stride-2 transposed conv with <= 4 output channels) instantiation by instantiation against float64
(oracle/tf_ops.py evaluated on the same fp32 inputs).  tests/test_packed_tile_coverage.py (no GPU) proves that the case tables below reach
every instantiation the launchers dispatch and hold the edges listed there.

Tolerance: the reduction class of tests/kernel_check.py, `close` (TOL = 1e-6 of the per-output sum of |terms|, from the same oracle call on
absolute values; |bias| included for the forward).  Every case carries two negative controls through `rejected` (factor 10): the reference
with bf16-rounded operands (the kernels promise exact fp32 products) and a structurally wrong one (forward / input gradient: one filter tap
dropped; filter gradients: the last image left out of the sum, or the last image row where n = 1).  Both wrong references are first told
from the float64 reference itself by the same bound, so the controls do not rest on the kernel's output.

Every output goes through `guarded` / `finish`: NaN-filled, guard words behind it, every owned element written; padding the header says is
zeroed is exactly 0.0, labels are copied bit for bit, and what the header does not give the kernel (dx columns beyond ci_p) keeps its NaN.
Input padding the kernels have no business reading (x channels beyond c_in / ci_p, dy channels beyond c_out) is NaN as well.  The filter
gradients run in a workspace of exactly the size the library asks for, guarded, twice: over finite garbage and over NaN, bit-identical."""
import numpy as np
import pytest
import torch

from oracle import tf_ops as T
from kernel_check import assert_bits, close, dev, finish, guarded, lib, ptr, rejected, st

pytestmark = pytest.mark.gpu


def pad32(c):
    return (c + 31) // 32 * 32


def _p(id, n, h, w, c_in, c_out, act, alpha, bias, lab_n, ld_y, ld_x, ld_dy):
    return dict(id=id, n=n, h=h, w=w, c_in=c_in, c_out=c_out, act=act, alpha=alpha, bias=bias, lab_n=lab_n, ld_y=ld_y, ld_x=ld_x, ld_dy=ld_dy)


# lab_n None: labels == NULL (channels behind the convolution's are zeros); act: none / relu / lrelu with slope alpha
PACKED_CASES = [
    _p('c1-32-h4-w16-n1-bare', 1, 4, 16, 1, 32, 'none', 0.0, False, None, 32, 1, 32),
    _p('c2-64-h8-w32-relu-lab1', 3, 8, 32, 2, 64, 'relu', 0.0, True, 1, 65, 32, 68),
    _p('c5-32-h12-w16-lrelu-lab10', 4, 12, 16, 5, 32, 'lrelu', 0.3, True, 10, 42, 5, 36),
    _p('c13-32-h20-w32-lrelu-lab10-wide', 3, 20, 32, 13, 32, 'lrelu', 0.05, True, 10, 128, 64, 32),
    _p('c16-64-h8-w16-n1-nobias-lab10', 1, 8, 16, 16, 64, 'none', 0.0, False, 10, 74, 16, 64),
    _p('c16-64-h20-w32-lrelu-lab1-wide', 5, 20, 32, 16, 64, 'lrelu', 0.1, True, 1, 160, 32, 68),
    _p('c3-64-h12-w32-relu', 3, 12, 32, 3, 64, 'relu', 0.0, True, None, 64, 3, 64),
    _p('c13-64-h4-w32-nolab-wide', 2, 4, 32, 13, 64, 'none', 0.0, True, None, 96, 13, 64),
    _p('c7-32-h8-w16-relu-lab1', 3, 8, 16, 7, 32, 'relu', 0.0, True, 1, 33, 7, 32),
]


def _n(id, n, h, w, c_out, c_in, ci_p, scale, ld_dy, ld_dx, ld_x):
    return dict(id=id, n=n, h=h, w=w, c_out=c_out, c_in=c_in, ci_p=ci_p, scale=scale, ld_dy=ld_dy, ld_dx=ld_dx, ld_x=ld_x)


NARROW_CASES = [
    _n('co1-ci32-h4-w16-n1', 1, 4, 16, 1, 32, 32, False, 1, 32, 32),
    _n('co1-ci256-h8-w32-big', 3, 8, 32, 1, 200, 256, True, 32, 288, 288),
    _n('co2-ci256-h12-w32-big-full', 3, 12, 32, 2, 256, 256, False, 2, 256, 256),
    _n('co2-ci64-h20-w16', 4, 20, 16, 2, 40, 64, True, 64, 96, 64),
    _n('co3-ci160-h8-w32-big', 3, 8, 32, 3, 138, 160, True, 3, 160, 192),
    _n('co3-ci160-h20-w16-n1', 1, 20, 16, 3, 160, 160, False, 32, 192, 160),
    _n('co4-ci128-h12-w32-most', 3, 12, 32, 4, 100, 128, True, 4, 128, 160),
    _n('co4-ci128-h4-w16', 2, 4, 16, 4, 128, 128, False, 32, 160, 128),
    _n('co3-ci32-h8-w16', 2, 8, 16, 3, 7, 32, True, 64, 32, 64),
    _n('co1-ci160-h4-w32-big', 3, 4, 32, 1, 150, 160, False, 1, 160, 160),
]


def packed_reach(c):
    """the instantiations a packed case launches (csrc/packed_conv.hip: NT = c_out / 32, wgrad_rows = 8 when 8 | h, else 4)."""
    nt = c['c_out'] // 32
    return [('packed_fwd', nt), ('packed_wgrad', nt, 8 if c['h'] % 8 == 0 else 4)]


def narrow_big(c):
    return c['w'] * (c['ci_p'] // 4) > 1024


def narrow_reach(c):
    """csrc/narrow.hip: the template argument is c_out; XU = 8 when an x row is more than 1024 16-byte units."""
    return [('narrow_dgrad', c['c_out']), ('narrow_wgrad', c['c_out'], 8 if narrow_big(c) else 4)]


f8 = lambda a: np.asarray(a, np.float64)
NAN = np.float32('nan')


def strided(a, ld, fill=NAN):
    """[..., c] -> [..., ld] fp32, the channels behind the data filled with `fill` (NaN: must never be read)."""
    out = np.full(a.shape[:-1] + (ld,), fill, np.float32)
    out[..., :a.shape[-1]] = a
    return out


def act_fn(act, alpha):
    if act == 'none':
        return lambda v: v
    slope = 0.0 if act == 'relu' else np.float64(np.float32(alpha))
    return lambda v: np.where(v > 0, v, slope * v)


def packed_inputs(c, seed=41):
    rng = np.random.default_rng(seed)
    n, h, w, cin, cout = c['n'], c['h'], c['w'], c['c_in'], c['c_out']
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wt = (rng.standard_normal((3, 3, cin, cout)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32) if c['bias'] else None
    lab = rng.random((n, c['lab_n'])).astype(np.float32) if c['lab_n'] else None
    dy = rng.standard_normal((n, h, w, cout)).astype(np.float32)
    return x, wt, bias, lab, dy


def packed_fwd_refs(c, x, wt, bias):
    """(ref, sum|terms|, bf16 control, one-tap-dropped control) of the forward, float64."""
    fn = act_fn(c['act'], c['alpha'])
    b = f8(bias) if bias is not None else 0.0
    conv = lambda a, k: T.conv2d(f8(a), f8(k), (1, 1), 'SAME')
    cut = wt.copy()
    cut[2, 2] = 0
    return (fn(conv(x, wt) + b), conv(np.abs(x), np.abs(wt)) + np.abs(b), fn(conv(T.bf16_round(x), T.bf16_round(wt)) + b), fn(conv(x, cut) + b))


def drop_last(a):
    """the last image left out of a sum over the batch (n = 1: its last row)."""
    a = a.copy()
    if a.shape[0] > 1:
        a[-1] = 0
    else:
        a[0, -1] = 0
    return a


def packed_wgrad_refs(c, x, dy):
    shape = (3, 3, c['c_in'], c['c_out'])
    g = lambda a, d: T.conv2d_bwd_filter(f8(a), f8(d), shape, (1, 1), 'SAME')
    return g(x, dy), g(np.abs(x), np.abs(dy)), g(T.bf16_round(x), T.bf16_round(dy)), g(x, drop_last(dy))


def narrow_inputs(c, seed=11):
    rng = np.random.default_rng(seed)
    n, h, w, cout, cin = c['n'], c['h'], c['w'], c['c_out'], c['c_in']
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wt = (rng.standard_normal((5, 5, cout, cin)) * 0.3).astype(np.float32)
    dy = rng.standard_normal((n, 2 * h, 2 * w, cout)).astype(np.float32)
    scale = (1 + 0.3 * rng.standard_normal(cout)).astype(np.float32) if c['scale'] else None
    return x, wt, dy, scale


def narrow_dgrad_refs(c, wt, dy, scale):
    # the kernel multiplies filter and scale in fp32 when it stages the filter: one rounding of an operand, within the reduction bound
    w_eff = f8(wt) if scale is None else f8(wt) * f8(scale)[None, None, :, None]
    g = lambda k, d: T.conv2d_transpose_bwd_input(f8(k), f8(d))
    cut = w_eff.copy()
    cut[4, 4] = 0
    return g(w_eff, dy), g(np.abs(w_eff), np.abs(dy)), g(T.bf16_round(w_eff.astype(np.float32)), T.bf16_round(dy)), g(cut, dy)


def narrow_wgrad_refs(c, x, dy):
    shape = (5, 5, c['c_out'], c['c_in'])
    g = lambda a, d: T.conv2d_transpose_bwd_filter(f8(a), f8(d), shape)
    return g(x, dy), g(np.abs(x), np.abs(dy)), g(T.bf16_round(x), T.bf16_round(dy)), g(drop_last(x), dy)


def check(got, refs, what):
    ref, sabs, bf, cut = refs
    assert rejected(ref, bf, sabs) and rejected(ref, cut, sabs), "%s: the inputs do not tell the controls from the float64 reference" % what
    close(got, ref, sabs, what)
    assert rejected(got, bf, sabs), "%s: the bound accepts bf16-rounded operands" % what
    assert rejected(got, cut, sabs), "%s: the bound accepts a reference with a tap / an image left out" % what


def _wgrad_twice(L, name, ws_bytes, n_out, launch):
    """run the filter gradient over a workspace of finite garbage, then over NaN: both within their guards, bit-identical."""
    outs = []
    for fill in (7.0, None):
        ws = guarded(ws_bytes // 4, fill=None if fill is None else np.full(ws_bytes // 4, fill, np.float32))
        dw = guarded(n_out)
        launch(ws, dw)
        outs.append(finish(dw))
        part = finish(ws)                                # every partial slab written, nothing behind the last
        assert np.isfinite(part).all()
    assert_bits(outs[0], outs[1], name + ": workspace content changes the result")
    return outs[1]


@pytest.mark.parametrize("c", PACKED_CASES, ids=[c['id'] for c in PACKED_CASES])
def test_packed_conv(c):
    L = lib()
    n, h, w, cin, cout, ld_y, ld_x, ld_dy = (c[k] for k in ('n', 'h', 'w', 'c_in', 'c_out', 'ld_y', 'ld_x', 'ld_dy'))
    assert L.call('tg_conv3x3_packed_supported', n, h, w, cin, cout) == 1
    x, wt, bias, lab, dy = packed_inputs(c)
    nlab = c['lab_n'] or 0
    xd, wd = dev(strided(x, ld_x)), dev(wt)
    y = guarded(n * h * w * ld_y)
    L.call('tg_conv3x3_packed_fwd_f32', ptr(xd), ld_x, cin, ptr(wd), ptr(dev(bias)) if bias is not None else None, L.ACT[c['act']], c['alpha'],
           ptr(dev(lab)) if lab is not None else None, nlab, y.ptr, ld_y, n, h, w, cout, st())
    got = finish(y, (n, h, w, ld_y))
    check(got[..., :cout], packed_fwd_refs(c, x, wt, bias), c['id'] + " fwd")
    if nlab:
        assert_bits(got[..., cout:cout + nlab], np.broadcast_to(lab[:, None, None, :], (n, h, w, nlab)), "labels")
    assert (got[..., cout + nlab:] == 0).all() and not np.signbit(got[..., cout + nlab:]).any(), "channels behind the labels are not +0.0"

    need = L.call('tg_conv3x3_packed_wgrad_workspace_bytes', n, h, w, cin, cout)
    assert need == n * (h // (8 if h % 8 == 0 else 4)) * 9 * cin * cout * 4
    dyd = dev(strided(dy, ld_dy))
    dw = _wgrad_twice(L, c['id'], need, 9 * cin * cout, lambda ws, o: L.call(
        'tg_conv3x3_packed_wgrad_f32', ptr(xd), ld_x, cin, ptr(dyd), ld_dy, n, h, w, cout, ws.ptr, o.ptr, st()))
    check(dw.reshape(3, 3, cin, cout), packed_wgrad_refs(c, x, dy), c['id'] + " wgrad")


@pytest.mark.parametrize("c", NARROW_CASES, ids=[c['id'] for c in NARROW_CASES])
def test_narrow_deconv_backward(c):
    L = lib()
    n, h, w, cout, cin, ci_p, ld_dy, ld_dx, ld_x = (c[k] for k in ('n', 'h', 'w', 'c_out', 'c_in', 'ci_p', 'ld_dy', 'ld_dx', 'ld_x'))
    assert L.call('tg_deconv5x5s2_narrow_supported', n, h, w, cout, ci_p) == 1
    x, wt, dy, scale = narrow_inputs(c)
    dyd, wd = dev(strided(dy, ld_dy)), dev(wt)
    dx = guarded(n * h * w * ld_dx)
    L.call('tg_deconv5x5s2_narrow_dgrad_f32', ptr(dyd), ld_dy, ptr(wd), ptr(dev(scale)) if scale is not None else None, n, h, w, cout, cin, ci_p,
           dx.ptr, ld_dx, st())
    owned = np.zeros((n, h, w, ld_dx), bool)
    owned[..., :ci_p] = True
    got = finish(dx, (n, h, w, ld_dx), owned)
    check(got[..., :cin], narrow_dgrad_refs(c, wt, dy, scale), c['id'] + " dgrad")
    assert (got[..., cin:ci_p] == 0).all(), "dx channels c_in .. ci_p are not zero"
    assert np.isnan(got[..., ci_p:]).all(), "dx columns beyond ci_p were written"

    need = L.call('tg_deconv5x5s2_narrow_wgrad_workspace_bytes', n, h, w, cout, ci_p)
    assert need == n * (h // 4) * 25 * cout * ci_p * 4
    xp = strided(strided(x, ci_p, 0.0), ld_x)            # zeros up to ci_p (the buffer's own padding), NaN behind
    xd = dev(xp)
    dw = _wgrad_twice(L, c['id'], need, 25 * cout * cin, lambda ws, o: L.call(
        'tg_deconv5x5s2_narrow_wgrad_f32', ptr(dyd), ld_dy, ptr(xd), ld_x, n, h, w, cout, cin, ci_p, ws.ptr, o.ptr, st()))
    check(dw.reshape(5, 5, cout, cin), narrow_wgrad_refs(c, x, dy), c['id'] + " wgrad")


# ---- the envelope: per term of the two shape_ok functions one shape just inside and one just outside -------------------------------------
# (n, h, w, c_in, c_out) of tg_conv3x3_packed_*; the LDS terms cannot be reached (tests/test_packed_tile_coverage.py shows the arithmetic)
PACKED_ENVELOPE = [
    ('n > 0', (1, 4, 16, 3, 32), (0, 4, 16, 3, 32)),
    ('h > 0', (1, 4, 16, 3, 32), (1, 0, 16, 3, 32)),
    ('w > 0', (1, 4, 16, 3, 32), (1, 4, 0, 3, 32)),
    ('c_in >= 1', (2, 4, 16, 1, 32), (2, 4, 16, 0, 32)),
    ('c_in <= MAX_CIN', (2, 4, 16, 16, 64), (2, 4, 16, 17, 64)),
    ('c_out == 32 || c_out == 64', (2, 4, 16, 3, 64), (2, 4, 16, 3, 96)),
    ('c_out == 32 || c_out == 64', (2, 4, 16, 3, 32), (2, 4, 16, 3, 16)),
    ('w % 16 == 0', (2, 4, 32, 3, 32), (2, 4, 24, 3, 32)),
    ('w <= 32', (2, 4, 32, 3, 32), (2, 4, 48, 3, 32)),
    ('h % 4 == 0', (2, 8, 16, 3, 32), (2, 6, 16, 3, 32)),
]
# (n, h, w, c_out, ci_p) of tg_deconv5x5s2_narrow_*; the filter gradient's LDS term cannot be reached
NARROW_ENVELOPE = [
    ('n > 0', (1, 4, 16, 3, 32), (0, 4, 16, 3, 32)),
    ('h > 0', (1, 4, 16, 3, 32), (1, 0, 16, 3, 32)),
    ('w > 0', (1, 4, 16, 3, 32), (1, 4, 0, 3, 32)),
    ('c_out >= 1', (2, 4, 16, 1, 32), (2, 4, 16, 0, 32)),
    ('c_out <= 4', (2, 4, 16, 4, 32), (2, 4, 16, 5, 32)),
    ('ci_p >= 32', (2, 4, 16, 3, 32), (2, 4, 16, 3, 0)),
    ('ci_p <= 32 * MAXQ', (2, 4, 16, 1, 256), (2, 4, 16, 1, 288)),
    ('ci_p % 32 == 0', (2, 4, 16, 3, 64), (2, 4, 16, 3, 48)),
    ('w % 16 == 0', (2, 4, 32, 3, 32), (2, 4, 24, 3, 32)),
    ('w <= 32', (2, 4, 32, 3, 32), (2, 4, 48, 3, 32)),
    ('h % RB == 0', (2, 8, 16, 3, 32), (2, 6, 16, 3, 32)),
    ('dgrad_lds_bytes', (2, 4, 16, 4, 128), (2, 4, 16, 4, 160)),
    ('dgrad_lds_bytes', (2, 4, 16, 3, 160), (2, 4, 16, 3, 192)),
    ('dgrad_lds_bytes', (2, 4, 16, 2, 256), (2, 4, 16, 4, 256)),
]


def _packed_case_of(shape):
    n, h, w, cin, cout = shape
    return _p('envelope', n, h, w, cin, cout, 'lrelu', 0.3, True, None, cout, cin, cout)


def _narrow_case_of(shape):
    n, h, w, cout, ci_p = shape
    return _n('envelope', n, h, w, cout, ci_p, ci_p, False, cout, ci_p, ci_p)


@pytest.mark.parametrize("term,inside,outside", PACKED_ENVELOPE, ids=["%s-%d" % (e[0], i) for i, e in enumerate(PACKED_ENVELOPE)])
def test_packed_envelope(term, inside, outside):
    L = lib()
    assert L.call('tg_conv3x3_packed_supported', *inside) == 1 and L.call('tg_conv3x3_packed_supported', *outside) == 0
    test_packed_conv(_packed_case_of(inside))
    with pytest.raises(L.TgError, match='tg_conv3x3_packed_wgrad_workspace_bytes'):
        L.call('tg_conv3x3_packed_wgrad_workspace_bytes', *outside)
    n, h, w, cin, cout = outside
    buf = guarded(4096)                                   # never touched: both launches are refused before any kernel starts
    with pytest.raises(L.TgError, match='tg_conv3x3_packed_fwd_f32'):
        L.call('tg_conv3x3_packed_fwd_f32', buf.ptr, max(cin, 1), cin, buf.ptr, None, L.ACT['none'], 0.0, None, 0, buf.ptr, max(cout, 1), n, h, w, cout, st())
    with pytest.raises(L.TgError, match='tg_conv3x3_packed_wgrad_f32'):
        L.call('tg_conv3x3_packed_wgrad_f32', buf.ptr, max(cin, 1), cin, buf.ptr, pad32(max(cout, 1)), n, h, w, cout, buf.ptr, buf.ptr, st())
    buf.check_guard()
    assert np.isnan(buf.get()).all()


@pytest.mark.parametrize("term,inside,outside", NARROW_ENVELOPE, ids=["%s-%d" % (e[0], i) for i, e in enumerate(NARROW_ENVELOPE)])
def test_narrow_envelope(term, inside, outside):
    L = lib()
    assert L.call('tg_deconv5x5s2_narrow_supported', *inside) == 1 and L.call('tg_deconv5x5s2_narrow_supported', *outside) == 0
    test_narrow_deconv_backward(_narrow_case_of(inside))
    with pytest.raises(L.TgError, match='tg_deconv5x5s2_narrow_wgrad_workspace_bytes'):
        L.call('tg_deconv5x5s2_narrow_wgrad_workspace_bytes', *outside)
    n, h, w, cout, ci_p = outside
    buf = guarded(4096)
    with pytest.raises(L.TgError, match='tg_deconv5x5s2_narrow_dgrad_f32'):
        L.call('tg_deconv5x5s2_narrow_dgrad_f32', buf.ptr, max(cout, 1), buf.ptr, None, n, h, w, cout, max(ci_p, 1), ci_p, buf.ptr, max(ci_p, 1), st())
    with pytest.raises(L.TgError, match='tg_deconv5x5s2_narrow_wgrad_f32'):
        L.call('tg_deconv5x5s2_narrow_wgrad_f32', buf.ptr, max(cout, 1), buf.ptr, max(ci_p, 1), n, h, w, cout, max(ci_p, 1), ci_p, buf.ptr, buf.ptr, st())
    buf.check_guard()
    assert np.isnan(buf.get()).all()


def test_leading_dimensions_the_header_refuses():
    """ld_x < c_in, ld_y < c_out (+ labels), ld_dy < c_out or not a multiple of 4, ld_dx / ld_x < ci_p: refused by name, nothing written."""
    L = lib()
    buf = guarded(4096)
    bad_fwd = [dict(ld_x=2), dict(ld_y=31), dict(ld_y=40, lab=True)]
    for b in bad_fwd:
        with pytest.raises(L.TgError, match='tg_conv3x3_packed_fwd_f32'):
            L.call('tg_conv3x3_packed_fwd_f32', buf.ptr, b.get('ld_x', 3), 3, buf.ptr, None, L.ACT['none'], 0.0, buf.ptr if b.get('lab') else None,
                   10 if b.get('lab') else 0, buf.ptr, b.get('ld_y', 32), 1, 4, 16, 32, st())
    for ld_x, ld_dy in ((2, 32), (3, 28), (3, 34)):
        with pytest.raises(L.TgError, match='tg_conv3x3_packed_wgrad_f32'):
            L.call('tg_conv3x3_packed_wgrad_f32', buf.ptr, ld_x, 3, buf.ptr, ld_dy, 1, 4, 16, 32, buf.ptr, buf.ptr, st())
    for ld_dy, c_in, ld_dx in ((2, 32, 32), (3, 33, 32), (3, 0, 32), (3, 32, 31)):
        with pytest.raises(L.TgError, match='tg_deconv5x5s2_narrow_dgrad_f32'):
            L.call('tg_deconv5x5s2_narrow_dgrad_f32', buf.ptr, ld_dy, buf.ptr, None, 1, 4, 16, 3, c_in, 32, buf.ptr, ld_dx, st())
    for ld_dy, ld_x in ((2, 32), (3, 31), (3, 34)):          # 34: not whole 16-byte units
        with pytest.raises(L.TgError, match='tg_deconv5x5s2_narrow_wgrad_f32'):
            L.call('tg_deconv5x5s2_narrow_wgrad_f32', buf.ptr, ld_dy, buf.ptr, ld_x, 1, 4, 16, 3, 32, 32, buf.ptr, buf.ptr, st())
    buf.check_guard()
    assert np.isnan(buf.get()).all()
