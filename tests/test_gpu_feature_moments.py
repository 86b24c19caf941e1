"""tg_feature_moments_f32 (include/tg_kernels.h, csrc/moments.hip) against float64 NumPy: the fp64 column sums and Gram matrix of an fp32
feature matrix, accumulated into the caller's buffers.

Tolerance (tests/sample_metrics_reference.py, TOL_MOMENTS = 1e-12 of the per-output sum of |terms|): every fp32 x fp32 product is exact in
fp64, so an output's only error is that of its n - 1 fp64 additions, at most n 2^-53 of sum |terms|, and n <= 4096 here.  The negative
control rounds the same data to bf16 (a relative change of up to 2^-9 per value) and must fail the bound.  Shapes: a single element, a
matrix smaller than one 32 x 32 block, one that is no multiple of the block in rows or columns with several row ranges, whole blocks, and
the trainer's feature width with padding columns — which hold NaN everywhere: a single read of one would poison an output."""
import numpy as np
import pytest
import torch

import sample_metrics_reference as R
from kernel_check import guarded, lib, ptr, st

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 8), (257, 33, 40), (64, 128, 128), (1000, 128, 160)]
TG_ERR_INVALID = -1
_DATA = {}


def data(n, c, ld):
    """normal values with a non-zero mean in columns 0..c-1, NaN in the padding; made once per shape and left unchanged."""
    key = (n, c, ld)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * n + 10 * c + ld)
        f = np.full((n, ld), np.nan, np.float32)
        f[:, :c] = (rng.standard_normal((n, c)) * 1.5 + 0.75).astype(np.float32)
        f.setflags(write=False)
        _DATA[key] = (f, R.moments64(f, c))
    return _DATA[key]


def f64_out(n):
    """a guarded, zeroed output of n doubles (the suite's guard words behind it) and its float64 view."""
    g = guarded(2 * n, fill=np.zeros(2 * n, np.float32))
    return g, g.t.view(torch.float64)


def workspace(n, c, fill=None):
    need = lib().call('tg_feature_moments_workspace_bytes', n, c)
    assert need % 8 == 0
    g = guarded(max(need // 4, 2), fill=fill)
    return g, need


def run(f, c, n=None, into=None):
    """one call on the first n rows of the host matrix f -> (sum, gram) host float64, guards checked."""
    L = lib()
    n = f.shape[0] if n is None else n
    ld = f.shape[1]
    fd = torch.from_numpy(np.array(f, np.float32)).cuda()
    (gs, s), (gg, g) = into if into is not None else (f64_out(c), f64_out(c * c))
    gw, need = workspace(n, c)
    L.call('tg_feature_moments_f32', ptr(fd), ld, n, c, ptr(s), ptr(g), gw.ptr, need, st())
    for x in (gs, gg, gw):
        x.check_guard()
    return s.cpu().numpy().copy(), g.cpu().numpy().reshape(c, c).copy()


def within(got, ref, sabs):
    return bool((np.abs(got - ref) <= R.TOL_MOMENTS * sabs).all())


@pytest.mark.parametrize("n,c,ld", SHAPES)
def test_moments_match_float64(n, c, ld):
    f, (s_ref, g_ref, s_abs, g_abs) = data(n, c, ld)
    s, g = run(f, c)
    print("n %d c %d ld %d: worst sum error %.3g, worst gram error %.3g of the bound" % (
        n, c, ld, (np.abs(s - s_ref) / (R.TOL_MOMENTS * s_abs)).max(), (np.abs(g - g_ref) / (R.TOL_MOMENTS * g_abs)).max()))
    assert np.isfinite(s).all() and np.isfinite(g).all()          # no padding column (NaN) was read
    assert within(s, s_ref, s_abs) and within(g, g_ref, g_abs)
    assert (g == g.T).all()                                       # both triangles, exactly equal
    s2, g2 = run(f, c)                                            # bit-identical from run to run
    assert (s.view(np.int64) == s2.view(np.int64)).all() and (g.view(np.int64) == g2.view(np.int64)).all()


@pytest.mark.parametrize("n,c,ld", [(257, 33, 40), (1000, 128, 160)])
def test_bound_rejects_bf16_rounded_data(n, c, ld):
    f, (s_ref, g_ref, s_abs, g_abs) = data(n, c, ld)
    fb = np.array(f)
    fb[:, :c] = R.to_bf16(f[:, :c])
    s, g = run(fb, c)
    assert not within(s, s_ref, s_abs) and not within(g, g_ref, g_abs)


@pytest.mark.parametrize("n,c,ld", [(257, 33, 40), (1000, 128, 160)])
def test_two_calls_on_the_halves_accumulate_to_the_whole(n, c, ld):
    f, (s_ref, g_ref, s_abs, g_abs) = data(n, c, ld)
    into = (f64_out(c), f64_out(c * c))
    h = n // 2 + 1
    run(f[:h], c, into=into)
    s, g = run(f[h:], c, into=into)
    assert within(s, s_ref, s_abs) and within(g, g_ref, g_abs) and (g == g.T).all()


def test_other_stream_and_dirty_workspace_give_the_same_bits():
    """the workspace needs no initialisation and the result does not depend on the stream."""
    n, c, ld = 257, 33, 40
    f, _ = data(n, c, ld)
    s0, g0 = run(f, c)
    L = lib()
    fd = torch.from_numpy(np.array(f, np.float32)).cuda()
    (gs, s), (gg, g) = f64_out(c), f64_out(c * c)
    gw, need = workspace(n, c, fill=np.full(L.call('tg_feature_moments_workspace_bytes', n, c) // 4, 1e30, np.float32))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        L.call('tg_feature_moments_f32', ptr(fd), ld, n, c, ptr(s), ptr(g), gw.ptr, need, st())
    side.synchronize()
    for x in (gs, gg, gw):
        x.check_guard()
    assert (s.cpu().numpy().view(np.int64) == s0.view(np.int64)).all()
    assert (g.cpu().numpy().reshape(c, c).view(np.int64) == g0.view(np.int64)).all()


def test_no_rows_is_a_no_op():
    L = lib()
    c = 5
    seed = np.arange(2 * (c + c * c), dtype=np.float32) + 1
    gs, gg = guarded(2 * c, fill=seed[:2 * c]), guarded(2 * c * c, fill=seed[2 * c:])
    assert L.call('tg_feature_moments_workspace_bytes', 0, c) == 0
    L.call('tg_feature_moments_f32', None, 8, 0, c, gs.ptr, gg.ptr, None, 0, st())
    assert (gs.get() == seed[:2 * c]).all() and (gg.get() == seed[2 * c:]).all()
    gs.check_guard(), gg.check_guard()


def test_bad_arguments_are_refused():
    L = lib()
    h = L.load()
    f = torch.zeros(16 * 16, dtype=torch.float32, device='cuda')
    (gs, s), (gg, g) = f64_out(600), f64_out(16 * 16)
    gw, need = workspace(16, 8)
    call = lambda ld, n, c, ws, nbytes: h.tg_feature_moments_f32(ptr(f), ld, n, c, ptr(s), ptr(g), ws, nbytes, st())
    assert call(8, 16, 0, gw.ptr, need) == TG_ERR_INVALID and b"c must be in 1..512" in h.tg_last_error_string()
    assert call(600, 16, 513, gw.ptr, need) == TG_ERR_INVALID
    assert call(7, 16, 8, gw.ptr, need) == TG_ERR_INVALID and b"ld" in h.tg_last_error_string()
    assert call(8, -1, 8, gw.ptr, need) == TG_ERR_INVALID
    assert call(8, 16, 8, gw.ptr, need - 8) == TG_ERR_INVALID and b"workspace" in h.tg_last_error_string()
    assert call(8, 16, 8, None, need) == TG_ERR_INVALID
    for bad in ((-1, 8), (4, 0), (4, 513)):
        with pytest.raises(L.TgError):
            L.call('tg_feature_moments_workspace_bytes', *bad)
    assert call(8, 16, 8, gw.ptr, need) == 0                      # the same call with its arguments in range goes through
    torch.cuda.synchronize()
    for x in (gs, gg, gw):
        x.check_guard()
    assert float(g.abs().sum()) == 0.0
