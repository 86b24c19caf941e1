"""Every tile instantiation and work-unit schedule of the generic MFMA kernels of csrc/igemm.hip against float64.

igemm_f32_kernel<BM, BN, ..., COLSUM, BF16, FIXUP> and wgrad_f32_kernel<CT, NT, ..., BF16> are reached through a handful of entry points; the
cost model of csrc/geom.cpp (tg::igemm_pick_tile, tg::igemm_schedule, tg::wgrad_tile) decides which instantiation and schedule a launch runs.
The tables below name, for every case, the tile and the schedule (uncut: one workgroup per tile; cut: tiles split along K, partial sums
through scratch and the FIXUP launch) it is meant to reach; each test asks the library (tg_igemm_tile, tg_igemm_workspace_bytes,
tg_wgrad_tile) before it launches, so a change of the cost model fails here instead of silently moving coverage.  The tables are plain
data: tests/test_gemm_tile_coverage.py imports them on a machine without a GPU and checks that every dispatched tile x operand type x
schedule x epilogue family is covered (or listed there as unreachable).

All launches run under tg_conv3x3_policy(2): the halo-tiled 3x3 kernels (csrc/conv3x3_bf16.hip, csrc/wgrad3x3.hip) take no shape here, and
tg_conv3x3_launches must not move.

Checks (tests/kernel_check.py, tests/test_gpu_igemm.py):
  * outputs, column sums and slabs come from kernel_check.guarded: NaN-filled with a guard behind; every owned element is written, the
    guard is intact, output channels in [n_store, ld_out) keep their NaN, and padding columns (zero filter rows and bias) are exactly 0;
  * reduction bound: |got - ref64| <= 1e-6 * sum|a||b| per output, ref64 = the descriptor's operation evaluated in float64 on the same
    operands (rounded with T.bf16_round for the bf16 entry points, whose products are then exact in fp32).  The activation is
    1-Lipschitz, so the bound of the accumulator carries over; tanhf adds its own few ulp (0.5 in units of the bound);
  * cut schedules: the launch with scratch, twice, is bit-identical, and the launch without scratch (one workgroup per tile) meets the
    same float64 bound;
  * column sums (and sums of squares; bnbwdstat: the sums of dy and of dy * x) against float64 sums of the STORED outputs, at the same bound
    of the sum of |terms|;
  * negative controls: the bound rejects the reference without its last K-tile (32 channels of one tap), and, for the filter gradient,
    without its last 32-pixel tile.

The float64 oracle runs on the device (torch float64 matrix products): the production-sized cut cases are tens of GFLOP each."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import kernel_check as kc
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

F32, BF16 = 'f32', 'bf16'
FAMILIES = ('plain', 'colsum', 'actsum', 'bnstat', 'bnbwdstat')


def _c(id, family, prec, op, args, tile, cut, segs=None, act=None, ld_out=None, n_store=None, live=None):
    """one igemm case: `op` ('conv' / 'dense' / 'deconv') with the positional `args` of the tg.geom builder of that name, the epilogue
    family, the tile (BM, BN) and schedule (cut along K or not) the cost model must pick, the application segments of the column-sum
    families, the activation, ld_out / n_store of the output, and `live`: output channels with nonzero filter rows (the rest up to the
    descriptor's c_out are channel padding that must come out exactly 0)."""
    return dict(id=id, family=family, prec=prec, op=op, args=tuple(args), tile=tuple(tile), cut=cut, segs=segs, act=act, ld_out=ld_out,
                n_store=n_store, live=live)


SVHN = (200, 8, 8, 512, 256, 3, 1, 'SAME')          # the SVHN classifier's 8x8 layer, 512 -> 256: bf16 128 x 128 tiles cut in two along K

IGEMM_CASES = [
    # ---- plain: bias + activation (tg_igemm_*, tg_igemm_multi_*) ----
    _c('plain-64x64-f32', 'plain', F32, 'conv', (7, 9, 7, 32, 96, 3, 2, 'SAME'), (64, 64), False, act='lrelu', live=80),
    _c('plain-64x64-bf16', 'plain', BF16, 'conv', (7, 9, 7, 32, 96, 3, 2, 'SAME'), (64, 64), False, act='relu', ld_out=104, n_store=90),
    _c('plain-64x64-f32-cut', 'plain', F32, 'dense', (100, 2048, 160), (64, 64), True, act='tanh', live=150),
    _c('plain-64x64-bf16-cut', 'plain', BF16, 'dense', (100, 2048, 160), (64, 64), True, act='lrelu', ld_out=168, n_store=156),
    _c('plain-64x64-f32-multi-cut', 'plain', F32, 'deconv', (6, 2, 3, 96, 64), (64, 64), True, act='relu'),
    _c('plain-64x64-bf16-multi-cut', 'plain', BF16, 'deconv', (20, 4, 4, 544, 256), (64, 64), True, act='relu', live=250),
    _c('plain-128x32-f32', 'plain', F32, 'dense', (300, 64, 32), (128, 32), False, act='lrelu', live=27),
    _c('plain-128x32-bf16', 'plain', BF16, 'dense', (300, 64, 32), (128, 32), False, act='tanh', ld_out=36, n_store=29),
    _c('plain-128x32-f32-cut', 'plain', F32, 'conv', (1, 4, 4, 96, 32, 3, 1, 'SAME'), (128, 32), True, act='lrelu'),
    _c('plain-128x32-bf16-cut', 'plain', BF16, 'conv', (3, 7, 7, 96, 32, 3, 1, 'SAME'), (128, 32), True, act='relu', live=30),
    _c('plain-128x32-f32-multi-cut', 'plain', F32, 'deconv', (1, 2, 2, 96, 32), (128, 32), True, act='tanh'),
    _c('plain-32x128-f32', 'plain', F32, 'dense', (20, 64, 32896), (32, 128), False, act='lrelu', live=32880),
    _c('plain-32x128-bf16', 'plain', BF16, 'dense', (20, 64, 32896), (32, 128), False, act='relu', ld_out=32900, n_store=32890),
    _c('plain-32x128-f32-cut', 'plain', F32, 'dense', (27, 3200, 16448), (32, 128), True, act='tanh'),
    _c('plain-32x128-bf16-cut', 'plain', BF16, 'dense', (27, 3200, 16448), (32, 128), True, act='lrelu', live=16400),
    _c('plain-64x128-bf16', 'plain', BF16, 'dense', (5000, 64, 256), (64, 128), False, act='lrelu', ld_out=264, n_store=250),
    _c('plain-64x128-bf16-cut', 'plain', BF16, 'dense', (5000, 3200, 256), (64, 128), True, act='tanh', live=240),
    _c('plain-128x128-bf16', 'plain', BF16, 'dense', (12750, 64, 256), (128, 128), False, act='relu', live=250),
    _c('plain-128x128-bf16-cut', 'plain', BF16, 'conv', SVHN, (128, 128), True, act='lrelu'),
    _c('plain-128x128-bf16-multi', 'plain', BF16, 'deconv', (250, 16, 16, 32, 256), (128, 128), False, act='relu', live=250),
]


# the column-sum families (tg_igemm_colsum_*, tg_igemm_actsum_*, tg_igemm_bnstat_*, tg_igemm_bnbwdstat_*) share one tile rule: every application segment has at least
# BM rows, so a tile straddles at most one boundary.  Per tile, operand type and schedule one shape, with a segment boundary inside a tile
# and a segment of exactly BM rows: (tile, prec, cut, op, args, segs, live)
_SEG_SHAPES = [
    ((64, 64), F32, False, 'conv', (4, 7, 7, 64, 96, 3, 1, 'SAME'), [64, 66, 66], 90),
    ((64, 64), BF16, False, 'conv', (4, 7, 7, 64, 96, 3, 1, 'SAME'), [64, 66, 66], None),
    ((64, 64), F32, True, 'conv', (8, 5, 5, 256, 160, 3, 1, 'SAME'), [64, 70, 66], None),
    ((64, 64), BF16, True, 'conv', (8, 5, 5, 256, 160, 3, 1, 'SAME'), [64, 70, 66], 150),
    ((128, 32), F32, False, 'conv', (6, 9, 9, 64, 32, 3, 1, 'SAME'), [128, 200, 158], None),
    ((128, 32), BF16, False, 'conv', (6, 9, 9, 64, 32, 3, 1, 'SAME'), [128, 200, 158], 28),
    ((128, 32), F32, True, 'conv', (6, 9, 9, 96, 32, 3, 1, 'SAME'), [128, 200, 158], 30),
    ((128, 32), BF16, True, 'conv', (6, 9, 9, 96, 32, 3, 1, 'SAME'), [128, 200, 158], None),
    ((32, 128), F32, False, 'conv', (4, 5, 5, 32, 160, 3, 1, 'SAME'), [32, 36, 32], 150),
    ((32, 128), BF16, False, 'conv', (4, 5, 5, 32, 160, 3, 1, 'SAME'), [32, 36, 32], None),
    ((32, 128), F32, True, 'conv', (4, 5, 5, 128, 160, 3, 1, 'SAME'), [32, 36, 32], None),
    ((32, 128), BF16, True, 'conv', (4, 5, 5, 128, 160, 3, 1, 'SAME'), [32, 36, 32], 140),
    ((64, 128), BF16, False, 'dense', (6400, 64, 160), [64, 100, 6236], None),
    ((64, 128), BF16, True, 'conv', (100, 8, 8, 544, 160, 3, 1, 'SAME'), [64, 100, 6236], 150),
    ((128, 128), BF16, False, 'dense', (12750, 64, 256), [128, 6000, 6622], 250),
    ((128, 128), BF16, True, 'conv', SVHN, [128, 6336, 6336], None),
]
_FAMILY_ACTS = {'colsum': [None], 'actsum': ['lrelu', 'relu'], 'bnstat': ['lrelu', 'relu', None], 'bnbwdstat': [None]}      # bnstat: the layer's own; actsum: act' of yact
# (bnbwdstat: the stored value is the raw accumulator dy, no bias, no activation; its second sum is of dy * x, x from kc.y_for)
IGEMM_CASES += [_c('%s-%dx%d-%s%s' % (fam, t[0], t[1], prec, '-cut' if cut else ''), fam, prec, op, args, t, cut, segs=segs,
                   act=_FAMILY_ACTS[fam][i % len(_FAMILY_ACTS[fam])], live=live)
                for fam in ('colsum', 'actsum', 'bnstat', 'bnbwdstat') for i, (t, prec, cut, op, args, segs, live) in enumerate(_SEG_SHAPES)]

# filter gradient (tg_wgrad_*): tile (CT, NT) = (tg::wgrad_tile(ld_in), tg::wgrad_tile(c_out)), every instantiation, 160 and 288 channels on
# 64-wide tiles whose last one overhangs.  (id, (CT, NT), (n, h, w, ld_in, c_out, k, stride, pad), ld_dy)
WGRAD_CASES = [
    ('128x128-3x3', (128, 128), (2, 9, 9, 128, 256, 3, 1, 'SAME'), None),
    ('128x64-s2', (128, 64), (3, 11, 9, 128, 160, 3, 2, 'SAME'), None),
    ('128x32-1x1', (128, 32), (5, 7, 6, 256, 96, 1, 1, 'SAME'), 128),
    ('64x128-valid', (64, 128), (2, 10, 9, 288, 128, 3, 1, 'VALID'), None),
    ('64x64-3x3', (64, 64), (3, 8, 8, 64, 288, 3, 1, 'SAME'), 320),
    ('64x32-s2', (64, 32), (4, 9, 9, 160, 32, 3, 2, 'SAME'), None),
    ('32x128-1x1', (32, 128), (4, 6, 5, 96, 128, 1, 1, 'SAME'), None),
    ('32x64-valid', (32, 64), (3, 9, 8, 32, 160, 3, 1, 'VALID'), 192),
    ('32x32-5x5s2', (32, 32), (2, 10, 10, 96, 96, 5, 2, 'SAME'), None),
]


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------
def _tg():
    from tg import lib, geom
    lib.load()
    return lib, geom


def descs_of(case):
    """the descriptors of an igemm case (list; several for a transposed conv's output parities)."""
    from tg import geom
    kw = dict(ld_out=case['ld_out'], n_store=case['n_store'])
    act = case['act'] if case['family'] in ('plain', 'bnstat') else None
    if case['op'] == 'conv':
        return [geom.conv_fwd(*case['args'], act=act, **kw)]
    if case['op'] == 'dense':
        return [geom.dense_fwd(*case['args'], act=act, **kw)]
    return list(geom.deconv_fwd(*case['args'], act=act, **kw))


def query_tile(descs, segs, bf16):
    """-> (BM, BN, cut): tg_igemm_tile and whether tg_igemm_workspace_bytes asks for scratch (the schedule cuts tiles along K)."""
    from tg import lib
    arr = lib.desc_array(descs)
    bm, bn = C.c_int32(), C.c_int32()
    sa = (C.c_int32 * len(segs))(*segs) if segs else None
    ns = len(segs) if segs else 0
    lib.call('tg_igemm_tile', C.cast(arr, C.c_void_p), len(descs), sa, ns, int(bf16), C.byref(bm), C.byref(bn))
    ws = lib.call('tg_igemm_workspace_bytes', C.cast(arr, C.c_void_p), len(descs), sa, ns, int(bf16))
    return bm.value, bn.value, ws > 0


def wgrad_desc(case):
    from tg import geom
    n, h, w, ld_in, c_out, k, s, pad = case[2]
    return geom.conv_wgrad(n, h, w, ld_in, c_out, k, s, pad, ld_dy=case[3])


def query_wgrad_tile(d):
    from tg import lib
    ct, nt = C.c_int32(), C.c_int32()
    lib.call('tg_wgrad_tile', C.byref(d), C.byref(ct), C.byref(nt))
    return ct.value, nt.value


@pytest.fixture(autouse=True)
def _generic_kernels_only():
    """tg_conv3x3_policy(2): the generic kernels serve every shape; restored afterwards.  No halo launch may happen."""
    lib, _ = _tg()
    was = lib.call('tg_conv3x3_policy', 2)
    n0 = lib.call('tg_conv3x3_launches')
    yield
    assert lib.call('tg_conv3x3_launches') == n0, "a halo-tiled kernel ran"
    lib.call('tg_conv3x3_policy', was)


def _q(prec, a):
    return T.bf16_round(a) if prec == BF16 else a


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def act64(t, act):
    if act == 'lrelu':
        return torch.where(t > 0, t, np.float64(kc.ALPHA) * t)
    if act == 'relu':
        return torch.where(t > 0, t, torch.zeros_like(t))
    if act == 'tanh':
        return torch.tanh(t)
    return t


def act_grad64(y, act):
    if act == 'lrelu':
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, np.float64(kc.ALPHA)))
    if act == 'relu':
        return (y > 0).to(y.dtype)
    return torch.ones_like(y)


def worst(got, ref, sab):
    """max over the outputs of |got - ref| / (TOL * sum|terms|) (<= 1 passes), on the device."""
    return float(((got.double() - ref).abs() / (kc.TOL * sab + 1e-300)).max())


def close(got, ref, sab, what):
    r = worst(got, ref, sab)
    assert r <= 1.0, "%s: error is %.2f x the reduction bound (TOL %.0e of the per-output sum |terms|)" % (what, r, kc.TOL)


def rejected(got, ref, sab, factor=10.0):
    return worst(got, ref, sab) > factor


def _seg_sums(rows, segs, square=False):
    """float64 per-segment column sums of rows [M, c] (and of |terms|)."""
    v = rows.double() * rows.double() if square else rows.double()
    parts = torch.split(v, list(segs), dim=0)
    return torch.stack([p.sum(0) for p in parts]), torch.stack([p.abs().sum(0) for p in parts])


def _rng_data(rng, shape, scale=1.0):
    return (rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)).astype(np.float32)


# ---- igemm: every tile x operand type x schedule x epilogue family -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", IGEMM_CASES, ids=[c['id'] for c in IGEMM_CASES])
def test_igemm_tile_against_float64(case):
    lib, geom = _tg()
    prec, fam, segs = case['prec'], case['family'], case['segs']
    descs = descs_of(case)
    d0 = descs[0]
    assert query_tile(descs, segs, prec == BF16) == case['tile'] + (case['cut'],), "the cost model no longer picks what %s names" % case['id']
    rng = np.random.default_rng(zlib.crc32(case['id'].encode()))
    live = case['live'] or d0.c_out
    M = d0.n_img * d0.h_v * d0.w_v
    # operands: every gathered channel is live (the last K-tile must matter); filter rows >= live and their bias are zero (channel padding)
    x = _rng_data(rng, (d0.n_img, d0.h_in, d0.w_in, d0.ld_in))
    # the filter extent the launcher maps: (c_out - 1) * w_sn + max tapw * w_st + ld_in floats
    w_rows = (d0.c_out - 1) * d0.w_sn + max(int(d.tapw[t]) for d in descs for t in range(d.n_taps)) * d0.w_st + d0.ld_in
    wf = _rng_data(rng, (w_rows,), 1.0 / np.sqrt(d0.ld_in * d0.n_taps))
    dead = np.zeros(w_rows, bool)
    for n in range(live, d0.c_out):
        for d in descs:
            for t in range(d.n_taps):
                o = n * d0.w_sn + int(d.tapw[t]) * d0.w_st
                dead[o:o + d0.ld_in] = True
    wf[dead] = 0
    bias = np.zeros(d0.c_out, np.float32)
    bias[:live] = _rng_data(rng, (live,))
    xq, wq = _f64(_q(prec, x)), _f64(_q(prec, wf))
    refs = kc.igemm_ref64(descs, xq, wq)

    out_shape = (d0.n_img, d0.h_out, d0.w_out, d0.ld_out)
    n_out = int(np.prod(out_shape))
    xd, wd, bd = kc.dev(x), kc.dev(wf), kc.dev(bias)
    st = lib.cur_stream()
    ns = len(segs) if segs else 0
    sa = (C.c_int32 * ns)(*segs) if segs else None
    yact = None
    if fam in ('actsum', 'bnbwdstat'):              # actsum: the activation output y; bnbwdstat: the batch norm's input x (both at the output's addresses)
        yact = kc.dev(kc.y_for(rng, out_shape, case['act']))
    n_sums = {'plain': 0, 'colsum': ns * d0.c_out, 'actsum': ns * d0.c_out, 'bnstat': 8 * ns * 2 * d0.c_out, 'bnbwdstat': 8 * ns * 2 * d0.c_out}[fam]

    def launch(scratch):
        g = kc.guarded(n_out)
        s = kc.guarded(2 * n_sums) if n_sums else None
        sp = s.ptr if s else None
        if fam == 'plain' and len(descs) > 1:
            arr = lib.desc_array(descs)
            lib.call_igemm('tg_igemm_multi_' + prec, C.cast(arr, C.c_void_p), len(descs), lib.ptr(xd), lib.ptr(wd), lib.ptr(bd), g.ptr, st, scratch=scratch)
        elif fam == 'plain':
            lib.call_igemm('tg_igemm_' + prec, d0, lib.ptr(xd), lib.ptr(wd), lib.ptr(bd), g.ptr, st, scratch=scratch)
        elif fam == 'colsum':
            lib.call_igemm('tg_igemm_colsum_' + prec, d0, lib.ptr(xd), lib.ptr(wd), g.ptr, sa, ns, sp, 0, st, scratch=scratch)
        elif fam == 'actsum':
            lib.call_igemm('tg_igemm_actsum_' + prec, d0, lib.ptr(xd), lib.ptr(wd), lib.ptr(yact), lib.ACT[case['act']], float(kc.ALPHA), g.ptr, sa, ns, sp,
                           0, st, scratch=scratch)
        elif fam == 'bnbwdstat':
            lib.call_igemm('tg_igemm_bnbwdstat_' + prec, d0, lib.ptr(xd), lib.ptr(wd), lib.ptr(yact), g.ptr, sa, ns, sp, 0, st, scratch=scratch)
        else:
            lib.call_igemm('tg_igemm_bnstat_' + prec, d0, lib.ptr(xd), lib.ptr(wd), lib.ptr(bd), g.ptr, sa, ns, sp, 0, st, scratch=scratch)
        g.check_guard()
        if s is not None:
            s.check_guard()
        return g.t.view(out_shape).clone(), (s.t.view(torch.float64).clone() if s is not None else None)

    # reference outputs (+ the control without the last K-tile) in the output's layout
    ref = torch.full(out_shape, float('nan'), dtype=torch.float64, device='cuda')
    sab, drop = torch.zeros_like(ref), torch.zeros_like(ref)
    bias64 = _f64(bias) if fam in ('plain', 'bnstat') else torch.zeros(d0.c_out, dtype=torch.float64, device='cuda')
    tanh_slack = 0.5 if case['act'] == 'tanh' and fam in ('plain', 'bnstat') else 0.0
    for d, (acc, s_, last) in zip(descs, refs):
        if fam == 'actsum':
            gy = act_grad64(yact.double()[:, d.oo_y::d.os_y, d.oo_x::d.os_x][:, :d.h_v, :d.w_v].reshape(M, -1)[:, :d.c_out], case['act'])
            kc.igemm_scatter(d, acc * gy, ref)
            kc.igemm_scatter(d, (acc - last) * gy, drop)
            kc.igemm_scatter(d, s_ * gy, sab)
        else:
            a = case['act'] if fam in ('plain', 'bnstat') else None
            kc.igemm_scatter(d, act64(acc + bias64, a), ref)
            kc.igemm_scatter(d, act64(acc - last + bias64, a), drop)
            kc.igemm_scatter(d, s_ + bias64.abs() + tanh_slack * (s_ > 0), sab)
    ns_ = d0.n_store

    def check_out(y, what):
        assert not torch.isnan(y[..., :ns_]).any(), "%s: %d owned outputs were never written" % (what, int(torch.isnan(y[..., :ns_]).sum()))
        assert torch.isnan(y[..., ns_:]).all(), "%s: a channel in [n_store, ld_out) was written" % what
        close(y[..., :ns_], ref[..., :ns_], sab[..., :ns_], what)
        assert (y[..., live:ns_] == 0).all(), "%s: channel padding is not exactly 0" % what

    def check_sums(y, s, what):
        rows = y[..., :ns_].reshape(M, ns_)
        if fam == 'bnstat':
            s = s.view(8, ns, 2, d0.c_out)
            assert (s[1:] == 0).all(), "%s: replicas 1..7 of the statistics buffer are not zero" % what
            for k, sq in ((0, False), (1, True)):
                r, a = _seg_sums(rows, segs, sq)
                close(s[0, :, k, :ns_], r, a, what + (' sums of squares' if sq else ' sums'))
                assert (s[0, :, k, ns_:] == 0).all()
        elif fam == 'bnbwdstat':                     # S0 = sum dy, S1 = sum dy * x
            s = s.view(8, ns, 2, d0.c_out)
            assert (s[1:] == 0).all(), "%s: replicas 1..7 of the statistics buffer are not zero" % what
            xr = yact[..., :ns_].reshape(M, ns_).double()
            for k, v, nm in ((0, rows, ' sums of dy'), (1, rows.double() * xr, ' sums of dy * x')):
                r, a = _seg_sums(v, segs)
                close(s[0, :, k, :ns_], r, a, what + nm)
                assert (s[0, :, k, ns_:] == 0).all()
        else:
            s = s.view(ns, d0.c_out)
            r, a = _seg_sums(rows, segs)
            close(s[:, :ns_], r, a, what + ' column sums')
            assert (s[:, ns_:] == 0).all()

    y, s = launch(True)
    check_out(y, case['id'])
    assert rejected(y[..., :ns_], drop[..., :ns_], sab[..., :ns_]), "negative control: the bound accepts a reference without its last K-tile"
    if s is not None:
        check_sums(y, s, case['id'])
    if case['cut']:
        y2, s2 = launch(True)
        assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), "the cut schedule is not deterministic"
        if s is not None:
            assert torch.equal(s.view(torch.int64), s2.view(torch.int64)), "the cut schedule's sums are not deterministic"
        y1, s1 = launch(False)                       # scratch = NULL: one workgroup per tile
        check_out(y1, case['id'] + ' uncut')
        if s1 is not None:
            check_sums(y1, s1, case['id'] + ' uncut')


# ---- wgrad: every (CT, NT) x operand type, the library's pixel split, one split, and splits that own no pixels ---------------------------------
def _empty_tail_split(M):
    """smallest split count whose last split owns no pixel (px_per_split = 32-rounded ceil(M / n_split))."""
    for ns in range(2, 4 * M):
        pps = (-(-M // ns) + 31) // 32 * 32
        if (ns - 1) * pps >= M:
            return ns
    raise AssertionError(M)


@pytest.mark.parametrize("prec", [F32, BF16])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad_tile_against_float64(case, prec):
    lib, geom = _tg()
    d = wgrad_desc(case)
    assert query_wgrad_tile(d) == case[1], "tg_wgrad_tile no longer picks what %s names" % case[0]
    rng = np.random.default_rng(zlib.crc32(case[0].encode()) + (prec == BF16))
    M = d.n_img * d.h_v * d.w_v
    x = _rng_data(rng, (d.n_img, d.h_in, d.w_in, d.ld_in))
    dy = _rng_data(rng, (d.n_img, d.h_out, d.w_out, d.ld_out))
    xd, dyd = kc.dev(x), kc.dev(dy)
    xq, dq = _f64(_q(prec, x)), _f64(_q(prec, dy))
    dm = dq[..., :d.c_out].reshape(M, d.c_out)                # os = 1: the output rows in pixel order
    a_taps = [kc.igemm_gather(xq, d, t) for t in range(d.n_taps)]
    st = lib.cur_stream()
    lib_split = geom.wgrad_splits(d, prec == BF16)
    for ns in sorted({lib_split, 1, _empty_tail_split(M)}):
        pps = ((M + ns - 1) // ns + 31) // 32 * 32
        g = kc.guarded(ns * d.n_taps * d.ld_in * d.c_out)
        lib.call('tg_wgrad_' + prec, d, lib.ptr(xd), lib.ptr(dyd), g.ptr, ns, st)
        g.check_guard()
        slab = g.t.view(ns, d.n_taps, d.ld_in, d.c_out)
        assert not torch.isnan(slab).any(), "n_split %d: %d slab elements were never written" % (ns, int(torch.isnan(slab).sum()))
        ref = torch.zeros(slab.shape, dtype=torch.float64, device='cuda')
        sab = torch.zeros_like(ref)
        for s in range(ns):
            r0, r1 = min(s * pps, M), min((s + 1) * pps, M)
            if r0 == r1:
                assert (slab[s] == 0).all(), "n_split %d: split %d owns no pixels and is not exactly 0" % (ns, s)
                continue
            for t in range(d.n_taps):
                a = a_taps[t][r0:r1]
                ref[s, t] = a.T @ dm[r0:r1]
                sab[s, t] = a.abs().T @ dm[r0:r1].abs()
        close(slab, ref, sab, "%s n_split %d" % (case[0], ns))
        # negative control: the reference without the last 32-pixel tile (owned by the split holding pixel M - 1)
        p0, s_last = (M - 1) // 32 * 32, (M - 1) // pps
        drop = ref.clone()
        for t in range(d.n_taps):
            drop[s_last, t] -= a_taps[t][p0:M].T @ dm[p0:M]
        assert rejected(slab, drop, sab), "negative control: the bound accepts a reference without its last pixel tile"
