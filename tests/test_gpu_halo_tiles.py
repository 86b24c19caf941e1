"""The halo-tiled 3x3 kernels (csrc/conv3x3_bf16.hip: conv3x3_pipe_kernel, csrc/wgrad3x3.hip: wgrad3x3_kernel) against float64.

conv3x3_pipe_kernel<W, COLSUM, BF16, STAT2, IN16> serves the forward pass and the input gradient (geom.conv_dgrad: transposed filter
layout, reversed tap order) of every 3x3 / stride-1 / SAME layer of width 16 / 32 / 64 with 256-pixel tiles of whole image rows x 128
output channels; wgrad3x3_kernel<W, BF16, IN16> serves the filter gradient.  HALO_CASES and WGRAD3_CASES are plain data: each case names
the entry point, hence the instantiation it must reach (ENTRY_KERNEL / WGRAD_ENTRY_KERNEL), and tests/test_halo_tile_coverage.py checks on
a machine without a GPU that every dispatched (W, instantiation, epilogue branch) is covered and that every case has the kernel's shape.

Image counts follow the compute-unit count (the library reads the same multiProcessorCount): a launch of T tiles runs on min(T, CUs)
resident workgroups, each walking its share (tiles_per_workgroup restates the kernel's distribution).  Per family and operand type three
regimes appear: one tile per workgroup, an odd number (3) of tiles on every workgroup (the k_tile & 1 column-sum buffers end on the parity
they started on), and a last round that is partly empty; each case asserts its regime at run time.

Every launch runs under tg_conv3x3_policy(1) (the halo kernels wherever the layer applies), except the ROUTING cases, which run under the
default policy 0 with image counts that make igemm_launch cut the launch into a halo head and a generic tail.  Checks per case
(tests/kernel_check.py, tests/test_gpu_gemm_tiles.py):
  * tg_conv3x3_launches moves by exactly 1: the halo kernel ran;
  * outputs and sums come from kernel_check.guarded (NaN-filled, guard behind): every owned element is written, channels in
    [n_store, ld_out) keep their NaN, channel padding (zero filter rows and bias) is exactly 0, the guard is intact;
  * reduction bound: |got - ref64| <= 1e-6 * sum|a||b| per output, ref64 the descriptor's operation in float64 on the same operands (bf16
    entry points: rounded to bf16 as the kernel rounds them; bf16-stored inputs: the stored values).  The halo kernel applies none / relu /
    leaky relu only (1-Lipschitz), so no tanh slack;
  * column sums, batch-norm sums and sums of squares, and the batch-norm backward sums S0 = sum dy, S1 = sum dy * x against float64 sums of
    the STORED outputs at the same bound of sum|terms|; replicas 1..7 of the [8][nseg][2][c_out] buffer and entries at or above n_store are 0;
  * negative controls: the bound rejects the reference without the last channel chunk of one tap (64 channels with bf16 operands, 32 with
    fp32 ones), and, for fp32 operands, the reference evaluated on bf16-rounded operands;
  * a second launch is bit-identical (every tile is summed by one workgroup in a fixed order; the fp64 sums use atomics and are held to the
    bound only);
  * wgrad3x3: every slab element written, float64 per pixel split at the library's split, one split, a split count that does not divide the
    tile count and one whose last split owns no tile (its slab exactly 0); the control drops the last pixel tile (64 pixels fp32, 128 bf16).

The float64 oracle runs on the device (torch float64 matrix products)."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import kernel_check as kc
import test_gpu_gemm_tiles as G

pytestmark = pytest.mark.gpu

F32, BF16, BF16IN = 'f32', 'bf16', 'bf16in'          # operand types: fp32, bf16-rounded fp32 tensors, bf16-stored input
TILE_PX, BN = 256, 128                               # conv3x3_pipe_kernel: pixels x output channels per tile
FAMILIES = ('plain', 'colsum', 'actsum', 'bnstat', 'bnbwdstat')
ACTS = ('none', 'relu', 'lrelu')
REGIMES = ('one', 'odd', 'partial')

# entry point -> (COLSUM, BF16, STAT2, IN16) of the conv3x3_pipe_kernel instantiation it launches (conv3x3_bf16.hip: launch_pipe)
ENTRY_KERNEL = {
    'tg_igemm_f32': (False, False, False, False),
    'tg_igemm_bf16': (False, True, False, False),
    'tg_igemm_colsum_f32': (True, False, False, False),
    'tg_igemm_colsum_bf16': (True, True, False, False),
    'tg_igemm_actsum_f32': (True, False, False, False),
    'tg_igemm_actsum_bf16': (True, True, False, False),
    'tg_igemm_bnstat_f32': (True, False, True, False),
    'tg_igemm_bnstat_bf16': (True, True, True, False),
    'tg_igemm_bnbwdstat_f32': (True, False, True, False),
    'tg_igemm_bnbwdstat_bf16': (True, True, True, False),
    'tg_igemm_bf16in_bf16': (False, True, False, True),
    'tg_igemm_bnstat_bf16in_bf16': (True, True, True, True),
}
# entry point -> (BF16, IN16) of the wgrad3x3_kernel instantiation (wgrad3x3.hip: launch)
WGRAD_ENTRY_KERNEL = {'tg_wgrad_f32': (False, False), 'tg_wgrad_bf16': (True, False), 'tg_wgrad_bf16in_bf16': (True, True)}


def entry_of(family, prec):
    if prec == BF16IN:
        return {'plain': 'tg_igemm_bf16in_bf16', 'bnstat': 'tg_igemm_bnstat_bf16in_bf16'}[family]
    return 'tg_igemm_%s%s' % ('' if family == 'plain' else family + '_', prec)


def _h(id, family, prec, op, W, h, ld_in, c_out, regime, nseg=0, act=None, ymul_act=None, bias=True, ld_out=None, n_store=None, live=None,
       live_in=None, policy=1):
    """one halo case: the epilogue family and operand type (hence the entry point), op 'fwd' (geom.conv_fwd, filter [c_out][9][ld_in]) or
    'dgrad' (geom.conv_dgrad with c_in_pad = c_out and ld_dy = ld_in: filter [9][c_out][ld_in], taps reversed), image W x h, channels
    ld_in (live_in of them nonzero) -> c_out (live of them with nonzero filter rows and bias; the rest is channel padding), the output's
    ld_out / n_store, the tiles-per-workgroup regime ('one' / 'odd' / 'partial'; 'head' / 'tail': a policy-0 launch cut into a halo head
    and a generic tail with a segment boundary in the head / in the tail), nseg application segments of whole images, the activation
    (plain, bnstat), the activation-gradient multiplier (actsum) and whether a bias is passed."""
    return dict(id=id, family=family, prec=prec, entry=entry_of(family, prec), op=op, W=W, h=h, ld_in=ld_in, c_out=c_out, regime=regime,
                nseg=nseg, act=act, ymul_act=ymul_act, bias=bias, ld_out=ld_out, n_store=n_store, live=live, live_in=live_in, policy=policy)


def _table():
    cases = []
    for wi, W in enumerate((16, 32, 64)):
        h = 2 * TILE_PX // W                          # two tiles per image column: a tile seam inside every image, an image seam between
        for pi, prec in enumerate((F32, BF16)):
            kch = 64 if prec == BF16 else 32
            rot = lambda k, seq: seq[(wi + pi + k) % len(seq)]
            reg = lambda fi: REGIMES[(wi + fi + pi) % 3]      # each (family, type) meets the three regimes over the three widths
            wide = lambda fi: 256 if (fi + pi) % 2 == 0 else 128        # each (width, family) has a case with two column tiles
            pad = lambda fi: dict(ld_out=wide(fi) + 8, n_store=wide(fi) - 6) if (wi + fi) % 2 else {}
            # ld_in: two channel chunks, or three with the last one partly live (padded input channels)
            cin = lambda fi: dict(ld_in=2 * kch) if (wi + fi) % 2 else dict(ld_in=3 * kch, live_in=2 * kch + kch // 2)
            tag = '%s-w%d' % (prec, W)
            cases += [
                _h('plain-fwd-' + tag, 'plain', prec, 'fwd', W, h, c_out=wide(0), regime=reg(0), act=rot(0, ACTS), live=wide(0) - 10, **cin(0), **pad(0)),
                _h('plain-dgrad-' + tag, 'plain', prec, 'dgrad', W, h, c_out=wide(1), regime=reg(1), act=rot(1, ACTS), **cin(1), **pad(1)),
                _h('plain-nobias-' + tag, 'plain', prec, 'fwd', W, h, c_out=wide(2), regime=reg(2), act=rot(2, ACTS), bias=False, **cin(2), **pad(2)),
                _h('colsum-' + tag, 'colsum', prec, 'fwd', W, h, c_out=wide(3), regime=reg(3), nseg=1 + (wi + pi) % 3, live=wide(3) - 20, **cin(3),
                   **pad(3)),
                _h('actsum-' + tag, 'actsum', prec, 'dgrad', W, h, c_out=wide(4), regime=reg(4), nseg=2, ymul_act=rot(0, ACTS), **cin(4), **pad(4)),
                _h('bnstat-' + tag, 'bnstat', prec, 'fwd', W, h, c_out=wide(5), regime=reg(5), nseg=8 if (wi, pi) == (0, 0) else 3,
                   act=rot(1, ACTS), live=wide(5) - 12, **cin(5), **pad(5)),
                _h('bnbwdstat-' + tag, 'bnbwdstat', prec, 'dgrad', W, h, c_out=wide(6), regime=reg(6), nseg=2 + wi, **cin(6), **pad(6)),
            ]
        # the bf16-stored-input pair (tg_igemm_bf16in_bf16 / tg_igemm_bnstat_bf16in_bf16)
        tag = 'bf16in-w%d' % W
        cases += [
            _h('plain-' + tag, 'plain', BF16IN, 'fwd', W, h, ld_in=128, c_out=256 if wi != 1 else 128, regime=REGIMES[wi], act=ACTS[wi],
               live=120, ld_out=136 if wi == 1 else None, n_store=122 if wi == 1 else None),
            _h('bnstat-' + tag, 'bnstat', BF16IN, 'fwd', W, h, ld_in=192, live_in=160, c_out=256 if wi == 1 else 128, regime=REGIMES[(wi + 1) % 3],
               nseg=2, act=ACTS[(wi + 2) % 3], ld_out=264 if wi == 1 else None, n_store=250 if wi == 1 else None),
        ]
    # default routing: 32 x 32 images, every column-sum family and operand type, a segment boundary in the halo head or the generic tail
    for fi, fam in enumerate(FAMILIES[1:]):
        for pi, prec in enumerate((F32, BF16)):
            cases.append(_h('route-%s-%s' % (fam, prec), fam, prec, 'dgrad' if fam in ('actsum', 'bnbwdstat') else 'fwd', 32, 32, ld_in=64, c_out=128,
                            regime=('head', 'tail')[(fi + pi) % 2], nseg=2, act='lrelu' if fam == 'bnstat' else None,
                            ymul_act='relu' if fam == 'actsum' else None, policy=0))
    return cases


HALO_CASES = _table()

# filter gradient: (id, entry, W, h, n_img, ld_in, c_out, ld_dy) — every <W, BF16, IN16>, one channel chunk (32) and several, c_out = 256,
# a gradient with ld_dy > c_out
WGRAD3_CASES = [
    ('f32-w16', 'tg_wgrad_f32', 16, 8, 10, 32, 128, None),
    ('f32-w32', 'tg_wgrad_f32', 32, 6, 7, 96, 256, None),
    ('f32-w64', 'tg_wgrad_f32', 64, 3, 9, 64, 128, 160),
    ('bf16-w16', 'tg_wgrad_bf16', 16, 16, 12, 64, 256, None),
    ('bf16-w32', 'tg_wgrad_bf16', 32, 8, 11, 32, 128, 160),
    ('bf16-w64', 'tg_wgrad_bf16', 64, 4, 9, 128, 128, None),
    ('bf16in-w16', 'tg_wgrad_bf16in_bf16', 16, 24, 5, 32, 128, 192),
    ('bf16in-w32', 'tg_wgrad_bf16in_bf16', 32, 12, 7, 96, 128, None),
    ('bf16in-w64', 'tg_wgrad_bf16in_bf16', 64, 6, 6, 64, 256, 288),
]


# ---- geometry shared with the coverage check --------------------------------------------------------------------------------------------------
def tiles_per_image(case):
    return case['h'] * case['W'] // TILE_PX * (case['c_out'] // BN)


def tiles_per_workgroup(ntiles, cus):
    """tiles each resident workgroup of conv3x3_pipe_kernel walks: grid = min(tiles, CUs); with 8 | grid XCD x (= blockIdx & 7) owns a
    contiguous share of q or q + 1 tiles and its grid / 8 workgroups stride through it, otherwise workgroup b takes tiles b, b + grid, ..."""
    grid = min(ntiles, cus)
    if grid % 8:
        return [len(range(b, ntiles, grid)) for b in range(grid)]
    q, r, per = ntiles >> 3, ntiles & 7, grid >> 3
    out = []
    for x in range(8):
        own = q + (1 if x < r else 0)
        out += [len(range(j, own, per)) for j in range(per)]
    return out


def regime_holds(regime, counts):
    if regime == 'one':
        return max(counts) == 1
    if regime == 'odd':
        return min(counts) == max(counts) and max(counts) % 2 == 1 and max(counts) > 1
    return min(counts) < max(counts) and max(counts) > 1           # 'partial': the last round leaves some workgroups without a tile


def head_images(n, tpi, cus, bf16):
    """tg::conv3x3_bf16_split_images under policy 0: the leading images a launch gives the halo kernel (0: no cut)."""
    pays = lambda k: k * tpi / (-(-k * tpi // cus) * cus) * (1.8 if bf16 else 1.07) >= 1.0
    tiles = n * tpi
    if tiles * 10 >= -(-tiles // cus) * cus * 9 or tiles // cus < 1:
        return 0
    head = tiles // cus * cus // tpi
    return head if 1 <= head < n and head * 10 >= n * 6 and pays(head) else 0


def n_images(case, cus):
    tpi = tiles_per_image(case)
    if case['regime'] == 'one':
        return max(1, (cus // 2 + 3) // tpi)
    if case['regime'] == 'odd':
        return 3 * cus // tpi
    if case['regime'] == 'partial':
        return (5 * cus // 2 + 1) // tpi
    return 2 * cus // tpi + 2                                        # head / tail: two whole rounds and two images more


def segments(case, n):
    """application segments in images: nseg parts of whole images, uneven; head / tail cases put the boundary inside that part."""
    k = case['nseg']
    if k == 0:
        return []
    if case['regime'] in ('head', 'tail'):
        return [n // 3, n - n // 3] if case['regime'] == 'head' else [n - 1, 1]
    base = n // k
    s = [base] * k
    s[-1] += n - base * k
    if k > 1 and s[0] > 1:
        s[0] -= 1
        s[1] += 1
    return s


def descriptor(case, n):
    from tg import geom, lib
    kw = dict(ld_out=case['ld_out'], n_store=case['n_store'])
    if case['op'] == 'fwd':
        d = geom.conv_fwd(n, case['h'], case['W'], case['ld_in'], case['c_out'], 3, 1, 'SAME', act=case['act'], **kw)
    else:
        (d,) = geom.conv_dgrad(n, case['h'], case['W'], case['c_out'], case['ld_in'], 3, 1, 'SAME', **kw)
        d.act, d.alpha = lib.ACT[case['act']], 0.2                  # the same register epilogue serves the input gradient
    return d


def wgrad3_desc(case, n=None):
    from tg import geom
    _, _, W, h, n_img, ld_in, c_out, ld_dy = case
    return geom.conv_wgrad(n_img if n is None else n, h, W, ld_in, c_out, 3, 1, 'SAME', ld_dy=ld_dy)


def wgrad3_splits(tiles):
    """(a split count that does not divide the tile count, the smallest one whose last split owns no tile) for tiles_per_split = ceil."""
    ragged = next(ns for ns in range(2, tiles) if tiles % ns and (ns - 1) * -(-tiles // ns) < tiles)
    empty = next(ns for ns in range(2, 2 * tiles) if (ns - 1) * -(-tiles // ns) >= tiles)
    return ragged, empty


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(autouse=True)
def _halo_kernels_wherever_they_apply():
    from tg import lib
    lib.load()
    was = lib.call('tg_conv3x3_policy', 1)
    try:
        yield
    finally:
        lib.call('tg_conv3x3_policy', was)


def _gen(seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return g


def _randn(g, shape, scale=1.0):
    return torch.randn(shape, generator=g, device='cuda', dtype=torch.float32) * scale


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _y_for(g, shape, act):
    """activation outputs with exact zeros (kc.y_for on the device): act'(y) takes both branches."""
    x = _randn(g, shape, 2.0)
    x[..., ::7] = 0
    return G.act64(x.double(), act).float() if act in ('relu', 'lrelu') else x


# ---- conv3x3_pipe_kernel: every case against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HALO_CASES, ids=[c['id'] for c in HALO_CASES])
def test_halo_conv_against_float64(case):
    from tg import lib
    lib.call('tg_conv3x3_policy', case['policy'])
    cus = _cus()
    fam, prec = case['family'], case['prec']
    n = n_images(case, cus)
    tpi = tiles_per_image(case)
    if case['policy'] == 1:
        counts = tiles_per_workgroup(n * tpi, cus)
        assert regime_holds(case['regime'], counts), "%s: %d tiles on %d CUs do not make regime %r (%s)" % (
            case['id'], n * tpi, cus, case['regime'], sorted(set(counts)))
    else:
        head = head_images(n, tpi, cus, prec != F32)
        assert 0 < head < n, "%s: %d images on %d CUs are not cut into a halo head and a generic tail" % (case['id'], n, cus)
    d = descriptor(case, n)
    segs = [s * case['h'] * case['W'] for s in segments(case, n)]
    if case['regime'] == 'head':
        assert segs[0] < head * case['h'] * case['W']
    elif case['regime'] == 'tail':
        assert sum(segs[:-1]) > head * case['h'] * case['W']
    ns = len(segs)
    M = n * case['h'] * case['W']
    c_out, ld_in, ns_ = d.c_out, d.ld_in, d.n_store
    live = case['live'] or ns_
    kch = 32 if prec == F32 else 64
    g = _gen(zlib.crc32(case['id'].encode()))

    x = _randn(g, (n, d.h_in, d.w_in, ld_in))
    if case['live_in']:
        x[..., case['live_in']:] = 0
    w_rows = (c_out - 1) * d.w_sn + max(int(d.tapw[t]) for t in range(9)) * d.w_st + ld_in
    wf = _randn(g, (w_rows,), 1.0 / np.sqrt(9 * ld_in))
    for o in range(live, c_out):                                     # channel padding: zero filter rows (and bias)
        for t in range(9):
            s0 = o * d.w_sn + int(d.tapw[t]) * d.w_st
            wf[s0:s0 + ld_in] = 0
    bias = torch.zeros(c_out, device='cuda')
    bias[:live] = _randn(g, (live,))
    out_shape = (n, d.h_out, d.w_out, d.ld_out)
    yact = _y_for(g, out_shape, case['ymul_act'] if fam == 'actsum' else None) if fam in ('actsum', 'bnbwdstat') else None
    xin = x.to(torch.bfloat16) if prec == BF16IN else x
    x64 = xin.double() if prec == BF16IN else (_bf(x) if prec == BF16 else x.double())
    w64 = wf.double() if prec == F32 else _bf(wf)

    st = lib.cur_stream()
    sa = (C.c_int32 * ns)(*segs) if ns else None
    n_sums = {'plain': 0, 'colsum': ns * c_out, 'actsum': ns * c_out}.get(fam, 8 * ns * 2 * c_out)
    bp = lib.ptr(bias) if case['bias'] else None

    def launch():
        o = kc.guarded(int(np.prod(out_shape)))
        s = kc.guarded(2 * n_sums) if n_sums else None
        sp = s.ptr if s else None
        n0 = lib.call('tg_conv3x3_launches')
        name, xp, wp = case['entry'], lib.ptr(xin), lib.ptr(wf)
        if fam == 'plain':
            lib.call_igemm(name, d, xp, wp, bp, o.ptr, st)
        elif fam == 'colsum':
            lib.call_igemm(name, d, xp, wp, o.ptr, sa, ns, sp, 0, st)
        elif fam == 'actsum':
            lib.call_igemm(name, d, xp, wp, lib.ptr(yact), lib.ACT[case['ymul_act']], float(kc.ALPHA), o.ptr, sa, ns, sp, 0, st)
        elif fam == 'bnstat':
            lib.call_igemm(name, d, xp, wp, bp, o.ptr, sa, ns, sp, 0, st)
        else:
            lib.call_igemm(name, d, xp, wp, lib.ptr(yact), o.ptr, sa, ns, sp, 0, st)
        o.check_guard()
        if s is not None:
            s.check_guard()
        assert lib.call('tg_conv3x3_launches') - n0 == 1, "%s: the halo kernel did not run exactly once" % case['id']
        return o.t.view(out_shape).clone(), (s.t.view(torch.float64).clone() if s is not None else None)

    # float64 reference in the output's layout, the control without the last channel chunk of the last tap, and (fp32) the oracle on
    # bf16-rounded operands
    (acc, sab_, last), = kc.igemm_ref64([d], x64, w64, last_k=kch)
    b64 = bias.double() if case['bias'] and fam in ('plain', 'bnstat') else torch.zeros(c_out, dtype=torch.float64, device='cuda')
    a = case['act'] if fam in ('plain', 'bnstat') else None
    if fam == 'actsum':
        gy = G.act_grad64(yact.double().reshape(M, -1)[:, :c_out], case['ymul_act'])
        val = lambda t: t * gy
        mag = sab_ * gy
    else:
        val = lambda t: G.act64(t + b64, a)
        mag = sab_ + b64.abs()
    ref, sab, drop = (torch.full(out_shape, float('nan'), dtype=torch.float64, device='cuda') for _ in range(3))
    kc.igemm_scatter(d, val(acc), ref)
    kc.igemm_scatter(d, mag, sab)
    kc.igemm_scatter(d, val(acc - last), drop)
    del last
    refq = None
    if prec == F32:
        (accq, _, _), = kc.igemm_ref64([d], _bf(x), _bf(wf))
        refq = torch.full(out_shape, float('nan'), dtype=torch.float64, device='cuda')
        kc.igemm_scatter(d, val(accq), refq)
        del accq
    del acc, sab_, mag

    y, s = launch()
    what = case['id']
    assert not torch.isnan(y[..., :ns_]).any(), "%s: %d owned outputs were never written" % (what, int(torch.isnan(y[..., :ns_]).sum()))
    assert torch.isnan(y[..., ns_:]).all(), "%s: a channel in [n_store, ld_out) was written" % what
    G.close(y[..., :ns_], ref[..., :ns_], sab[..., :ns_], what)
    assert (y[..., live:ns_] == 0).all(), "%s: channel padding is not exactly 0" % what
    assert G.rejected(y[..., :ns_], drop[..., :ns_], sab[..., :ns_]), "negative control: the bound accepts a reference without its last channel chunk"
    if refq is not None:
        assert G.rejected(y[..., :ns_], refq[..., :ns_], sab[..., :ns_]), "negative control: the bound accepts the oracle on bf16-rounded operands"
    if s is not None:
        rows = y[..., :ns_].reshape(M, ns_).double()
        if fam in ('colsum', 'actsum'):
            s = s.view(ns, c_out)
            r, ab = G._seg_sums(rows, segs)
            G.close(s[:, :ns_], r, ab, what + ' column sums')
            assert (s[:, ns_:] == 0).all(), "%s: a column sum at or above n_store is not 0" % what
        else:
            s = s.view(8, ns, 2, c_out)
            assert (s[1:] == 0).all(), "%s: replicas 1..7 of the statistics buffer are not zero" % what
            if fam == 'bnstat':
                terms = ((rows, ' sums'), (rows * rows, ' sums of squares'))
            else:
                terms = ((rows, ' sums of dy'), (rows * yact[..., :ns_].reshape(M, ns_).double(), ' sums of dy * x'))
            for k, (v, nm) in enumerate(terms):
                r, ab = G._seg_sums(v, segs)
                G.close(s[0, :, k, :ns_], r, ab, what + nm)
                assert (s[0, :, k, ns_:] == 0).all(), "%s: a statistic at or above n_store is not 0" % what
    y2, _ = launch()
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), "%s: a second launch is not bit-identical" % what


def test_halo_entry_points_refuse_nine_segments():
    """ConvParams and the generic kernels' parameters hold seg_rows[8]: a ninth segment is refused (TgError), nothing runs."""
    from tg import lib, geom
    n, hw = 9, 16
    d = geom.conv_fwd(n, hw, hw, 64, 128, 3, 1, 'SAME')
    x = torch.zeros((n, hw, hw, 64), device='cuda')
    xb = x.to(torch.bfloat16)
    wf = torch.zeros(128 * 9 * 64, device='cuda')
    out = torch.full((n, hw, hw, 128), 7.0, device='cuda')
    sums = torch.zeros(2 * 8 * 9 * 2 * 128, device='cuda')
    scratch = torch.zeros(1 << 20, device='cuda')
    sa = (C.c_int32 * 9)(*([hw * hw] * 9))
    st = lib.cur_stream()
    sc = (lib.ptr(scratch), scratch.numel() * 4)
    P = lib.ptr
    calls = []
    for prec in (F32, BF16):
        calls += [('tg_igemm_colsum_' + prec, (d, P(x), P(wf), P(out), sa, 9, P(sums), 0) + sc + (st,)),
                  ('tg_igemm_actsum_' + prec, (d, P(x), P(wf), P(out), lib.ACT['relu'], 0.2, P(out), sa, 9, P(sums), 0) + sc + (st,)),
                  ('tg_igemm_bnstat_' + prec, (d, P(x), P(wf), None, P(out), sa, 9, P(sums), 0) + sc + (st,)),
                  ('tg_igemm_bnbwdstat_' + prec, (d, P(x), P(wf), P(x), P(out), sa, 9, P(sums), 0) + sc + (st,))]
    calls.append(('tg_igemm_bnstat_bf16in_bf16', (d, P(xb), P(wf), None, P(out), sa, 9, P(sums), 0) + sc + (st,)))
    assert {c[0] for c in calls} == {e for e, k in ENTRY_KERNEL.items() if k[0]}
    n0 = lib.call('tg_conv3x3_launches')
    for name, args in calls:
        with pytest.raises(lib.TgError, match='bad args'):
            lib.call(name, *args)
    torch.cuda.synchronize()
    assert lib.call('tg_conv3x3_launches') == n0
    assert (out == 7.0).all()


# ---- wgrad3x3_kernel: every <W, BF16, IN16> at four pixel splits ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WGRAD3_CASES, ids=[c[0] for c in WGRAD3_CASES])
def test_wgrad3x3_against_float64(case):
    from tg import lib, geom
    cid, entry, W = case[0], case[1], case[2]
    bf16, in16 = WGRAD_ENTRY_KERNEL[entry]
    d = wgrad3_desc(case)
    bmw = 128 if bf16 else 64                                        # pixels per tile
    M = d.n_img * d.h_v * d.w_v
    T = M // bmw
    g = _gen(zlib.crc32(cid.encode()))
    x = _randn(g, (d.n_img, d.h_in, d.w_in, d.ld_in))
    dy = _randn(g, (d.n_img, d.h_out, d.w_out, d.ld_out))
    xin = x.to(torch.bfloat16) if in16 else x
    x64 = xin.double() if in16 else (_bf(x) if bf16 else x.double())
    d64 = _bf(dy) if bf16 else dy.double()
    dm = d64[..., :d.c_out].reshape(M, d.c_out)
    a_taps = [kc.igemm_gather(x64, d, t) for t in range(9)]
    st = lib.cur_stream()
    ragged, empty = wgrad3_splits(T)
    for ns in sorted({geom.wgrad_splits(d, bf16), 1, ragged, empty}):
        tps = -(-T // ns)
        pps = tps * bmw
        o = kc.guarded(ns * 9 * d.ld_in * d.c_out)
        n0 = lib.call('tg_conv3x3_launches')
        lib.call(entry, d, lib.ptr(xin), lib.ptr(dy), o.ptr, ns, st)
        o.check_guard()
        assert lib.call('tg_conv3x3_launches') - n0 == 1, "%s n_split %d: wgrad3x3 did not run" % (cid, ns)
        slab = o.t.view(ns, 9, d.ld_in, d.c_out)
        assert not torch.isnan(slab).any(), "%s n_split %d: %d slab elements were never written" % (cid, ns, int(torch.isnan(slab).sum()))
        # per split: [ns, pps, .] blocks of the pixel rows, zero rows past M
        pad = ns * pps - M
        dmp = torch.nn.functional.pad(dm, (0, 0, 0, pad)).view(ns, pps, d.c_out)
        ref = torch.zeros(slab.shape, dtype=torch.float64, device='cuda')
        sab = torch.zeros_like(ref)
        for t in range(9):
            ap = torch.nn.functional.pad(a_taps[t], (0, 0, 0, pad)).view(ns, pps, d.ld_in)
            ref[:, t] = ap.transpose(1, 2) @ dmp
            sab[:, t] = ap.abs().transpose(1, 2) @ dmp.abs()
        for sp in range(ns):
            if sp * tps >= T:
                assert (slab[sp] == 0).all(), "%s n_split %d: split %d owns no tile and is not exactly 0" % (cid, ns, sp)
        G.close(slab, ref, sab, "%s n_split %d" % (cid, ns))
        p0, s_last = (T - 1) * bmw, (T - 1) // tps                   # the last pixel tile and the split that owns it
        drop = ref.clone()
        for t in range(9):
            drop[s_last, t] -= a_taps[t][p0:M].T @ dm[p0:M]
        assert G.rejected(slab, drop, sab), "negative control: the bound accepts a reference without its last pixel tile"
