"""Per-kernel float64 tests of the fused training-mode batch norm (tg_bn_train_f32 / _bf16, tg_bn_train_apply_f32 / _bf16, tg_bn_train_bwd_f32,
tg_bn_train_bwd_act_f32; tf.contrib.layers.batch_norm, Model/modle_base.py:229-237) and of the forward mean-only batch norm with the 2x2
max pool behind it (tg_mobn_apply_f32, tg_mobn_apply_pool_f32, tg_maxpool2_fwd_f32; Model/nn.py:147-187, Good_GAN_cifar10.py:121-124).

Batch norm.  Widths where bn_sums and the apply passes change shape: c = 1 (one column group, 256 row lanes), 10 (3 groups, 85 lanes, one
idle thread), 256 (one full block), 260 (the second block has one group), 300 (11 groups, 23 lanes in block 1), 512 (two blocks); the four
leading dimensions differ from each other and leave at least one untouched 16-byte group behind the padded width; the segments are those of
tests/test_gpu_norm_finalize.py (one, and eight ragged ones with one-row segments).  x = 30 + N(0,1): S1/n - mean^2 cancels 900 : 1, so
statistics taken in fp32 miss the bounds of mean_inv by two to three orders of magnitude.  The reference takes mean and variance in two
float64 passes.

Tolerance classes (tests/kernel_check.py; one per fp32 rounding, +2 per sqrtf or division):
  pointwise  mean: K = 1 on |mean| (the cast of the fp64 mean).
             inverse standard deviation: K = 6 on itself (cast of var 1, + eps 1, sqrtf 2, the division 2).
             y = x scale + shift on |x||scale| + |mean||scale| + |beta| with K = 11, the count of the |mean||scale| term: cast of the mean 1,
             scale = gamma inv 6 + 1, mean * scale 1, beta - . 1, the final addition 1 (the |x||scale| term has 9, |beta| 2).
             moving statistics: 5 (mean) / 6 (variance) roundings per segment of the chain, as test_bn_moving_update allows.
             dx = (A dy + B x + C) act'(x) on |A||dy| + |B||x| + |C|, |C| the expression of C on absolute values (|A||S_dy|/m + |B||mean|:
             B x + C cancels 30 : 1 for x = 30 + N(0,1)), with K = 10 (+1 for the multiplication by the leaky slope): B = -g inv inv dgm / m
             carries the cast of S_dyx - mean S_dy 1, inv * . 1, three products 3 and the division 2 = 7; B x: + 1 product + 2 additions = 10;
             B mean inside C: + 1 product + 1 subtraction + 1 addition = 10; A dy: 4; A S_dy / m: 7.
  bit-exact  y of the _bf16 forms = round-to-nearest-even of the fp32 form's y; their mean_inv and moving statistics = the fp32 form's;
             moving_mean = moving_var = NULL changes nothing else; columns [c, ceil4(c)) are 0, columns behind keep their NaN fill;
             sums_zeroed = 2 leaves the given sums untouched (a statistics launch would add to them).
  reduction  dgamma, dbeta, dbias and the sums a launch leaves behind: TOL of the sum |terms| per column, negative control = the reference
             without the last row of the last segment.

Mean-only BN and the pool.  c = 4, 12, 300, 512; (h, w) = (2, 2), (4, 6), (2, 34) — the last makes wo * c/4 > 256 at c = 300 and 512, so
the inner stride loop runs; images per segment 1, 3, 9, 2 and a single segment; ld, ld_out, ld_mask distinct and > c.
  pointwise  y = lrelu(x - mean_seg + b) on |x| + |mean| + |b| with K = 4 (cast of the mean, b - mean, x + shift, the leaky slope);
             pop_mean over the chain with 4 roundings per segment (+2), as test_mobn_finalize_train_and_eval;
             pooled = max * (mask * mscale) with K = 2 on the maximum's magnitude.
  bit-exact  the in-place pass leaves columns [c, ld) as they were; the pooled tensor without a mask is the fp32 maximum of the four
             activated values the kernel itself stored (a selection); a dropped position is exactly 0; tg_mobn_apply_pool_f32 equals
             tg_mobn_apply_f32 followed by tg_maxpool2_fwd_f32 bit for bit; evaluation leaves pop_mean alone."""
import functools

import numpy as np
import pytest

from kernel_check import (ALPHA, act64, act_grad64, assert_bits, assert_pointwise, bf16_rne_bits, bits, close, dev, finish, finish16, guarded,
                          guarded16, lib, ptr, rejected, st, NAN16_BITS, U)
from oracle import tf_ops as T
from test_gpu_norm_finalize import DECAY, EPS, SEGS, bn_sums, f8, seg_arr, seg_bounds, seg_index
from tg.ops import STATS_REPLICAS as REPL

pytestmark = pytest.mark.gpu

BN_WIDTHS = [1, 10, 256, 260, 300, 512]
SEG_TABLE = dict(SEGS, chunk64=[40000, 1, 30000])          # chunk64: tests/test_gpu_stats_chunk.py
K_MEAN, K_INV, K_Y, K_DX = 1, 6, 11, 10


def ceil4(c):
    return (c + 3) // 4 * 4


def lds(c):
    """ld_x, ld_y, ld_dy, ld_dx: all different, each >= ceil4(c) + 4"""
    return ceil4(c) + 4, ceil4(c) + 8, ceil4(c) + 12, ceil4(c) + 16


def padded(a, ld):
    out = np.zeros((a.shape[0], ld), np.float32)
    out[:, :a.shape[1]] = a
    return out


class Case(dict):
    __getattr__ = dict.__getitem__


def seg_moments64(x64, segs):
    mu = np.stack([x64[a:b].mean(0) for a, b in seg_bounds(segs)])
    var = np.stack([np.square(x64[a:b] - x64[a:b].mean(0)).mean(0) for a, b in seg_bounds(segs)])
    return mu, var


@functools.lru_cache(maxsize=None)
def fwd_case(segs_name, c):
    """inputs of the forward launch and its float64 reference (shared by the tests below; read-only)"""
    segs = SEG_TABLE[segs_name]
    rows, nseg = sum(segs), len(segs)
    rng = np.random.default_rng(7000 + 10 * c + nseg)
    x = (30 + rng.standard_normal((rows, c))).astype(np.float32)
    gamma = ((rng.random(c) + 0.5) * np.where(rng.random(c) < 0.5, -1.0, 1.0)).astype(np.float32)
    beta = rng.standard_normal(c).astype(np.float32)
    mm0, mv0 = rng.standard_normal(c).astype(np.float32), (rng.random(c) + 0.5).astype(np.float32)
    mu, var = seg_moments64(f8(x), segs)
    inv = 1 / np.sqrt(var + f8(EPS))
    scale, idx = f8(gamma) * inv, seg_index(segs)
    y = f8(x) * scale[idx] + (f8(beta) - mu[idx] * scale[idx])
    mag = np.abs(f8(x) * scale[idx]) + np.abs(mu[idx] * scale[idx]) + np.abs(f8(beta))
    rm, rv, mag_m, mag_v = f8(mm0), f8(mv0), np.abs(f8(mm0)), f8(mv0)
    for s, n in enumerate(segs):
        rm, rv = T.batch_norm_moving_update(rm, rv, mu[s], var[s], n, f8(DECAY), fused=True)
        mag_m, mag_v = mag_m + np.abs(mu[s]), mag_v + 2 * var[s]
    return Case(segs=segs, rows=rows, nseg=nseg, c=c, x=x, gamma=gamma, beta=beta, mm0=mm0, mv0=mv0, mu=mu, var=var, inv=inv, y=y, mag=mag, rm=rm, rv=rv,
                mag_m=mag_m, mag_v=mag_v, sums=bn_sums(rng, x, segs, c))


def run_forward(name, cs, moving=True, sums=None, zeroed=0):
    """one forward entry point on the case: -> (y [rows, ld_y] float32 or bf16 halfwords, mean_inv [nseg, 2, c], moving mean, moving var, the sums buffer)"""
    L = lib()
    c, rows, nseg = cs.c, cs.rows, cs.nseg
    ld_x, ld_y, _, _ = lds(c)
    y16, apply_only = name.endswith('bf16'), '_apply_' in name
    y = (guarded16 if y16 else guarded)(rows * ld_y)
    mi = guarded(nseg * 2 * c)
    mm, mv = guarded(c, fill=cs.mm0), guarded(c, fill=cs.mv0)
    sd = dev(np.full((REPL, nseg, 2, c), 5.0) if sums is None else sums, np.float64)          # 5.0: not zeroed, the call clears it
    args = [ptr(dev(padded(cs.x, ld_x))), ld_x, y.ptr, ld_y, rows, c, seg_arr(cs.segs), nseg, ptr(dev(cs.gamma)), ptr(dev(cs.beta)), float(EPS), float(DECAY),
            mm.ptr if moving else None, mv.ptr if moving else None, ptr(sd)] + ([] if apply_only else [zeroed]) + [mi.ptr, st()]
    L.call(name, *args)
    owned = np.broadcast_to(np.arange(ld_y) < ceil4(c), (rows, ld_y))
    got_y = (finish16 if y16 else finish)(y, (rows, ld_y), owned=owned)
    return got_y, finish(mi, (nseg, 2, c)), finish(mm), finish(mv), sd.cpu().numpy()


def check_forward(cs, y, mi, mm, mv, what):
    c, cp = cs.c, ceil4(cs.c)
    assert_pointwise(mi[:, 0], cs.mu, np.abs(cs.mu), K_MEAN, what + ": mean")
    assert_pointwise(mi[:, 1], cs.inv, cs.inv, K_INV, what + ": inverse standard deviation")
    assert_pointwise(y[:, :c], cs.y, cs.mag, K_Y, what + ": y")
    assert (bits(y[:, c:cp]) == 0).all(), what + ": columns [c, ceil4(c)) are not 0"
    assert np.isnan(y[:, cp:]).all(), what + ": wrote behind ceil4(c)"
    if mm is not None:
        assert_pointwise(mm, cs.rm, cs.mag_m, 5 * cs.nseg + 2, what + ": moving mean")
        assert_pointwise(mv, cs.rv, cs.mag_v, 6 * cs.nseg + 4, what + ": moving var")


def check_sums(got, x64, y64, segs, what):
    """the replica sums a statistics launch left behind, [REPL][nseg][2][c]: S0 = sum x, S1 = sum x * y, with the negative control"""
    tot = got.sum(0)
    for j, t in enumerate((x64, x64 * y64)):
        for s, (a, b) in enumerate(seg_bounds(segs)):
            close(tot[s, j], t[a:b].sum(0), np.abs(t[a:b]).sum(0), "%s: S%d of segment %d" % (what, j, s))
        a, b = seg_bounds(segs)[-1]
        assert rejected(tot[-1, j], t[a:b - 1].sum(0), np.abs(t[a:b]).sum(0)), "%s: S%d does not miss the last row" % (what, j)


@pytest.mark.parametrize("segs", list(SEGS), ids=str)
@pytest.mark.parametrize("c", BN_WIDTHS)
def test_bn_train_forward(segs, c):
    """tg_bn_train_f32: statistics + apply; the same launch with sums_zeroed = 1 on a zeroed buffer and without moving statistics; the _bf16
    form; tg_bn_train_apply_f32 / _bf16 on hand-built fp64 sums split at random over the replicas."""
    cs = fwd_case(segs, c)
    cp = ceil4(c)
    y, mi, mm, mv, sums = run_forward('tg_bn_train_f32', cs)
    check_forward(cs, y, mi, mm, mv, "bn_train")
    check_sums(sums, f8(cs.x), f8(cs.x), cs.segs, "bn_train")
    y1, mi1, mm1, mv1, _ = run_forward('tg_bn_train_f32', cs, sums=np.zeros((REPL, cs.nseg, 2, c)), zeroed=1)
    check_forward(cs, y1, mi1, mm1, mv1, "bn_train, sums_zeroed = 1")
    y2, mi2, mm2, mv2, _ = run_forward('tg_bn_train_f32', cs, moving=False)
    check_forward(cs, y2, mi2, None, None, "bn_train without moving statistics")
    assert_bits(y2[:, :cp], y[:, :cp], "y without moving statistics")
    assert_bits(mi2, mi, "mean_inv without moving statistics")
    assert_bits(mm2, cs.mm0, "moving mean given as NULL")            # the guarded copies were not handed in: still the initial values
    y16, mi16, mm16, mv16, _ = run_forward('tg_bn_train_bf16', cs)
    # no segment here has more than REPL statistics workgroups, so every replica receives one addition: the sums of two launches are the same bits
    assert_bits(mi16, mi, "mean_inv of the bf16 form")
    assert_bits(mm16, mm, "moving mean of the bf16 form")
    assert_bits(mv16, mv, "moving var of the bf16 form")
    assert (y16[:, :cp] == bf16_rne_bits(y[:, :cp])).all(), "y of the bf16 form is not RNE of the fp32 form's"
    assert (y16[:, cp:] == NAN16_BITS).all()
    ya, mia, mma, mva, sa = run_forward('tg_bn_train_apply_f32', cs, sums=cs.sums)
    check_forward(cs, ya, mia, mma, mva, "bn_train_apply on given sums")
    assert (sa == cs.sums).all(), "bn_train_apply wrote to the sums"
    yb, mib, mmb, mvb, _ = run_forward('tg_bn_train_apply_bf16', cs, sums=cs.sums)
    assert_bits(mib, mia, "mean_inv of apply_bf16")
    assert_bits(mmb, mma, "moving mean of apply_bf16")
    assert_bits(mvb, mva, "moving var of apply_bf16")
    assert (yb[:, :cp] == bf16_rne_bits(ya[:, :cp])).all() and (yb[:, cp:] == NAN16_BITS).all()


def test_fp32_statistics_would_miss_the_mean_inv_bounds():
    """the reason for x = 30 + N(0,1): S0 and S1 accumulated in fp32 (row lanes of four rows, then the lanes in order) put mean and inverse
    standard deviation outside K_MEAN / K_INV by a wide margin — on the CPU, no launch."""
    cs = fwd_case('one', 256)
    x = cs.x
    s0, s1 = np.zeros(x.shape[1], np.float32), np.zeros(x.shape[1], np.float32)
    for r in range(cs.rows):
        s0, s1 = (s0 + x[r]).astype(np.float32), (s1 + x[r] * x[r]).astype(np.float32)
    mu = f8(s0) / cs.rows
    inv = 1 / np.sqrt(np.maximum(f8(s1) / cs.rows - mu * mu, 0) + f8(EPS))
    assert (np.abs(inv - cs.inv[0]) / (K_INV * U * cs.inv[0])).max() > 100           # two orders of magnitude
    assert (np.abs(mu - cs.mu[0]) / (K_MEAN * U * np.abs(cs.mu[0]))).max() > 1


# ---------------------------------------------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=None)
def bwd_case(segs_name, c, act):
    """dy, x (act = none: 30 + N(0,1); relu / lrelu: the output of that activation, with exact zeros), mean_inv as the forward pass would leave it (the
    float64 statistics cast to float: an INPUT of the backward pass), and the float64 reference on these fp32 inputs"""
    segs = SEG_TABLE[segs_name]
    rows, nseg = sum(segs), len(segs)
    rng = np.random.default_rng(8000 + 10 * c + nseg + len(act))
    pre = rng.standard_normal((rows, c))
    dy = rng.standard_normal((rows, c))
    pre[-1], dy[-1] = 1.5 + rng.random(c), np.where(rng.random(c) < 0.5, -1.0, 1.0) * (1 + rng.random(c))     # a moderate last row: the negative controls drop it
    if act == 'none':
        x = (30 + pre).astype(np.float32)
    else:
        pre = pre * 2 + 0.5
        pre[:-1][rng.random((rows - 1, c)) < 0.15] = 0
        x = act64(pre, act).astype(np.float32)
    dy = dy.astype(np.float32)
    gamma = ((rng.random(c) + 0.5) * np.where(rng.random(c) < 0.5, -1.0, 1.0)).astype(np.float32)
    mu64, var64 = seg_moments64(f8(x), segs)
    mean_inv = np.stack([mu64, 1 / np.sqrt(var64 + f8(EPS))], 1).astype(np.float32)              # [nseg, 2, c]
    mu, inv, g, idx = f8(mean_inv[:, 0]), f8(mean_inv[:, 1]), f8(gamma), seg_index(segs)
    m = np.asarray(segs, np.float64)[:, None]
    x64, dy64 = f8(x), f8(dy)
    xc = x64 - mu[idx]
    sdy = np.stack([dy64[a:b].sum(0) for a, b in seg_bounds(segs)])
    dgm = inv * np.stack([(dy64[a:b] * xc[a:b]).sum(0) for a, b in seg_bounds(segs)])
    A = g * inv
    B = -g * inv * inv * dgm / m
    t1 = -A * sdy / m
    Cc, mag_C = t1 - B * mu, np.abs(t1) + np.abs(B * mu)
    dact, dact_mag = act_grad64(x, act)
    dx = (A[idx] * dy64 + B[idx] * x64 + Cc[idx]) * dact
    mag = (np.abs(A[idx] * dy64) + np.abs(B[idx] * x64) + mag_C[idx]) * dact_mag
    tg = inv[idx] * dy64 * xc                                                                      # the terms of dgamma
    sums = np.zeros((REPL, nseg, 2, c))
    sums[0, :, 0], sums[0, :, 1] = sdy, np.stack([(dy64[a:b] * x64[a:b]).sum(0) for a, b in seg_bounds(segs)])
    return Case(segs=segs, rows=rows, nseg=nseg, c=c, act=act, x=x, dy=dy, gamma=gamma, mean_inv=mean_inv, dx=dx, mag=mag, tg=tg, dy64=dy64, x64=x64,
                sums=sums, rng_seed=int(rng.integers(1 << 30)))


def run_backward(cs, entry, sums=None, zeroed=0, dsum=False, dsum_zeroed=0):
    """-> dx [rows, ld_dx], dgamma, dbeta, dbias or None, the sums buffer after the call"""
    L = lib()
    c, rows, nseg = cs.c, cs.rows, cs.nseg
    ld_x, _, ld_dy, ld_dx = lds(c)
    dx, dg, db = guarded(rows * ld_dx), guarded(c), guarded(c)
    sd = dev(np.full((REPL, nseg, 2, c), 5.0) if sums is None else sums, np.float64)
    head = [ptr(dev(padded(cs.dy, ld_dy))), ld_dy, ptr(dev(padded(cs.x, ld_x))), ld_x, dx.ptr, ld_dx, rows, c, seg_arr(cs.segs), nseg, ptr(dev(cs.gamma)),
            ptr(dev(cs.mean_inv))]
    dbias = None
    if entry == 'tg_bn_train_bwd_f32':
        L.call(entry, *(head + [{'none': 0, 'relu': 1}[cs.act], ptr(sd), zeroed, dg.ptr, db.ptr, st()]))
    else:
        dbias = guarded(c) if dsum else None
        ds = dev(np.zeros((REPL, c)) if dsum_zeroed else np.full((REPL, c), 5.0), np.float64) if dsum else None
        L.call(entry, *(head + [L.ACT[cs.act], float(ALPHA), ptr(sd), zeroed, dg.ptr, db.ptr, ptr(ds), dsum_zeroed, dbias.ptr if dsum else None, st()]))
    owned = np.broadcast_to(np.arange(ld_dx) < ceil4(c), (rows, ld_dx))
    return finish(dx, (rows, ld_dx), owned=owned), finish(dg), finish(db), finish(dbias) if dsum else None, sd.cpu().numpy()


def check_backward(cs, dx, dg, db, dbias, what):
    c, cp = cs.c, ceil4(cs.c)
    assert_pointwise(dx[:, :c], cs.dx, cs.mag, K_DX + (cs.act == 'lrelu'), what + ": dx")
    assert (dx[:, c:cp] == 0).all() and np.isnan(dx[:, cp:]).all(), what + ": padding"
    for got, t, name in ((dg, cs.tg, "dgamma"), (db, cs.dy64, "dbeta")) + (((dbias, cs.dx, "dbias"),) if dbias is not None else ()):
        sabs = np.abs(t).sum(0) if name != "dbias" else cs.mag.sum(0)
        close(got, t.sum(0), sabs, "%s: %s" % (what, name))
        assert rejected(got, t[:-1].sum(0), sabs), "%s: %s does not miss the last row" % (what, name)


@pytest.mark.parametrize("segs", list(SEGS), ids=str)
@pytest.mark.parametrize("c", BN_WIDTHS)
@pytest.mark.parametrize("relu_input", [0, 1])
def test_bn_train_bwd(segs, c, relu_input):
    """tg_bn_train_bwd_f32 with the three ways to hand in the accumulator: cleared by the call, zeroed by the caller (sums_zeroed = 1), and
    the statistics given (sums_zeroed = 2: fp64 sums split over the replicas, which the call must read and leave as they are)."""
    cs = bwd_case(segs, c, 'relu' if relu_input else 'none')
    dx, dg, db, _, sums = run_backward(cs, 'tg_bn_train_bwd_f32')
    check_backward(cs, dx, dg, db, None, "bn_train_bwd")
    check_sums(sums, cs.dy64, cs.x64, cs.segs, "bn_train_bwd")
    dx, dg, db, _, _ = run_backward(cs, 'tg_bn_train_bwd_f32', sums=np.zeros((REPL, cs.nseg, 2, c)), zeroed=1)
    check_backward(cs, dx, dg, db, None, "bn_train_bwd, sums_zeroed = 1")
    rng = np.random.default_rng(cs.rng_seed)
    w = rng.random((REPL,) + cs.sums.shape[1:])
    given = w / w.sum(0) * cs.sums[0]
    given[-1] = cs.sums[0] - given[:-1].sum(0)
    dx, dg, db, _, after = run_backward(cs, 'tg_bn_train_bwd_f32', sums=given, zeroed=2)
    check_backward(cs, dx, dg, db, None, "bn_train_bwd, sums given")
    assert (after == given).all(), "sums_zeroed = 2: a statistics launch ran on top of the given sums"


@pytest.mark.parametrize("segs", list(SEGS), ids=str)
@pytest.mark.parametrize("c", BN_WIDTHS + [64])
@pytest.mark.parametrize("act", ['none', 'relu', 'lrelu'])
def test_bn_train_bwd_act(segs, c, act):
    """tg_bn_train_bwd_act_f32: dx times act'(x), and where the column layout allows it the bias gradient = the column sums of dx, with
    dsum cleared by the call and zeroed by the caller.  The other widths are refused with the launcher's message and run without dsum."""
    L = lib()
    cs = bwd_case(segs, c, act)
    ncol = min(c, 256)
    if c % 4 == 0 and 256 % ((ncol + 3) // 4) == 0 and (c <= 256 or c % 256 == 0):
        for dsum_zeroed in (0, 1):
            dx, dg, db, dbias, _ = run_backward(cs, 'tg_bn_train_bwd_act_f32', dsum=True, dsum_zeroed=dsum_zeroed)
            check_backward(cs, dx, dg, db, dbias, "bn_train_bwd_act, dsum_zeroed = %d" % dsum_zeroed)
    else:
        buf = dev(np.zeros(max(cs.rows * (ceil4(c) + 16), REPL * 2 * cs.nseg * c * 2)))
        with pytest.raises(L.TgError, match='bias-gradient sums'):
            L.call('tg_bn_train_bwd_act_f32', ptr(buf), ceil4(c), ptr(buf), ceil4(c), ptr(buf), ceil4(c), cs.rows, c, seg_arr(cs.segs), cs.nseg, ptr(buf),
                   ptr(buf), L.ACT[act], float(ALPHA), ptr(buf), 0, None, None, ptr(buf), 0, ptr(buf), st())
        dx, dg, db, _, _ = run_backward(cs, 'tg_bn_train_bwd_act_f32')
        check_backward(cs, dx, dg, db, None, "bn_train_bwd_act without dsum")


# ---------------------------------------------------------------------------------------------------------------- mean-only BN forward + max pool
MOBN_WIDTHS = [4, 12, 300, 512]
POOL_HW = [(2, 2), (4, 6), (2, 34)]
POOL_SEGS = {'one': [15], 'four': [1, 3, 9, 2]}
MSCALE = np.float32(1 / 0.7)                         # not a power of two: max * (mask * mscale) rounds
MODES = [(1, True, True), (1, True, False), (1, False, True), (0, True, False), (0, False, True)]        # train, with b, with mask
PATTERN = np.float32(-77.25)                         # columns [c, ld) of the in-place tensor


@pytest.mark.parametrize("imgs", list(POOL_SEGS), ids=str)
@pytest.mark.parametrize("hw", POOL_HW, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("c", MOBN_WIDTHS)
def test_mobn_apply_and_pool(imgs, hw, c):
    """tg_mobn_apply_f32 followed by tg_maxpool2_fwd_f32, and tg_mobn_apply_pool_f32 on the same input, each against float64 in every mode of MODES
    (training / evaluation, b given / NULL, with / without a keep-mask), then against each other bit for bit."""
    L = lib()
    imgs, (h, w) = POOL_SEGS[imgs], hw
    n, nseg = sum(imgs), len(imgs)
    segs = [m * h * w for m in imgs]
    rows, npix = n * h * w, n * (h // 2) * (w // 2)
    ld, ld_out, ld_m = c + 4, c + 8, c + 12
    rng = np.random.default_rng(9000 + c + 7 * h + w + nseg)
    x = np.full((rows, ld), PATTERN, np.float32)
    x[:, :c] = (rng.standard_normal((rows, c)) * 2 + 1).astype(np.float32)
    b, pop0 = rng.standard_normal(c).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    mask = np.full((npix, ld_m), np.nan, np.float32)
    mask[:, :c] = (rng.random((npix, c)) < 0.5).astype(np.float32)
    x64, idx = f8(x[:, :c]), seg_index(segs)
    sums = np.stack([x64[a_:b_].sum(0) for a_, b_ in seg_bounds(segs)])                 # [nseg, c] fp64: what the convolution's epilogue leaves
    mean = sums / np.asarray(segs, np.float64)[:, None]
    sd, sa = dev(sums, np.float64), seg_arr(segs)
    for train, with_b, with_mask in MODES:
        what = "train=%d b=%d mask=%d" % (train, with_b, with_mask)
        bb = f8(b) if with_b else np.zeros(c)
        bd, md, sdd = ptr(dev(b)) if with_b else None, ptr(dev(mask)) if with_mask else None, ptr(sd) if train else None
        sub = mean[idx] if train else np.broadcast_to(f8(pop0), (rows, c))
        ref = act64(x64 - sub + bb, 'lrelu')
        mag = np.abs(x64) + np.abs(sub) + np.abs(bb)
        # tg_mobn_apply_f32, then tg_maxpool2_fwd_f32 on what it stored
        xa, pa, oa = guarded(rows * ld, fill=x), guarded(c, fill=pop0), guarded(npix * ld_out)
        L.call('tg_mobn_apply_f32', xa.ptr, ld, rows, c, sa, nseg, sdd, bd, pa.ptr, float(DECAY), L.ACT['lrelu'], float(ALPHA), st())
        L.call('tg_maxpool2_fwd_f32', xa.ptr, ld, oa.ptr, ld_out, md, ld_m, float(MSCALE), n, h, w, c, st())
        # tg_mobn_apply_pool_f32 on the same input
        xb, pb, ob = guarded(rows * ld, fill=x), guarded(c, fill=pop0), guarded(npix * ld_out)
        L.call('tg_mobn_apply_pool_f32', xb.ptr, ld, n, h, w, c, sa, nseg, sdd, bd, pb.ptr, float(DECAY), L.ACT['lrelu'], float(ALPHA), ob.ptr, ld_out, md, ld_m,
               float(MSCALE), st())
        owned = np.broadcast_to(np.arange(ld_out) < c, (npix, ld_out))
        got = {}
        for name, xg, pg, og in (('apply + maxpool2_fwd', xa, pa, oa), ('apply_pool', xb, pb, ob)):
            act, pop, out = finish(xg, (rows, ld)), finish(pg), finish(og, (npix, ld_out), owned=owned)
            got[name] = (act, pop, out)
            tag = "%s, %s" % (name, what)
            assert_pointwise(act[:, :c], ref, mag, 4, tag + ": activated")
            assert (act[:, c:] == PATTERN).all(), tag + ": the in-place pass touched columns [c, ld)"
            assert np.isnan(out[:, c:]).all(), tag + ": wrote behind c in the pooled tensor"
            own = act[:, :c].reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(npix, 4, c).max(1)        # of what the kernel stored
            if with_mask:
                keep = mask[:, :c] > 0
                assert_pointwise(out[:, :c], f8(own) * f8(mask[:, :c]) * f8(MSCALE), np.abs(f8(own)) * f8(MSCALE), 2, tag + ": pooled")
                assert (out[:, :c][~keep] == 0).all(), tag + ": a dropped position is not 0"
            else:
                assert_bits(out[:, :c], own, tag + ": pooled")
            if train:
                rp, mp = f8(pop0), np.abs(f8(pop0))
                for s in range(nseg):
                    rp, mp = rp * f8(DECAY) + mean[s] * (1 - f8(DECAY)), mp + np.abs(mean[s])
                assert_pointwise(pop, rp, mp, 4 * nseg + 2, tag + ": pop_mean")
            else:
                assert_bits(pop, pop0, tag + ": evaluation changed pop_mean")
        for k, part in enumerate(("activated", "pop_mean", "pooled")):
            assert_bits(got['apply_pool'][k][..., :c], got['apply + maxpool2_fwd'][k][..., :c], "%s: %s of the fused launch" % (what, part))
    if nseg > 1:                                                        # a segment boundary inside an image is refused
        bad = list(segs)
        bad[0], bad[1] = bad[0] + 1, bad[1] - 1
        xb, pb, ob = guarded(rows * ld, fill=x), guarded(c, fill=pop0), guarded(npix * ld_out)
        with pytest.raises(L.TgError, match='whole number'):
            L.call('tg_mobn_apply_pool_f32', xb.ptr, ld, n, h, w, c, seg_arr(bad), nseg, ptr(sd), ptr(dev(b)), pb.ptr, float(DECAY), L.ACT['lrelu'], float(ALPHA),
                   ob.ptr, ld_out, None, ld_m, float(MSCALE), st())
        xb.check_guard()
