"""Per-kernel float64 tests of tg_colstats_f32 (csrc/norm.hip: colstats_stage1 / colstats_stage2), all five modes:
  0 SUM(a)   1 SUM(a), SUM(a^2)   2 SUM(a * act'(b))   3 SUM(a), SUM(a * b)   4 SUM((a - mu)^2), mu = b * alpha (b: the mode-0 sums).

Shapes: c = 1, 10 and 130 (c4 = 33 column groups: blockIdx.x = 1 holds one group and a padded tail), ld_a != ld_b, every column behind c
poisoned with NaN (the sums of the padded columns stay in the workspace); segments of 300, 7, 1025, 1 and 2400 rows: several chunks of
RCH = 256 rows per segment, and ten in the last one, so the lane loop of colstats_stage2 takes a second turn (lanes 0 and 1 own chunks 8 and
9); mode 4 runs on one segment of 2400 rows with b = the mode-0 sums of the launch before it.

Tolerance class (tests/kernel_check.py): reduction — every output within TOL of the sum |terms| of its (segment, column), terms being what the
kernel adds in fp64: a, a^2, a b, a act'(b) (one fp32 product plus the roundings of act', at most 7 u |a| times act' evaluated on absolute
values, 1 + y^2 for tanh — tests/test_gpu_norm_finalize.py, test_seg_actgrad_shift; that magnitude is the |term| of mode 2) and (a - mu)^2.
In mode 4 the kernel rounds mu to fp32 (at most u |mu| off), which moves the sum by at most 2 u |mu| |SUM(a - mu)| + n (u mu)^2: that is added
to the bound (a = 30 + N(0,1): a - mu itself is exact in fp32).  Negative control of every
output: the reference without the last row of the last segment.  Two launches give the same bits (fixed-order two-stage reduction), and the
guard behind a workspace of exactly tg_colstats_workspace_floats(rows, nseg, c) floats is intact."""
import numpy as np
import pytest

from kernel_check import ACTS, ALPHA, TOL, U, act64, act_grad64, assert_bits, close, dev, finish, guarded, lib, ptr, rejected, st, y_for
from test_gpu_norm_finalize import f8, seg_arr, seg_bounds

pytestmark = pytest.mark.gpu

SEGS = [300, 7, 1025, 1, 2400]
WIDTHS = [1, 10, 130]


def ceil4(c):
    return (c + 3) // 4 * 4


def poisoned(a, ld):
    out = np.full((a.shape[0], ld), np.nan, np.float32)
    out[:, :a.shape[1]] = a
    return out


def launch(mode, a, b, segs, c, act='none', want_s2=True, ld_b=None):
    """-> s1 [nseg, c], s2 [nseg, c] or None; a, b: [rows, c] float32 (b may be None, or for mode 4 a device buffer of ceil4(c) floats)"""
    L = lib()
    rows, nseg = a.shape[0], len(segs)
    ld_a = ceil4(c) + 4
    ld_b = ceil4(c) + 8 if ld_b is None else ld_b
    wsn = L.call('tg_colstats_workspace_floats', rows, nseg, c)
    out = []
    for rep in range(2):
        work, s1, s2 = guarded(wsn), guarded(nseg * c), guarded(nseg * c) if want_s2 else None
        bd = None if b is None else b if mode == 4 else ptr(dev(poisoned(b, ld_b)))
        alpha = float(ALPHA) if mode != 4 else float(np.float32(1.0 / rows))
        L.call('tg_colstats_f32', mode, ptr(dev(poisoned(a, ld_a))), ld_a, bd, ld_b, rows, c, seg_arr(segs), nseg, L.ACT[act], alpha, work.ptr, s1.ptr,
               s2.ptr if want_s2 else None, st())
        work.check_guard()
        out.append((finish(s1, (nseg, c)), finish(s2, (nseg, c)) if want_s2 else None))
    for k in range(2):
        if out[0][k] is not None:
            assert_bits(out[1][k], out[0][k], "mode %d: the second launch" % mode)
    return out[0]


def check(got, t64, segs, what, extra=0.0, mag=None):
    """got [nseg, c] against the column sums of the terms t64 [rows, c] per segment; mag: the terms evaluated on absolute values (default |t64|);
    extra: an absolute allowance, as a multiple of TOL"""
    mag = np.abs(t64) if mag is None else mag
    for s, (r0, r1) in enumerate(seg_bounds(segs)):
        close(got[s], t64[r0:r1].sum(0), mag[r0:r1].sum(0) + extra, "%s: segment %d" % (what, s))
    r0, r1 = seg_bounds(segs)[-1]
    assert rejected(got[-1], t64[r0:r1 - 1].sum(0), mag[r0:r1].sum(0) + extra), "%s does not miss the last row" % what


def inputs(c, seed):
    rng = np.random.default_rng(seed + c)
    rows = sum(SEGS)
    a = (rng.standard_normal((rows, c)) * 2 + 1).astype(np.float32)
    a[-1] = 2 + rng.random(c)                                     # a moderate last row: the negative controls drop it
    return rng, rows, a


@pytest.mark.parametrize("c", WIDTHS)
def test_modes_0_1_3(c):
    rng, rows, a = inputs(c, 100)
    b = rng.standard_normal((rows, c)).astype(np.float32)
    b[-1] = 1 + rng.random(c)
    s1, s2 = launch(0, a, None, SEGS, c, want_s2=False)
    assert s2 is None
    check(s1, f8(a), SEGS, "mode 0")
    s1, s2 = launch(1, a, None, SEGS, c)
    check(s1, f8(a), SEGS, "mode 1, sum a")
    check(s2, f8(a) ** 2, SEGS, "mode 1, sum a^2")
    s1, s2 = launch(3, a, b, SEGS, c)
    check(s1, f8(a), SEGS, "mode 3, sum a")
    check(s2, f8(a) * f8(b), SEGS, "mode 3, sum a b")


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("act", ACTS)
def test_mode_2(c, act):
    """SUM(a * act'(b)), b the activation's output: every activation has a derivative through its output (kernel_check.act_grad64)"""
    rng, rows, a = inputs(c, 200 + len(act))
    y = y_for(rng, (rows, c), act)
    y[-1] = np.float32(act64(1.0, act))                           # act'(y) of the row the negative control drops is not 0
    g, g_mag = act_grad64(y, act)                                 # g_mag: 1 + y^2 for tanh, whose 1 - y^2 cancels near |y| = 1
    s1, s2 = launch(2, a, y, SEGS, c, act=act, want_s2=False)
    check(s1, f8(a) * g, SEGS, "mode 2, " + act, mag=np.abs(f8(a)) * g_mag)


@pytest.mark.parametrize("c", WIDTHS)
def test_mode_4_after_mode_0(c):
    """the centred second pass of tf.nn.moments: mode 0 on one segment of 2400 rows, then mode 4 with b = those sums and alpha = 1 / rows"""
    L = lib()
    rng = np.random.default_rng(300 + c)
    segs, rows = [2400], 2400
    a = (30 + rng.standard_normal((rows, c))).astype(np.float32)
    ld_a = ceil4(c) + 4
    wsn = L.call('tg_colstats_workspace_floats', rows, 1, c)
    work, s0 = guarded(wsn), guarded(ceil4(c))                      # mode 4 reads b in groups of four: ceil4(c) readable floats
    L.call('tg_colstats_f32', 0, ptr(dev(poisoned(a, ld_a))), ld_a, None, 0, rows, c, seg_arr(segs), 1, 0, 0.0, work.ptr, s0.ptr, None, st())
    work.check_guard()
    sums = finish(s0, owned=np.arange(ceil4(c)) < c)[:c]
    check(sums[None], f8(a), segs, "mode 0")
    alpha = np.float32(1.0 / rows)                                  # the argument as the kernel receives it
    mu = f8(sums) * f8(alpha)
    d = f8(a) - mu
    extra = (2 * U * np.abs(mu) * np.abs(d.sum(0)) + rows * (U * mu) ** 2) / TOL
    s1, _ = launch(4, a, s0.ptr, segs, c, want_s2=False, ld_b=0)
    check(s1, d * d, segs, "mode 4", extra=extra)
