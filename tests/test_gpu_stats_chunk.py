"""The statistics kernels of csrc/norm.hip at a chunk size training uses.  Every statistics workgroup (bn_sums, mobn_bwd_sums,
maxpool2_bwd_actsum, actgrad_bias) owns `chunk` rows of one segment, chunk = stats_chunk(rows) = max(32, ceil32(ceil(rows / 2048))): 32 up to
65 536 rows, 128 for the classifier's 200 k-row activations.  The width tests of tests/test_gpu_norm_finalize.py and
tests/test_gpu_norm_forward.py all run chunk = 32; here segments of 40 000, 1 and 30 000 rows (70 001 in all) give chunk = 64, with
c = 128: 32 column groups, eight row lanes, eight rows per lane and workgroup, 1 095 workgroups over eight replicas.

Bounds: those of the width tests with R = chunk - 1 fp32 additions on a term's way into its column sum (the batch norm's sums are
accumulated in fp64 and do not depend on it).  Every reduction's negative control — the reference without the last row of the last
segment, 30 to 40 times the bound for N(0,1) and for 30 + N(0,1) inputs by rough arithmetic — is asserted."""
import numpy as np
import pytest

from kernel_check import ALPHA, act_grad64, assert_pointwise, dev, finish, guarded, lib, ptr, st, y_for
import test_gpu_norm_finalize as F
import test_gpu_norm_forward as N
from test_gpu_norm_finalize import REPL, f8, seg_arr

pytestmark = pytest.mark.gpu

SEGS = N.SEG_TABLE['chunk64']
ROWS, C_ = sum(SEGS), 128
CHUNK = 64


def stats_chunk(rows):
    """csrc/norm.hip: stats_chunk restated"""
    return max(32, ((rows + 2047) // 2048 + 31) // 32 * 32)


def test_the_chunk_size_assumed_here():
    assert stats_chunk(ROWS) == CHUNK and stats_chunk(65536) == 32 and stats_chunk(65537) == 64 and stats_chunk(200000) == 128
    assert stats_chunk(sum(F.SEGS['ragged'])) == F.CHUNK == 32


def test_bn_train_forward_chunk64():
    cs = N.fwd_case('chunk64', C_)
    y, mi, mm, mv, sums = N.run_forward('tg_bn_train_f32', cs)
    N.check_forward(cs, y, mi, mm, mv, "bn_train, chunk 64")
    N.check_sums(sums, f8(cs.x), f8(cs.x), cs.segs, "bn_train, chunk 64")


@pytest.mark.parametrize("relu_input", [0, 1])
def test_bn_train_bwd_chunk64(relu_input):
    cs = N.bwd_case('chunk64', C_, 'relu' if relu_input else 'none')
    dx, dg, db, _, sums = N.run_backward(cs, 'tg_bn_train_bwd_f32')
    N.check_backward(cs, dx, dg, db, None, "bn_train_bwd, chunk 64")
    N.check_sums(sums, cs.dy64, cs.x64, cs.segs, "bn_train_bwd, chunk 64")


def test_mobn_bwd_chunk64():
    """tg_mobn_bwd_f32 as test_mobn_bwd_widths: sums and db to the reduction bound, dx on |t| + mean_seg |t| with K = R + 3"""
    L = lib()
    nseg, c = len(SEGS), C_
    dy, y, t64 = F.mobn_bwd_case(SEGS, c)
    sums = dev(np.full((REPL, nseg, c), 5.0), np.float64)
    dx, db = guarded(ROWS * c), guarded(c)
    L.call('tg_mobn_bwd_f32', ptr(dev(dy)), c, ptr(dev(y)), c, dx.ptr, c, ROWS, c, seg_arr(SEGS), nseg, L.ACT['lrelu'], float(ALPHA), ptr(sums), 0, db.ptr, st())
    got_dx, got_db = finish(dx, (ROWS, c)), finish(db)
    F.check_column_sums(sums.cpu().numpy().sum(0), got_db, t64, SEGS, "mobn_bwd, chunk 64")
    _, _, mean, mean_abs = F.seg_stats(t64, SEGS)
    assert_pointwise(got_dx, t64 - mean, np.abs(t64) + mean_abs, CHUNK - 1 + 3, "dx")


def test_maxpool_bwd_actsum_chunk64():
    """tg_maxpool2_bwd_actsum_f32 on 2x2 images, 40 000, 1 and 30 000 of them per application (one pooled pixel per image, so the pooled pixels
    are the statistics rows): t pointwise with K = 3 and exact zeros off the arg-max, the replica sums to the reduction bound."""
    L = lib()
    n, nseg, c = ROWS, len(SEGS), C_
    rng = np.random.default_rng(5000)
    y = rng.standard_normal((n, 4, c)).astype(np.float32)
    dpool = rng.standard_normal((n, c)).astype(np.float32)
    mask = (rng.random((n, c)) < 0.5).astype(np.float32)
    dpool[-1], mask[-1] = 1 + rng.random(c), 1.0                       # a moderate last row: the negative control drops it
    am = y.argmax(1)                                                    # the first maximum
    ymax = np.take_along_axis(y, am[:, None, :], 1)[:, 0]
    tv = f8(dpool) * f8(mask) * 2.0 * act_grad64(ymax, 'lrelu')[0]      # [n, c]: the term of every pooled pixel
    sums = dev(np.full((REPL, nseg, c), 5.0), np.float64)
    t = guarded(4 * n * c)
    L.call('tg_maxpool2_bwd_actsum_f32', ptr(dev(dpool)), c, ptr(dev(mask)), c, 2.0, ptr(dev(y)), c, t.ptr, c, n, 2, 2, c, seg_arr([4 * s for s in SEGS]), nseg,
           L.ACT['lrelu'], float(ALPHA), ptr(sums), 0, st())
    got_t = finish(t, (n, 4, c))
    hit = np.arange(4)[None, :, None] == am[:, None, :]
    assert (got_t[~hit] == 0).all(), "a gradient off the arg-max"
    assert_pointwise(got_t[hit], np.broadcast_to(tv[:, None, :], hit.shape)[hit], np.abs(np.broadcast_to(tv[:, None, :], hit.shape)[hit]), 3, "t")
    F.check_column_sums(sums.cpu().numpy().sum(0), None, tv, SEGS, "maxpool2_bwd_actsum, chunk 64")


def test_actgrad_bias_chunk64():
    """tg_actgrad_bias_f32 at 70 001 rows: dpre pointwise with K = 1, the bias gradient and the replica sums to the reduction bound"""
    L = lib()
    c = C_
    rng = np.random.default_rng(5001)
    dy = rng.standard_normal((ROWS, c)).astype(np.float32)
    y = y_for(rng, (ROWS, c), 'lrelu')
    dy[-1], y[-1] = 1 + rng.random(c), 1.0
    t64 = f8(dy) * act_grad64(y, 'lrelu')[0]
    out, bg = guarded(ROWS * c), guarded(c)
    sums = dev(np.full((REPL, c), 5.0), np.float64)
    L.call('tg_actgrad_bias_f32', ptr(dev(dy)), c, ptr(dev(y)), c, out.ptr, c, ROWS, c, L.ACT['lrelu'], float(ALPHA), ptr(sums), 0, bg.ptr, st())
    assert_pointwise(finish(out, (ROWS, c)), t64, np.abs(t64), 1, "dpre")
    F.check_column_sums(sums.cpu().numpy().sum(0)[None], finish(bg), t64, [ROWS], "actgrad_bias, chunk 64")
