"""Per-kernel float64 tests of the finalisers and apply passes of csrc/norm.hip: training / inference batch norm (tf.contrib.layers.batch_norm,
Model/modle_base.py:229-237; oracle.tf_ops.batch_norm_train / _bwd), the moving-statistics update, and mean-only batch norm by
application segment (Model/nn.py:147-187; oracle.tf_ops.mobn_train / _eval / _train_bwd) — a single segment, eight ragged segments and a
one-row segment (variance 0: eps dominates).

The moving variance is held to oracle.tf_ops.batch_norm_moving_update(fused=True): the Bessel-corrected (unbiased) batch variance
var * n / (n - 1), and the biased one for a one-row segment (n / max(n - 1, 1)), updated sequentially over the segments.

Tolerance classes (tests/kernel_check.py):
  bit-exact   dbeta of bn_bwd_finalize (a copy), the db of mobn_bwd_finalize (an fp32 sum over the segments in segment order; also held to
              the reduction bound with a negative control that drops the last segment), bn_moving_update against the moving statistics
              of tg_bn_train_apply_f32 on the same sums ("bit-identical to re-running tg_bn_train_f32", tg_kernels.h);
  pointwise   every finaliser and apply pass: |got - ref64| <= K u mag, mag the expression on absolute values (so the cancellation in
              beta - mean * scale or A dy + B x + C is covered), K the count of fp32 roundings on the way, +2 per sqrtf / division and
              +4 per transcendental activation; the moving statistics allow 5 (mean) / 6 (variance) roundings per segment of the chain;
  reduction   the column sums behind the fused mean-only-BN backward passes (tg_mobn_bwd_f32, tg_maxpool2_bwd_actsum_f32,
              tg_actgrad_bias_f32, and the db of tg_mobn_center_f32): TOL of the sum |terms| per output, negative control = the reference
              without the last row of the last segment.

The fused mean-only-BN family at the widths where its shared workgroup tail (csrc/norm.hip: colsum_tail) changes shape: c = 4 (one column
group, 256 row lanes), 12 (85 lanes, one idle thread), 300 (3 lanes, 31 idle threads), 512 (2 lanes), and 256 column groups x one lane
(tg_actgrad_bias_f32 at ld_out = 1024); the ragged segments add one-row segments, segments shorter than the lane count and more workgroups
than replicas.  Every statistics workgroup there owns at most CHUNK = 32 rows, so a term of a column sum meets at most CHUNK - 1 fp32
additions before the fp64 atomics: that is the R in the pointwise bounds of dx below (tests/test_gpu_stats_chunk.py runs the same kernels at
CHUNK = 64, the chunk of a tensor of more than 65 536 rows)."""
import ctypes as C

import numpy as np
import pytest

from kernel_check import ACTS, ALPHA, act64, act_grad64, assert_bits, assert_pointwise, bits, close, dev, finish, guarded, lib, ptr, rejected, seq_sum32, st, y_for
from oracle import tf_ops as T
from tg.ops import STATS_REPLICAS as REPL

pytestmark = pytest.mark.gpu

EPS = np.float32(1e-5)
DECAY = np.float32(0.9)
SEGS = {'one': [250], 'ragged': [1, 7, 250, 3, 64, 1, 100, 33]}
CHUNK = 32                                      # rows of a statistics workgroup below 65 536 rows (csrc/norm.hip: stats_chunk)


def seg_arr(segs):
    return (C.c_int32 * len(segs))(*segs)


def seg_index(segs):
    return np.repeat(np.arange(len(segs)), segs)


f8 = lambda a: np.asarray(a, np.float64)


@pytest.mark.parametrize("rows", [1, 250])
@pytest.mark.parametrize("c", [1, 3, 130])
@pytest.mark.parametrize("bessel", [0, 1])
def test_bn_finalize(rows, c, bessel):
    """tg_bn_finalize_f32 from s1 = sum x, s2 = sum (x - mean)^2: scale, shift, mean_inv and (bessel) the moving statistics."""
    L = lib()
    rng = np.random.default_rng(rows + c + bessel)
    x = (rng.standard_normal((rows, c)) * 2 + 3).astype(np.float32)
    s1 = x.astype(np.float64).sum(0).astype(np.float32)
    s2 = np.square(x - x.astype(np.float64).mean(0)).sum(0).astype(np.float32)
    gamma, beta = (rng.random(c) + 0.5).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    mm0, mv0 = rng.standard_normal(c).astype(np.float32), (rng.random(c) + 0.5).astype(np.float32)
    sc, sh, mi = guarded(c), guarded(c), guarded(2 * c)
    mm, mv = guarded(c, fill=mm0), guarded(c, fill=mv0)
    L.call('tg_bn_finalize_f32', ptr(dev(s1)), ptr(dev(s2)), rows, c, ptr(dev(gamma)), ptr(dev(beta)), float(EPS), sc.ptr, sh.ptr, mi.ptr, mm.ptr,
           mv.ptr, float(DECAY), bessel, st())
    mu, var = f8(s1) / rows, f8(s2) / rows
    inv = 1 / np.sqrt(var + f8(EPS))
    scale = f8(gamma) * inv
    shift = f8(beta) - mu * scale
    assert_pointwise(finish(sc), scale, np.abs(scale), 6, "scale")
    assert_pointwise(finish(sh), shift, np.abs(f8(beta)) + np.abs(mu * scale), 9, "shift")
    got_mi = finish(mi)
    assert_pointwise(got_mi[:c], mu, np.abs(mu), 2, "mean")
    assert_pointwise(got_mi[c:], inv, inv, 5, "inv")
    rm, rv = T.batch_norm_moving_update(f8(mm0), f8(mv0), mu, var, rows, f8(DECAY), fused=bool(bessel))
    assert_pointwise(finish(mm), rm, np.abs(f8(mm0)) + np.abs(mu), 4, "moving mean")
    assert_pointwise(finish(mv), rv, np.abs(f8(mv0)) + var * 2, 8, "moving var")


def test_bn_eval_finalize():
    """tg_bn_eval_finalize_f32 (is_training=False): scale = gamma / sqrt(mv + eps), shift = beta - mm * scale; c = 1 and two blocks."""
    L = lib()
    rng = np.random.default_rng(5)
    for c in (1, 130):
        gamma, beta = (rng.random(c) + 0.5).astype(np.float32), rng.standard_normal(c).astype(np.float32)
        mm, mv = (rng.standard_normal(c) * 3).astype(np.float32), rng.random(c).astype(np.float32)
        mv[0] = 0.0                                                     # eps alone
        sc, sh = guarded(c), guarded(c)
        L.call('tg_bn_eval_finalize_f32', c, ptr(dev(gamma)), ptr(dev(beta)), ptr(dev(mm)), ptr(dev(mv)), float(EPS), sc.ptr, sh.ptr, st())
        scale = f8(gamma) / np.sqrt(f8(mv) + f8(EPS))
        assert_pointwise(finish(sc), scale, np.abs(scale), 5, "scale")
        assert_pointwise(finish(sh), f8(beta) - f8(mm) * scale, np.abs(f8(beta)) + np.abs(f8(mm) * scale), 8, "shift")


def bn_sums(rng, x, segs, c):
    """the [REPL][nseg][2][c] fp64 replicas of S0 = sum x, S1 = sum x^2 per segment, the total split at random over the replicas."""
    nseg = len(segs)
    out = np.zeros((REPL, nseg, 2, c))
    b = 0
    for s, n in enumerate(segs):
        xs = f8(x[b:b + n])
        b += n
        for j, tot in enumerate((xs.sum(0), np.square(xs).sum(0))):
            w = rng.random((REPL, c))
            w /= w.sum(0)
            out[:, s, j] = w * tot
            out[REPL - 1, s, j] = tot - out[:REPL - 1, s, j].sum(0)
    return out


@pytest.mark.parametrize("segs", list(SEGS), ids=str)
@pytest.mark.parametrize("c", [1, 130, 300])
def test_bn_moving_update(segs, c):
    """tg_bn_moving_update_f32: the moving-statistics chain from the sums a forward launch left behind — bit-identical to the chain of
    tg_bn_train_apply_f32 on the same sums, and within the pointwise bound of the oracle's fused-kernel update applied segment by segment."""
    L = lib()
    segs = SEGS[segs]
    rows, nseg = sum(segs), len(segs)
    rng = np.random.default_rng(c + nseg)
    ld = (c + 31) // 32 * 32
    x = np.zeros((rows, ld), np.float32)
    x[:, :c] = (rng.standard_normal((rows, c)) * 2 + 1).astype(np.float32)
    sums = bn_sums(rng, x[:, :c], segs, c)
    sd = dev(sums, np.float64)
    gamma, beta = (rng.random(c) + 0.5).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    mm0, mv0 = rng.standard_normal(c).astype(np.float32), (rng.random(c) + 0.5).astype(np.float32)
    mm, mv = guarded(c, fill=mm0), guarded(c, fill=mv0)
    L.call('tg_bn_moving_update_f32', ptr(sd), rows, c, seg_arr(segs), nseg, float(DECAY), mm.ptr, mv.ptr, st())
    got_m, got_v = finish(mm), finish(mv)
    rm, rv, mag_m, mag_v = f8(mm0), f8(mv0), np.abs(f8(mm0)), f8(mv0)
    tot = sums.sum(0)
    for s, n in enumerate(segs):
        mu = tot[s, 0] / n
        var = np.maximum(tot[s, 1] / n - mu * mu, 0)
        rm, rv = T.batch_norm_moving_update(rm, rv, mu, var, n, f8(DECAY), fused=True)
        mag_m, mag_v = mag_m + np.abs(mu), mag_v + 2 * var
    assert_pointwise(got_m, rm, mag_m, 5 * nseg + 2, "moving mean")
    assert_pointwise(got_v, rv, mag_v, 6 * nseg + 4, "moving var")
    mm2, mv2 = guarded(c, fill=mm0), guarded(c, fill=mv0)
    y, mi = guarded(rows * ld), guarded(nseg * 2 * c)
    L.call('tg_bn_train_apply_f32', ptr(dev(x)), ld, y.ptr, ld, rows, c, seg_arr(segs), nseg, ptr(dev(gamma)), ptr(dev(beta)), float(EPS),
           float(DECAY), mm2.ptr, mv2.ptr, ptr(sd), mi.ptr, st())
    assert_bits(finish(mm2), got_m, "moving mean: bn_train_apply vs bn_moving_update")
    assert_bits(finish(mv2), got_v, "moving var: bn_train_apply vs bn_moving_update")


@pytest.mark.parametrize("rows", [1, 250])
@pytest.mark.parametrize("c", [1, 13, 130])
def test_bn_bwd_finalize(rows, c):
    """tg_bn_bwd_finalize_f32: dgamma = inv (S_dyx - mu S_dy), dbeta = S_dy, and dx = A dy + B x + C (oracle.tf_ops.batch_norm_train_bwd)."""
    L = lib()
    rng = np.random.default_rng(rows * c)
    x = (rng.standard_normal((rows, c)) * 2 + 1).astype(np.float32)
    dy = rng.standard_normal((rows, c)).astype(np.float32)
    gamma, beta = (rng.random(c) + 0.5).astype(np.float32), np.zeros(c, np.float32)
    mu64 = f8(x).mean(0)
    inv64 = 1 / np.sqrt(np.square(f8(x) - mu64).mean(0) + f8(EPS))
    mean_inv = np.concatenate([mu64, inv64]).astype(np.float32)
    s_dy = f8(dy).sum(0).astype(np.float32)
    s_dyx = (f8(dy) * f8(x)).sum(0).astype(np.float32)
    abc, dg, db = guarded(3 * c), guarded(c), guarded(c)
    L.call('tg_bn_bwd_finalize_f32', ptr(dev(s_dy)), ptr(dev(s_dyx)), rows, c, ptr(dev(gamma)), ptr(dev(mean_inv)), abc.ptr, dg.ptr, db.ptr, st())
    mu, inv, g, sdy = f8(mean_inv[:c]), f8(mean_inv[c:]), f8(gamma), f8(s_dy)
    dgm = inv * (f8(s_dyx) - mu * sdy)
    mag_dgm = inv * (np.abs(f8(s_dyx)) + np.abs(mu * sdy))
    A = g * inv
    B = -g * inv * inv * dgm / rows
    Cc = -A * sdy / rows - B * mu
    mag_B = g * inv * inv * mag_dgm / rows
    got = finish(abc).reshape(3, c)
    assert_pointwise(finish(dg), dgm, mag_dgm, 4, "dgamma")
    assert_bits(finish(db), s_dy, "dbeta")
    assert_pointwise(got[0], A, np.abs(A), 2, "A")
    assert_pointwise(got[1], B, mag_B, 10, "B")
    assert_pointwise(got[2], Cc, np.abs(A * sdy) / rows + mag_B * np.abs(mu), 14, "C")
    if rows > 1:                                        # the closed form is the oracle's batch-norm gradient
        _, cache = T.batch_norm_train(f8(x), g, f8(beta), float(EPS))
        ref_dx, ref_dg, _ = T.batch_norm_train_bwd(f8(dy), g, cache)
        np.testing.assert_allclose(A * f8(dy) + B * f8(x) + Cc, ref_dx, rtol=1e-5, atol=1e-5 * np.abs(ref_dx).max())
        np.testing.assert_allclose(dgm, ref_dg, rtol=1e-5, atol=1e-5 * np.abs(ref_dg).max())


def prefill(rows, ld, owned, pad_value=9.0):
    a = np.full((rows, ld), pad_value, np.float32)
    a[:, :owned] = np.nan
    return a


@pytest.mark.parametrize("rows,c,ld", [(250, 13, 16), (250, 64, 96), (1, 1, 4), (70000, 64, 64)])
@pytest.mark.parametrize("relu_mask", [0, 1])
def test_bn_bwd_apply(rows, c, ld, relu_mask):
    """tg_bn_bwd_apply_f32: dx = (A dy + B x + C) * (x > 0 when relu_mask) — the generator's ReLU -> BN (Good_GAN_cifar10.py:41-42); columns
    [c, ceil4(c)) are written as 0, columns behind them are not the kernel's; 70 000 rows run the grid-stride loop past 4 096 workgroups."""
    L = lib()
    rng = np.random.default_rng(rows + c + relu_mask)
    dy, x = rng.standard_normal((rows, ld)).astype(np.float32), rng.standard_normal((rows, ld)).astype(np.float32)
    x[:, :c][:, ::3] = 0.0
    abc = rng.standard_normal(3 * c).astype(np.float32)
    cp = (c + 3) // 4 * 4
    out = guarded(rows * ld, fill=prefill(rows, ld, cp))
    L.call('tg_bn_bwd_apply_f32', ptr(dev(dy)), ld, ptr(dev(x)), ld, out.ptr, ld, rows, c, ptr(dev(abc)), relu_mask, st())
    got = finish(out, (rows, ld))
    A, B, Cc = f8(abc[:c]), f8(abc[c:2 * c]), f8(abc[2 * c:])
    ref = A * f8(dy[:, :c]) + B * f8(x[:, :c]) + Cc
    mag = np.abs(A * f8(dy[:, :c])) + np.abs(B * f8(x[:, :c])) + np.abs(Cc)
    if relu_mask:
        keep = x[:, :c] > 0
        ref, mag = np.where(keep, ref, 0.0), np.where(keep, mag, 0.0)
    assert_pointwise(got[:, :c], ref, mag, 4)
    assert (bits(got[:, c:cp]) == 0).all() and (got[:, cp:] == 9.0).all()


@pytest.mark.parametrize("segs", list(SEGS), ids=str)
@pytest.mark.parametrize("c", [1, 13, 130])
@pytest.mark.parametrize("with_b", [True, False])
def test_mobn_finalize_train_and_eval(segs, c, with_b):
    """tg_mobn_finalize_f32 (Model/nn.py:147-187): train: shift[s] = b - sums[s] / rows_s, pop_mean <- decay pop_mean + (1 - decay) mean_s
    sequentially over the segments; eval: shift[s] = b - pop_mean (pop_mean untouched).  b = NULL: no offset."""
    L = lib()
    segs = SEGS[segs]
    nseg, rows = len(segs), sum(segs)
    rng = np.random.default_rng(nseg * c)
    sums = (rng.standard_normal((nseg, c)) * np.array(segs)[:, None]).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    pm0 = rng.standard_normal(c).astype(np.float32)
    bb = f8(b) if with_b else 0.0
    for train in (1, 0):
        pm, sh = guarded(c, fill=pm0), guarded(nseg * c)
        L.call('tg_mobn_finalize_f32', ptr(dev(sums)), seg_arr(segs), nseg, rows, c, ptr(dev(b)) if with_b else None, pm.ptr, float(DECAY), train,
               sh.ptr, st())
        got_sh, got_pm = finish(sh, (nseg, c)), finish(pm)
        if train:
            mean = f8(sums) / np.array(segs)[:, None]
            assert_pointwise(got_sh, bb - mean, np.abs(bb) + np.abs(mean), 3, "train shift")
            ref, mag = f8(pm0), np.abs(f8(pm0))
            for s in range(nseg):
                ref, mag = ref * f8(DECAY) + mean[s] * (1 - f8(DECAY)), mag + np.abs(mean[s])
            assert_pointwise(got_pm, ref, mag, 4 * nseg + 2, "pop_mean")
        else:
            assert_pointwise(got_sh, np.broadcast_to(bb - f8(pm0), (nseg, c)), np.broadcast_to(np.abs(bb) + np.abs(f8(pm0)), (nseg, c)), 1,
                             "eval shift")
            assert_bits(got_pm, pm0, "eval leaves pop_mean")


@pytest.mark.parametrize("segs", list(SEGS), ids=str)
@pytest.mark.parametrize("c", [1, 13, 130])
def test_mobn_bwd_finalize(segs, c):
    """tg_mobn_bwd_finalize_f32 (oracle.tf_ops.mobn_train_bwd): shift[s] = -sums[s] / rows_s, db = sum_s sums[s] in segment order."""
    L = lib()
    segs = SEGS[segs]
    nseg, rows = len(segs), sum(segs)
    rng = np.random.default_rng(nseg + c)
    sums = (rng.standard_normal((nseg, c)) * 10).astype(np.float32)
    sh, db = guarded(nseg * c), guarded(c)
    L.call('tg_mobn_bwd_finalize_f32', ptr(dev(sums)), seg_arr(segs), nseg, rows, c, sh.ptr, db.ptr, st())
    ref = -f8(sums) / np.array(segs)[:, None]
    assert_pointwise(finish(sh, (nseg, c)), ref, np.abs(ref), 1, "shift")
    got_db = finish(db)
    assert_bits(got_db, seq_sum32(list(sums)), "db")
    close(got_db, f8(sums).sum(0), np.abs(f8(sums)).sum(0), "db")
    if nseg > 1:
        assert rejected(got_db, f8(sums)[:-1].sum(0), np.abs(f8(sums)).sum(0))


SEG_APPLY = [  # segs, c, ld_x, c_zero_to, ld_y
    ('one', 13, 16, 32, 40),          # c % 4 != 0, zeros up to 32, columns behind untouched
    ('ragged', 64, 64, 64, 64),
    ('ragged', 1, 4, 1, 8),
    ('big', 128, 128, 128, 128),      # 40 000 rows x 32 float4 groups > 4 096 x 256 lanes
]
SEGS_BIG = [10000, 1, 19999, 10000]


def _segs(name):
    return SEGS_BIG if name == 'big' else SEGS[name]


@pytest.mark.parametrize("case", SEG_APPLY, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("with_scale", [True, False])
def test_seg_scale_shift_act(case, with_scale):
    """tg_seg_scale_shift_act_f32: y = act(x * scale + shift[seg]) for k < c, 0 for c <= k < c_zero_to (the mean-only BN / batch-norm apply
    of evaluation mode); every activation."""
    L = lib()
    name, c, ld_x, czt, ld_y = case
    segs = _segs(name)
    rows, nseg = sum(segs), len(segs)
    rng = np.random.default_rng(c + nseg + with_scale)
    x = np.full((rows, ld_x), np.nan, np.float32)
    x[:, :c] = (rng.standard_normal((rows, c)) * 2).astype(np.float32)
    scale = (rng.random(c) + 0.5).astype(np.float32)
    shift = rng.standard_normal((nseg, c)).astype(np.float32)
    xd = dev(x)
    cz4 = (czt + 3) // 4 * 4
    for a in ACTS:
        out = guarded(rows * ld_y, fill=prefill(rows, ld_y, cz4))
        L.call('tg_seg_scale_shift_act_f32', ptr(xd), ld_x, out.ptr, ld_y, rows, c, czt, seg_arr(segs), nseg, ptr(dev(scale)) if with_scale else None,
               ptr(dev(shift)), L.ACT[a], float(ALPHA), st())
        got = finish(out, (rows, ld_y))
        xs = f8(x[:, :c]) * (f8(scale) if with_scale else 1.0)
        pre = xs + f8(shift)[seg_index(segs)]
        ref = act64(pre, a)
        assert_pointwise(got[:, :c], ref, np.abs(xs) + np.abs(f8(shift)[seg_index(segs)]) + np.abs(ref), 3 if a in ('none', 'relu', 'lrelu') else 8,
                         a)
        assert (bits(got[:, c:cz4]) == 0).all() and (got[:, cz4:] == 9.0).all()


@pytest.mark.parametrize("case", SEG_APPLY, ids=lambda s: "x".join(map(str, s)))
def test_seg_actgrad_shift(case):
    """tg_seg_actgrad_shift_f32: dx = dy * act'(yact) + shift[seg] (backward of mean-only BN + nonlinearity, Model/nn.py:147-187)."""
    L = lib()
    name, c, ld, _, ld_dx = case
    segs = _segs(name)
    rows, nseg = sum(segs), len(segs)
    rng = np.random.default_rng(c * 3 + nseg)
    dy = np.full((rows, ld), np.nan, np.float32)
    dy[:, :c] = rng.standard_normal((rows, c)).astype(np.float32)
    shift = rng.standard_normal((nseg, c)).astype(np.float32)
    cp = (c + 3) // 4 * 4
    for a in ACTS:
        y = np.full((rows, ld), np.nan, np.float32)
        y[:, :c] = y_for(rng, (rows, c), a)
        y[:, c:cp] = 0.5
        dy[:, c:cp] = 0.5
        out = guarded(rows * ld_dx, fill=prefill(rows, ld_dx, cp))
        L.call('tg_seg_actgrad_shift_f32', ptr(dev(dy)), ld, ptr(dev(y)), ld, out.ptr, ld_dx, rows, c, seg_arr(segs), nseg, ptr(dev(shift)),
               L.ACT[a], float(ALPHA), st())
        got = finish(out, (rows, ld_dx))
        g, gm = act_grad64(y[:, :c], a)
        sh = f8(shift)[seg_index(segs)]
        ref = f8(dy[:, :c]) * g + sh
        assert_pointwise(got[:, :c], ref, np.abs(f8(dy[:, :c])) * gm + np.abs(sh), {'tanh': 5, 'sigmoid': 5, 'softplus': 7}.get(a, 2), a)
        assert (bits(got[:, c:cp]) == 0).all() and (got[:, cp:] == 9.0).all()


# ---- the fused mean-only-BN backward family at the widths where the shared workgroup tail changes shape ----
WIDTHS = [4, 12, 300, 512]


def seg_bounds(segs):
    e = np.cumsum(segs)
    return list(zip(e - np.asarray(segs), e))


def seg_stats(t64, segs):
    """per segment of t64 [rows, c]: column sums, column sums of |t|, and per row the segment mean of t and of |t|."""
    tot = np.stack([t64[a:b].sum(0) for a, b in seg_bounds(segs)])
    sab = np.stack([np.abs(t64[a:b]).sum(0) for a, b in seg_bounds(segs)])
    n = np.asarray(segs, np.float64)[:, None]
    return tot, sab, (tot / n)[seg_index(segs)], (sab / n)[seg_index(segs)]


def check_column_sums(got_seg, got_db, t64, segs, what, drop=1):
    """reduction bound on the per-segment sums (got_seg [nseg, c], None: not read) and on db = their sum; negative control: the reference
    without the last `drop` rows of the last segment."""
    tot, sab, _, _ = seg_stats(t64, segs)
    cut, _, _, _ = seg_stats(t64[:-drop], segs[:-1] + [segs[-1] - drop] if segs[-1] > drop else segs[:-1])
    if got_seg is not None:
        for s in range(len(segs)):
            close(got_seg[s], tot[s], sab[s], "%s: sums of segment %d" % (what, s))
        assert rejected(got_seg[-1], cut[-1] if segs[-1] > drop else 0.0, sab[-1]), what
    if got_db is not None:
        close(got_db, tot.sum(0), sab.sum(0), what + ": db")
        assert rejected(got_db, cut.sum(0), sab.sum(0)), what


def mobn_bwd_case(segs, c):
    """dy, y = lrelu output (sign decides the derivative), t = dy * lrelu'(y) in float64"""
    rng = np.random.default_rng(1000 * len(segs) + c)
    rows = sum(segs)
    dy = rng.standard_normal((rows, c)).astype(np.float32)
    y = y_for(rng, (rows, c), 'lrelu')
    return dy, y, f8(dy) * act_grad64(y, 'lrelu')[0]


@pytest.mark.parametrize("segs", list(SEGS), ids=str)
@pytest.mark.parametrize("c", WIDTHS)
def test_mobn_bwd_widths(segs, c):
    """tg_mobn_bwd_f32 (oracle.tf_ops.mobn_train_bwd behind lrelu'): the replica sums per segment and db to the reduction bound, dx = t - mean_seg(t)
    pointwise on |t| + mean_seg |t| with K = R + 3: one rounding of t, R = CHUNK - 1 additions on a term's way into the sum, the cast of the
    mean, the final addition."""
    L = lib()
    segs = SEGS[segs]
    nseg, rows = len(segs), sum(segs)
    dy, y, t64 = mobn_bwd_case(segs, c)
    sums = dev(np.full((REPL, nseg, c), 5.0), np.float64)                   # not zeroed: the call clears it
    dx, db = guarded(rows * c), guarded(c)
    L.call('tg_mobn_bwd_f32', ptr(dev(dy)), c, ptr(dev(y)), c, dx.ptr, c, rows, c, seg_arr(segs), nseg, L.ACT['lrelu'], float(ALPHA), ptr(sums), 0,
           db.ptr, st())
    got_dx, got_db = finish(dx, (rows, c)), finish(db)
    check_column_sums(sums.cpu().numpy().sum(0), got_db, t64, segs, "mobn_bwd c=%d" % c)
    _, _, mean, mean_abs = seg_stats(t64, segs)
    assert_pointwise(got_dx, t64 - mean, np.abs(t64) + mean_abs, CHUNK - 1 + 3, "dx")


def split_over_replicas(rng, tot, n_repl):
    """[n_repl][...] float64 summing to tot, split at random as bn_sums() does"""
    if n_repl == 1:
        return tot[None].copy()
    w = rng.random((n_repl,) + tot.shape)
    out = w / w.sum(0) * tot
    out[-1] = tot - out[:-1].sum(0)
    return out


@pytest.mark.parametrize("segs", list(SEGS), ids=str)
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("n_repl", [1, REPL])
def test_mobn_center_widths(segs, c, n_repl):
    """tg_mobn_center_f32 on given fp64 sums (one copy, or REPL replicas read in order): dx = t - sums[seg] / rows_seg pointwise with K = 2 (the cast
    of the mean, the addition), db = the sum over replicas and segments to the reduction bound."""
    L = lib()
    segs = SEGS[segs]
    nseg, rows = len(segs), sum(segs)
    rng = np.random.default_rng(2000 * nseg + c + n_repl)
    t = rng.standard_normal((rows, c)).astype(np.float32)
    tot, _, mean, _ = seg_stats(f8(t), segs)
    sums = split_over_replicas(rng, tot, n_repl)
    dx, db = guarded(rows * c), guarded(c)
    L.call('tg_mobn_center_f32', ptr(dev(t)), c, dx.ptr, c, rows, c, seg_arr(segs), nseg, ptr(dev(sums, np.float64)), n_repl, db.ptr, st())
    assert_pointwise(finish(dx, (rows, c)), f8(t) - mean, np.abs(f8(t)) + np.abs(mean), 2, "dx")
    check_column_sums(None, finish(db), f8(t), segs, "mobn_center c=%d n_repl=%d" % (c, n_repl))


POOL_IMGS = [1, 3, 9, 2]


def pool_case(c, h, with_mask):
    """y [n,h,h,c], pooled gradient, keep-mask (or None) and t = routed gradient * mask * 2 * lrelu'(y) in float64, [n*h*h, c]"""
    rng = np.random.default_rng(3000 + 10 * c + h + with_mask)
    n = sum(POOL_IMGS)
    y = rng.standard_normal((n, h, h, c)).astype(np.float32)
    dpool = rng.standard_normal((n, h // 2, h // 2, c)).astype(np.float32)
    mask = (rng.random(dpool.shape) < 0.5).astype(np.float32) if with_mask else None
    _, idx = T.maxpool2(f8(y))
    gy = T.maxpool2_bwd(f8(dpool) * (f8(mask) * 2.0 if with_mask else 1.0), idx, y.shape)
    return y, dpool, mask, (gy * act_grad64(y, 'lrelu')[0]).reshape(-1, c)


@pytest.mark.parametrize("c", [12, 300])
@pytest.mark.parametrize("h", [2, 4])
@pytest.mark.parametrize("with_mask", [True, False], ids=['mask', 'nomask'])
def test_maxpool_bwd_actsum_center_widths(c, h, with_mask):
    """tg_maxpool2_bwd_actsum_f32 -> tg_mobn_center_f32(n_repl = REPL), images per application 1, 3, 9, 2: h = 2 is one pooled pixel per image
    (chunks shorter than the lane count).  t pointwise with K = 3 (mask * scale, * gradient, * lrelu'), exact zeros off the arg-max; the replica
    sums and db to the reduction bound — the negative control drops the last image row of t, whose pooled pixels are the kernel's last work
    units; dx on |t| + mean_seg |t| with K = R + 5: the three roundings of a term, R = CHUNK - 1 additions, the cast of the mean, the addition."""
    L = lib()
    y, dpool, mask, t64 = pool_case(c, h, with_mask)
    n, nseg = sum(POOL_IMGS), len(POOL_IMGS)
    segs = [m * h * h for m in POOL_IMGS]
    rows = n * h * h
    sums = dev(np.full((REPL, nseg, c), 5.0), np.float64)
    t = guarded(rows * c)
    L.call('tg_maxpool2_bwd_actsum_f32', ptr(dev(dpool)), c, ptr(dev(mask)) if with_mask else None, c, 2.0 if with_mask else 1.0, ptr(dev(y)), c, t.ptr, c,
           n, h, h, c, seg_arr(segs), nseg, L.ACT['lrelu'], float(ALPHA), ptr(sums), 0, st())
    got_t = finish(t, (rows, c))
    assert_pointwise(got_t, t64, np.abs(t64), 3, "t")
    assert (got_t[t64 == 0] == 0).all()
    dx, db = guarded(rows * c), guarded(c)
    L.call('tg_mobn_center_f32', t.ptr, c, dx.ptr, c, rows, c, seg_arr(segs), nseg, ptr(sums), REPL, db.ptr, st())
    got_dx, got_db = finish(dx, (rows, c)), finish(db)
    check_column_sums(sums.cpu().numpy().sum(0), got_db, t64, segs, "maxpool2_bwd_actsum c=%d h=%d" % (c, h), drop=h)
    _, _, mean, mean_abs = seg_stats(t64, segs)
    assert_pointwise(got_dx, t64 - mean, np.abs(t64) + mean_abs, CHUNK - 1 + 5, "dx")


def actgrad_bias_case():
    rows, c = 300, 1000
    rng = np.random.default_rng(4000)
    dy = rng.standard_normal((rows, c)).astype(np.float32)
    y = y_for(rng, (rows, c), 'lrelu')
    return dy, y, f8(dy) * act_grad64(y, 'lrelu')[0]


def test_actgrad_bias_256_column_groups():
    """tg_actgrad_bias_f32 at (rows, c, ld_out) = (300, 1000, 1024): 256 column groups, one row lane, six of the groups all padding.  dpre
    pointwise with K = 1, zeroed padding; the bias gradient to the reduction bound."""
    L = lib()
    rows, c, ld = 300, 1000, 1024
    dy, y, t64 = actgrad_bias_case()
    out, bg = guarded(rows * ld), guarded(c)
    sums = dev(np.full((REPL, c), 5.0), np.float64)
    L.call('tg_actgrad_bias_f32', ptr(dev(dy)), c, ptr(dev(y)), c, out.ptr, ld, rows, c, L.ACT['lrelu'], float(ALPHA), ptr(sums), 0, bg.ptr, st())
    got = finish(out, (rows, ld))
    assert_pointwise(got[:, :c], t64, np.abs(t64), 1, "dpre")
    assert (bits(got[:, c:]) == 0).all()
    check_column_sums(sums.cpu().numpy().sum(0)[None], finish(bg), t64, [rows], "actgrad_bias")
