"""csrc/rng.hip drawn value by drawn value against tests/rng_reference.py (Philox4x32-10 on the known-answer block of
tests/augment_reference.py): a wrong counter word, a swapped key half, a grid-stride pass that repeats a block or a changed word order
inside a block of four fails here, where the statistical tests of tests/test_gpu_kernels.py cannot see it.

Tolerance classes (tests/kernel_check.py):
  bit-exact  tg_rng_keep_mask_f32, tg_rng_onehot_f32, tg_rng_uniform_f32 and the same modes of tg_rng_multi_f32.  The uniform expression
             lo + (hi - lo) * u is NOT contracted: csrc/Makefile builds with -ffp-contract=off and rng.hip's code object multiplies
             (v_pk_mul_f32) and then adds (v_pk_add_f32), so the reference rounds the difference, the product and the sum to fp32 one by
             one, for the whole array (no per-element choice between a fused and an unfused form);
  pointwise  tg_rng_normal_f32 against float64 Box-Muller on the same fp32 u, |got - ref| <= K_NORMAL u stddev r, r = sqrt(-2 ln u0)
             the radius of the element's pair (the angle's error is absolute, so the bound is relative to the radius, not to |sin|).

K_NORMAL = 32, to first order in u = 2^-24, from  v = (stddev * r) * c,  r = sqrtf(-2 logf(u0)),  c = cos or sin of fl(fl(2 pi) * u1):
   3     logf within 3 ulp = 6 u of ln u0; the factor -2 is exact; the square root halves a relative error
   6     sqrtf within 3 ulp
  12.57  the angle: fl(2 pi) is within u of 2 pi and the product is rounded once, so |dt| <= 2 u t <= 4 pi u, and |d sin|, |d cos| <= |dt|
   8     sincosf within 4 ulp of a value of magnitude <= 1
   2     the two fp32 products stddev * r and (stddev * r) * c
  -----
  31.57  (the ulp bounds are those of the OpenCL full profile, which the ROCm device library implements; a correctly rounded sqrtf, as
         the default build gives, lowers the sum to 26.6)
Worst measured ratio |err| / (u stddev r): 7.35 (MI355X, ROCm's device library, 2026-10-16; stddev 0.15, 2097157 elements; every
run prints its own figure as "normal: worst ... u"), well inside the derived bound; the references of the negative controls (sine and
cosine exchanged, the word pairs exchanged) are off by far more than 10 K.

The committed EDGE draw (tests/test_rng_reference.py proves the word is there) holds the one word value, x >> 8 == 0xFFFFFF, for which
u01 is exactly 1.0.  The uniform and keep-mask draws clamp it to 1 - 2^-24: test_uniform_stays_below_hi_at_the_u01_edge states the header's
[lo, hi) contract on it.  The normal draw is left on the unclamped value (radius 0 or angle 2 pi: both harmless), because the noise of every
seeded training run comes from it and a clamp there would move those runs; the reference restates exactly that split."""
import ctypes as C

import numpy as np
import pytest
import torch

import rng_reference as R
from kernel_check import U, assert_bits, assert_pointwise, finish, guarded, lib, ptr, st
from test_rng_reference import EDGE

pytestmark = pytest.mark.gpu

K_NORMAL = 32
SEED, STEP = 0x9E3779B97F4A7C15, (7 << 32) + 3          # both with bits above 32: the key is (lo32(seed), hi32(seed) ^ hi32(step))
GRID = 2048 * 256 * 4                                   # elements of one pass of the capped grid (2048 workgroups x 256 threads x 4 words)
SIZES = [(1, 0), (3, 0), (4, 0), (5, 0), (5, 1), (GRID - 5, 0), (GRID + 5, 0), (GRID + 5, 1)]      # (n, float offset of the output)
SIZE_IDS = ["n%d+%d" % s for s in SIZES]


def _state(seed, step):
    return torch.from_numpy(np.array([seed, step], np.uint64).view(np.int64).copy()).cuda()


def _ratio(got, ref64, mag):
    return float((np.abs(np.asarray(got, np.float64) - ref64) / (U * mag)).max())


def _check_normal(got, n, stddev, seed, step, sid, what):
    ref, mag = R.normal64(n, stddev, seed, step, sid)
    live = mag > 0                                    # a radius word of exactly 1.0 gives r = 0: assert_pointwise then asks for exactly 0
    print("normal: worst %.2f u of stddev * r (%s, K = %d)" % (_ratio(got[live], ref[live], mag[live]), what, K_NORMAL))
    assert_pointwise(got, ref, mag, K_NORMAL, what)
    if n >= 2:
        for kw in ({'swap_sincos': True}, {'swap_pairs': True}):
            if n < 4 and 'swap_pairs' in kw:
                continue
            wrong, _ = R.normal64(n, stddev, seed, step, sid, **kw)
            assert _ratio(got[live], wrong[live], mag[live]) > 10 * K_NORMAL, "%s: the bound accepts the reference with %s" % (what, kw)


@pytest.mark.parametrize("n,off", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("lo,hi,sid", [(-1.0, 1.0, 1), (0.0, 1.0, 12), (2.0, 5.0, 0xFFFFFFFF)])
def test_uniform_bits(lo, hi, sid, n, off):
    L = lib()
    state = _state(SEED, STEP)
    g = guarded(n, offset=off)
    L.call('tg_rng_uniform_f32', g.ptr, n, lo, hi, ptr(state), sid, st())
    got = finish(g)
    assert_bits(got, R.uniform(n, lo, hi, SEED, STEP, sid), "uniform(%g, %g) n %d stream %d" % (lo, hi, n, sid))
    assert (state.cpu().numpy().view(np.uint64) == [SEED, STEP]).all()


def test_two_stream_ids_are_the_references_two_streams():
    L = lib()
    state = _state(SEED, STEP)
    n = 4099
    a, b = guarded(n), guarded(n)
    L.call('tg_rng_uniform_f32', a.ptr, n, -1.0, 1.0, ptr(state), 1, st())
    L.call('tg_rng_uniform_f32', b.ptr, n, -1.0, 1.0, ptr(state), 2, st())
    ga, gb = finish(a), finish(b)
    ra, rb = R.uniform(n, -1.0, 1.0, SEED, STEP, 1), R.uniform(n, -1.0, 1.0, SEED, STEP, 2)
    assert (ra != rb).mean() > 0.99
    assert_bits(ga, ra, "stream 1")
    assert_bits(gb, rb, "stream 2")
    # a seed / step without high bits, and the high halves entering only as their exclusive or
    for seed, step in ((5, 9), (SEED ^ (1 << 40), STEP ^ (1 << 40))):
        s2 = _state(seed, step)
        c = guarded(n)
        L.call('tg_rng_uniform_f32', c.ptr, n, -1.0, 1.0, ptr(s2), 1, st())
        assert_bits(finish(c), R.uniform(n, -1.0, 1.0, seed, step, 1), "seed %x step %x" % (seed, step))


@pytest.mark.parametrize("n,off", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("p", [0.8, 0.5])
def test_keep_mask_bits(p, n, off):
    L = lib()
    state = _state(SEED, STEP)
    g = guarded(n, offset=off)
    L.call('tg_rng_keep_mask_f32', g.ptr, n, p, ptr(state), 3, st())
    assert_bits(finish(g), R.keep_mask(n, p, SEED, STEP, 3), "keep_mask(%g) n %d" % (p, n))


@pytest.mark.parametrize("n,off", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("stddev", [0.15, 1.0])
def test_normal_pointwise(stddev, n, off):
    L = lib()
    state = _state(SEED, STEP)
    g = guarded(n, offset=off)
    L.call('tg_rng_normal_f32', g.ptr, n, stddev, ptr(state), 4, st())
    _check_normal(finish(g), n, stddev, SEED, STEP, 4, "normal(%g) n %d" % (stddev, n))


def test_onehot_bits():
    L = lib()
    state = _state(SEED, STEP)
    for rows in (1, 127, 128, 129, 1000):
        for k in (2, 10, 100, 1024):
            g = guarded(rows * k, offset=1 if rows == 129 else 0)
            L.call('tg_rng_onehot_f32', g.ptr, rows, k, ptr(state), 5, st())
            assert_bits(finish(g, (rows, k)), R.onehot(rows, k, SEED, STEP, 5), "onehot rows %d k %d" % (rows, k))


@pytest.mark.parametrize("step", [STEP, (7 << 32) + 0xFFFFFFFF], ids=["step", "carry"])
def test_advance_moves_the_step_alone(step):
    """state[1] + 1 (a carry into the high half changes the key), state[0] untouched, the next draws are the reference's at step + 1."""
    L = lib()
    state = _state(SEED, step)
    L.call('tg_rng_advance', ptr(state), st())
    torch.cuda.synchronize()
    assert state.cpu().numpy().view(np.uint64).tolist() == [SEED, step + 1]
    n = 1027
    g, m = guarded(n), guarded(40 * 10)
    L.call('tg_rng_uniform_f32', g.ptr, n, -1.0, 1.0, ptr(state), 1, st())
    L.call('tg_rng_onehot_f32', m.ptr, 40, 10, ptr(state), 5, st())
    got = finish(g)
    assert_bits(got, R.uniform(n, -1.0, 1.0, SEED, step + 1, 1), "uniform after advance")
    assert (bits_differ(got, R.uniform(n, -1.0, 1.0, SEED, step, 1))) > 0.99
    assert_bits(finish(m, (40, 10)), R.onehot(40, 10, SEED, step + 1, 5), "onehot after advance")


def bits_differ(a, b):
    return float((np.asarray(a, np.float32).view(np.int32) != np.asarray(b, np.float32).view(np.int32)).mean())


def test_multi_launch_mixing_the_modes():
    """one tg_rng_multi_f32 launch: every mode, sizes around the block of four and past one grid pass, an unaligned output."""
    L = lib()
    state = _state(SEED, STEP)
    specs = [(0, 1, -1.0, 1.0, 0), (1, 5, 0.7, 0.0, 1), (2, 7, 0.15, 0.0, 0), (3, 129, 10.0, 0.0, 0), (0, GRID + 5, -1.0, 1.0, 1), (2, GRID + 5, 1.0, 0.0, 0),
             (1, 4099, 0.5, 0.0, 0), (3, 1, 2.0, 0.0, 1), (0, 9, 2.0, 5.0, 0), (3, 1000, 100.0, 0.0, 0), (2, 3, 2.0, 0.0, 1), (0, 4, 0.0, 1.0, 0)]
    jobs = (L.RngJob * len(specs))()
    outs = []
    for i, (mode, n, a, b, off) in enumerate(specs):
        o = guarded(n * int(a) if mode == 3 else n, offset=off)
        outs.append(o)
        jobs[i] = L.RngJob(o.t.data_ptr(), n, mode, a, b, 200 + i)
    L.call('tg_rng_multi_f32', C.cast(jobs, C.c_void_p), len(specs), ptr(state), st())
    for i, (mode, n, a, b, off) in enumerate(specs):
        what, sid = "job %d (mode %d, n %d)" % (i, mode, n), 200 + i
        if mode == 0:
            assert_bits(finish(outs[i]), R.uniform(n, a, b, SEED, STEP, sid), what)
        elif mode == 1:
            assert_bits(finish(outs[i]), R.keep_mask(n, a, SEED, STEP, sid), what)
        elif mode == 2:
            _check_normal(finish(outs[i]), n, a, SEED, STEP, sid, what)
        else:
            assert_bits(finish(outs[i], (n, int(a))), R.onehot(n, int(a), SEED, STEP, sid), what)


def test_uniform_stays_below_hi_at_the_u01_edge():
    """include/tg_kernels.h: uniform in [lo, hi) for (-1, 1) and (0, 1).  Element EDGE[4] of this draw comes from the word with
    x >> 8 == 0xFFFFFF: before the clamp in u01 it was exactly hi.  Every other element is what it was before the clamp (the reference
    without the clamp differs at that element alone)."""
    L = lib()
    seed, step, sid, n, e = EDGE
    state = _state(seed, step)
    for lo, hi in ((-1.0, 1.0), (0.0, 1.0)):
        g = guarded(n)
        L.call('tg_rng_uniform_f32', g.ptr, n, lo, hi, ptr(state), sid, st())
        got = finish(g)
        before = R.uniform(n, lo, hi, seed, step, sid, clamp=False)
        assert before[e] == np.float32(hi)
        assert got[e] != np.float32(hi), "element %d of uniform(%g, %g) is exactly hi = %r" % (e, lo, hi, got[e])
        assert (got >= lo).all() and (got < hi).all()
        assert_bits(got, R.uniform(n, lo, hi, seed, step, sid), "uniform(%g, %g) at the edge draw" % (lo, hi))
        keep = np.arange(n) != e
        assert_bits(got[keep], before[keep], "every other element")
    # a keep probability of 1 keeps everything (u < 1), and the normal draw of that word (unclamped there) is finite and within its bound
    g = guarded(n)
    L.call('tg_rng_keep_mask_f32', g.ptr, n, 1.0, ptr(state), sid, st())
    assert (finish(g) == 1).all()
    g = guarded(n)
    L.call('tg_rng_normal_f32', g.ptr, n, 1.0, ptr(state), sid, st())
    _check_normal(finish(g), n, 1.0, seed, step, sid, "normal at the edge draw")
