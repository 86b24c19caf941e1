"""tests/rng_reference.py without a GPU: the vectorised Philox block against the scalar known-answer block and the Random123 known answers,
the counter / key layout against the scalar block call by call, u01 in fp32 (its rounding above 2^23, the clamp, the committed edge
draw of tests/test_gpu_rng.py), and the header's range contract evaluated at the largest and smallest u."""
from fractions import Fraction

import numpy as np

import augment_reference as A
import rng_reference as R

# the committed draw whose element EDGE[4] comes from a word with x >> 8 == 0xFFFFFF (found by searching stream ids with edge_elements)
EDGE = (0x9E3779B97F4A7C15, (7 << 32) + 3, 12, 6157, 6153)        # seed, step, stream_id, n, element


def test_vectorised_block_meets_the_known_answers_and_the_scalar_block():
    for counter, key, want in A.PHILOX_KAT:
        assert tuple(int(v) for v in R.philox_blocks(*counter, key)[0]) == want
    rng = np.random.default_rng(5)
    c = rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64)
    c[0], c[1] = 0, A.M32
    key = (0xDEADBEEF, 0x00C0FFEE)
    got = R.philox_blocks(c[:, 0], c[:, 1], c[:, 2], c[:, 3], key)
    for row, g in zip(c, got):
        assert tuple(int(v) for v in g) == A.philox4x32_10(tuple(int(v) for v in row), key)
    # scalars broadcast against the block index
    got = R.philox_blocks(np.arange(5), 0, 9, 3, key)
    assert [tuple(int(v) for v in g) for g in got] == [A.philox4x32_10((i, 0, 9, 3), key) for i in range(5)]


def test_counter_and_key_layout():
    seed, step, sid = 0x0123456789ABCDEF, (0xFEDC << 32) + 0x1234, 77
    assert R.key_of(seed, step) == (0x89ABCDEF, 0x01234567 ^ 0xFEDC)
    w = R.words(10, seed, step, sid)
    assert w.shape == (3, 4)
    for i in range(3):
        assert tuple(int(v) for v in w[i]) == A.philox4x32_10((i, 0, sid, 0x1234), (0x89ABCDEF, 0x01234567 ^ 0xFEDC))
    # block indices beyond 32 bits carry into the second counter word
    w = R.words(4, seed, step, sid, first_block=(3 << 32) + 5)
    assert tuple(int(v) for v in w[0]) == A.philox4x32_10((5, 3, sid, 0x1234), (0x89ABCDEF, 0x01234567 ^ 0xFEDC))
    # stream id, step and seed each select a different stream; the high half of the step enters through the key only
    base = R.words(8, seed, step, sid)
    for other in (R.words(8, seed, step, sid + 1), R.words(8, seed, step + 1, sid), R.words(8, seed ^ 1, step, sid),
                  R.words(8, seed, step + (1 << 32), sid), R.words(8, seed ^ (1 << 32), step, sid)):
        assert (other != base).all()
    assert (R.words(8, seed ^ (1 << 40), step ^ (1 << 40), sid) == base).all()      # hi32(seed) ^ hi32(step) is all the key sees of them
    # one-hot: one block per row, counter (row, 0, stream, lo32(step)), class (word x * k) >> 32
    cls = R.onehot_classes(300, 10, seed, step, sid)
    for r in (0, 1, 299):
        x = A.philox4x32_10((r, 0, sid, 0x1234), R.key_of(seed, step))[0]
        assert cls[r] == (x * 10) >> 32
    oh = R.onehot(300, 10, seed, step, sid)
    assert (oh.sum(axis=1) == 1).all() and (oh.argmax(axis=1) == cls).all() and len(set(cls.tolist())) == 10


def test_u01_is_the_fp32_expression():
    x = np.array([0, 0xFF, 0x100, 0x7FFFFF00, 0x80000000, 0x80000100, 0xFFFFFD00, 0xFFFFFE00, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], np.uint32)
    raw, u = R.u01(x, clamp=False), R.u01(x)
    assert raw.dtype == u.dtype == np.float32
    k = (x >> 8).astype(np.int64)
    exact = [Fraction(2 * int(v) + 1, 1 << 25) for v in k]
    for v, r, e in zip(k, raw, exact):
        if v < (1 << 23):
            assert Fraction(float(r)) == e                                     # k + 0.5 representable: the exact midpoint of the bin
        else:
            assert Fraction(float(r)) == Fraction(int(v) + (int(v) & 1), 1 << 24)   # rounded to the even neighbour
    assert raw[-1] == raw[-2] == np.float32(1.0)                                # the finding: exactly 1.0 for x >> 8 == 0xFFFFFF
    assert u[-1] == u[-2] == R.U_MAX and R.U_MAX.view(np.uint32) == 0x3F7FFFFF and R.U_MAX < 1
    assert (u[:-2] == raw[:-2]).all()                                           # the clamp changes that one word value only
    assert u[0] == np.float32(2.0 ** -25) and (u > 0).all() and (u < 1).all()
    # all 2^24 values of x >> 8: only the last differs, all lie in (0, 1)
    allk = (np.arange(1 << 24, dtype=np.uint64) << np.uint64(8)).astype(np.uint32)
    raw, u = R.u01(allk, clamp=False), R.u01(allk)
    assert np.flatnonzero(raw != u).tolist() == [R.EDGE_WORD]
    assert u.min() == np.float32(2.0 ** -25) and u.max() == R.U_MAX and (np.diff(u) >= 0).all()


def test_the_committed_edge_draw_has_the_word():
    seed, step, sid, n, e = EDGE
    assert e < n and n % 4
    blk = A.philox4x32_10((e // 4, 0, sid, step & A.M32), R.key_of(seed, step))
    assert blk[e % 4] >> 8 == R.EDGE_WORD
    assert R.edge_elements(n, seed, step, sid).tolist() == [e]
    before, after = R.uniform(n, -1.0, 1.0, seed, step, sid, clamp=False), R.uniform(n, -1.0, 1.0, seed, step, sid)
    assert before[e] == np.float32(1.0) and after[e] < 1 and np.flatnonzero(before != after).tolist() == [e]
    before, after = R.uniform(n, 0.0, 1.0, seed, step, sid, clamp=False), R.uniform(n, 0.0, 1.0, seed, step, sid)
    assert before[e] == np.float32(1.0) and after[e] == R.U_MAX and np.flatnonzero(before != after).tolist() == [e]


def _uniform_of(u, lo, hi):
    lo, hi = np.float32(lo), np.float32(hi)
    return np.float32(lo + np.float32(np.float32(hi - lo) * np.float32(u)))


def test_range_contract_at_the_extreme_u():
    """include/tg_kernels.h: uniform draws lie in [lo, hi) for (-1, 1) and (0, 1) — the largest u gives a value below hi, the smallest one a
    value >= lo — while for a general range the fp32 rounding of lo + (hi - lo) u can still return hi itself."""
    u_min = np.float32(2.0 ** -25)
    for lo, hi in ((-1.0, 1.0), (0.0, 1.0)):
        assert lo <= _uniform_of(u_min, lo, hi) and _uniform_of(R.U_MAX, lo, hi) < hi
    assert _uniform_of(R.U_MAX, -1.0, 1.0) == np.float32(1.0) - np.float32(2.0 ** -23)
    assert _uniform_of(np.float32(1.0), -1.0, 1.0) == 1.0 and _uniform_of(np.float32(1.0), 0.0, 1.0) == 1.0      # what the clamp removes
    assert _uniform_of(R.U_MAX, 2.0, 5.0) == np.float32(5.0)                    # a general range: hi is reachable, as the header now says
    # keep-mask: u < p; p = 1 keeps everything only with the clamp
    assert (np.float32(1.0) < np.float32(1.0)) == False and R.U_MAX < np.float32(1.0)


def test_modes_share_the_words_in_order():
    seed, step, sid, n = 3, 9, 4, 11
    u = R.u01(R.words(n, seed, step, sid)).reshape(-1)[:n]
    assert (R.uniform(n, 0.0, 1.0, seed, step, sid) == u).all()
    assert (R.keep_mask(n, 0.5, seed, step, sid) == (u < 0.5)).all()
    v, mag = R.normal64(n, 2.0, seed, step, sid)
    assert v.shape == mag.shape == (n,)
    u64 = u.astype(np.float64)
    assert v[0] == 2.0 * np.sqrt(-2 * np.log(u64[0])) * np.cos(2 * np.pi * u64[1])
    assert v[7] == 2.0 * np.sqrt(-2 * np.log(u64[6])) * np.sin(2 * np.pi * u64[7])
    assert mag[5] == 2.0 * np.sqrt(-2 * np.log(u64[4]))
    # the normal draw runs on the unclamped u: a radius word of exactly 1.0 gives the pair (0, 0), an angle word of 1.0 the angle 2 pi
    seed_e, step_e, sid_e, n_e, e = EDGE
    ve, me = R.normal64(n_e, 1.0, seed_e, step_e, sid_e)
    ue = R.u01(R.words(n_e, seed_e, step_e, sid_e), clamp=False).reshape(-1).astype(np.float64)
    assert ue[e] == 1.0 and e % 2 == 1 and ve[e] == me[e] * np.sin(2 * np.pi) and ve[e - 1] == me[e]
    assert R.normal64(4, 1.0, seed, step, sid)[1].min() > 0 and np.sqrt(-2.0 * np.log(np.float64(1.0))) == 0
    sw, _ = R.normal64(n, 2.0, seed, step, sid, swap_sincos=True)
    assert sw[1] == v[0] and sw[0] == v[1]
    sp, _ = R.normal64(8, 2.0, seed, step, sid, swap_pairs=True)
    assert (sp[[2, 3, 0, 1]] == v[:4]).all()
