"""tg_poly3_sums_f32 (csrc/kernel_distance.hip) held to its float64 restatement tests/kernel_distance_reference.py: against the reference
within sum_bound at shapes ragged differently in rows and columns (NaN padding columns, guard words behind the output and the workspace, a
dirty workspace), bit for bit on integer data where every quantity is exactly representable — one segment, the self case without its
diagonal, and a segment table with unaligned offsets — reproducibility across runs and streams, and the refusal of every bad argument
before any launch.  Only the masks (ragged tails, segment ends, the diagonal) see the f64 MFMA's C/D layout, so the exact cases are built
around them: a wrong map drops the wrong elements, whose values differ from their neighbours'."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_distance_reference as R
from kernel_check import guarded, lib, ptr, st

pytestmark = pytest.mark.gpu

INVALID = -1                     # TG_ERR_INVALID


def seg32(offsets):
    return (C.c_int32 * len(offsets))(*[int(v) for v in offsets])


class Out64(object):
    """`n` doubles inside a guarded float allocation: NaN before the launch, pattern words behind."""

    def __init__(self, n):
        self.n = int(n)
        self.g = guarded(2 * self.n)
        assert self.g.t.data_ptr() % 8 == 0

    @property
    def ptr(self):
        return self.g.ptr

    def get(self):
        self.g.check_guard()
        return self.g.get().view(np.float64).copy()

    def untouched(self):
        self.g.check_guard()
        return bool(np.isnan(self.g.get()).all())


class Work(object):
    """a workspace of exactly `need` bytes (a multiple of 8), dirty (NaN words), with pattern words behind it."""

    def __init__(self, need):
        assert need % 8 == 0
        self.bytes = int(need)
        self.g = guarded(self.bytes // 4)
        assert self.g.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.g.ptr

    def check(self):
        self.g.check_guard()

    def untouched(self):
        self.g.check_guard()
        return bool(np.isnan(self.g.get()).all())


def run(a, b, c, seg_a, seg_b, exclude_diag, stream=None):
    """a, b: host [rows, ld] float32 (padding columns included) -> float64 [nseg] of the kernel, guards checked."""
    L = lib()
    nseg = len(seg_a) - 1
    sa, sb = seg32(seg_a), seg32(seg_b)
    need = L.call('tg_poly3_sums_workspace_bytes', sa, sb, nseg)
    assert need > 0
    out, work = Out64(nseg), Work(need)
    da, db = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
    torch.cuda.synchronize()
    L.call('tg_poly3_sums_f32', ptr(da), a.shape[1], ptr(db), b.shape[1], c, sa, sb, nseg, int(exclude_diag), out.ptr, work.ptr, work.bytes,
           st() if stream is None else C.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize()
    work.check()
    return out.get()


inputs = R.inputs


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%dx%d_ld%d" % s)
def test_against_the_reference_within_the_bound(shape):
    m, n, c, ld = shape
    a, b = inputs(shape)
    ref, tol = R.poly3_sums(a, b, [0, m], [0, n]), R.sum_bound(a, b, [0, m], [0, n])
    got = run(R.padded(a, ld), R.padded(b, ld), c, [0, m], [0, n], False)
    err = np.abs(got - ref)
    print("poly3 %r: got %.17g ref %.17g err %.3g bound %.3g" % (shape, got[0], ref[0], err[0], tol[0]))
    assert np.isfinite(got).all() and (err <= tol).all(), (shape, got, ref, err, tol)
    # the self case of the same rows, without the diagonal, and a table that splits the rows unevenly
    ref_s, tol_s = R.poly3_sums(a, a, [0, m], [0, m], True), R.sum_bound(a, a, [0, m], [0, m], True)
    got_s = run(R.padded(a, ld), R.padded(a, ld), c, [0, m], [0, m], True)
    assert (np.abs(got_s - ref_s) <= tol_s).all(), (shape, got_s, ref_s, tol_s)
    sa, sb = [0, m // 3, m // 3, m], [0, n // 2, n // 2, n]
    ref_t, tol_t = R.poly3_sums(a, b, sa, sb), R.sum_bound(a, b, sa, sb)
    got_t = run(R.padded(a, ld), R.padded(b, ld), c, sa, sb, False)
    assert (np.abs(got_t - ref_t) <= tol_t).all() and got_t[1] == 0.0, (shape, got_t, ref_t, tol_t)


def integers(rng, rows, c):
    return rng.integers(-4, 5, (rows, c)).astype(np.float32)


def assert_exact(got, ref, what):
    assert got.dtype == np.float64 and (got.view(np.int64) == np.asarray(ref, np.float64).view(np.int64)).all(), (what, got, ref)


@pytest.mark.parametrize("c", (4, 32))
def test_integer_data_is_exact_with_one_segment(c):
    rng = np.random.default_rng(50 + c)
    for m, n in ((1, 1), (37, 91), (130, 67), (193, 129)):
        a, b = integers(rng, m, c), integers(rng, n, c)
        ref = R.poly3_sums(a, b, [0, m], [0, n])
        assert_exact(run(R.padded(a, c + 3), R.padded(b, c + 1), c, [0, m], [0, n], False), ref, (m, n, c))


@pytest.mark.parametrize("c", (4, 32))
def test_integer_data_is_exact_without_the_diagonal(c):
    """a == b: the diagonal values |x|^2 / c + 1 differ from their neighbours, so dropping any other element changes the sum."""
    rng = np.random.default_rng(60 + c)
    for m in (2, 17, 64, 83, 150):
        a = integers(rng, m, c)
        ref = R.poly3_sums(a, a, [0, m], [0, m], True)
        full = R.poly3_sums(a, a, [0, m], [0, m], False)
        assert ref[0] != full[0]
        pa = R.padded(a, c + 5)
        assert_exact(run(pa, pa, c, [0, m], [0, m], True), ref, ('diag', m, c))
        assert_exact(run(pa, pa, c, [0, m], [0, m], False), full, ('full', m, c))
    # the diagonal of a segment that starts at different rows on the two sides: local indices, not row numbers
    a, b = integers(rng, 90, c), integers(rng, 120, c)
    sa, sb = [3, 80], [40, 117]
    assert_exact(run(R.padded(a, c), R.padded(b, c + 2), c, sa, sb, True), R.poly3_sums(a, b, sa, sb, True), ('offset diag', c))


@pytest.mark.parametrize("c", (4, 32))
def test_integer_data_is_exact_per_segment(c):
    """offsets that are no multiple of the tile, an empty segment, a 1-row segment, a segment crossing several tiles, rows in front of the
    first and behind the last segment that belong to none."""
    rng = np.random.default_rng(70 + c)
    a, b = integers(rng, 400, c), integers(rng, 350, c)
    sa = [5, 5, 6, 75, 270, 270, 397]
    sb = [0, 9, 10, 10, 141, 200, 349]
    for diag in (False, True):
        ref = R.poly3_sums(a, b, sa, sb, diag)
        got = run(R.padded(a, c + 4), R.padded(b, c + 7), c, sa, sb, diag)
        assert_exact(got, ref, ('segments', c, diag))
        assert got[0] == 0.0 and got[2] == 0.0 and got[4] == 0.0          # empty on one side or both


def test_two_runs_and_a_second_stream_give_the_same_bits():
    shape = R.SHAPES[3]
    m, n, c, ld = shape
    a, b = inputs(shape)
    sa, sb = [0, 100, 100, m], [0, 1, 64, n]
    pa, pb = R.padded(a, ld), R.padded(b, ld)
    first = run(pa, pb, c, sa, sb, False)
    assert_exact(run(pa, pb, c, sa, sb, False), first, 'second run')
    side = torch.cuda.Stream()
    assert_exact(run(pa, pb, c, sa, sb, False, stream=side), first, 'second stream')


def test_bad_arguments_are_refused_before_any_launch():
    L = lib()
    raw = L.load()
    m, n, c = 70, 40, 6
    rng = np.random.default_rng(9)
    da, db = torch.from_numpy(R.features(rng, m, c)).cuda(), torch.from_numpy(R.features(rng, n, c)).cuda()
    sa, sb = seg32([0, 30, m]), seg32([0, 10, n])
    need = L.call('tg_poly3_sums_workspace_bytes', sa, sb, 2)
    good = dict(a=ptr(da), ld_a=c, b=ptr(db), ld_b=c, c=c, seg_a=sa, seg_b=sb, nseg=2, exclude_diag=0, workspace_bytes=need)
    bad = [dict(a=None), dict(b=None), dict(seg_a=None), dict(seg_b=None), dict(out=None), dict(workspace=None),
           dict(seg_a=seg32([0, 50, 40])), dict(seg_b=seg32([0, 30, 20])), dict(seg_a=seg32([-1, 30, m])),
           dict(exclude_diag=2), dict(exclude_diag=-1), dict(workspace_bytes=need - 8), dict(workspace_bytes=0),
           dict(c=0), dict(c=513, ld_a=600, ld_b=600), dict(ld_a=c - 1), dict(ld_b=c - 1), dict(nseg=0), dict(nseg=1025)]
    for change in bad:
        out, work = Out64(2), Work(need)
        kw = dict(good, out=out.ptr, workspace=work.ptr)
        kw.update(change)
        torch.cuda.synchronize()
        rc = raw.tg_poly3_sums_f32(kw['a'], kw['ld_a'], kw['b'], kw['ld_b'], kw['c'], kw['seg_a'], kw['seg_b'], kw['nseg'], kw['exclude_diag'],
                                   kw['out'], kw['workspace'], kw['workspace_bytes'], st())
        torch.cuda.synchronize()
        assert rc == INVALID, (change, rc)
        assert out.untouched() and work.untouched(), change
    for sa_bad, sb_bad, nseg in ((seg32([0, 5, 3]), sb, 2), (sa, seg32([4, 2, 9]), 2), (None, sb, 2), (sa, None, 2), (sa, sb, 0), (sa, sb, 1025)):
        assert raw.tg_poly3_sums_workspace_bytes(sa_bad, sb_bad, nseg) < 0
        with pytest.raises(L.TgError):
            L.call('tg_poly3_sums_workspace_bytes', sa_bad, sb_bad, nseg)
    # and the good call still runs
    out, work = Out64(2), Work(need)
    L.call('tg_poly3_sums_f32', good['a'], c, good['b'], c, c, sa, sb, 2, 0, out.ptr, work.ptr, need, st())
    torch.cuda.synchronize()
    work.check()
    ha, hb = da.cpu().numpy(), db.cpu().numpy()
    ref, tol = R.poly3_sums(ha, hb, [0, 30, m], [0, 10, n]), R.sum_bound(ha, hb, [0, 30, m], [0, 10, n])
    assert (np.abs(out.get() - ref) <= tol).all()
