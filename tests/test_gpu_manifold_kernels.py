"""tg_knn_self_f32 and tg_manifold_query_f32 (include/tg_kernels.h, csrc/knn.hip) against tests/manifold_reference.py.

Everything is exact.  The distance is a fixed fp32 chain (one accumulator, ascending channels, subtract / multiply / add each rounded,
no contraction) which NumPy restates operation for operation, so out_d2 and nn_d2 are compared BIT FOR BIT and count and nn_idx for
equality; there is no tolerance to state.  (That the chain itself is within (c + 3) 2^-24 of float64 is tests/
test_manifold_reference.py, on these same shapes, without a device.)

Shapes (n reference rows, m query rows, c, ld, k): the minimum; below one 64 x 64 tile; k = n - 1; no multiple of any tile with several
reference ranges and a ragged channel chunk; whole tiles; the trainer's feature width with padding columns.  Every padding column holds
NaN — one read of it would poison an output — and every output and workspace is followed by guard words."""
import numpy as np
import pytest
import torch

import manifold_reference as R
from kernel_check import assert_bits, guarded, lib, ptr, st

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 1, 1, 1), (5, 7, 3, 8, 1), (17, 4, 5, 8, 16), (257, 130, 33, 40, 3), (64, 64, 128, 128, 5), (1000, 777, 128, 160, 3)]
TG_ERR_INVALID = -1
FILL = 0x0BADF00D                # what an int32 output holds before a launch
_DATA = {}


def data(n, m, c, ld, k):
    """per shape, made once and left unchanged: (r [n, ld], q [m, ld]) with NaN padding, and the reference's outputs on columns 0..c-1."""
    key = (n, m, c, ld, k)
    if key not in _DATA:
        r, q = R.features(n, c, ld, 100 * n + c), R.features(m, c, ld, 100 * m + c + 7)
        r.setflags(write=False), q.setflags(write=False)
        knn = R.knn_self(r[:, :c], k)
        r2 = np.ascontiguousarray(knn[:, k - 1])
        _DATA[key] = (r, q, knn, r2, R.query(q[:, :c], r[:, :c], r2))
    return _DATA[key]


def int_out(n):
    """a guarded output of n int32 holding FILL, and its int32 view."""
    g = guarded(n, fill=np.full(n, FILL, np.int32).view(np.float32))
    return g, g.t.view(torch.int32)


def ints(g):
    return g.get().view(np.int32)


def workspace(name, *shape, dirty=False):
    need = lib().call(name, *shape)
    assert need > 0 and need % 4 == 0
    return guarded(need // 4, fill=np.full(need // 4, 1e30, np.float32) if dirty else None), need


def run_self(x, c, k, dirty=False):
    """tg_knn_self_f32 on the host matrix x [n, ld] on the current stream -> out_d2 [n, k], guards checked."""
    n, ld = x.shape
    out = guarded(n * k)
    gw, need = workspace('tg_knn_self_workspace_bytes', n, k, dirty=dirty)
    lib().call('tg_knn_self_f32', ptr(torch.from_numpy(np.array(x)).cuda()), ld, n, c, k, out.ptr, gw.ptr, need, st())
    for g in (out, gw):
        g.check_guard()
    return out.get((n, k))


def run_query(q, r, c, r2, dirty=False, count=True):
    """tg_manifold_query_f32 on host matrices q [m, ld_q], r [n, ld_r] -> (count int32 [m], nn_d2 [m], nn_idx int32 [m]), guards checked."""
    (m, ld_q), (n, ld_r) = q.shape, r.shape
    (gc, _), nn, (gi, _) = int_out(m), guarded(m), int_out(m)
    gw, need = workspace('tg_manifold_query_workspace_bytes', m, n, dirty=dirty)
    r2d = None if r2 is None else torch.from_numpy(np.ascontiguousarray(r2, np.float32)).cuda()
    lib().call('tg_manifold_query_f32', ptr(torch.from_numpy(np.array(q)).cuda()), ld_q, m, ptr(torch.from_numpy(np.array(r)).cuda()), ld_r, n, c,
               ptr(r2d), gc.ptr if count else None, nn.ptr, gi.ptr, gw.ptr, need, st())
    for g in (gc, nn, gi, gw):
        g.check_guard()
    return ints(gc), nn.get(), ints(gi)


@pytest.mark.parametrize("n,m,c,ld,k", SHAPES)
def test_outputs_are_the_reference_chain_bit_for_bit(n, m, c, ld, k):
    r, q, knn_ref, r2, (count_ref, nn_ref, idx_ref) = data(n, m, c, ld, k)
    knn = run_self(r, c, k)
    assert np.isfinite(knn).all()                                      # written everywhere, and no padding column (NaN) was read
    assert_bits(knn, knn_ref, "out_d2")
    assert (np.diff(knn, axis=1) >= 0).all()
    count, nn, idx = run_query(q, r, c, r2)
    assert_bits(nn, nn_ref, "nn_d2")
    assert (idx == idx_ref).all() and (count == count_ref).all()
    assert 0 <= idx.min() and idx.max() < n and 0 <= count.min() and count.max() <= n


def test_ties_duplicates_and_exclusion_by_index():
    """every row twice, the twins 35 rows apart (so in different 64-row tiles for some, in the same for others): the nearest other row is
    the twin at distance 0 — leaving a row out by VALUE would lose it — and a query that equals both twins reports the lower index."""
    c, ld = 3, 4
    base = R.features(35, c, ld, 11)
    x = np.concatenate([base, base])
    knn = run_self(x, c, 2)
    assert_bits(knn, R.knn_self(x[:, :c], 2), "out_d2 with twins")
    assert (knn[:, 0] == 0).all() and (knn[:, 1] > 0).all()
    r2 = np.ascontiguousarray(knn[:, 0])                               # radius 0: a ball holds exactly the points at distance 0
    count, nn, idx = run_query(base, x, c, r2)
    assert (nn == 0).all() and (idx == np.arange(35)).all() and (count == 2).all()
    # five identical rows: each has four neighbours at distance 0
    same = np.repeat(R.features(1, c, ld, 12), 5, axis=0)
    assert (run_self(same, c, 4) == 0).all()
    # twins in different reference ranges (n = 257 is cut into five): the lower index wins across the merge too
    r, q, _, _, _ = data(257, 130, 33, 40, 3)
    r = np.array(r)
    r[200] = r[3]
    r[256] = r[3]
    count, nn, idx = run_query(r[[3, 200, 256]], r, 33, None, count=False)
    assert (nn == 0).all() and (idx == 3).all()
    knn = run_self(r, 33, 3)
    assert_bits(knn, R.knn_self(r[:, :33], 3), "out_d2 with twins across ranges")
    assert (knn[[3, 200, 256], :2] == 0).all() and (knn[[3, 200, 256], 2] > 0).all()


@pytest.mark.parametrize("n,m,c,ld,k", [(5, 7, 3, 8, 1), (257, 130, 33, 40, 3)])
def test_without_radii_count_keeps_its_prior_fill(n, m, c, ld, k):
    r, q, _, _, (_, nn_ref, idx_ref) = data(n, m, c, ld, k)
    count, nn, idx = run_query(q, r, c, None)
    assert (count == FILL).all()
    assert_bits(nn, nn_ref, "nn_d2")
    assert (idx == idx_ref).all()
    _, nn2, idx2 = run_query(q, r, c, None, count=False)               # and the pointer may be null then
    assert_bits(nn2, nn_ref, "nn_d2")
    assert (idx2 == idx_ref).all()


@pytest.mark.parametrize("n,m,c,ld,k", [(257, 130, 33, 40, 3), (1000, 777, 128, 160, 3)])
def test_a_second_run_and_another_stream_give_the_same_bits(n, m, c, ld, k):
    """the workspace needs no initialisation and the result does not depend on the stream."""
    r, q, knn_ref, r2, (count_ref, nn_ref, idx_ref) = data(n, m, c, ld, k)
    assert_bits(run_self(r, c, k, dirty=True), knn_ref, "second run")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        knn = run_self(r, c, k, dirty=True)
        count, nn, idx = run_query(q, r, c, r2, dirty=True)
    side.synchronize()
    assert_bits(knn, knn_ref, "other stream")
    assert_bits(nn, nn_ref, "other stream")
    assert (count == count_ref).all() and (idx == idx_ref).all()


def test_bad_arguments_are_refused_before_any_launch():
    """every case breaks ONE rule — the buffers are large enough for each case's other arguments and the workspace size handed in is
    generous except where it is the rule under test — and the message is the one of that rule's check."""
    L = lib()
    h = L.load()
    n, m, c, ld, k = 17, 4, 5, 8, 3
    x = torch.zeros(32 * 600, dtype=torch.float32, device='cuda')      # 32 rows of up to 600 columns
    qd = torch.zeros(m * 600, dtype=torch.float32, device='cuda')
    r2 = torch.ones(n, dtype=torch.float32, device='cuda')
    out = guarded(32 * 17)
    ws, roomy = guarded(4096), 4096 * 4
    need_s = L.call('tg_knn_self_workspace_bytes', n, k)
    assert need_s < roomy and L.call('tg_knn_self_workspace_bytes', 20, 16) < roomy
    self_call = lambda xp, ld_, n_, c_, k_, op, wp, nbytes: h.tg_knn_self_f32(xp, ld_, n_, c_, k_, op, wp, nbytes, st())
    good = (ptr(x), ld, n, c, k, out.ptr, ws.ptr, roomy)
    bad_self = {
        'c = 0': (dict(c=0), b"c must be in 1..512"), 'c = 513': (dict(c=513, ld=600), b"c must be in 1..512"),
        'k = 0': (dict(k=0), b"k must be in 1..16"), 'k = 17': (dict(k=17, n=20), b"k must be in 1..16"),
        'n = k': (dict(n=3), b"must be at least k + 1"), 'ld < c': (dict(ld=4), b"ld (4) must be at least c (5)"),
        'null x': (dict(x=None), b"null pointer"), 'null out': (dict(out=None), b"null pointer"),
        'null workspace': (dict(ws=None), b"null pointer"), 'workspace one byte short': (dict(nbytes=need_s - 1), b"workspace of"),
    }
    names = ('x', 'ld', 'n', 'c', 'k', 'out', 'ws', 'nbytes')
    for what, (over, message) in bad_self.items():
        args = [over.get(nm, v) for nm, v in zip(names, good)]
        assert self_call(*args) == TG_ERR_INVALID, what
        assert h.tg_last_error_string().startswith(b"knn_self") and message in h.tg_last_error_string(), (what, h.tg_last_error_string())
    (gc, _), nn, (gi, _) = int_out(m), guarded(m), int_out(m)
    wq = guarded(4096)
    need_q = L.call('tg_manifold_query_workspace_bytes', m, n)
    assert need_q < roomy
    query_call = lambda qp, ldq, m_, rp, ldr, n_, c_, r2p, cp, dp, ip, wp, nbytes: h.tg_manifold_query_f32(qp, ldq, m_, rp, ldr, n_, c_, r2p, cp,
                                                                                                    dp, ip, wp, nbytes, st())
    goodq = (ptr(qd), ld, m, ptr(x), ld, n, c, ptr(r2), gc.ptr, nn.ptr, gi.ptr, wq.ptr, roomy)
    namesq = ('q', 'ld_q', 'm', 'r', 'ld_r', 'n', 'c', 'r2', 'count', 'nn_d2', 'nn_idx', 'ws', 'nbytes')
    bad_query = {
        'c = 0': (dict(c=0), b"c must be in 1..512"), 'c = 513': (dict(c=513, ld_q=600, ld_r=600), b"c must be in 1..512"),
        'ld_q < c': (dict(ld_q=4), b"must be at least c (5)"), 'ld_r < c': (dict(ld_r=4), b"must be at least c (5)"),
        'm = 0': (dict(m=0), b"m and n must be at least 1"), 'n = 0': (dict(n=0), b"m and n must be at least 1"),
        'null q': (dict(q=None), b"null pointer"), 'null r': (dict(r=None), b"null pointer"),
        'null nn_d2': (dict(nn_d2=None), b"null pointer"), 'null nn_idx': (dict(nn_idx=None), b"null pointer"),
        'radii without count': (dict(count=None), b"count must not be null"), 'null workspace': (dict(ws=None), b"null pointer"),
        'workspace one byte short': (dict(nbytes=need_q - 1), b"workspace of"),
    }
    for what, (over, message) in bad_query.items():
        args = [over.get(nm, v) for nm, v in zip(namesq, goodq)]
        assert query_call(*args) == TG_ERR_INVALID, what
        assert h.tg_last_error_string().startswith(b"manifold_query") and message in h.tg_last_error_string(), (what, h.tg_last_error_string())
    # nothing was launched: every output is what it was
    torch.cuda.synchronize()
    assert np.isnan(out.get()).all() and np.isnan(nn.get()).all() and (ints(gc) == FILL).all() and (ints(gi) == FILL).all()
    assert np.isnan(ws.get()).all() and np.isnan(wq.get()).all()
    # the same calls with their arguments in range, and workspaces of exactly the queried size, go through
    assert self_call(*(good[:7] + (need_s,))) == 0 and query_call(*(goodq[:12] + (need_q,))) == 0
    torch.cuda.synchronize()
    for g in (out, ws, gc, nn, gi, wq):
        g.check_guard()
    assert (out.get()[:n * k] == 0).all() and np.isnan(out.get()[n * k:]).all()        # zero rows: every distance is 0; nothing past n * k
    assert np.isnan(ws.get()[need_s // 4:]).all() and np.isnan(wq.get()[need_q // 4:]).all()       # nothing beyond the queried size is written
    assert (nn.get() == 0).all() and (ints(gi) == 0).all() and (ints(gc) == n).all()   # ... the lowest index is 0, and 0 <= r2 = 1 for all n
