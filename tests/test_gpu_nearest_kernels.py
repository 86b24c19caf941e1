"""tg_nearest_u8_i32 and tg_f32_quantize_u8 (include/tg_kernels.h, csrc/nearest.hip) against tests/nearest_reference.py.

Everything is exact: the distance is an integer, the selection a total order on (d2, index), the quantiser a fixed fp32 chain restated
in NumPy float32 — every comparison is ==, there is no tolerance to state.

Shapes: d in {1, 63, 64, 65, 784, 3072} (below, at and above a 64-byte group; MNIST's ragged 784 = 6 x 128 + 16; CIFAR's 3072),
m in {1, 63, 65} (one row, below and above one query tile), k in {1, 3, 16} (both list widths of the kernel), n in {1, k - 1 (sentinels),
127, 129, 300} — picked pairwise, not as the full product.  n = 300 must be cut into at least three reference ranges with a ragged last
one, which the test asserts.  Those shapes give one reference tile per range; n = 33 001 gives two tiles per range and 258 ranges,
the paths of the real workload, and a case with misaligned base pointers takes the bytewise loader at a d that is a multiple of 16.
Every output and workspace is followed by guard words, and the workspace starts dirty."""
import ctypes as C

import numpy as np
import pytest
import torch

import nearest_reference as R
from kernel_check import lib, st

pytestmark = pytest.mark.gpu

N_MANY = 300
# (d, m, k, n); n None: k - 1
CASES = [(1, 1, 1, 1), (1, 63, 3, None), (1, 65, 16, 127), (63, 1, 3, 129), (63, 63, 16, N_MANY), (63, 65, 1, 1), (64, 1, 16, None),
         (64, 63, 1, 127), (64, 65, 3, N_MANY), (65, 1, 1, 129), (65, 63, 16, 1), (65, 65, 3, 127), (784, 1, 3, N_MANY), (784, 63, 1, 129),
         (784, 65, 16, None), (3072, 1, 16, 129), (3072, 63, 3, 1), (3072, 65, 1, N_MANY), (784, 65, 3, None), (3072, 63, 16, 127),
         (64, 63, 3, 129)]
GUARD, GUARD_WORD, FILL = 64, 0x5A17C0DE, 0x0BADF00D
_DATA = {}


def data(d, m, n, seed=0):
    """(q [m, d], r [n, d]) uint8, made once per shape and left unchanged: random bytes plus planted rows — r[5] a copy of r[2] (one
    tile), r[n - 1] a copy of r[0] (the last tile, so another range when there are several), q[0] a copy of r[0] (d2 = 0, and two
    references at that distance: the lower index must win)."""
    key = (d, m, n, seed)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * d + 10 * m + n + seed)
        q, r = rng.integers(0, 256, (m, d), dtype=np.uint8), rng.integers(0, 256, (n, d), dtype=np.uint8)
        if n > 5:
            r[5] = r[2]
            r[n - 1] = r[0]
        q[0] = r[0]
        q.setflags(write=False), r.setflags(write=False)
        _DATA[key] = (q, r)
    return _DATA[key]


class Ints(object):
    """n int32 on the device holding `fill`, followed by GUARD guard words."""

    def __init__(self, n, fill=FILL):
        self.n = n
        self.base = torch.full((n + GUARD,), GUARD_WORD, dtype=torch.int32, device='cuda')
        self.t = self.base[:n]
        self.t.fill_(fill)

    def put(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.int32).reshape(-1)))
        return self

    def get(self, shape):
        torch.cuda.synchronize()
        assert (self.base[self.n:].cpu().numpy() == GUARD_WORD).all(), "write past the end"
        return self.t.cpu().numpy().reshape(shape).copy()


def dev_u8(a):
    return torch.from_numpy(np.array(a, np.uint8)).cuda()


def run(q, r, k, base=0, prev=None, q_dev=None, r_dev=None):
    """one tg_nearest_u8_i32 call on the current stream with a dirty workspace of exactly the queried size -> (d2, idx) int32 [m, k]."""
    L = lib()
    (m, d), n = q.shape, r.shape[0]
    need = L.call('tg_nearest_u8_workspace_bytes', m, n, d, k)
    assert need > 0 and need % 4 == 0
    work = Ints(need // 4, fill=0x7F7F7F7F)
    out_d, out_i = Ints(m * k), Ints(m * k)
    if prev is not None:
        out_d.put(prev[0]), out_i.put(prev[1])
    qd = dev_u8(q) if q_dev is None else q_dev
    rd = dev_u8(r) if r_dev is None else r_dev
    L.call('tg_nearest_u8_i32', C.c_void_p(qd.data_ptr()), m, C.c_void_p(rd.data_ptr()), n, d, k, base, int(prev is not None),
           C.c_void_p(out_d.t.data_ptr()), C.c_void_p(out_i.t.data_ptr()), C.c_void_p(work.t.data_ptr()), need, st())
    got = out_d.get((m, k)), out_i.get((m, k))
    work.get((-1,))                                                    # (its guard: nothing beyond the queried size is written)
    return got


def same(got, want, what=""):
    assert got[0].dtype == want[0].dtype == np.int32
    bad = (got[0] != want[0]) | (got[1] != want[1])
    assert not bad.any(), "%s: %d pairs differ, first at %s: got (%d, %d) want (%d, %d)" % (
        (what, int(bad.sum()), np.argwhere(bad)[0]) + tuple(int(a[tuple(np.argwhere(bad)[0])]) for a in (got[0], got[1], want[0], want[1])))


@pytest.mark.parametrize("d,m,k,n", CASES)
def test_the_k_best_pairs_are_the_reference(d, m, k, n):
    n = k - 1 if n is None else n
    q, r = data(d, m, n)
    if n == N_MANY:                                                    # several ranges, the last one ragged
        assert lib().call('tg_nearest_u8_ranges', m, n) >= 3 and n % 64 != 0
    got = run(q, r, k)
    want = R.nearest(q, r, k)
    same(got, want, "d %d m %d k %d n %d" % (d, m, k, n))
    assert got[0][0, 0] == 0 and got[1][0, 0] == 0                     # the planted query: its twin r[0], not r[n - 1]
    if n < k:
        assert (got[0][:, n:] == R.NONE_D2).all() and (got[1][:, n:] == R.NONE_IDX).all()
    if n > 5 and k >= 3 and d >= 63:                                   # r[0] = r[n - 1]: both at distance 0, the lower index first
        assert tuple(got[1][0, :2]) == (0, n - 1) and tuple(got[0][0, :2]) == (0, 0)


@pytest.mark.parametrize("d", [3072, 16384])
def test_the_largest_distance_is_exact(d):
    """all-0 against all-255: d2 = 255^2 d, the largest value the interface holds (1 065 369 600 at d = 16 384, below 2^31)."""
    q = np.stack([np.zeros(d, np.uint8), np.full(d, 255, np.uint8)])
    r = q[::-1].copy()
    got = run(q, r, 2)
    same(got, R.nearest(q, r, 2), "extremes")
    assert (got[0] == np.array([[0, 255 * 255 * d]] * 2)).all() and (got[1] == np.array([[1, 0], [0, 1]])).all()


N_DEEP = 33001                   # 516 reference tiles: 258 ranges of two tiles each for one or two query tiles
TWINS = (128 * 5 + 3, 128 * 5 + 70, 128 * 69 + 1, 128 * 70 + 9)        # see test_several_tiles_per_range_and_more_ranges_than_lanes


@pytest.mark.parametrize("d,m,k", [(1, 1, 16), (1, 65, 3), (64, 1, 3), (64, 65, 16)])
def test_several_tiles_per_range_and_more_ranges_than_lanes(d, m, k):
    """the shape of the real workload (64 queries against 50 000 rows: 391 ranges of two tiles), at the smallest n that has it: a
    workgroup walks TWO reference tiles — the running k-best list, the accumulators and the norms cross a tile boundary — and the
    finishing launch merges 258 ranges, more than its 64 lanes, so a lane takes several ranges and lane 0 merges many non-empty lane
    lists.  Four copies of one row are planted: in the first and in the second tile of range 5 (one workgroup), in range 69 (the same
    lane of the finishing launch, its second turn) and in range 70 (another lane); query 0 equals them.  At d = 1 every distance has
    about 129 ties, so the order among equal distances is tested throughout."""
    assert lib().call('tg_nearest_u8_ranges', m, N_DEEP) == 258 and -(-N_DEEP // 64) == 2 * 258 and N_DEEP % 64 != 0
    q, r = data(d, m, N_DEEP, seed=2)
    q, r = np.array(q), np.array(r)
    for j in TWINS[1:]:
        r[j] = r[TWINS[0]]
    q[0] = r[TWINS[0]]
    got = run(q, r, k)
    same(got, R.nearest(q, r, k), "d %d m %d k %d n %d" % (d, m, k, N_DEEP))
    assert (got[0][0, :3] == 0).all()
    if d == 64:                                                        # (at d = 1 other rows hold the same byte, some at lower indices)
        assert tuple(got[1][0, :min(k, 4)]) == TWINS[:min(k, 4)] and (got[0][0, :min(k, 4)] == 0).all()
        assert k <= 4 or got[0][0, 4] > 0


def test_a_misaligned_base_pointer_takes_the_bytewise_loader():
    """d = 64 is a multiple of 16, so the 16-byte loads are taken whenever both base pointers are 16-byte aligned — and must not be when
    one is not: q starts 3 bytes and r 5 bytes into their allocations."""
    d, m, k, n = 64, 65, 3, N_MANY
    q, r = data(d, m, n)
    want = R.nearest(q, r, k)
    qbuf, rbuf = torch.zeros(m * d + 16, dtype=torch.uint8, device='cuda'), torch.zeros(n * d + 16, dtype=torch.uint8, device='cuda')
    qd, rd = qbuf[3:3 + m * d].view(m, d), rbuf[5:5 + n * d].view(n, d)
    qd.copy_(dev_u8(q)), rd.copy_(dev_u8(r))
    assert qd.data_ptr() % 16 == 3 and rd.data_ptr() % 16 == 5
    same(run(q, r, k, q_dev=qd, r_dev=rd), want, "both misaligned")
    same(run(q, r, k, r_dev=rd), want, "r misaligned")
    same(run(q, r, k, q_dev=qd), want, "q misaligned")


@pytest.mark.parametrize("d,k", [(65, 16), (784, 3)])
def test_chunking_and_chunk_order_do_not_change_the_answer(d, k):
    m, n = 65, N_MANY
    q, r = data(d, m, n, seed=1)
    r = np.array(r)
    r[250] = r[3]                                                      # duplicates in different chunks
    q = np.array(q)
    q[7] = r[3]                                                        # and a query equal to both
    whole = run(q, r, k)
    same(whole, R.nearest(q, r, k), "one call")
    assert tuple(whole[1][7, :2]) == (3, 250) and tuple(whole[0][7, :2]) == (0, 0)
    cuts = [(0, 100), (100, 171), (171, n)]
    rd = dev_u8(r)
    for order, what in ((cuts, "three chunks"), (cuts[::-1], "three chunks, reversed")):
        prev = None
        for lo, hi in order:
            prev = run(q, r[lo:hi], k, base=lo, prev=prev, r_dev=rd[lo:hi])     # views at row offsets: d = 65 is the unaligned path
        same(prev, whole, what)


def test_two_runs_on_two_streams_are_bit_identical():
    d, m, k, n = 784, 65, 16, N_MANY
    q, r = data(d, m, n)
    first = run(q, r, k)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        second = run(q, r, k)
    side.synchronize()
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


def quantize(x, scale, shift):
    L = lib()
    n = x.size
    src = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    base = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    L.call('tg_f32_quantize_u8', C.c_void_p(src.data_ptr()), C.c_void_p(base.data_ptr()), n, scale, shift, st())
    torch.cuda.synchronize()
    host = base.cpu().numpy()
    assert (host[n:] == 0xA5).all(), "write past the end"
    return host[:n].copy()


@pytest.mark.parametrize("scale,shift", [(2.0, -1.0), (1.0, 0.0)])
def test_the_quantiser_is_its_float32_restatement(scale, shift):
    j = np.arange(-2, 258, dtype=np.float64)
    edges = ((j + 0.5) / 255.0 * scale + shift).astype(np.float32)     # every j + 0.5 boundary, with its fp32 neighbours on both sides
    sweep = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf)),
                            np.linspace(shift - 1.0, shift + scale + 1.0, 4001).astype(np.float32),
                            np.array([-1e30, 1e30, -np.inf, np.inf, np.nan, 0.0, -0.0], np.float32)])
    got = quantize(sweep, scale, shift)
    want = R.quantize(sweep, scale, shift)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    assert got[np.isnan(sweep)].tolist() == [0] and set(got) == set(range(256))
    for n in (0, 1, 255, 257):
        part = sweep[100:100 + n]
        assert (quantize(part, scale, shift) == R.quantize(part, scale, shift)).all()
    # the device round trip with tg_u8_affine_f32 returns every byte
    L = lib()
    u = torch.arange(256, dtype=torch.uint8, device='cuda')
    x = torch.empty(256, dtype=torch.float32, device='cuda')
    L.call('tg_u8_affine_f32', C.c_void_p(u.data_ptr()), C.c_void_p(x.data_ptr()), 256, scale, shift, st())
    torch.cuda.synchronize()
    assert (x.cpu().numpy() == R.affine(np.arange(256), scale, shift)).all()
    assert (quantize(x.cpu().numpy(), scale, shift) == np.arange(256)).all()
