"""Shared checks of the per-kernel float64 tests (tests/test_gpu_elementwise.py, _prep.py, _norm_finalize.py, _loss_heads.py, _gemm_tiles.py, _halo_tiles.py,
_packed_tiles.py, _rng.py, _norm_forward.py, _colstats.py, _stats_chunk.py, _updates.py, _small_heads.py, _wgan_kernels.py and its reference
tests/wgan_kernels_reference.py with the CPU check tests/test_wgan_kernels_reference.py), of the route-level float64 test
of tg/ops.py (tests/test_gpu_ops_routes.py and its reference tests/ops_reference.py, which propagates the tolerance classes below through
whole ops: guarded allocations, U, TOL, ALPHA, worst / rejected, bf16_rne_bits), and the float64 oracle of an implicit-GEMM descriptor
(igemm_ref64, on the device).

Every output a test reads is allocated by `guarded`: the buffer is followed by GUARD floats holding a fixed bit pattern, and the output
itself starts as NaN.  After the launch every element the kernel owns must hold a number (no NaN left = it was written), the guard must
hold its pattern bit for bit (nothing was written past the end), and padding the kernel must zero is exactly 0.0.  The guard is part of
the same allocation: nothing is read or written outside a buffer.  `guarded16` is the same for an output of 2-byte elements (bf16).

Tolerance classes (each test module states which one applies to which output):
  bit-exact  got == the fp32 value NumPy computes in the kernel's order (data movement, selection, one correctly rounded operation,
             fixed-order fp32 sums);
  pointwise  |got - ref64| <= K * u * mag with u = 2^-24 (the fp32 unit roundoff), ref64 the float64 restatement evaluated on the same
             fp32 inputs and mag the same expression evaluated on absolute values (one rounding of an intermediate of size |t| costs at
             most u * |t|, so K counts the roundings plus the ulp of the device library's transcendentals);
  reduction  |got - ref64| <= TOL * sum |terms| per output, TOL = 1e-6 (the rule of tests/test_gpu_igemm.py), with a negative control
             showing that the bound rejects a reference that is off by one row / slab / tile."""
import ctypes as C

import numpy as np
import torch

GUARD = 67                       # floats behind every output (odd: the guard also covers a partial 16-byte group)
GUARD_BITS = 0x5A17C0DE          # a finite float no kernel computes here
U = 2.0 ** -24
TOL = 1e-6
FLT_MIN = 2.0 ** -126            # below this an fp32 intermediate may be flushed to zero (expf of a logit 88 below the row maximum)


def lib():
    from tg import lib as L
    L.load()
    return L


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


_ALIVE = []      # tensors handed to a launch as raw pointers: kept until the next synchronisation (`finish`), so that a temporary such as
                 # ptr(dev(x)) cannot go back to the caching allocator and be handed out again while the launch may still read it


def ptr(t):
    if t is None:
        return None
    _ALIVE.append(t)
    return C.c_void_p(t.data_ptr())


class Guarded(object):
    """an output of `n` floats at float offset `offset` of its allocation, NaN-filled, followed by GUARD pattern floats."""

    def __init__(self, n, offset=0, fill=None):
        self.n, self.offset = int(n), int(offset)
        self.base = torch.empty(self.offset + self.n + GUARD, dtype=torch.float32, device='cuda')
        self.base.view(torch.int32).fill_(GUARD_BITS)
        self.t = self.base[self.offset:self.offset + self.n]
        if fill is None:
            self.t.fill_(float('nan'))
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.float32).reshape(-1)))

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def get(self, shape=None):
        torch.cuda.synchronize()
        a = self.t.cpu().numpy().copy()
        return a if shape is None else a.reshape(shape)

    def check_guard(self):
        torch.cuda.synchronize()
        del _ALIVE[:]
        raw = self.base.view(torch.int32).cpu().numpy()
        tail = raw[self.offset + self.n:]
        head = raw[:self.offset]
        assert (tail == GUARD_BITS).all(), "write past the end of the output: guard word %d changed" % int(np.argmax(tail != GUARD_BITS))
        assert (head == GUARD_BITS).all(), "write in front of the output"


def guarded(n, offset=0, fill=None):
    return Guarded(n, offset, fill)


GUARD16_BITS = 0x5A17            # the guard pattern of a 2-byte output
NAN16_BITS = 0x7FC0              # bf16 quiet NaN: the "never written" fill of a 2-byte output


class Guarded16(object):
    """an output of `n` 2-byte elements (bf16), every element the bf16 NaN, followed by 2 * GUARD pattern halfwords (the same number of
    guard bytes as behind a float output)."""

    def __init__(self, n):
        self.n = int(n)
        self.base = torch.empty(self.n + 2 * GUARD, dtype=torch.int16, device='cuda')
        self.base.fill_(GUARD16_BITS)
        self.t = self.base[:self.n]
        self.t.fill_(NAN16_BITS)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def get(self, shape=None):
        """the raw halfwords (uint16)"""
        torch.cuda.synchronize()
        a = self.t.cpu().numpy().view(np.uint16).copy()
        return a if shape is None else a.reshape(shape)

    def check_guard(self):
        torch.cuda.synchronize()
        del _ALIVE[:]
        tail = self.base[self.n:].cpu().numpy()
        assert (tail == GUARD16_BITS).all(), "write past the end of the 2-byte output: guard halfword %d changed" % int(np.argmax(tail != GUARD16_BITS))


def guarded16(n):
    return Guarded16(n)


def finish16(g, shape=None, owned=None):
    """`finish` for a Guarded16: guard intact, no owned halfword still the NaN fill; returns the raw bf16 bits (uint16)."""
    g.check_guard()
    a = g.get(shape)
    m = np.ones(a.shape, bool) if owned is None else owned
    assert not (a[m] == NAN16_BITS).any(), "%d owned 2-byte elements were never written" % int((a[m] == NAN16_BITS).sum())
    return a


def bf16_rne_bits(a):
    """the bf16 halfwords of finite fp32 values rounded to nearest even (what __builtin_convertvector(float -> __bf16) stores)."""
    x = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((x + np.uint32(0x7FFF) + ((x >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def finish(g, shape=None, owned=None):
    """guard intact and every owned element written (owned: boolean mask over the output, default all); returns the output."""
    g.check_guard()
    a = g.get(shape)
    m = np.ones(a.shape, bool) if owned is None else owned
    assert not np.isnan(a[m]).any(), "%d owned elements were never written" % int(np.isnan(a[m]).sum())
    return a


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_bits(got, ref, what=""):
    g, r = bits(got), bits(ref)
    bad = g != r
    assert not bad.any(), "%s: %d elements differ from the bit-exact reference (first at %s: got %r want %r)" % (
        what, int(bad.sum()), np.argwhere(bad)[0], np.asarray(got).reshape(g.shape)[tuple(np.argwhere(bad)[0])],
        np.asarray(ref, np.float32).reshape(g.shape)[tuple(np.argwhere(bad)[0])])


def assert_pointwise(got, ref64, mag, k, what="", floor=0.0):
    """|got - ref64| <= k u mag + floor (floor: what flushing intermediates below FLT_MIN can cost, where a test has such values)."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref64)
    lim = k * U * np.asarray(mag, np.float64) + floor
    assert np.isfinite(got).all(), "%s: non-finite output" % what
    bad = err > lim
    if bad.any():
        r = err / (lim + 1e-300)
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        g, rf, m = got[i], np.broadcast_to(ref64, r.shape)[i], np.broadcast_to(np.asarray(mag, np.float64), r.shape)[i]
        raise AssertionError("%s: %d elements beyond %g u * magnitude; worst at %s: got %.9g, ref %.9g, magnitude %.3g" % (
            what, int(bad.sum()), k, i, g, rf, m))


def worst(got, ref64, sabs):
    """max over the outputs of |got - ref| / (TOL * sum|terms|): <= 1 passes."""
    err = np.abs(np.asarray(got, np.float64) - ref64)
    return float((err / (TOL * np.asarray(sabs, np.float64) + 1e-300)).max())


def close(got, ref64, sabs, what=""):
    r = worst(got, ref64, sabs)
    assert r <= 1.0, "%s: error is %.2f x the reduction bound (TOL %.0e of the per-output sum |terms|)" % (what, r, TOL)


def rejected(got, ref64, sabs, factor=10.0):
    """the bound tells `got` from `ref64` with room to spare (negative controls)."""
    return worst(got, ref64, sabs) > factor


def seq_sum32(parts, init=None):
    """fp32 sum of parts[0] + parts[1] + ... in that order (NumPy's own reductions are pairwise: they cannot restate a loop)."""
    acc = np.zeros(np.shape(parts[0]), np.float32) if init is None else np.array(init, np.float32)
    for p in parts:
        acc = (acc + np.asarray(p, np.float32)).astype(np.float32)
    return acc


# activations (Model/modle_base.py:176-188, Good_GAN_cifar10.py:19-27) in float64, and their derivatives through the OUTPUT
ACTS = ['none', 'lrelu', 'relu', 'tanh', 'sigmoid', 'softplus']
ALPHA = np.float32(0.2)


def act64(x, a):
    x = np.asarray(x, np.float64)
    if a == 'relu':
        return np.where(x > 0, x, 0.0)
    if a == 'lrelu':
        return np.where(x > 0, x, np.float64(ALPHA) * x)       # Good_GAN_cifar10.py:26-27 (max(x, alpha x) for alpha < 1)
    if a == 'tanh':
        return np.tanh(x)
    if a == 'sigmoid':
        return 1.0 / (1.0 + np.exp(-x))
    if a == 'softplus':
        return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))
    return x


def act_grad64(y, a):
    """derivative through the activation OUTPUT (what the forward keeps) and the magnitude of its evaluation."""
    y = np.asarray(y, np.float64)
    if a == 'relu':
        g = np.where(y > 0, 1.0, 0.0)
        return g, g
    if a == 'lrelu':
        g = np.where(y > 0, 1.0, np.float64(ALPHA))
        return g, g
    if a == 'tanh':
        return 1 - y * y, 1 + y * y
    if a == 'sigmoid':
        return y * (1 - y), np.abs(y) * (1 + np.abs(y))
    if a == 'softplus':
        return 1 - np.exp(-y), 1 + np.exp(-y)
    return np.ones_like(y), np.ones_like(y)


def y_for(rng, shape, a):
    """activation outputs of the right range for act'(y), with exact zeros for the relu family."""
    x = rng.standard_normal(shape) * 2
    x[..., ::7] = 0
    y = act64(x, a)
    return y.astype(np.float32)


# ---- float64 oracle of a tg_igemm_desc (csrc/igemm.hip's operation restated on the device in torch float64) ----
def igemm_gather(x, d, tap):
    """rows of the gathered operand of tap `tap` of descriptor d: x [n, h_in, w_in, ld_in] -> [M, ld_in], zeros outside the image."""
    dy, dx = int(d.dy[tap]), int(d.dx[tap])
    iy = torch.arange(d.h_v, device=x.device) * d.s_y + dy
    ix = torch.arange(d.w_v, device=x.device) * d.s_x + dx
    my, mx = (iy >= 0) & (iy < d.h_in), (ix >= 0) & (ix < d.w_in)
    g = x[:, iy.clamp(0, d.h_in - 1)][:, :, ix.clamp(0, d.w_in - 1)]
    g = g * (my[:, None] & mx[None, :]).to(x.dtype)[None, :, :, None]
    return g.reshape(-1, d.ld_in)


def igemm_filter(wf, d, tap):
    """[c_out, ld_in] filter rows of tap `tap`: w[n * w_sn + tapw * w_st + c]."""
    return wf.as_strided((d.c_out, d.ld_in), (d.w_sn, 1), int(d.tapw[tap]) * d.w_st)


def igemm_ref64(descs, x, wf, last_k=32):
    """float64 accumulators of every descriptor: [(acc, sum|a||b|, the last K-tile's share of acc)], each [M, c_out].  The last K-tile is
    channels [ld_in - last_k, ld_in) of the descriptor's last tap (32: the generic kernels' K-tile; the halo kernels' channel chunk is 64
    with bf16 operands)."""
    out = []
    for d in descs:
        acc = sab = last = None
        for t in range(d.n_taps):
            a, w = igemm_gather(x, d, t), igemm_filter(wf, d, t)
            p, s = a @ w.T, a.abs() @ w.abs().T
            acc = p if acc is None else acc + p
            sab = s if sab is None else sab + s
        last = a[:, -last_k:] @ w[:, -last_k:].T
        out.append((acc, sab, last))
    return out


def igemm_scatter(d, vals, out):
    """store [M, n_store] rows of descriptor d into out [n, h_out, w_out, ld_out] as the kernel does."""
    v = vals.reshape(d.n_img, d.h_v, d.w_v, -1)
    out[:, d.oo_y::d.os_y, d.oo_x::d.os_x][:, :d.h_v, :d.w_v, :d.n_store] = v[..., :d.n_store]
