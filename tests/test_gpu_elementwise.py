"""Per-kernel float64 tests of the HBM-bound kernels of csrc/elementwise.hip and the batched RNG of csrc/rng.hip, called through the C ABI
at their edge shapes: both code paths of the kernels that move 16 bytes per lane, grid-stride loops past the 4 096-workgroup cap of
ew_grid, one row / one channel / one pixel, padding columns, writes past the end (tests/kernel_check.py: NaN-filled outputs followed by
a guard region).

Tolerance classes (tests/kernel_check.py):
  bit-exact   pad_add (x, or x + add: one correctly rounded addition), cond_concat and maxpool2_bwd (x * (mask * mscale) with a 0/1 mask:
              one rounding), copy_multi, copy2d, add, gmaxpool_fwd / _bwd, im2col3x3_add, gavgpool_concat (fp32 sum over the pixels in
              pixel order, then one division), splitk_reduce (bias + sum_s in slab order), act for none / relu / lrelu (one rounding),
              tg_rng_multi_f32 against the single-draw entry points, u8_affine (the fp32 host expression) and onehot_i32;
  pointwise   act: tanh K = 4 (the device library's tanhf is within 2 ulp, 1 ulp <= 2u relative), sigmoid and softplus K = 6 (expf 2 ulp,
              then one addition and one division / log1pf of condition <= 1); actgrad: K = 3 for none / relu / lrelu (three products),
              6 for tanh / sigmoid (1 - y*y / y*(1 - y) add two roundings, mag evaluates them on |y| so cancellation is covered), 8 for
              softplus (1 - expf(-y)); gavgpool_bwd K = 4 on top of the derivative's own count (1/hw, two products);
  reduction   gavgpool_concat is also held to 1e-6 * sum|x| against float64, with a negative control that drops the last pixel;
              splitk_reduce likewise, the control dropping the last slab."""
import ctypes as C

import numpy as np
import pytest
import torch

from kernel_check import ACTS, ALPHA, act64, act_grad64, assert_bits, assert_pointwise, bits, close, dev, finish, guarded, lib, ptr, rejected, seq_sum32, st, y_for

pytestmark = pytest.mark.gpu

MSCALE = np.float32(1.0 / 0.7)            # inverted-dropout scale of keep 0.7 (not a power of two: the product rounds)


def padded(rng, rows, c, ld, scale=1.0, fill=np.nan):
    """[rows, ld] float32 with columns [c, ld) set to `fill` (NaN: a kernel that reads them into a result is caught)."""
    a = np.full((rows, ld), fill, np.float32)
    a[:, :c] = (rng.standard_normal((rows, c)) * scale).astype(np.float32)
    return a


# ------------------------------------------------------------------ act / actgrad

ACT_SHAPES = [  # rows, c, ld_x, ld_y
    (300, 64, 64, 96),          # 16-byte path
    (300, 30, 32, 32),          # c % 4 != 0: scalar path
    (37, 13, 15, 17),           # ld % 4 != 0: scalar path
    (1, 1, 1, 1),               # smallest
    (36000, 32, 32, 36),        # scalar: 1.3 M elements > 4 096 x 256 lanes
    (72000, 64, 64, 64),        # 16-byte path: 1.15 M float4 > 4 096 x 256 lanes
]


@pytest.mark.parametrize("shape", ACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_act(shape):
    """tg_act_f32 = an activation called on a tensor (Model/modle_base.py:176-188, Good_GAN_cifar10.py:19-27)."""
    L = lib()
    rows, c, ld_x, ld_y = shape
    rng = np.random.default_rng(rows + c)
    x = padded(rng, rows, c, ld_x, scale=6.0)
    x[:, :c][:, ::5] = 0.0
    xd = dev(x)
    for a in ACTS:
        out = guarded(rows * ld_y)
        L.call('tg_act_f32', ptr(xd), ld_x, out.ptr, ld_y, rows, c, L.ACT[a], float(ALPHA), st())
        y = finish(out, (rows, ld_y))
        assert (bits(y[:, c:]) == 0).all(), "%s: padding columns not +0.0" % a
        ref = act64(x[:, :c], a)
        if a in ('none', 'relu', 'lrelu'):
            assert_bits(y[:, :c], ref.astype(np.float32), a)
        else:
            assert_pointwise(y[:, :c], ref, np.abs(ref), {'tanh': 4, 'sigmoid': 6, 'softplus': 6}[a], a)


ACTGRAD_CASES = [  # rows, c, ld_dy, ld_y, ld_m, ld_out, mask, yact
    (300, 64, 64, 64, 64, 96, True, True),      # 16-byte loads and stores
    (300, 64, 64, 64, 64, 64, False, False),    # 16-byte path, neither mask nor yact
    (300, 64, 64, 64, 68, 64, False, True),     # yact only
    (77, 30, 32, 32, 32, 32, True, True),       # c % 4 != 0: 16-byte stores, scalar loads
    (77, 32, 33, 32, 32, 32, True, True),       # ld_dy % 4 != 0: scalar loads
    (77, 13, 13, 15, 14, 17, True, False),      # ld_out % 4 != 0: scalar path
    (1, 1, 1, 1, 1, 1, True, True),
    (40000, 64, 64, 64, 64, 128, True, True),   # 1.28 M float4 groups > 4 096 x 256 lanes
    (40000, 27, 27, 27, 27, 29, False, True),   # scalar path, 1.16 M elements
]


@pytest.mark.parametrize("case", ACTGRAD_CASES, ids=lambda s: "x".join(map(str, s)))
def test_actgrad(case):
    """tg_actgrad_f32: gradient of dropout + activation (modle_base.py:190-191 and the activations above), padding zeroed."""
    L = lib()
    rows, c, ld_dy, ld_y, ld_m, ld_out, has_mask, has_y = case
    rng = np.random.default_rng(rows * 7 + c)
    dy = padded(rng, rows, c, ld_dy)
    mask = np.full((rows, ld_m), np.nan, np.float32)
    mask[:, :c] = (rng.random((rows, c)) < 0.7).astype(np.float32)
    dyd, md = dev(dy), dev(mask)
    for a in ACTS if has_y else ['none']:
        y = np.full((rows, ld_y), np.nan, np.float32)
        y[:, :c] = y_for(rng, (rows, c), a)
        yd = dev(y)
        out = guarded(rows * ld_out)
        L.call('tg_actgrad_f32', ptr(dyd), ld_dy, ptr(yd) if has_y else None, ld_y, ptr(md) if has_mask else None, ld_m, float(MSCALE), out.ptr,
               ld_out, rows, c, L.ACT[a], float(ALPHA), st())
        got = finish(out, (rows, ld_out))
        assert (bits(got[:, c:]) == 0).all(), "%s: padding columns not +0.0" % a
        ms = (mask[:, :c].astype(np.float64) * np.float64(MSCALE)) if has_mask else 1.0
        g, gm = act_grad64(y[:, :c], a) if has_y else (1.0, 1.0)
        ref = dy[:, :c].astype(np.float64) * ms * g
        mag = np.abs(dy[:, :c].astype(np.float64)) * np.abs(ms) * gm
        k = {'none': 3, 'relu': 3, 'lrelu': 3, 'tanh': 6, 'sigmoid': 6, 'softplus': 8}[a]
        assert_pointwise(got[:, :c], ref, mag, k, a)


# ------------------------------------------------------------------ pad_add / add / copies

@pytest.mark.parametrize("rows,c,ld_x,ld_add,ld_out", [(250, 3, 3, 3, 32), (1, 1, 1, 1, 1), (40000, 27, 27, 28, 32), (7, 13, 16, 13, 13)])
@pytest.mark.parametrize("with_add", [False, True])
def test_pad_add(rows, c, ld_x, ld_add, ld_out, with_add):
    """tg_pad_add_f32: Gaussian input noise of the classifier (modle_base.py:193-202) + channel padding; bit-exact (one rounding)."""
    L = lib()
    rng = np.random.default_rng(rows + c)
    x, add = padded(rng, rows, c, ld_x), padded(rng, rows, c, ld_add, 0.15)
    out = guarded(rows * ld_out)
    L.call('tg_pad_add_f32', ptr(dev(x)), ld_x, c, ptr(dev(add)) if with_add else None, ld_add, out.ptr, ld_out, rows, st())
    got = finish(out, (rows, ld_out))
    ref = x[:, :c] + add[:, :c] if with_add else x[:, :c]
    assert_bits(got[:, :c], ref)
    assert (bits(got[:, c:]) == 0).all()


def test_add_in_place_and_out_of_place():
    """tg_add_f32 (sums per-application gradient buffers): dst = a + b bit-exact, odd n past the grid cap, dst aliasing a."""
    L = lib()
    rng = np.random.default_rng(3)
    for n in (1, 5, 1200001):
        a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        ad, bd = dev(a), dev(b)
        out = guarded(n)
        L.call('tg_add_f32', out.ptr, ptr(ad), ptr(bd), n, st())
        assert_bits(finish(out), a + b)
        dst = guarded(n, fill=a)
        L.call('tg_add_f32', dst.ptr, dst.ptr, ptr(bd), n, st())
        assert_bits(finish(dst), a + b)


@pytest.mark.parametrize("n_jobs", [1, 3, 16])
@pytest.mark.parametrize("misalign", [False, True])
def test_copy_multi(n_jobs, misalign):
    """tg_copy_multi_f32 (batch concatenation, placeholder feeds): 16-byte path when both ends are 16-byte aligned, else the scalar one;
    lengths with n % 4 != 0, one job past the 4 096-workgroup cap; bit-exact."""
    L = lib()
    rng = np.random.default_rng(n_jobs)
    sizes = [4099, 5 * 1048576 + 3, 1, 3, 4, 5, 31, 1024, 17, 2, 250, 4096, 8, 9, 10, 11][:n_jobs]
    keep, jobs, outs = [], (L.CopyJob * n_jobs)(), []
    for i, n in enumerate(sizes):
        src = rng.standard_normal(n + 1).astype(np.float32)
        sd = dev(src)
        keep.append((src, sd))
        so = 1 if (misalign and i % 2 == 0) else 0           # 4-byte offset of src, or of dst, or both
        do = 1 if (misalign and i % 3 != 1) else 0
        out = guarded(n, offset=do)
        outs.append((out, src[so:so + n]))
        jobs[i] = L.CopyJob(sd.data_ptr() + 4 * so, out.t.data_ptr(), n)
    L.call('tg_copy_multi_f32', C.cast(jobs, C.c_void_p), n_jobs, st())
    for out, ref in outs:
        assert_bits(finish(out), ref)


def test_copy_multi_rejects_seventeen_jobs():
    L = lib()
    h = L.load()
    a = torch.zeros(4, device='cuda')
    jobs = (L.CopyJob * 17)(*[L.CopyJob(a.data_ptr(), a.data_ptr(), 4) for _ in range(17)])
    assert h.tg_copy_multi_f32(C.cast(jobs, C.c_void_p), 17, st()) == -1
    assert b"n_jobs=17" in h.tg_last_error_string()
    assert h.tg_copy_multi_f32(C.cast(jobs, C.c_void_p), 0, st()) == -1


@pytest.mark.parametrize("rows,c,ld_s,ld_d,off", [(100, 32, 32, 64, 0), (100, 32, 32, 64, 1), (33, 13, 15, 14, 0), (1, 1, 1, 1, 0),
                                                  (1200000, 4, 4, 8, 0)])
def test_copy2d(rows, c, ld_s, ld_d, off):
    """tg_copy2d_f32: 16-byte path (c, strides multiple of 4, aligned pointers) and scalar path; columns [c, ld_d) untouched."""
    L = lib()
    rng = np.random.default_rng(rows)
    src = rng.standard_normal((rows, ld_s)).astype(np.float32)
    dst0 = np.full((rows, ld_d), 7.5, np.float32)
    dst0[:, :c] = np.nan
    out = guarded(rows * ld_d, offset=off, fill=dst0)
    L.call('tg_copy2d_f32', ptr(dev(src)), ld_s, out.ptr, ld_d, rows, c, st())
    got = finish(out, (rows, ld_d))
    assert_bits(got[:, :c], src[:, :c])
    assert_bits(got[:, c:], dst0[:, c:])


# ------------------------------------------------------------------ cond_concat

COND_CASES = [  # n_img, hw, c, ld_x, ld_m, ncls, ld_out, mask
    (10, 64, 64, 64, 64, 10, 96, True),       # 16-byte path (discriminator feature maps, Good_GAN_cifar10.py:66-91)
    (10, 64, 64, 64, 64, 10, 96, False),
    (10, 16, 30, 32, 32, 10, 64, True),       # c % 4 != 0
    (10, 16, 32, 33, 32, 10, 64, True),       # ld_x % 4 != 0
    (10, 16, 32, 32, 34, 10, 64, True),       # ld_mask % 4 != 0
    (1, 1, 1, 1, 1, 1, 4, True),              # smallest
    (5, 7, 3, 3, 3, 0, 4, False),             # no labels
    (250, 1024, 8, 8, 8, 10, 20, True),       # 1.28 M float4 groups > 4 096 x 256 lanes
]


@pytest.mark.parametrize("case", COND_CASES, ids=lambda s: "x".join(map(str, s)))
def test_cond_concat(case):
    """tg_cond_concat_f32: out[n,p,:] = [x * mask * mscale, y[n], 0...] (dropout modle_base.py:190-191 + _conv_cond_concat :239-244)."""
    L = lib()
    n, hw, c, ld_x, ld_m, ncls, ld_out, has_mask = case
    rng = np.random.default_rng(n * hw + c)
    rows = n * hw
    x = padded(rng, rows, c, ld_x)
    m = np.full((rows, ld_m), np.nan, np.float32)
    m[:, :c] = (rng.random((rows, c)) < 0.7).astype(np.float32)
    y = rng.standard_normal((n, max(ncls, 1))).astype(np.float32)
    out = guarded(rows * ld_out)
    L.call('tg_cond_concat_f32', ptr(dev(x)), ld_x, c, ptr(dev(m)) if has_mask else None, ld_m, float(MSCALE), ptr(dev(y[:, :ncls])) if ncls else
           ptr(dev(y)), ncls, out.ptr, ld_out, n, hw, st())
    got = finish(out, (rows, ld_out))
    ref = x[:, :c] * (m[:, :c] * MSCALE) if has_mask else x[:, :c]
    assert_bits(got[:, :c], ref)
    assert_bits(got[:, c:c + ncls], np.repeat(y[:, :ncls], hw, axis=0))
    assert (bits(got[:, c + ncls:]) == 0).all()


# ------------------------------------------------------------------ pooling

def test_maxpool2_bwd_ties_go_to_the_first_maximum():
    """tg_maxpool2_bwd_f32 (gradient of tf.nn.max_pool 2x2 + dropout, Good_GAN_cifar10.py:123-124): TF's MaxPoolGrad routes a tie to the
    first maximum in row-major window order; the routed gradient is conserved; ld_dy > c keeps its padding untouched."""
    L = lib()
    rng = np.random.default_rng(11)
    for (n, h, w, c, ld_y, ld_do, ld_dy, with_mask) in [(4, 8, 8, 13, 16, 13, 16, True), (2, 2, 2, 1, 1, 1, 1, False),
                                                         (200, 32, 32, 32, 32, 32, 32, True)]:
        y = rng.integers(-2, 2, (n, h, w, ld_y)).astype(np.float32)       # few distinct values: ties everywhere
        y[0, :2, :2, :] = -3.0                                             # an all-equal window
        dout = rng.standard_normal((n, h // 2, w // 2, ld_do)).astype(np.float32)
        m = (rng.random((n, h // 2, w // 2, c)) < 0.7).astype(np.float32)
        dy = guarded(n * h * w * ld_dy, fill=np.full(n * h * w * ld_dy, 9.0, np.float32))
        dy.t.view(n * h * w, ld_dy)[:, :c] = float('nan')
        L.call('tg_maxpool2_bwd_f32', ptr(dev(dout)), ld_do, ptr(dev(m)) if with_mask else None, c, float(MSCALE), ptr(dev(y)), ld_y, dy.ptr, ld_dy,
               n, h, w, c, st())
        got = finish(dy, (n, h, w, ld_dy))
        assert (got[..., c:] == 9.0).all(), "maxpool2_bwd wrote the padding of dy"
        win = y[..., :c].reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4, c)
        first = np.argmax(win, axis=3)                                     # NumPy: first occurrence of the maximum
        g = dout[..., :c] * (m * MSCALE) if with_mask else dout[..., :c]
        ref = np.zeros((n, h // 2, w // 2, 4, c), np.float32)
        np.put_along_axis(ref, first[:, :, :, None, :], g[:, :, :, None, :], axis=3)
        ref = ref.reshape(n, h // 2, w // 2, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h, w, c)
        assert_bits(got[..., :c], ref)
        assert_bits(got[..., :c].reshape(n, h // 2, 2, w // 2, 2, c).sum(axis=(2, 4)), g + np.float32(0))   # conserved (three +0 and g; -0 + 0 = +0)


GPOOL_CASES = [  # n, hw, c, ld_x, ld_out, ncls
    (100, 36, 192, 192, 224, 10),   # the 6x6 window of Good_GAN_cifar10.py:163, c + ncls < ld_out
    (100, 64, 128, 128, 160, 10),   # average_pooling2d(8) of Good_GAN_cifar10.py:94
    (7, 1, 5, 5, 8, 0),             # hw = 1, no labels
    (1, 36, 1, 1, 1, 0),            # one image, one channel
    (50, 64, 30, 32, 33, 3),        # c, ld not multiples of 4
    (5000, 4, 250, 256, 256, 0),    # 1.28 M outputs > 4 096 x 256 lanes
]


@pytest.mark.parametrize("case", GPOOL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_global_max_pool_forward_backward(case):
    """tg_gmaxpool_fwd_f32 / _bwd_f32 (the layer named avg_pool_0 is a global MAX pool, Good_GAN_cifar10.py:163): all-negative inputs (the
    maximum starts from p[0], not 0), forced ties (the gradient goes to the first pixel holding the maximum and is conserved)."""
    L = lib()
    n, hw, c, ld_x, ld_out, _ = case
    rng = np.random.default_rng(n + hw)
    x = -np.abs(rng.standard_normal((n, hw, ld_x))).astype(np.float32) - 0.5   # all negative
    x[:, :, :c][:, :, ::3] = np.round(x[:, :, :c][:, :, ::3])                   # ties
    x[:, :, c:] = np.nan
    xd = dev(x)
    out = guarded(n * ld_out)
    L.call('tg_gmaxpool_fwd_f32', ptr(xd), ld_x, out.ptr, ld_out, n, hw, c, st())
    got = finish(out, (n, ld_out))
    assert_bits(got[:, :c], x[:, :, :c].max(axis=1))
    assert (bits(got[:, c:]) == 0).all()
    dfeat = rng.standard_normal((n, ld_out)).astype(np.float32)
    ld_dx = ld_x + 3
    dx0 = np.full((n, hw, ld_dx), 9.0, np.float32)
    dx0[..., :c] = np.nan
    dx = guarded(n * hw * ld_dx, fill=dx0)
    L.call('tg_gmaxpool_bwd_f32', ptr(dev(dfeat)), ld_out, ptr(xd), ld_x, dx.ptr, ld_dx, n, hw, c, st())
    g = finish(dx, (n, hw, ld_dx))
    assert (g[..., c:] == 9.0).all(), "gmaxpool_bwd wrote the padding of dx"
    ref = np.zeros((n, hw, c), np.float32)
    np.put_along_axis(ref, np.argmax(x[:, :, :c], axis=1)[:, None, :], dfeat[:, None, :c], axis=1)
    assert_bits(g[..., :c], ref)
    assert_bits(g[..., :c].sum(axis=1), dfeat[:, :c])


@pytest.mark.parametrize("case", GPOOL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_global_avg_pool_concat(case):
    """tg_gavgpool_concat_f32 (average_pooling2d(8) + squeeze + concat(y), Good_GAN_cifar10.py:94-96): the comment's "same order of
    additions" holds — bit-exact against the fp32 sum in pixel order; also within the reduction bound of the float64 mean, which rejects
    a mean that misses the last pixel.  y = NULL with ncls = 0."""
    L = lib()
    n, hw, c, ld_x, ld_out, ncls = case
    rng = np.random.default_rng(n * 3 + hw)
    x = rng.standard_normal((n, hw, ld_x)).astype(np.float32)
    x[:, :, c:] = np.nan
    y = rng.standard_normal((n, max(ncls, 1))).astype(np.float32)
    out = guarded(n * ld_out)
    L.call('tg_gavgpool_concat_f32', ptr(dev(x)), ld_x, c, ptr(dev(y[:, :ncls])) if ncls else None, ncls, out.ptr, ld_out, n, hw, st())
    got = finish(out, (n, ld_out))
    seq = seq_sum32([x[:, q, :c] for q in range(hw)]) / np.float32(hw)
    assert_bits(got[:, :c], seq)
    x64 = x[:, :, :c].astype(np.float64)
    close(got[:, :c], x64.mean(axis=1), np.abs(x64).sum(axis=1) / hw)
    if hw > 1:
        assert rejected(got[:, :c], x64[:, :-1].sum(axis=1) / hw, np.abs(x64).sum(axis=1) / hw)
    assert_bits(got[:, c:c + ncls], y[:, :ncls])
    assert (bits(got[:, c + ncls:]) == 0).all()


@pytest.mark.parametrize("case", [(100, 64, 192, 192, 192, 192), (3, 1, 5, 8, 6, 7), (20, 36, 30, 32, 33, 34), (5000, 64, 4, 4, 4, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_global_avg_pool_backward(case):
    """tg_gavgpool_bwd_f32: out[n,p,k] = dfeat[n,k] / hw * act'(y[n,p,k]), padding zeroed (pointwise, K = 4 + the derivative's 2)."""
    L = lib()
    n, hw, c, ld_d, ld_y, ld_out = case
    rng = np.random.default_rng(hw + c)
    dfeat = padded(rng, n, c, ld_d)
    for a in ('lrelu', 'tanh'):
        y = np.full((n * hw, ld_y), np.nan, np.float32)
        y[:, :c] = y_for(rng, (n * hw, c), a)
        out = guarded(n * hw * ld_out)
        L.call('tg_gavgpool_bwd_f32', ptr(dev(dfeat)), ld_d, ptr(dev(y)), ld_y, out.ptr, ld_out, n, hw, c, L.ACT[a], float(ALPHA), st())
        got = finish(out, (n * hw, ld_out))
        assert (bits(got[:, c:]) == 0).all()
        g, gm = act_grad64(y[:, :c], a)
        d = np.repeat(dfeat[:, :c].astype(np.float64), hw, axis=0) / hw
        assert_pointwise(got[:, :c], d * g, np.abs(d) * gm, 6, a)


# ------------------------------------------------------------------ im2col / split-K reduction

@pytest.mark.parametrize("n,h,w,c,ld_out", [(4, 32, 32, 3, 32), (3, 5, 7, 13, 120), (2, 1, 6, 3, 28), (2, 6, 1, 3, 28), (1, 1, 1, 1, 12),
                                            (160, 32, 32, 3, 32)])
@pytest.mark.parametrize("with_add", [False, True])
def test_im2col3x3_add(n, h, w, c, ld_out, with_add):
    """tg_im2col3x3_add_f32 (the classifier's first conv as a K = 27 -> 32 product, Good_GAN_cifar10.py:104-106): 3x3 SAME patches of
    x + add, zero outside the image (every border, h = 1, w = 1) and in [9c, ld_out); bit-exact (one addition)."""
    L = lib()
    rng = np.random.default_rng(n * h + w * c)
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    add = (rng.standard_normal((n, h, w, c)) * 0.15).astype(np.float32)
    out = guarded(n * h * w * ld_out)
    L.call('tg_im2col3x3_add_f32', ptr(dev(x)), ptr(dev(add)) if with_add else None, n, h, w, c, out.ptr, ld_out, st())
    got = finish(out, (n, h, w, ld_out))
    src = x + add if with_add else x
    sp = np.zeros((n, h + 2, w + 2, c), np.float32)
    sp[:, 1:-1, 1:-1] = src
    ref = np.concatenate([sp[:, ty:ty + h, tx:tx + w] for ty in range(3) for tx in range(3)], axis=-1)
    assert_bits(got[..., :9 * c], ref)
    assert (bits(got[..., 9 * c:]) == 0).all()


@pytest.mark.parametrize("m,s_dim,n,ld_out,with_bias", [(100, 4, 192, 192, True), (1, 1, 4, 4, False), (3, 3, 8, 12, True),
                                                        (4500, 2, 1024, 1024, True)])
def test_splitk_reduce(m, s_dim, n, ld_out, with_bias):
    """tg_splitk_reduce_f32 (finishes a split-K dense product, the ZCA matmul of Good_GAN_cifar10.py:296): bias + sum_s part in slab
    order — bit-exact against that fp32 order, within the reduction bound of float64, and the bound rejects a sum missing the last slab.
    Columns [n, ld_out) are not the kernel's: they keep their contents."""
    L = lib()
    rng = np.random.default_rng(m + s_dim)
    part = rng.standard_normal((m, s_dim, n)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    o0 = np.full((m, ld_out), 3.25, np.float32)
    o0[:, :n] = np.nan
    out = guarded(m * ld_out, fill=o0)
    L.call('tg_splitk_reduce_f32', ptr(dev(part)), ptr(dev(bias)) if with_bias else None, out.ptr, ld_out, m, s_dim, n, st())
    got = finish(out, (m, ld_out))
    b32 = bias if with_bias else np.zeros(n, np.float32)
    assert_bits(got[:, :n], seq_sum32([part[:, s] for s in range(s_dim)], init=np.broadcast_to(b32, (m, n))))
    assert (got[:, n:] == 3.25).all()
    p64 = part.astype(np.float64)
    sabs = np.abs(p64).sum(axis=1) + np.abs(b32)
    close(got[:, :n], p64.sum(axis=1) + b32, sabs)
    assert rejected(got[:, :n], p64[:, :-1].sum(axis=1) + b32, sabs)


# ------------------------------------------------------------------ RNG

def test_rng_multi_equals_the_single_draws():
    """tg_rng_multi_f32 "bit-identical to the single calls (same counters)": every mode, n % 4 != 0, one job past the grid cap, 16 jobs,
    against tg_rng_uniform_f32 / _keep_mask_f32 / _normal_f32 / _onehot_f32 at the same (seed, step, stream_id)."""
    L = lib()
    state = torch.tensor([0x1234567890ABCDEF, (1 << 32) + 5], dtype=torch.int64, device='cuda')
    specs = [(0, 1, -1.0, 1.0), (1, 5, 0.7, 0.0), (2, 6, 0.15, 0.0), (3, 7, 10.0, 0.0), (0, 2100003, -1.0, 1.0), (2, 1, 1.0, 0.0),
             (1, 4096, 0.5, 0.0), (3, 1, 3.0, 0.0), (0, 250 * 100, -1.0, 1.0), (2, 3 * 32 * 32 * 50 + 1, 0.15, 0.0), (3, 250, 10.0, 0.0),
             (1, 33, 0.8, 0.0), (0, 9, 2.0, 5.0), (2, 10, 2.0, 0.0), (1, 11, 0.1, 0.0), (3, 2, 1.0, 0.0)]
    jobs = (L.RngJob * len(specs))()
    outs = []
    for i, (mode, n, a, b) in enumerate(specs):
        size = n * int(a) if mode == 3 else n
        o = guarded(size)
        outs.append(o)
        jobs[i] = L.RngJob(o.t.data_ptr(), n, mode, a, b, 100 + i)
    L.call('tg_rng_multi_f32', C.cast(jobs, C.c_void_p), len(specs), ptr(state), st())
    for i, (mode, n, a, b) in enumerate(specs):
        size = n * int(a) if mode == 3 else n
        ref = guarded(size)
        sid = 100 + i
        if mode == 0:
            L.call('tg_rng_uniform_f32', ref.ptr, n, a, b, ptr(state), sid, st())
        elif mode == 1:
            L.call('tg_rng_keep_mask_f32', ref.ptr, n, a, ptr(state), sid, st())
        elif mode == 2:
            L.call('tg_rng_normal_f32', ref.ptr, n, a, ptr(state), sid, st())
        else:
            L.call('tg_rng_onehot_f32', ref.ptr, n, int(a), ptr(state), sid, st())
        got = finish(outs[i])
        assert_bits(got, finish(ref), "job %d (mode %d, n %d)" % (i, mode, n))
        if mode == 0:
            assert (got >= a).all() and (got <= b).all()
        if mode == 3:
            assert (got.reshape(n, int(a)).sum(axis=1) == 1).all()


# ------------------------------------------------------------------ the input pipeline's device tail
U8_N = 4096 * 256 + 77                    # past the 4 096-workgroup cap of ew_grid: the grid-stride loop takes a second turn


@pytest.mark.parametrize("scale,shift", [(2.0, -1.0), (1.0, 0.0)], ids=['cifar', 'mnist'])
def test_u8_affine(scale, shift):
    """tg_u8_affine_f32: float(x) / 255 * scale + shift (Input_Pipeline/cifar10Dataset.py:52-60: x / 255 * 2 - 1; MNIST: x / 255) — all 256 byte
    values, a source at an odd byte offset, n past the grid cap.  Bit-exact against the fp32 host expression: the division is correctly
    rounded on both sides, and both scales are powers of two, so the product is exact and a contraction of `* scale + shift` into an FMA
    could not change a bit (the library is built with -ffp-contract=off in any case)."""
    L = lib()
    rng = np.random.default_rng(int(scale))
    src = rng.integers(0, 256, U8_N + 1).astype(np.uint8)
    src[1:257] = np.arange(256)
    src[-256:] = np.arange(256)[::-1]
    sd = torch.from_numpy(src).cuda()
    out = guarded(U8_N)
    L.call('tg_u8_affine_f32', C.c_void_p(sd.data_ptr() + 1), out.ptr, U8_N, scale, shift, st())
    ref = src[1:].astype(np.float32) / np.float32(255) * np.float32(scale) + np.float32(shift)
    assert ref.dtype == np.float32 and len(np.unique(src[1:])) == 256
    assert_bits(finish(out), ref, "u8_affine")


@pytest.mark.parametrize("k,n", [(1, U8_N), (10, 104900), (100, 10500)])
def test_onehot_i32(k, n):
    """tg_onehot_i32_f32: out[r][j] = (labels[r] == j); labels -1 and k give an all-zero row; n * k past the grid cap of ew_grid."""
    L = lib()
    assert n * k > 4096 * 256
    rng = np.random.default_rng(k)
    lab = rng.integers(0, k, n).astype(np.int32)
    lab[3], lab[4], lab[n - 1], lab[n - 2] = -1, k, k - 1, -1
    ld = torch.from_numpy(lab).cuda()
    out = guarded(n * k)
    L.call('tg_onehot_i32_f32', C.c_void_p(ld.data_ptr()), out.ptr, n, k, st())
    ref = (lab[:, None] == np.arange(k)[None, :]).astype(np.float32)
    assert not ref[3].any() and not ref[4].any() and ref[n - 1, k - 1] == 1
    assert_bits(finish(out, (n, k)), ref, "onehot_i32")
