"""tg_r1_penalty_f32 (csrc/wgan_gp.hip; config.R1_GAMMA) called directly, against float64 (math.fsum of the exact products).

What is required of every case: r is BIT-equal to the float32 restatement r = g * (float)((double)gamma / (double)n) (one fp32 multiply
per element, tests/r1_reference.penalty_kernel32); out[0] = gamma / 2 * mean_i ||g_i||^2 and out[1] = mean_i ||g_i||^2 are within 1
float32 ulp of the fsum value — the kernel squares in double (the product of two floats is exact there) and sums at most 2^21 of them
in double, which errs by less than 2^21 * 2^-53 = 2^-32 relative, far inside the half ulp of the final rounding to float32, so 1 ulp is
derived, not measured; padding columns c..ld_r of r are exactly 0 (the input's padding holds NaN); an all-zero image gives r = 0 and
finite outputs; two launches give the same bits; a new value in gamma_dev changes the result of the same call.  Outputs are
kernel_check.guarded allocations.  Bad sizes and null pointers return the error code with a message; nothing here can fault the device."""
import math

import numpy as np
import pytest

import r1_reference as R
from kernel_check import assert_bits, bits, dev, finish, guarded, lib, ptr, st
from test_gpu_wgan_kernels import finish_doubles, twice

pytestmark = pytest.mark.gpu
ids = lambda s: "x".join(map(str, s))

#        n, rows,    c, ld_g, ld_r
CASES = [(1, 1, 1, 1, 1),                       # minimum size
         (2, 1, 3, 3, 3),                       # scalar path
         (3, 1, 4, 4, 4),                       # one float4
         (2, 1, 1029, 1029, 1029),              # a long row across block strides; an odd row stride keeps it off the float4 path
         (7, 5, 3, 32, 32),                     # channel-padded NHWC: float4 rows whose components at and beyond c do not count
         (1, 4096, 3, 3, 32),                   # one image larger than a workgroup holds: 12 288 values, scalar reads, padded r
         (5, 1, 784, 784, 784),                 # MNIST: float4 body across block strides
         (3, 1, 782, 784, 784),                 # float4 body across block strides whose LAST vector holds two valid columns and two of padding
         (2, 3, 6, 8, 8)]                       # several float4 rows per image, each row's second vector half valid


def _case(case, seed=0):
    n, rows, c, ld_g, ld_r = case
    rng = np.random.default_rng(seed + n * rows * c)
    g = np.full((n, rows, ld_g), np.nan, np.float32)
    g[..., :c] = (rng.standard_normal((n, rows, c)) * np.exp(rng.uniform(-3, 3, (n, 1, 1)))).astype(np.float32)
    if n >= 2:
        g[1, :, :c] = 0.0                                            # an all-zero image: r = 0, outputs finite
    return g


def _reference(g, c, gamma):
    """(out[0], out[1]) in float64 by fsum over the exact products, gamma as the float32 the device holds."""
    n = g.shape[0]
    v = g[..., :c].astype(np.float64).reshape(-1)
    m = math.fsum((v * v).tolist()) / n
    return 0.5 * float(np.float32(gamma)) * m, m


def _within_one_ulp(got, ref, what):
    assert np.isfinite(got), what
    assert abs(float(got) - ref) <= float(np.spacing(np.float32(ref))), "%s: got %.9g, fsum %.17g" % (what, got, ref)


def _launch(gd, case, gamma_dev):
    n, rows, c, ld_g, ld_r = case
    r, out, part = guarded(n * rows * ld_r), guarded(2), guarded(2 * n)
    lib().call('tg_r1_penalty_f32', ptr(gd), ld_g, n, rows, c, ptr(gamma_dev), r.ptr, ld_r, part.ptr, out.ptr, st())
    return finish(r, (n, rows, ld_r)), finish(out), finish_doubles(part).view(np.float32)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_r1_penalty(case):
    n, rows, c, ld_g, ld_r = case
    gamma = 10.0
    g = _case(case)
    gd, gamma_dev = dev(g), dev([gamma])
    got_r, got_out, part = twice(lambda: _launch(gd, case, gamma_dev))
    assert_bits(got_r[..., :c], R.penalty_kernel32(g[..., :c], gamma, n), "r")
    assert (bits(got_r[..., c:]) == 0).all(), "r: padding not exactly 0.0"
    ref = _reference(g, c, gamma)
    _within_one_ulp(got_out[0], ref[0], "out[0] = gamma / 2 * mean ||g||^2")
    _within_one_ulp(got_out[1], ref[1], "out[1] = mean ||g||^2")
    per_image = part.view(np.float64)
    for i in range(n):                                               # the partials are the per-image sums, in index order
        want = math.fsum((g[i, :, :c].astype(np.float64).reshape(-1) ** 2).tolist())
        assert abs(per_image[i] - want) <= 2.0 ** -32 * want, (i, per_image[i], want)
    if n >= 2:
        assert per_image[1] == 0.0 and (bits(got_r[1]) == 0).all(), "an all-zero image gives r = 0"
    # negative control: 1 ulp tells the sum from one that misses the last valid element of the last image
    short = g.copy()
    short[-1, -1, c - 1] = 0.0
    if g[-1, -1, c - 1] != 0.0 and abs(_reference(short, c, gamma)[1] - ref[1]) > 4 * float(np.spacing(np.float32(ref[1]))):
        assert abs(float(got_out[1]) - _reference(short, c, gamma)[1]) > float(np.spacing(np.float32(ref[1])))


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[6]], ids=ids)
def test_a_new_gamma_on_the_device_changes_the_same_call(case):
    """gamma is read from device memory by the kernels: the same arguments, another value behind the pointer."""
    n, rows, c, ld_g, ld_r = case
    g = _case(case, seed=3)
    gd, gamma_dev = dev(g), dev([10.0])
    r10, out10, _ = _launch(gd, case, gamma_dev)
    gamma_dev.fill_(0.3)
    r03, out03, _ = _launch(gd, case, gamma_dev)
    assert_bits(r10[..., :c], R.penalty_kernel32(g[..., :c], 10.0, n), "r at gamma 10")
    assert_bits(r03[..., :c], R.penalty_kernel32(g[..., :c], 0.3, n), "r at gamma 0.3")
    _within_one_ulp(out03[0], _reference(g, c, 0.3)[0], "out[0] at gamma 0.3")
    assert bits(out10[1]) == bits(out03[1]) and out10[0] != out03[0]          # the mean does not depend on gamma


def test_a_misaligned_pointer_takes_the_scalar_path_with_the_same_bits():
    case = (3, 2, 8, 8, 8)
    n, rows, c, ld_g, ld_r = case
    g = _case(case, seed=5)
    gamma_dev = dev([2.0])
    aligned = _launch(dev(g), case, gamma_dev)
    gbuf = dev(np.concatenate([[np.nan], g.reshape(-1)]))
    assert gbuf[1:].data_ptr() % 16 != 0
    shifted = _launch(gbuf[1:], case, gamma_dev)
    assert_bits(shifted[0], aligned[0], "r")
    # the per-thread order of the two paths differs, the double sums agree to their last bits' worth and the float32 results to 1 ulp
    for k in range(2):
        _within_one_ulp(shifted[1][k], _reference(g, c, 2.0)[k], "out[%d], scalar path" % k)
        _within_one_ulp(aligned[1][k], _reference(g, c, 2.0)[k], "out[%d], float4 path" % k)


def test_a_non_finite_gradient_propagates():
    case = (2, 1, 4, 4, 4)
    g = np.ones((2, 1, 4), np.float32)
    g[0, 0, 2] = np.inf
    r, out, _ = _launch(dev(g), case, dev([1.0]))
    assert np.isinf(r[0, 0, 2]) and np.isfinite(r[1]).all() and not np.isfinite(out).any()


def test_bad_arguments_return_the_error_code():
    """bad sizes and null pointers only: every one is refused before anything is launched, with a message naming the entry point."""
    L = lib()
    buf = dev(np.zeros(4096))
    good = dict(gx=ptr(buf), ld_g=4, n=2, rows=3, c=4, gamma=ptr(buf), r=ptr(buf), ld_r=4, partials=ptr(buf), out=ptr(buf))
    order = ('gx', 'ld_g', 'n', 'rows', 'c', 'gamma', 'r', 'ld_r', 'partials', 'out')
    bad = [dict(n=0), dict(n=-1), dict(rows=0), dict(c=0), dict(c=5), dict(ld_r=3), dict(ld_g=0), dict(n=(1 << 20) + 1),
           dict(rows=(1 << 21) + 1, c=1, ld_g=1, ld_r=1), dict(rows=1 << 27, c=1, ld_g=16, ld_r=16),
           dict(gx=None), dict(gamma=None), dict(r=None), dict(partials=None), dict(out=None)]
    for change in bad:
        args = dict(good, **change)
        with pytest.raises(L.TgError, match='r1_penalty'):
            L.call('tg_r1_penalty_f32', *[args[k] for k in order], st())
    import torch
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                             # nothing ran
