"""Per-kernel float64 tests of csrc/wgan_gp.hip called directly: the interpolation of _gradient_penalty (Training/train_base.py:601-606), the
penalty on an NHWC input gradient (slopes over H) and on a rank-2 one (slopes over the features), the stand-alone WGAN loss and the three
replayable heads of the training step.  References, inputs, bounds and their derivation: tests/wgan_kernels_reference.py (which states the
tolerance class of every output and each pointwise K as a count of roundings); tests/test_wgan_kernels_reference.py shows on the CPU that
an fp32 evaluation of the same inputs passes these bounds and that every negative control used here is rejected.

Every test: outputs are kernel_check.guarded allocations (NaN before the launch, a bit pattern behind them) read through `finish`; every
launch runs twice into fresh buffers and must give the same bits; input padding holds NaN; padding the kernel owns is exactly 0.0; the
deliberate s = 0 column / row is non-finite (as TF's sqrt gradient) and excluded from `finish` through its `owned` mask."""
import numpy as np
import pytest

import wgan_kernels_reference as R
from kernel_check import U, assert_bits, assert_pointwise, bits, close, dev, finish, guarded, lib, ptr, rejected, st

pytestmark = pytest.mark.gpu
ids = lambda s: "x".join(map(str, s))
f4, f8 = np.float32, R.f8


def twice(run):
    """two launches into fresh buffers: the same bits; returns the first launch's outputs."""
    a, b = run(), run()
    for i, (x, y) in enumerate(zip(a, b)):
        assert (bits(x) == bits(y)).all(), "output %d differs between two launches" % i
    return a


def finish_doubles(g):
    """`finish` for the penalty's block partials, doubles in a guarded float allocation of exactly twice their number: guard intact, and
    every double written (half of a double may look like a float NaN: the never-written fill is read as doubles, where it is NaN too)."""
    g.check_guard()
    d = g.get().view(np.float64)
    assert not np.isnan(d).any(), "%d partials were never written" % int(np.isnan(d).sum())
    return d


def zero_padding(got, c, what):
    assert (bits(got[..., c:]) == 0).all(), "%s: padding not exactly 0.0" % what


@pytest.mark.parametrize("case", R.INTERP_CASES, ids=ids)
def test_interp(case):
    """tg_wgan_interp_f32: out = real + alpha (fake - real), one alpha per image, three different row strides; the second case is just past
    4096 x 256 elements, so the grid-stride loop takes a second turn."""
    L = lib()
    n, hw, c, ld_r, ld_f, ld_out = case
    real, fake, alpha = R.interp_case(case)
    rd, fd, ad = dev(real), dev(fake), dev(alpha)

    def run():
        out = guarded(n * hw * ld_out)
        L.call('tg_wgan_interp_f32', ptr(rd), ld_r, ptr(fd), ld_f, ptr(ad), out.ptr, ld_out, n, hw, c, st())
        return (finish(out, (n * hw, ld_out)),)

    got, = twice(run)
    ref, mag = R.interp(real, fake, alpha, hw, c)
    assert_pointwise(got[:, :c], ref, mag, R.K_INTERP, "interp")
    assert_bits(got[:hw, :c], real[:hw, :c], "rows of alpha = 0")
    zero_padding(got, c, "out")


@pytest.mark.parametrize("case", R.GP_CASES, ids=ids)
def test_grad_penalty(case):
    """tg_grad_penalty_f32: one thread per column of the padded [n, w, ld_r] index; n w ld_r is below, a non-multiple of and above the block."""
    L = lib()
    n, h, w, c, ld_g, ld_r = case
    weight = R.GP_WEIGHT
    g = R.gp_case(case)
    gd = dev(g)
    nb = (n * w * ld_r + R.BLK - 1) // R.BLK
    r_ref, mag, gp_ref, bound, s = R.gp_columns(g, c, weight)
    ok = np.broadcast_to(s > 0, r_ref.shape)
    owned = np.ones((n, h, w, ld_r), bool)
    owned[..., :c] = ok

    def run():
        r, gp, part = guarded(n * h * w * ld_r), guarded(1), guarded(2 * nb)
        L.call('tg_grad_penalty_f32', ptr(gd), ld_g, n, h, w, c, weight, r.ptr, ld_r, part.ptr, gp.ptr, st())
        return finish(r, (n, h, w, ld_r), owned=owned), finish(gp), finish_doubles(part).view(np.float32)

    got_r, got_gp, part = twice(run)
    assert not np.isfinite(got_r[..., :c][~ok]).any(), "s = 0 gives a non-finite gradient, as TF's sqrt gradient (not masked)"
    assert_pointwise(got_r[..., :c][ok], r_ref[ok], mag[ok], R.k_gp_r(h), "r")
    zero_padding(got_r, c, "r")
    close(got_gp[0], gp_ref, R.as_terms(bound), "gp")
    close(part.view(np.float64).sum() * weight / (n * w * c), gp_ref, R.as_terms(bound), "sum of the block partials")
    r_short, _, gp_short, _, _ = R.gp_columns(g, c, weight, drop_last=True)
    assert rejected(got_gp[0], gp_short, R.as_terms(bound)), "the bound on gp does not reject the slopes without their last y"
    if h > 1:
        col = (n - 1, slice(None), w - 1, c - 1)
        assert rejected(got_r[col], r_short[col], R.as_terms(R.k_gp_r(h) * U * mag[col])), "the bound on r does not reject a column without its last y"


def run_rows(case, misalign=None):
    L = lib()
    n, f, ld_g, ld_r = case
    weight = R.GP_WEIGHT
    vec = R.rows_vec(case, aligned=misalign is None)
    g = R.rows_case(case)
    gbuf = dev(np.concatenate([[np.nan], g.reshape(-1)]))                      # gx one float into its allocation, or at its start
    gd = gbuf[1:] if misalign == 'gx' else dev(g)
    assert (gd.data_ptr() % 16 != 0) == (misalign == 'gx')
    r_ref, mag, gp_ref, bound, s = R.gp_rows(g, f, weight)
    ok = np.broadcast_to(s > 0, r_ref.shape)
    owned = np.ones((n, ld_r), bool)
    owned[:, :f] = ok

    def run():
        r, gp, part = guarded(n * ld_r, offset=1 if misalign == 'r' else 0), guarded(1), guarded(2 * n)
        assert (r.t.data_ptr() % 16 != 0) == (misalign == 'r')
        L.call('tg_grad_penalty_rows_f32', ptr(gd), ld_g, n, f, weight, r.ptr, ld_r, part.ptr, gp.ptr, st())
        return finish(r, (n, ld_r), owned=owned), finish(gp), finish_doubles(part).view(np.float32)

    got_r, got_gp, part = twice(run)
    assert (n >= 3) == (not ok.all())
    assert not np.isfinite(got_r[:, :f][~ok]).any(), "s = 0 gives a non-finite gradient, as TF's sqrt gradient (not masked)"
    assert_pointwise(got_r[:, :f][ok], r_ref[ok], mag[ok], R.K_ROWS_R, "r")
    zero_padding(got_r, f, "r")
    close(got_gp[0], gp_ref, R.as_terms(bound), "gp")
    close(part.view(np.float64).sum() * weight / n, gp_ref, R.as_terms(bound), "sum of the row partials")
    r_short, _, gp_short, _, _ = R.gp_rows(g, f, weight, drop=vec)
    assert rejected(got_gp[0], gp_short, R.as_terms(bound)), "the bound on gp does not reject the row sums without their last vector"
    if f > vec:
        assert rejected(got_r[0, :f], r_short[0], R.as_terms(R.K_ROWS_R * U * mag[0])), "the bound on r does not reject a row sum without its last vector"


@pytest.mark.parametrize("case", R.ROWS_CASES, ids=ids)
def test_grad_penalty_rows(case):
    """tg_grad_penalty_rows_f32: one workgroup per row; float4 and scalar loads, each with rows inside and beyond the 4 x 256 vectors a
    workgroup keeps in registers (the tail loops of the sum and of the write)."""
    run_rows(case)


@pytest.mark.parametrize("misalign", ['r', 'gx'])
def test_grad_penalty_rows_misaligned_pointer(misalign):
    """f, ld_g and ld_r are multiples of 4 but r (or gx) starts 4 bytes off a 16-byte boundary: the launch must take the scalar path."""
    run_rows(R.ROWS_MISALIGNED, misalign)


def launch_wgan_loss(L, zd, groups, ld, ld_d, ld_df, with_dfake=True):
    n = sum(groups)
    dz, loss = guarded(n * ld_d), guarded(5)
    dfake = guarded(groups[1] * ld_df) if with_dfake else None
    L.call('tg_wgan_loss_f32', ptr(zd), ld, groups[0], groups[1], groups[2], float(R.LAMBDAS[0]), float(R.LAMBDAS[1]), dz.ptr, ld_d,
           dfake.ptr if with_dfake else None, ld_df, loss.ptr, st())
    return (finish(dz, (n, ld_d)), finish(loss)) + ((finish(dfake, (groups[1], ld_df)),) if with_dfake else ())


def check_wasserstein(z, groups, got_vals, got_dz, which=range(5)):
    """values (d_loss, g_loss, wd1, wd2, wd3)[which] in the reduction class with each group's control, dz pointwise, its padding 0."""
    vals, sabs, g, gmag, gfake = R.wasserstein(z, groups, R.LAMBDAS)
    for i, got in zip(which, got_vals):
        close(got, vals[i], sabs[i], "value %d" % i)
    for grp, rows in enumerate(groups):
        if rows > 1:
            short = R.wasserstein(z, groups, R.LAMBDAS, drop=grp)[0]
            for i, got in zip(which, got_vals):
                if i in R.WD_GROUP_VALUES[grp]:
                    assert rejected(got, short[i], sabs[i]), "the bound on value %d does not reject the mean without the last row of group %d" % (i, grp)
    assert_pointwise(got_dz[:, 0], g, gmag, R.K_DZ, "dz")
    zero_padding(got_dz, 1, "dz")
    return gfake


@pytest.mark.parametrize("case,with_dfake", [(c, True) for c in R.WGAN_LOSS_CASES] + [(R.WGAN_LOSS_CASES[1], False)],
                         ids=lambda v: ids(v) if isinstance(v, tuple) else ("dfake" if v else "null"))
def test_wgan_loss(case, with_dfake):
    """tg_wgan_loss_f32: loss[5] = {d_loss, g_loss, wd1, wd2, wd3} against wgan_gp_reference.wgan_loss_head; 558 rows wrap the 256-thread row
    loop; dfake may be NULL."""
    L = lib()
    groups, (ld, ld_d, ld_df) = case[:3], case[3:]
    z = R.wd_case(groups, ld)
    zd = dev(z)
    out = twice(lambda: launch_wgan_loss(L, zd, groups, ld, ld_d, ld_df, with_dfake))
    gfake = check_wasserstein(z, groups, out[1], out[0])
    if with_dfake:
        assert_pointwise(out[2][:, 0], gfake, np.abs(gfake), R.K_DFAKE, "dfake")
        zero_padding(out[2], 1, "dfake")
    else:
        assert_bits(out[0], launch_wgan_loss(L, zd, groups, ld, ld_d, ld_df)[0], "dz with and without dfake")


@pytest.mark.parametrize("case", R.D_HEAD_CASES, ids=ids)
def test_d_head(case):
    """tg_wgan_d_head_f32: lambdas and the weighted penalty from device memory.  wgan_d_head and wgan_loss inline the same `wasserstein`
    (csrc/wgan_gp.hip) and the lambdas reach it as the same fp32 values, so terms[:3] and dz are the bits tg_wgan_loss_f32 writes on the same
    rows and loss is the fp32 sum of its d_loss and gp_w; terms may be NULL."""
    L = lib()
    groups, (ld, ld_d) = case[:3], case[3:]
    n = sum(groups)
    z = R.wd_case(groups, ld)
    gp_w, gp_weight = f4(3.25), 10.0
    zd, lam, gpd = dev(z), dev(R.LAMBDAS), dev([gp_w])

    def run(with_terms=True):
        dz, loss, terms = guarded(n * ld_d), guarded(1), guarded(4) if with_terms else None
        L.call('tg_wgan_d_head_f32', ptr(zd), ld, groups[0], groups[1], groups[2], ptr(lam), ptr(gpd), gp_weight, dz.ptr, ld_d, loss.ptr,
               terms.ptr if with_terms else None, st())
        return (finish(dz, (n, ld_d)), finish(loss)) + ((finish(terms),) if with_terms else ())

    got_dz, got_loss, got_terms = twice(run)
    no_terms = twice(lambda: run(False))
    assert_bits(no_terms[0], got_dz, "dz without terms")
    assert_bits(no_terms[1], got_loss, "loss without terms")
    check_wasserstein(z, groups, got_terms[:3], got_dz, which=[2, 3, 4])
    vals, sabs = R.wasserstein(z, groups, R.LAMBDAS)[:2]
    close(got_loss[0], vals[0] + f8(gp_w), sabs[0] + f8(gp_w), "loss")
    assert_pointwise(got_terms[3], f8(gp_w) / gp_weight, f8(gp_w) / gp_weight, 1, "terms[3]")
    ref_dz, ref_loss, _ = launch_wgan_loss(L, zd, groups, ld, ld_d, 1)
    assert_bits(got_dz, ref_dz, "dz of the d head vs tg_wgan_loss_f32")
    assert_bits(got_terms[:3], ref_loss[2:], "terms[:3] of the d head vs tg_wgan_loss_f32")
    assert_bits(got_loss, ref_loss[:1] + gp_w, "loss of the d head vs d_loss of tg_wgan_loss_f32 + gp_w")


@pytest.mark.parametrize("case", R.G_HEAD_CASES, ids=ids)
def test_g_head(case):
    """tg_wgan_g_head_f32: loss = -mean z, dz = -1 / n."""
    L = lib()
    n, ld, ld_d = case
    z = R.g_head_case(n, ld)
    zd = dev(z)

    def run():
        dz, loss = guarded(n * ld_d), guarded(1)
        L.call('tg_wgan_g_head_f32', ptr(zd), ld, n, dz.ptr, ld_d, loss.ptr, st())
        return finish(dz, (n, ld_d)), finish(loss)

    got_dz, got_loss = twice(run)
    val, sabs, dz = R.g_head(z)
    close(got_loss[0], val, sabs, "loss")
    if n > 1:
        assert rejected(got_loss[0], R.g_head(z, drop=True)[0], sabs), "the bound does not reject the mean without the last row"
    assert_pointwise(got_dz[:, 0], dz, np.abs(dz), R.K_DFAKE, "dz")
    zero_padding(got_dz, 1, "dz")


@pytest.mark.parametrize("case", R.C_HEAD_CASES, ids=ids)
def test_c_head(case):
    """tg_wgan_c_head_f32: rows [real | zero | fake]; the zero rows' logits are NaN throughout (the kernel writes 0 there and reads nothing);
    without fake rows y_fake and lambdas are NULL; terms may be NULL."""
    L = lib()
    n_real, n_zero, n_fake, k, ld, ld_d = case
    n = n_real + n_zero + n_fake
    z, y_real, y_fake = R.c_head_case(case)
    zd, yr = dev(z), dev(y_real)
    yf, lam = (dev(y_fake), dev(R.C_LAMBDAS)) if n_fake else (None, None)

    def run(with_terms=True):
        dl, loss, terms = guarded(n * ld_d), guarded(1), guarded(2) if with_terms else None
        L.call('tg_wgan_c_head_f32', ptr(zd), ld, n_real, n_zero, n_fake, k, ptr(yr), ptr(yf), ptr(lam), dl.ptr, ld_d, loss.ptr,
               terms.ptr if with_terms else None, st())
        return (finish(dl, (n, ld_d)), finish(loss)) + ((finish(terms),) if with_terms else ())

    got_dl, got_loss, got_terms = twice(run)
    no_terms = twice(lambda: run(False))
    assert_bits(no_terms[0], got_dl, "dl without terms")
    assert_bits(no_terms[1], got_loss, "loss without terms")
    vals, sabs, dl, mag = R.c_head(z, y_real, y_fake, case, R.C_LAMBDAS)
    got_vals = np.array([got_loss[0], got_terms[0], got_terms[1]])
    close(got_vals, vals, sabs, "(loss, t_real, t_fake)")
    for grp, rows in enumerate((n_real, n_fake)):
        if rows > 1:
            short = R.c_head(z, y_real, y_fake, case, R.C_LAMBDAS, drop=grp)[0]
            assert rejected(got_vals[1 + grp], short[1 + grp], sabs[1 + grp]) and rejected(got_vals[0], short[0], sabs[0]), \
                "the bounds do not reject the mean without the last row of group %d" % grp
    if n_fake == 0:
        assert bits(got_terms[1]) == 0, "t_fake without fake rows"
    lab = np.r_[0:n_real, n_real + n_zero:n]
    assert_pointwise(got_dl[lab, :k], dl[lab], mag[lab], R.k_c_head(k), "dl")
    assert (bits(got_dl[n_real:n_real + n_zero]) == 0).all(), "the zero rows' gradient is not exactly 0.0"
    zero_padding(got_dl, k, "dl")
