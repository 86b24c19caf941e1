"""CPU check of tests/wgan_kernels_reference.py on the very inputs the GPU tests use (its case builders): an fp32 NumPy evaluation in the
kernel's order stays inside every bound the GPU tests apply, and every negative control (without the last row of a group, the last slab,
the last y of a column, the last vector of a row) is rejected by kernel_check.rejected with factor 10 — so a GPU test that fails means the
kernel, and one that passes could have failed."""
import numpy as np
import pytest

import wgan_kernels_reference as R
from kernel_check import U, assert_bits, assert_pointwise, bits, close, rejected

ids = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("case", R.INTERP_CASES, ids=ids)
def test_interp(case):
    n, hw, c, ld_r, ld_f, ld_out = case
    real, fake, alpha = R.interp_case(case)
    assert np.isnan(real[:, c:]).all() and np.isnan(fake[:, c:]).all() and n * hw * ld_out > (4096 * 256 if n > 3 else 0)
    ref, mag = R.interp(real, fake, alpha, hw, c)
    got = R.interp32(real, fake, alpha, hw, c)
    assert_pointwise(got, ref, mag, R.K_INTERP, "interp")
    assert_bits(got[:hw], real[:hw, :c], "alpha = 0")


@pytest.mark.parametrize("case", R.GP_CASES, ids=ids)
def test_gp_columns(case):
    n, h, w, c, ld_g, ld_r = case
    g = R.gp_case(case)
    r, mag, gp, bound, s = R.gp_columns(g, c, R.GP_WEIGHT)
    got_r, got_gp = R.gp_columns32(g, c, R.GP_WEIGHT)
    ok = np.broadcast_to(s > 0, r.shape)
    assert (n * w * c == 1) == bool(ok.all()), "one s = 0 column wherever there is more than one column"
    assert not np.isfinite(got_r[~ok]).any()
    assert_pointwise(got_r[ok], r[ok], mag[ok], R.k_gp_r(h), "r")
    close(got_gp, gp, R.as_terms(bound), "gp")
    r_short, _, gp_short, _, _ = R.gp_columns(g, c, R.GP_WEIGHT, drop_last=True)
    assert rejected(got_gp, gp_short, R.as_terms(bound)), "gp without the last y"
    if h > 1:
        col = (n - 1, slice(None), w - 1, c - 1)
        assert rejected(got_r[col], r_short[col], R.as_terms(R.k_gp_r(h) * U * mag[col])), "one column of r without its last y"


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("case", R.ROWS_CASES + [R.ROWS_MISALIGNED], ids=ids)
def test_gp_rows(case, aligned):
    n, f, ld_g, ld_r = case
    vec = R.rows_vec(case, aligned)
    g = R.rows_case(case)
    r, mag, gp, bound, s = R.gp_rows(g, f, R.GP_WEIGHT)
    got_r, got_gp = R.gp_rows32(g, f, R.GP_WEIGHT, vec)
    ok = np.broadcast_to(s > 0, r.shape)
    assert (n >= 3) == (not ok.all())
    assert not np.isfinite(got_r[~ok]).any()
    assert_pointwise(got_r[ok], r[ok], mag[ok], R.K_ROWS_R, "r")
    close(got_gp, gp, R.as_terms(bound), "gp")
    r_short, _, gp_short, _, _ = R.gp_rows(g, f, R.GP_WEIGHT, drop=vec)
    assert rejected(got_gp, gp_short, R.as_terms(bound)), "gp without the last vector"
    if f > vec:
        assert rejected(got_r[0], r_short[0], R.as_terms(R.K_ROWS_R * U * mag[0])), "a row of r without its last vector"


def test_rows_cases_reach_both_paths_and_their_tail_loops():
    """float4 and scalar, each with a row that fits the registers (4 x 256 vectors) and one that does not; the misaligned case would be
    float4 if aligned."""
    seen = {(R.rows_vec(c), c[1] // R.rows_vec(c) > 4 * R.BLK) for c in R.ROWS_CASES}
    assert seen == {(4, False), (4, True), (1, False), (1, True)}
    assert R.rows_vec(R.ROWS_MISALIGNED) == 4 and R.rows_vec(R.ROWS_MISALIGNED, aligned=False) == 1


def check_wasserstein(z, groups, got):
    vals, sabs, g, gmag, gfake = R.wasserstein(z, groups, R.LAMBDAS)
    got_vals, got_dz, got_df = got
    close(got_vals, vals, sabs, "(d_loss, g_loss, wd1, wd2, wd3)")
    assert_pointwise(got_dz, g, gmag, R.K_DZ, "dz")
    assert_pointwise(got_df, gfake, np.abs(gfake), R.K_DFAKE, "dfake")
    for grp, rows in enumerate(groups):
        if rows > 1:
            short = R.wasserstein(z, groups, R.LAMBDAS, drop=grp)[0]
            for i in R.WD_GROUP_VALUES[grp]:
                assert rejected(got_vals[i], short[i], sabs[i]), "value %d without the last row of group %d" % (i, grp)


@pytest.mark.parametrize("case", R.WGAN_LOSS_CASES + [c + (1,) for c in R.D_HEAD_CASES], ids=ids)
def test_wasserstein(case):
    groups, ld = case[:3], case[3]
    z = R.wd_case(groups, ld)
    assert np.isnan(z[:, 1:]).all()
    check_wasserstein(z, groups, R.wasserstein32(z, groups, R.LAMBDAS))


@pytest.mark.parametrize("case", R.G_HEAD_CASES, ids=ids)
def test_g_head(case):
    n, ld, ld_d = case
    z = R.g_head_case(n, ld)
    val, sabs, dz = R.g_head(z)
    got, got_dz = R.g_head32(z)
    close(got, val, sabs, "loss")
    assert_pointwise(got_dz, dz, np.abs(dz), R.K_DFAKE, "dz")
    if n > 1:
        assert rejected(got, R.g_head(z, drop=True)[0], sabs)


@pytest.mark.parametrize("case", R.C_HEAD_CASES, ids=ids)
def test_c_head(case):
    n_real, n_zero, n_fake, k, ld, ld_d = case
    z, y_real, y_fake = R.c_head_case(case)
    assert np.isnan(z[n_real:n_real + n_zero]).all() and np.isnan(z[:, k:]).all()
    vals, sabs, dl, mag = R.c_head(z, y_real, y_fake, case, R.C_LAMBDAS)
    got_vals, got_dl = R.c_head32(z, y_real, y_fake, case, R.C_LAMBDAS)
    close(got_vals, vals, sabs, "(loss, t_real, t_fake)")
    lab = np.r_[0:n_real, n_real + n_zero:len(z)]
    assert_pointwise(got_dl[lab], dl[lab], mag[lab], R.k_c_head(k), "dl")
    for grp, rows in enumerate((n_real, n_fake)):
        if rows > 1:
            short = R.c_head(z, y_real, y_fake, case, R.C_LAMBDAS, drop=grp)[0]
            assert rejected(got_vals[1 + grp], short[1 + grp], sabs[1 + grp]) and rejected(got_vals[0], short[0], sabs[0]), grp


@pytest.mark.parametrize("case", R.G_LOSS_CASES, ids=ids)
def test_g_loss(case):
    n, ld, ld_d = case
    z = R.g_loss_case(case)
    assert np.isnan(z[:, 1:]).all() and (n < 17 or ((z[:, 0] == 80).any() and (z[:, 0] == -80).any()))
    val, sabs, dz, mag = R.g_loss(z)
    got, got_dz = R.g_loss32(z)
    close(got, val, sabs, "g_loss")
    assert_pointwise(got_dz, dz, mag, R.K_G_LOSS_DZ, "dz")
    if n > 1:
        assert rejected(got, R.g_loss(z, drop=True)[0], sabs)


@pytest.fixture(scope="module")
def slabs():
    return {case: R.slab_case(case) for case in R.SLAB_CASES}


@pytest.mark.parametrize("case", R.SLAB_CASES, ids=ids)
def test_slab_reduce(case, slabs):
    n_split, t, c_pad, n_pad, c, n = case
    slab = slabs[case]
    assert R.slab_path(case) == ('wide' if case in R.SLAB_WIDE else 'narrow')
    assert np.isnan(slab[:, :, c:]).all() and np.isnan(slab[:, :, :, n:]).all()
    got = R.slab32(case, slab)
    ref, sabs = R.slab64(slab, c, n)
    close(got, ref, sabs, "slab sum")
    assert rejected(got, R.slab64(slab, c, n, drop_last=True)[0], sabs), "the sum without the last slab"


def test_slab_paths_and_order(slabs):
    """the cases sit at the kernel's edges (the path switch at 32 slabs and 65536 outputs, the grid-stride wrap past 4096 x 256
    outputs, an empty trailing range), and the in-order restatements are not what a pairwise np.sum gives, nor each other."""
    total = lambda s: s[1] * s[4] * s[5]
    assert {total(s) for s in R.SLAB_WIDE} >= {65536} and 65792 in {total(s) for s in R.SLAB_NARROW}
    assert max(total(s) for s in R.SLAB_NARROW) == 1052703 > 4096 * 256
    assert (33 + 7) // 8 * 7 >= 33, "n_split = 33 leaves lane group 7 without slabs"
    differs = []
    for case in ((512, 1, 32, 128, 27, 128), (40, 1, 32, 32, 5, 7)):
        n_split, t, c_pad, n_pad, c, n = case
        slab = slabs[case]
        pairwise = np.ascontiguousarray(np.moveaxis(slab[:, :, :c, :n], 0, -1)).sum(axis=-1, dtype=np.float32)   # the slabs contiguous: pairwise
        wide, narrow = R.slab_wide32(slab, c, n), R.slab_narrow32(slab, c, n)
        differs.append(((bits(wide) != bits(pairwise)).any(), (bits(narrow) != bits(pairwise)).any(), (bits(wide) != bits(narrow)).any()))
    assert any(d[0] for d in differs) and any(d[1] for d in differs) and any(d[2] for d in differs), differs
    for case in R.SLAB_WIDE:                           # the bit-exact check sees the order of the partial sums (ranges 0 and 1 alone commute)
        slab = slabs[case]
        swapped = R.slab_wide32(slab, case[4], case[5], order=[0, 2, 1, 3, 4, 5, 6, 7])
        assert (bits(swapped) != bits(R.slab_wide32(slab, case[4], case[5]))).any(), case
