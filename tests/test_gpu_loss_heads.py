"""Per-kernel float64 tests of the stand-alone loss heads of csrc/loss.hip (the Train_base helper methods, Training/train_base.py:43-57,
75-84: softmax cross-entropy, sigmoid cross-entropy, entropy and balance entropy; restated as in oracle.tf_ops.softmax_ce_mean, bce_mean,
entropy, balance_entropy), of the discriminator head with its three terms (tg_d_loss_terms_f32), of the generator head (tg_g_loss_f32;
reference, inputs and bounds in tests/wgan_kernels_reference.py), of the squared row difference
(tg_sqdiff_rows_loss_f32, train_base.py:299) and of minibatch discrimination (csrc/mbd.hip, Model/modle_base.py:110-128) called directly.

The heads are single-workgroup loops: n = 1, 255, 256, 257 and 1000 rows; logits up to |z| = 80 (no inf / NaN: the stable forms
max(z,0) - z t + log1p(exp(-|z|)) and m + log sum exp(l - m) are what the kernels compute); accumulate = 1 adds onto an existing
gradient and leaves its padding as it was; accumulate = 0 zeroes the padding up to ld_d.

Tolerance classes (tests/kernel_check.py):
  reduction   the loss values (means over the rows) within TOL * sum|terms| / n, each with a negative control that drops the last row;
              the balance entropy within TOL of the sum of its terms' magnitudes and condition; minibatch discrimination f and dact within
              TOL * sum_j |term_j| (1 + s_j) (s = the L1 distance: exp(-s) turns an absolute error of s into a relative one), with the
              negative control dropping the last j; db = sum_i df in row order, bit-exact and within the bound;
  pointwise   the gradients: 2u times a magnitude that carries each softmax probability's condition (20 + |l - max l|: the rounding of
              l - max l, expf, the sum of ten terms and the division) — so a logit 160 below the row maximum is allowed its larger relative
              error while its absolute error stays far below the bound of the row's large entries; plus FLT_MIN (times the balance
              term's |dq|), since a probability below FLT_MIN may be flushed to zero."""
import numpy as np
import pytest

import wgan_kernels_reference as WR
from kernel_check import FLT_MIN, TOL, U, assert_bits, assert_pointwise, bits, close, dev, finish, guarded, lib, ptr, rejected, seq_sum32, st

pytestmark = pytest.mark.gpu

K = 10
NS = [1, 255, 256, 257, 1000]
f8 = lambda a: np.asarray(a, np.float64)


def logits(rng, n, ld, scale=30.0):
    z = np.full((n, ld), np.nan, np.float32)
    v = np.clip(rng.standard_normal((n, K)) * scale, -80, 80)
    v[::17, 3] = 80.0
    v[::13, 5] = -80.0
    v[-1] = rng.standard_normal(K)                 # a moderate last row: the negative controls drop it
    z[:, :K] = v.astype(np.float32)
    return z


def softmax64(l):
    m = l.max(axis=1, keepdims=True)
    e = np.exp(l - m)
    s = e.sum(axis=1, keepdims=True)
    return e / s, (m + np.log(s))[:, 0], l - m


def grad_buffer(n, ld_d, acc, rng):
    """dlogits before the call: NaN (accumulate = 0), or existing values with NaN padding that must stay (accumulate = 1)."""
    g0 = np.full((n, ld_d), np.nan, np.float32)
    if acc:
        g0[:, :K] = (rng.standard_normal((n, K)) * 1e-2).astype(np.float32)
    return g0


def check_padding(got, g0, c, acc):
    if acc:
        assert_bits(got[:, c:], g0[:, c:], "accumulate = 1 touched the padding")
    else:
        assert (bits(got[:, c:]) == 0).all(), "padding not zeroed"


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("acc", [0, 1])
def test_softmax_ce(n, acc):
    """tg_softmax_ce_f32: T = mean_n (lse * sum_k y - sum_k y l) (tf.nn.softmax_cross_entropy_with_logits_v2 + reduce_mean,
    train_base.py:75-79), loss = {w T, T}, d/dlogits = w (p sum_k y - y) / n written or added."""
    L = lib()
    rng = np.random.default_rng(n + acc)
    ld, ld_d, w = 16, 32, np.float32(0.3)
    z = logits(rng, n, ld)
    y = np.eye(K, dtype=np.float32)[rng.integers(0, K, n)]
    y[::3] = rng.random((len(y[::3]), K)).astype(np.float32)      # soft labels (sum != 1) as well
    g0 = grad_buffer(n, ld_d, acc, rng)
    dz, loss = guarded(n * ld_d, fill=g0), guarded(2)
    L.call('tg_softmax_ce_f32', ptr(dev(z)), ld, ptr(dev(y)), n, K, float(w), dz.ptr, ld_d, acc, loss.ptr, st())
    got, lv = finish(dz, (n, ld_d), owned=np.broadcast_to(np.arange(ld_d) < K, (n, ld_d)) if acc else None), finish(loss)
    l, y64 = f8(z[:, :K]), f8(y)
    p, lse, d = softmax64(l)
    ysum = y64.sum(1)
    terms = lse * ysum - (y64 * l).sum(1)
    mag = np.abs(lse * ysum) + np.abs(y64 * l).sum(1)
    close(lv[1], terms.sum() / n, mag.sum() / n, "T")
    close(lv[0], f8(w) * terms.sum() / n, abs(f8(w)) * mag.sum() / n, "w T")
    assert rejected(lv[1], terms[:-1].sum() / n, mag.sum() / n), "the bound does not reject a mean without the last row"
    ref = f8(w) * (p * ysum[:, None] - y64) / n + (f8(g0[:, :K]) if acc else 0)
    gmag = abs(f8(w)) / n * (p * np.abs(ysum)[:, None] * (20 + np.abs(d)) + np.abs(y64)) + (np.abs(f8(g0[:, :K])) if acc else 0)
    assert_pointwise(got[:, :K], ref, gmag, 2, "dlogits", floor=FLT_MIN)
    check_padding(got, g0, K, acc)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("labels", ['given', 'ones', 'zeros'])
@pytest.mark.parametrize("acc", [0, 1])
def test_bce_logits(n, labels, acc):
    """tg_bce_logits_f32: T = mean over n*c of max(z,0) - z t + log1p(exp(-|z|)) (tf.nn.sigmoid_cross_entropy_with_logits + reduce_mean,
    train_base.py:81-84); labels NULL = the constant label (tf.ones_like / zeros_like, :123-128), held to the same reference as the
    equal labels given as a tensor; d/dlogits = w (sigmoid(z) - t) / (n c)."""
    L = lib()
    rng = np.random.default_rng(n * 3 + acc)
    c, ld, ld_y, ld_d, w = 3, 4, 5, 8, np.float32(0.5)
    if labels == 'given':
        t = np.full((n, ld_y), np.nan, np.float32)
        t[:, :c] = rng.random((n, c)).astype(np.float32)
        t64, lab, const = f8(t[:, :c]), dev(t), 0.0
    else:
        const = 1.0 if labels == 'ones' else 0.0
        t64, lab = np.full((n, c), const), None
    z = np.full((n, ld), np.nan, np.float32)
    zz = np.clip(rng.standard_normal((n, c)) * 30, -80, 80)
    zz[::7, 0], zz[::11, 1] = 80.0, -80.0
    zz[-1] = np.where(t64[-1] < 0.5, 5.0, -5.0)           # a last row of large terms: the negative control drops it
    z[:, :c] = zz.astype(np.float32)
    g0 = np.full((n, ld_d), np.nan, np.float32)
    if acc:
        g0[:, :c] = (rng.standard_normal((n, c)) * 1e-2).astype(np.float32)
    dz, loss = guarded(n * ld_d, fill=g0), guarded(2)
    L.call('tg_bce_logits_f32', ptr(dev(z)), ld, ptr(lab), ld_y, const, n, c, float(w), dz.ptr, ld_d, acc, loss.ptr, st())
    got, lv = finish(dz, (n, ld_d), owned=np.broadcast_to(np.arange(ld_d) < c, (n, ld_d)) if acc else None), finish(loss)
    v = f8(z[:, :c])
    terms = np.maximum(v, 0) - v * t64 + np.log1p(np.exp(-np.abs(v)))
    mag = np.maximum(v, 0) + np.abs(v * t64) + 1
    m = n * c
    close(lv[1], terms.sum() / m, mag.sum() / m, "T")
    close(lv[0], f8(w) * terms.sum() / m, abs(f8(w)) * mag.sum() / m, "w T")
    assert rejected(lv[1], terms[:-1].sum() / m, mag.sum() / m)
    sig = 1 / (1 + np.exp(-v))
    ref = f8(w) * (sig - t64) / m + (f8(g0[:, :c]) if acc else 0)
    gmag = abs(f8(w)) / m * (sig + np.abs(t64)) + (np.abs(f8(g0[:, :c])) if acc else 0)
    assert_pointwise(got[:, :c], ref, gmag, 8, "dlogits", floor=FLT_MIN)
    if acc:
        assert_bits(got[:, c:], g0[:, c:], "accumulate = 1 touched the padding")
    else:
        assert (bits(got[:, c:]) == 0).all()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("acc", [0, 1])
def test_entropy_terms(n, acc):
    """tg_entropy_terms_f32: H = mean_n (lse - sum_k p_k l_k) (_entropy, train_base.py:43-48), Bal = -sum_k (1/K) log(mean_n p_k + 1e-12)
    (_balance_entropy, :50-57) with class 0's mean probability below 1e-12; loss = {w_h H + w_bal Bal, H, Bal}."""
    L = lib()
    rng = np.random.default_rng(n * 5 + acc)
    ld, ld_d, w_h, w_bal = 12, 16, np.float32(0.7), np.float32(0.3)
    z = logits(rng, n, ld, scale=20.0)
    z[:, 0] = z[:, 1:K].max(axis=1) - 45.0                                # p_0 < e^-45 in every row
    g0 = grad_buffer(n, ld_d, acc, rng)
    dz, loss = guarded(n * ld_d, fill=g0), guarded(3)
    L.call('tg_entropy_terms_f32', ptr(dev(z)), ld, n, K, float(w_h), float(w_bal), dz.ptr, ld_d, acc, loss.ptr, st())
    got, lv = finish(dz, (n, ld_d), owned=np.broadcast_to(np.arange(ld_d) < K, (n, ld_d)) if acc else None), finish(loss)
    l = f8(z[:, :K])
    p, lse, d = softmax64(l)
    q = p.mean(0)
    assert q[0] < 1e-12
    pl = (p * l).sum(1)
    h_terms, h_mag = lse - pl, np.abs(lse) + (p * np.abs(l) * (1 + np.abs(d))).sum(1)
    close(lv[1], h_terms.sum() / n, h_mag.sum() / n, "H")
    assert rejected(lv[1], h_terms[:-1].sum() / n, h_mag.sum() / n)
    bal = -np.sum(np.log(q + 1e-12) / K)
    cond = (p * (1 + np.abs(d))).sum(0) / np.maximum(p.sum(0), 1e-300)
    bal_mag = np.sum(np.abs(np.log(q + 1e-12))) / K + np.sum(q / (q + 1e-12) * cond) / K
    close(lv[2], bal, bal_mag, "Bal")
    q_short = p[:-1].sum(0) / n
    assert rejected(lv[2], -np.sum(np.log(q_short + 1e-12) / K), bal_mag)
    close(lv[0], f8(w_h) * h_terms.sum() / n + f8(w_bal) * bal, f8(w_h) * h_mag.sum() / n + f8(w_bal) * bal_mag, "w_h H + w_bal Bal")
    dq = -1.0 / (K * (q + 1e-12)) / n
    pdq = (p * dq).sum(1, keepdims=True)
    ref = f8(w_h) * (p - p * (1 + l - pl[:, None])) / n + f8(w_bal) * p * (dq - pdq) + (f8(g0[:, :K]) if acc else 0)
    bal_part = f8(w_bal) * p * (np.abs(dq) + (p * np.abs(dq)).sum(1, keepdims=True))
    gmag = (f8(w_h) / n * p * (2 + np.abs(l) + (p * np.abs(l)).sum(1, keepdims=True)) + bal_part) * (20 + np.abs(d))
    err = np.abs(f8(got[:, :K]) - ref)
    lim = 2 * U * (gmag + (np.abs(f8(g0[:, :K])) if acc else 0)) + 2 * TOL * bal_part * (1 + cond) + FLT_MIN * (1 + f8(w_bal) * np.abs(dq))
    i = np.unravel_index(int(np.argmax(err / lim)), err.shape)
    assert np.isfinite(got[:, :K]).all() and (err <= lim).all(), "dlogits: %.3g x the bound at %s: got %.9g ref %.9g" % (
        float((err / lim)[i]), i, got[i], ref[i])
    check_padding(got, g0, K, acc)


MBD_CASES = [  # n, nk, dim, c, ld_x, ld_a, ld_out, ld_df, ld_da
    (37, 20, 3, 13, 16, 64, 64, 25, 64),
    (1, 1, 8, 0, 4, 8, 4, 1, 9),
    (200, 40, 5, 64, 64, 256, 128, 45, 250),
]


@pytest.mark.parametrize("case", MBD_CASES, ids=lambda s: "x".join(map(str, s)))
def test_minibatch_discrimination_kernels(case):
    """tg_minibatch_disc_fwd_f32 / _bwd_f32 called directly at shapes other than the SVHN layer's (Model/Good_GAN.py:159-162: 100 kernels
    of dimension 5): out = [x, f, 0...], f[i,k] = sum_j exp(-|A_ik - A_jk|_1) + b_k; dact[i,k,d] = -sum_j (g_ik + g_jk) e_ijk sign(A_ikd -
    A_jkd) with its padding zeroed, db = sum_i g."""
    L = lib()
    n, nk, dim, c, ld_x, ld_a, ld_out, ld_df, ld_da = case
    rng = np.random.default_rng(n + nk)
    a = np.full((n, ld_a), np.nan, np.float32)
    a[:, :nk * dim] = (rng.standard_normal((n, nk * dim)) * 0.4).astype(np.float32)
    x = np.full((n, ld_x), np.nan, np.float32)
    x[:, :c] = rng.standard_normal((n, c)).astype(np.float32)
    b = rng.standard_normal(nk).astype(np.float32)
    ad = dev(a)
    out = guarded(n * ld_out)
    L.call('tg_minibatch_disc_fwd_f32', ptr(ad), ld_a, ptr(dev(x)), ld_x, c, ptr(dev(b)), out.ptr, ld_out, n, nk, dim, st())
    got = finish(out, (n, ld_out))
    A = f8(a[:, :nk * dim]).reshape(n, nk, dim)
    diff = A[:, None] - A[None, :]                               # [i, j, k, d]
    s = np.abs(diff).sum(-1)                                     # [i, j, k]
    e = np.exp(-s)
    f = e.sum(1) + f8(b)
    sabs = (e * (1 + s)).sum(1) + np.abs(f8(b))
    assert_bits(got[:, :c], x[:, :c])
    close(got[:, c:c + nk], f, sabs, "f")
    if n > 1:
        assert rejected(got[:, c:c + nk], e[:, :-1].sum(1) + f8(b), sabs)
    assert (bits(got[:, c + nk:]) == 0).all()
    df = np.full((n, ld_df), np.nan, np.float32)
    df[:, :nk] = rng.standard_normal((n, nk)).astype(np.float32)
    dact, db = guarded(n * ld_da), guarded(nk)
    L.call('tg_minibatch_disc_bwd_f32', ptr(ad), ld_a, ptr(dev(df)), ld_df, dact.ptr, ld_da, db.ptr, n, nk, dim, st())
    got_da = finish(dact, (n, ld_da))
    g = f8(df[:, :nk])
    wgt = (g[:, None, :] + g[None, :, :]) * e                    # [i, j, k]
    ref = -(wgt[..., None] * np.sign(diff)).sum(1).reshape(n, nk * dim)
    sab = (np.abs(wgt[..., None]) * (1 + s[..., None]) * np.abs(np.sign(diff))).sum(1).reshape(n, nk * dim)
    close(got_da[:, :nk * dim], ref, sab, "dact")
    if n > 1:
        short = -(wgt[:, :-1, :, None] * np.sign(diff[:, :-1])).sum(1).reshape(n, nk * dim)
        assert rejected(got_da[:, :nk * dim], short, sab)
    assert (bits(got_da[:, nk * dim:]) == 0).all()
    got_db = finish(db)
    assert_bits(got_db, seq_sum32(list(df[:, :nk])), "db")
    close(got_db, g.sum(0), np.abs(g).sum(0), "db")
    if n > 1:
        assert rejected(got_db, g[:-1].sum(0), np.abs(g).sum(0))


def test_d_loss_terms():
    """tg_d_loss_terms_f32 on 700 rows in uneven thirds (the 256-thread row loop takes three turns): terms = {BCE(real, 1), .5 BCE(fake, 0),
    .5 BCE(unl, 0)} (means over their rows) against float64 to the reduction bound, each with the negative control that drops the last row
    of its group; loss and dlogits are the bits tg_d_loss_f32 writes on the same input; dlogits' padding up to ld_d = 4 is exactly 0."""
    L = lib()
    rng = np.random.default_rng(77)
    groups = [(230, 1.0, 1.0), (250, 0.0, 0.5), (220, 0.0, 0.5)]                  # rows, target, weight
    n, ld, ld_d = sum(g[0] for g in groups), 3, 4
    z = np.full((n, ld), np.nan, np.float32)
    v = np.clip(rng.standard_normal(n) * 30, -80, 80)
    v[::17], v[::13] = 80.0, -80.0
    ends = np.cumsum([g[0] for g in groups])
    v[ends - 1] = [-3.0, 3.0, 3.0]                                                # the last row of each group has a large term
    z[:, 0] = v.astype(np.float32)
    zd = dev(z)
    dz, loss, terms = guarded(n * ld_d), guarded(1), guarded(3)
    L.call('tg_d_loss_terms_f32', ptr(zd), ld, groups[0][0], groups[1][0], groups[2][0], dz.ptr, ld_d, loss.ptr, terms.ptr, st())
    dz0, loss0 = guarded(n * ld_d), guarded(1)
    L.call('tg_d_loss_f32', ptr(zd), ld, groups[0][0], groups[1][0], groups[2][0], dz0.ptr, ld_d, loss0.ptr, st())
    got_dz, got_terms = finish(dz, (n, ld_d)), finish(terms)
    assert_bits(got_dz, finish(dz0, (n, ld_d)), "dlogits of d_loss_terms vs d_loss")
    assert_bits(finish(loss), finish(loss0), "loss of d_loss_terms vs d_loss")
    assert (bits(got_dz[:, 1:]) == 0).all(), "padding not zeroed"
    z64, total, total_mag = f8(z[:, 0]), 0.0, 0.0
    for i, (rows, t, w) in enumerate(groups):
        x = z64[ends[i] - rows:ends[i]]
        term = w / rows * (np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x))))
        mag = w / rows * (np.maximum(x, 0) + np.abs(x * t) + np.log1p(np.exp(-np.abs(x))))
        close(got_terms[i], term.sum(), mag.sum(), "terms[%d]" % i)
        assert rejected(got_terms[i], term[:-1].sum(), mag.sum()), "the bound on terms[%d] does not reject the mean without the last row" % i
        total, total_mag = total + term.sum(), total_mag + mag.sum()
    close(finish(loss), total, total_mag, "loss")


@pytest.mark.parametrize("case", WR.G_LOSS_CASES, ids=lambda s: "x".join(map(str, s)))
def test_g_loss(case):
    """tg_g_loss_f32 (0.5 BCE(D_fake, 1), train_base.py:123-128) on 1, 100 and 700 rows (three turns of the 256-thread row loop), logits as
    in test_d_loss_terms with NaN padding, fresh guarded dz and loss, two launches with the same bits: the value in the reduction class
    with the negative control that drops the last row, dz[:, 0] pointwise (tests/wgan_kernels_reference.py counts its K), dz's padding up
    to ld_d exactly 0."""
    L = lib()
    n, ld, ld_d = case
    z = WR.g_loss_case(case)
    zd = dev(z)
    outs = []
    for _ in range(2):
        dz, loss = guarded(n * ld_d), guarded(1)
        L.call('tg_g_loss_f32', ptr(zd), ld, n, dz.ptr, ld_d, loss.ptr, st())
        outs.append((finish(dz, (n, ld_d)), finish(loss)))
    (got_dz, got_loss), (dz2, loss2) = outs
    assert_bits(dz2, got_dz, "dz of a second launch")
    assert_bits(loss2, got_loss, "loss of a second launch")
    val, sabs, ref_dz, mag = WR.g_loss(z)
    close(got_loss[0], val, sabs, "g_loss")
    if n > 1:
        assert rejected(got_loss[0], WR.g_loss(z, drop=True)[0], sabs), "the bound does not reject the mean without the last row"
    assert_pointwise(got_dz[:, 0], ref_dz, mag, WR.K_G_LOSS_DZ, "dz")
    assert (bits(got_dz[:, 1:]) == 0).all(), "padding not zeroed"


@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("acc", [0, 1])
def test_sqdiff_rows_loss(k, pad, acc):
    """tg_sqdiff_rows_loss_f32: T = mean_n sum_k (a - b)^2 (train_base.py:299), loss = {w T, T}, da = 2 w (a - b) / n written or added, db = -da;
    ld == k and ld > k; each of da and db may be NULL.  The loss is a reduction (TOL of the sum of the terms, negative control = without the
    last row); the gradients are pointwise with K = 4 on |g| (a - b, the product with 2 w, the division 2) plus one rounding and the
    existing value's magnitude when accumulating; the padding is zeroed only when not accumulating."""
    L = lib()
    n, w = 37, np.float32(0.3)
    ld_a, ld_b, ld_da, ld_db = k + pad, k + 2 * pad, k + pad, k + 2 * pad
    rng = np.random.default_rng(k + pad + acc)
    a, b = np.full((n, ld_a), np.nan, np.float32), np.full((n, ld_b), np.nan, np.float32)
    a[:, :k], b[:, :k] = rng.standard_normal((n, k)), rng.standard_normal((n, k))
    a[-1, :k] = b[-1, :k] + 2                                                       # a large last row: the negative control drops it
    d = f8(a[:, :k]) - f8(b[:, :k])
    terms = (d * d).sum(1) / n
    g = 2 * f8(w) * d / n
    for with_da, with_db in ((True, True), (True, False), (False, True)):
        bufs = {}
        for name, ld, on in (('da', ld_da, with_da), ('db', ld_db, with_db)):
            g0 = np.full((n, ld), np.nan, np.float32)
            if acc:
                g0[:, :k] = (rng.standard_normal((n, k)) * 1e-2).astype(np.float32)
            bufs[name] = (guarded(n * ld, fill=g0) if on else None, g0, ld)
        loss = guarded(2)
        L.call('tg_sqdiff_rows_loss_f32', ptr(dev(a)), ld_a, ptr(dev(b)), ld_b, n, k, float(w), bufs['da'][0].ptr if with_da else None, ld_da, acc,
               bufs['db'][0].ptr if with_db else None, ld_db, acc, loss.ptr, st())
        lv = finish(loss)
        close(lv[1], terms.sum(), terms.sum(), "T")
        close(lv[0], f8(w) * terms.sum(), f8(w) * terms.sum(), "w T")
        assert rejected(lv[1], terms[:-1].sum(), terms.sum()), "the bound does not reject the mean without the last row"
        for name, sign in (('da', 1.0), ('db', -1.0)):
            buf, g0, ld = bufs[name]
            if buf is None:
                continue
            got = finish(buf, (n, ld), owned=np.broadcast_to(np.arange(ld) < k, (n, ld)) if acc else None)
            ref = sign * g + (f8(g0[:, :k]) if acc else 0)
            assert_pointwise(got[:, :k], ref, np.abs(g) + (np.abs(f8(g0[:, :k])) if acc else 0), 4 + acc, name)
            check_padding(got, g0, k, acc)
