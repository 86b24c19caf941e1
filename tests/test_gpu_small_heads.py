"""Per-kernel tests of the small heads: tg_argmax_onehot_f32 (csrc/elementwise.hip), tg_accuracy_count_f32, tg_feature_match_f32 and
tg_pull_away_f32 (csrc/loss.hip; Training/train_base.py:172-182,202-207, Train_goodGAN.py:428-447).

Shapes: argmax over n = 300 rows (three 128-thread workgroups) and k = 2, 10, 100 classes with ld > k and NaN behind k, ties (the first
index wins, tf.argmax) and an all-equal row (index 0); the accuracy counter over n = 700 rows (the 256-thread stride loop takes three turns)
accumulating over two calls; feature matching at c = 1 and 300 (the k += 256 column loop) with n_fake != n_unl and with one row each; the
pull-away term at n = 2, 37 and c = 1, 300, masked and unmasked, on a guarded scratch of exactly n c + n n + n floats.

Tolerance classes (tests/kernel_check.py):
  bit-exact  the one-hot rows and the counters (selection and counting of small integers in fp32).
  reduction  the feature-matching loss, TOL of sum_k (mean_n |f_fake| + mean_n |f_unl|) / c, negative control = f_unl without its last row.
  pointwise  the feature-matching gradients, K = 2 on 1 / (c n) (two divisions, each correctly rounded); a column whose two means are
             equal gives exactly 0.
             The pull-away term, counted from its c-term fp32 dot products (u per operation; a sequential fp32 sum of c terms costs
             c u of the sum of their magnitudes):
               |f|^2                   c   (all terms positive)
               fn = f / sqrt(|f|^2)    e_fn = c/2 + 4   (half of |f|^2's, sqrtf 2, division 2)
               cos_ab = sum fn_a fn_b  e_d = 2 e_fn + 1 + c = 2c + 9   on D_ab = sum_k |fn_a||fn_b| (<= 1)
               loss                    K_loss = 2 e_d + 14 + ceil(n^2 / 256) = 4c + 32 + ceil(n^2 / 256) on sum_ab w D_ab^2 (masked, w = 0.8 / (n (n-1)),
                                       a != b) or sum_ab w D_ab (unmasked, w = 0.8 / n^2): the square doubles e_d, five roundings of the
                                       term, the thread's own additions and the workgroup's tree (6 + 3)
               CS_ab = d loss / d cos  e_d + 5 on 2 w D_ab (masked) or w (unmasked)
               G_rk = sum_b (CS_rb + CS_br) fn_bk      e_G = e_d + e_fn + 7 + n   on GA_rk = sum_b 2 CS_rb |fn_bk|
               dot_r = sum_k G_rk fn_rk                e_dot = e_G + e_fn + 1 + c  on DA_r = sum_k GA_rk |fn_rk|
               df = (G - fn dot) / |f|                 K_grad = e_dot + e_fn + 4 = 4.5 c + n + 33   on (GA_rk + |fn_rk| DA_r) / |f_r|
             The masked and the unmasked reference reject each other under these bounds (factor 10)."""
import numpy as np
import pytest

from kernel_check import U, assert_bits, assert_pointwise, close, dev, finish, guarded, lib, ptr, rejected, st
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

KS = [2, 10, 100]
f8 = lambda a: np.asarray(a, np.float64)


def logits_case(rng, n, k, ld):
    z = np.full((n, ld), np.nan, np.float32)
    v = rng.standard_normal((n, k)).astype(np.float32)
    v[5, 0] = v[5, k - 1] = 9.0                                  # a tie between the first and the last class
    if k > 3:
        v[6, 1] = v[6, 3] = 9.0                                  # a tie inside the row
    v[7] = np.float32(0.25)                                      # all equal: index 0
    v[n - 1, k - 1] = 9.0                                        # the last class of the last row
    z[:, :k] = v
    return z, v


@pytest.mark.parametrize("k", KS)
def test_argmax_onehot(k):
    L = lib()
    n, ld = 300, k + 3
    z, v = logits_case(np.random.default_rng(k), n, k, ld)
    out = guarded(n * k)
    L.call('tg_argmax_onehot_f32', ptr(dev(z)), ld, n, k, out.ptr, st())
    am = np.argmax(v, axis=1)                                    # the first maximum
    assert am[5] == 0 and am[7] == 0 and am[n - 1] == k - 1
    assert_bits(finish(out, (n, k)), np.eye(k, dtype=np.float32)[am], "one-hot of the arg-max")
    assert_bits(np.eye(k, dtype=np.float32)[am], T.argmax_onehot(v, k), "the oracle's form")


@pytest.mark.parametrize("k", KS)
def test_accuracy_count(k):
    L = lib()
    n, ld = 700, k + 3
    rng = np.random.default_rng(10 + k)
    z, v = logits_case(rng, n, k, ld)
    lab = rng.integers(0, k, n)
    lab[5], lab[7], lab[n - 1] = 0, 0, k - 1
    lab[::2] = np.argmax(v, axis=1)[::2]                          # half of the rows correct for certain
    cnt = guarded(2, fill=np.zeros(2, np.float32))
    labels = dev(np.eye(k, dtype=np.float32)[lab])
    correct = int((np.argmax(v, axis=1) == lab).sum())
    assert n // 2 <= correct < n
    for call in (1, 2):
        L.call('tg_accuracy_count_f32', ptr(dev(z)), ld, ptr(labels), n, k, cnt.ptr, st())
        assert_bits(finish(cnt), np.array([call * correct, call * n], np.float32), "counters after call %d" % call)


@pytest.mark.parametrize("c", [1, 300])
@pytest.mark.parametrize("rows", [(5, 9), (1, 1)], ids=lambda r: "%dx%d" % r)
def test_feature_match(c, rows):
    L = lib()
    n_f, n_u = rows
    rng = np.random.default_rng(100 + c + n_f)
    ff, fu = rng.standard_normal((n_f, c)).astype(np.float32), (rng.standard_normal((n_u, c)) + 0.5).astype(np.float32)
    fu[-1] = 3 + rng.random(c)                                    # a large last row: the negative control drops it
    if c > 7:
        ff[:, 7], fu[:, 7] = 1.0, 1.0                             # both means are exactly 1: gradient 0
    da, db, loss = guarded(n_f * c), guarded(n_u * c), guarded(1)
    L.call('tg_feature_match_f32', ptr(dev(ff)), n_f, ptr(dev(fu)), n_u, c, da.ptr, db.ptr, loss.ptr, st())
    d = f8(ff).mean(0) - f8(fu).mean(0)
    sabs = (np.abs(f8(ff)).mean(0) + np.abs(f8(fu)).mean(0)).sum() / c
    got = finish(loss)[0]
    close(got, np.abs(d).sum() / c, sabs, "loss")
    if n_u > 1:
        assert rejected(got, np.abs(f8(ff).mean(0) - f8(fu[:-1]).mean(0)).sum() / c, sabs), "the bound does not reject f_unl without its last row"
    val, ga, gb = T.feature_match(f8(ff), f8(fu))
    assert abs(val - np.abs(d).sum() / c) <= 1e-15 * sabs
    got_a, got_b = finish(da, (n_f, c)), finish(db, (n_u, c))
    assert_pointwise(got_a, ga, np.full(ga.shape, 1.0 / (c * n_f)), 2, "d f_fake")
    assert_pointwise(got_b, gb, np.full(gb.shape, 1.0 / (c * n_u)), 2, "d f_unl")
    if c > 7:
        assert (got_a[:, 7] == 0).all() and (got_b[:, 7] == 0).all() and (got_a[:, :7] != 0).all()


def pull_away_bounds(f, masked):
    """float64 magnitudes of the module docstring -> (loss magnitude, K_loss, gradient magnitude [n, c], K_grad)"""
    n, c = f.shape
    nr = np.sqrt((f * f).sum(1, keepdims=True))
    fa = np.abs(f / nr)
    D = fa @ fa.T
    off = 1.0 - np.eye(n)
    if masked:
        w = 0.8 / (n * (n - 1))
        loss_mag, CS = (w * D * D * off).sum(), 2 * w * D * off
    else:
        w = 0.8 / (n * n)
        loss_mag, CS = (w * D).sum(), np.full((n, n), w)
    GA = 2 * CS @ fa
    DA = (GA * fa).sum(1, keepdims=True)
    return loss_mag, 4 * c + 32 + -(-n * n // 256), (GA + fa * DA) / nr, 4.5 * c + n + 33


@pytest.mark.parametrize("n", [2, 37])
@pytest.mark.parametrize("c", [1, 300])
def test_pull_away(n, c):
    L = lib()
    rng = np.random.default_rng(200 + n + c)
    f = (rng.standard_normal((n, c)) + 0.3).astype(np.float32)
    if c == 1:
        f[::2] = -np.abs(f[::2])                                  # one-dimensional rows are +-1 after normalisation: mix the signs
        f[1::2] = np.abs(f[1::2])
    res = {}
    for masked, fn in ((1, T.pull_away_masked), (0, T.pull_away_unmasked)):
        scratch, df, loss = guarded(n * c + n * n + n), guarded(n * c), guarded(1)
        L.call('tg_pull_away_f32', ptr(dev(f)), n, c, masked, scratch.ptr, df.ptr, loss.ptr, st())
        finish(scratch)                                           # all of it is written, none of it behind its end
        val, grad = fn(f8(f))
        loss_mag, k_loss, grad_mag, k_grad = pull_away_bounds(f8(f), masked)
        res[masked] = (finish(loss)[0], finish(df, (n, c)), val, grad, k_loss * U * loss_mag, k_grad * U * grad_mag)
        assert_pointwise(res[masked][0], val, loss_mag, k_loss, "loss, masked = %d" % masked)
        assert_pointwise(res[masked][1], grad, grad_mag, k_grad, "gradient, masked = %d" % masked)
    for masked in (0, 1):
        got_l, got_g, _, _, lim_l, lim_g = res[masked]
        _, _, other_l, other_g, _, _ = res[1 - masked]
        assert abs(got_l - other_l) > 10 * lim_l, "the bound on the loss does not tell masked from unmasked"
        if c > 1:
            assert (np.abs(got_g - other_g) > 10 * lim_g).any(), "the bound on the gradient does not tell masked from unmasked"
