"""The classifier's loss heads at any class count K (csrc/loss.hip: one body per head, the one-thread-per-row layout at K = 10 and the
one-wave-per-row layout at any other 2 <= K <= 1024) against the float64 restatement of tests/loss_heads_k_reference.py:
tg_c_loss_k_f32, tg_c_loss_terms_k_f32, tg_true_fake_loss_k_f32, tg_softmax_ce_f32 and tg_entropy_terms_f32, called directly, and the
entry points without _k (tg_c_loss_f32, tg_c_loss_terms_f32, tg_true_fake_loss_f32), which are the same launch at K = 10.

Logits carry NaN in their padding columns (ld > K: a head that reads past K fails), gradient buffers start NaN so that every owned
element must be written; with accumulate = 0 the gradient padding up to ld_d must be 0, with accumulate = 1 it must be left as it was.
Values within 1e-5 relative, gradients within 1e-5 of their largest entry; two launches bit-identical; the _k entry points at K = 10
bit-identical to the ten-class entry point; K outside 2..1024 rejected.  The *_row_stride tests run more rows than a workgroup has
row owners (256 threads at K = 10, 16 waves otherwise), so that every owner takes a second row, and a single row per group."""
import numpy as np
import pytest

from kernel_check import dev, finish, guarded, lib, ptr, st
import loss_heads_k_reference as R

pytestmark = pytest.mark.gpu

KS = [2, 3, 7, 10, 33, 64, 65, 100, 1000]
ROWS = [37, 50, 80, 100, 250]
STRIDE_KS = [7, 10, 65]                      # both layouts; 65 needs a second class slot per lane
STRIDE_ROWS = [1, 257, 300]                  # one row; one row past the 256 row owners of the K = 10 layout; a ragged second pass
W6 = [1.0, 0.5, 0.3, 0.7, 0.4, 0.6]          # every term of c_loss_terms weighted so that each one shows in the gradient


def logits(rng, n, k, scale=3.0):
    ld = k + 5
    z = np.full((n, ld), np.nan, np.float32)
    z[:, :k] = (rng.standard_normal((n, k)) * scale).astype(np.float32)
    return z


def onehot(rng, n, k):
    return np.eye(k, dtype=np.float32)[rng.integers(0, k, n)]


def close_value(got, ref, what):
    assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)), "%s: %r vs %r" % (what, got, ref)


def close_grad(got, ref, what, floor=0.0):
    err = np.abs(np.asarray(got, np.float64) - ref).max()
    assert err <= 1e-5 * max(np.abs(ref).max(), 1e-30) + floor, "%s: max error %g, largest entry %g" % (what, err, np.abs(ref).max())


def check_pad(g, g0, k, acc, what):
    if acc:
        assert (g[:, k:].view(np.int32) == g0[:, k:].view(np.int32)).all(), "%s: accumulate = 1 touched the padding" % what
    else:
        assert (g[:, k:].view(np.int32) == 0).all(), "%s: padding not zeroed" % what


def run_c_loss(with_terms, k, z, n_real, n_unl, n_rep, n_fake, y_real, y_fake, d_unl, w, ten_class=False):
    """with_terms: tg_c_loss_terms_k_f32 (host weights w, terms written), else tg_c_loss_k_f32 (device lambdas w[4:6]); ten_class: the
    entry point without _k of the same head instead.  Returns (loss, terms, grad)."""
    import ctypes as C
    L = lib()
    n, ld = z.shape
    ld_d = ld - 2
    g = guarded(n * ld_d)
    loss = guarded(1)
    terms = guarded(6) if with_terms else None
    if with_terms and ten_class:
        L.call('tg_c_loss_terms_f32', ptr(dev(z)), ld, n_real, n_unl, n_rep, n_fake, ptr(dev(y_real)), ptr(dev(y_fake)) if n_fake else None,
               ptr(dev(d_unl)), 1, (C.c_float * 6)(*w), g.ptr, ld_d, loss.ptr, terms.ptr, st())
    elif with_terms:
        L.call('tg_c_loss_terms_k_f32', ptr(dev(z)), ld, n_real, n_unl, n_rep, n_fake, k, ptr(dev(y_real)), ptr(dev(y_fake)) if n_fake else None,
               ptr(dev(d_unl)), 1, (C.c_float * 6)(*w), g.ptr, ld_d, loss.ptr, terms.ptr, st())
    elif ten_class:
        L.call('tg_c_loss_f32', ptr(dev(z)), ld, n_real, n_unl, n_rep, n_fake, ptr(dev(y_real)), ptr(dev(y_fake)), ptr(dev(d_unl)), 1,
               ptr(dev(np.array(w[4:6], np.float32))), g.ptr, ld_d, loss.ptr, st())
    else:
        L.call('tg_c_loss_k_f32', ptr(dev(z)), ld, n_real, n_unl, n_rep, n_fake, k, ptr(dev(y_real)), ptr(dev(y_fake)), ptr(dev(d_unl)), 1,
               ptr(dev(np.array(w[4:6], np.float32))), g.ptr, ld_d, loss.ptr, st())
    gg = finish(g, (n, ld_d))
    return float(finish(loss)[0]), (finish(terms) if terms is not None else None), gg


def check_c_loss_terms_k(k, sizes, rep):
    rng = np.random.default_rng(k * 1000 + sum(sizes))
    n_real, n_unl, n_fake = sizes
    n_rep = n_unl if rep else 0
    n = n_real + n_unl + n_rep + n_fake
    z = logits(rng, n, k)
    y_real, y_fake = onehot(rng, n_real, k), onehot(rng, max(n_fake, 1), k)
    d_unl = (rng.standard_normal(n_unl) * 2).astype(np.float32)
    l64 = z[:, :k].astype(np.float64)
    o = np.cumsum([0, n_real, n_unl, n_rep, n_fake])
    ref_loss, ref_terms, ref_g = R.c_loss(l64[o[0]:o[1]], l64[o[1]:o[2]], l64[o[2]:o[3]] if rep else None, l64[o[3]:o[4]], y_real,
                                          y_fake[:n_fake], d_unl.astype(np.float64), W6)
    loss, terms, g = run_c_loss(True, k, z, n_real, n_unl, n_rep, n_fake, y_real, y_fake, d_unl, W6)
    close_value(loss, ref_loss, "loss")
    for i in range(6):
        close_value(float(terms[i]), ref_terms[i], "term %d" % i)
    close_grad(g[:, :k], ref_g, "gradient")
    check_pad(g, None, k, 0, "c_loss_terms_k")
    again = run_c_loss(True, k, z, n_real, n_unl, n_rep, n_fake, y_real, y_fake, d_unl, W6)
    assert np.float32(loss).view(np.int32) == np.float32(again[0]).view(np.int32)
    assert (again[1].view(np.int32) == terms.view(np.int32)).all() and (again[2].view(np.int32) == g.view(np.int32)).all(), "not deterministic"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sizes", [(50, 50, 100), (20, 80, 100), (7, 13, 5), (50, 100, 0)])
@pytest.mark.parametrize("rep", [True, False])
def test_c_loss_terms_k(k, sizes, rep):
    check_c_loss_terms_k(k, sizes, rep)


@pytest.mark.parametrize("k", STRIDE_KS)
@pytest.mark.parametrize("sizes", [(300, 270, 257), (1, 1, 1)])
@pytest.mark.parametrize("rep", [True, False])
def test_c_loss_terms_k_row_stride(k, sizes, rep):
    check_c_loss_terms_k(k, sizes, rep)


def check_c_loss_k(k, sizes, rep=True):
    """the _loss_GAN head: weights {1, .005, 1e-6, 1e-3} and {lambda_1, lambda_2} read from the device."""
    rng = np.random.default_rng(k + 7)
    n_real, n_unl, n_fake = sizes
    n_rep = n_unl if rep else 0
    n = n_real + n_unl + n_rep + n_fake
    z = logits(rng, n, k)
    y_real, y_fake = onehot(rng, n_real, k), onehot(rng, n_fake, k)
    d_unl = (rng.standard_normal(n_unl) * 2).astype(np.float32)
    w = [1.0, 0.005, 1e-6, 1e-3, 0.3, 0.5]
    l64 = z[:, :k].astype(np.float64)
    o = np.cumsum([0, n_real, n_unl, n_rep, n_fake])
    ref_loss, _, ref_g = R.c_loss(l64[o[0]:o[1]], l64[o[1]:o[2]], l64[o[2]:o[3]] if rep else None, l64[o[3]:o[4]], y_real, y_fake,
                                  d_unl.astype(np.float64), w)
    loss, _, g = run_c_loss(False, k, z, n_real, n_unl, n_rep, n_fake, y_real, y_fake, d_unl, w)
    close_value(loss, ref_loss, "loss")
    close_grad(g[:, :k], ref_g, "gradient")
    check_pad(g, None, k, 0, "c_loss_k")
    if k == 10:                                          # the _k entry point at K = 10 is the ten-class launch
        for with_terms in (False, True):
            a = run_c_loss(with_terms, k, z, n_real, n_unl, n_rep, n_fake, y_real, y_fake, d_unl, w)
            b = run_c_loss(with_terms, k, z, n_real, n_unl, n_rep, n_fake, y_real, y_fake, d_unl, w, ten_class=True)
            assert np.float32(a[0]).view(np.int32) == np.float32(b[0]).view(np.int32) and (a[2].view(np.int32) == b[2].view(np.int32)).all()
            assert with_terms is False or (a[1].view(np.int32) == b[1].view(np.int32)).all()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sizes", [(50, 50, 100), (7, 13, 5)])
def test_c_loss_k_with_device_lambdas(k, sizes):
    check_c_loss_k(k, sizes)


@pytest.mark.parametrize("k", STRIDE_KS)
@pytest.mark.parametrize("sizes", [(300, 270, 257), (1, 1, 1)])
@pytest.mark.parametrize("rep", [True, False])
def test_c_loss_k_row_stride(k, sizes, rep):
    check_c_loss_k(k, sizes, rep)


def run_true_fake(k, zu, zf, acc, g0u, g0f, ten_class=False):
    """tg_true_fake_loss_k_f32, or (ten_class) tg_true_fake_loss_f32."""
    L = lib()
    gu, gf = guarded(g0u.size, fill=g0u), guarded(g0f.size, fill=g0f)
    loss = guarded(3)
    if ten_class:
        L.call('tg_true_fake_loss_f32', ptr(dev(zu)), zu.shape[1], len(zu), ptr(dev(zf)), zf.shape[1], len(zf), 0.7, 1.3, gu.ptr, g0u.shape[1],
               acc, gf.ptr, g0f.shape[1], acc, loss.ptr, st())
    else:
        L.call('tg_true_fake_loss_k_f32', ptr(dev(zu)), zu.shape[1], len(zu), ptr(dev(zf)), zf.shape[1], len(zf), k, 0.7, 1.3, gu.ptr,
               g0u.shape[1], acc, gf.ptr, g0f.shape[1], acc, loss.ptr, st())
    return finish(loss), finish(gu, g0u.shape, np.broadcast_to(np.arange(g0u.shape[1]) < k, g0u.shape) if acc else None), finish(gf, g0f.shape, None)


def check_true_fake_loss_k(k, rows, acc):
    rng = np.random.default_rng(k * 3 + rows[0] + acc)
    zu, zf = logits(rng, rows[0], k), logits(rng, rows[1], k)
    g0u = np.full((rows[0], k + 3), np.nan, np.float32)
    g0f = np.zeros((rows[1], k + 2), np.float32)
    if acc:
        g0u[:, :k] = rng.standard_normal((rows[0], k)).astype(np.float32) * 1e-4
        g0f[:, :] = rng.standard_normal(g0f.shape).astype(np.float32) * 1e-4
    ref, gu64, gf64 = R.true_fake(zu[:, :k].astype(np.float64), zf[:, :k].astype(np.float64), 0.7, 1.3)
    loss, gu, gf = run_true_fake(k, zu, zf, acc, g0u, g0f)
    for i in range(3):
        close_value(float(loss[i]), ref[i], "loss[%d]" % i)
    # w (-0.5 + 0.5 sigmoid(lse)) / n cancels in fp32 when lse is large (the ten-class kernel's formula): an absolute floor of a few
    # ulps of w / n, which is far below the gradient's largest entry otherwise
    close_grad(gu[:, :k] - (g0u[:, :k] if acc else 0), gu64, "d_unl", floor=1e-6 * 0.7 / rows[0])
    close_grad(gf[:, :k] - (g0f[:, :k] if acc else 0), gf64, "d_fake")
    check_pad(gu, g0u, k, acc, "d_unl")
    check_pad(gf, g0f, k, acc, "d_fake")
    again = run_true_fake(k, zu, zf, acc, g0u, g0f)
    assert all((a.view(np.int32) == b.view(np.int32)).all() for a, b in zip(again, (loss, gu, gf))), "not deterministic"
    if k == 10:
        old = run_true_fake(k, zu, zf, acc, g0u, g0f, ten_class=True)
        assert all((a.view(np.int32) == b.view(np.int32)).all() for a, b in zip(old, (loss, gu, gf))), "K = 10 is not the ten-class launch"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("rows", [(50, 100), (80, 20), (37, 13)])
@pytest.mark.parametrize("acc", [0, 1])
def test_true_fake_loss_k(k, rows, acc):
    check_true_fake_loss_k(k, rows, acc)


@pytest.mark.parametrize("k", STRIDE_KS)
@pytest.mark.parametrize("rows", [(300, 257), (1, 1)])
@pytest.mark.parametrize("acc", [0, 1])
def test_true_fake_loss_k_row_stride(k, rows, acc):
    check_true_fake_loss_k(k, rows, acc)


def run_softmax_ce(k, z, y, acc, g0):
    L = lib()
    g = guarded(g0.size, fill=g0)
    loss = guarded(2)
    L.call('tg_softmax_ce_f32', ptr(dev(z)), z.shape[1], ptr(dev(y)), len(z), k, 0.8, g.ptr, g0.shape[1], acc, loss.ptr, st())
    return finish(loss), finish(g, g0.shape, np.broadcast_to(np.arange(g0.shape[1]) < k, g0.shape) if acc else None)


def run_entropy(k, z, acc, g0):
    L = lib()
    g = guarded(g0.size, fill=g0)
    loss = guarded(3)
    L.call('tg_entropy_terms_f32', ptr(dev(z)), z.shape[1], len(z), k, 0.6, 0.9, g.ptr, g0.shape[1], acc, loss.ptr, st())
    return finish(loss), finish(g, g0.shape, np.broadcast_to(np.arange(g0.shape[1]) < k, g0.shape) if acc else None)


def grad0(rng, n, k, acc):
    g0 = np.full((n, k + 3), np.nan, np.float32)
    if acc:
        g0[:, :k] = rng.standard_normal((n, k)).astype(np.float32) * 1e-4
    return g0


def check_softmax_ce(k, n, acc):
    rng = np.random.default_rng(k * 7 + n + acc)
    z, y = logits(rng, n, k), onehot(rng, n, k)
    g0 = grad0(rng, n, k, acc)
    t, g64 = R.ce(z[:, :k].astype(np.float64), y.astype(np.float64))
    loss, g = run_softmax_ce(k, z, y, acc, g0)
    close_value(float(loss[1]), t, "T")
    close_value(float(loss[0]), 0.8 * t, "w T")
    close_grad(g[:, :k] - (g0[:, :k] if acc else 0), 0.8 * g64, "gradient")
    check_pad(g, g0, k, acc, "softmax_ce")
    again = run_softmax_ce(k, z, y, acc, g0)
    assert all((a.view(np.int32) == b.view(np.int32)).all() for a, b in zip(again, (loss, g))), "not deterministic"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("acc", [0, 1])
def test_softmax_ce_any_k(k, n, acc):
    check_softmax_ce(k, n, acc)


@pytest.mark.parametrize("k", STRIDE_KS)
@pytest.mark.parametrize("n", STRIDE_ROWS)
@pytest.mark.parametrize("acc", [0, 1])
def test_softmax_ce_row_stride(k, n, acc):
    check_softmax_ce(k, n, acc)


def check_entropy_terms(k, n, acc):
    rng = np.random.default_rng(k * 11 + n + acc)
    z = logits(rng, n, k)
    g0 = grad0(rng, n, k, acc)
    l64 = z[:, :k].astype(np.float64)
    h, gh = R.entropy(l64)
    b, gb = R.balance(l64)
    loss, g = run_entropy(k, z, acc, g0)
    close_value(float(loss[1]), h, "H")
    close_value(float(loss[2]), b, "Bal")
    close_value(float(loss[0]), 0.6 * h + 0.9 * b, "loss")
    close_grad(g[:, :k] - (g0[:, :k] if acc else 0), 0.6 * gh + 0.9 * gb, "gradient")
    check_pad(g, g0, k, acc, "entropy_terms")
    again = run_entropy(k, z, acc, g0)
    assert all((a.view(np.int32) == b.view(np.int32)).all() for a, b in zip(again, (loss, g))), "not deterministic"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("acc", [0, 1])
def test_entropy_terms_any_k(k, n, acc):
    check_entropy_terms(k, n, acc)


@pytest.mark.parametrize("k", STRIDE_KS)
@pytest.mark.parametrize("n", STRIDE_ROWS)
@pytest.mark.parametrize("acc", [0, 1])
def test_entropy_terms_row_stride(k, n, acc):
    check_entropy_terms(k, n, acc)


@pytest.mark.parametrize("k", [0, 1, 1025, 4096])
def test_class_count_outside_the_range_is_rejected(k):
    L = lib()
    z = np.zeros((4, 1100), np.float32)
    y = np.zeros((4, max(k, 1)), np.float32)
    g = guarded(4 * 1100)
    loss = guarded(3)
    calls = [('tg_softmax_ce_f32', lambda: L.call('tg_softmax_ce_f32', ptr(dev(z)), 1100, ptr(dev(y)), 4, k, 1.0, g.ptr, 1100, 0, loss.ptr, st())),
             ('tg_entropy_terms_f32', lambda: L.call('tg_entropy_terms_f32', ptr(dev(z)), 1100, 4, k, 1.0, 1.0, g.ptr, 1100, 0, loss.ptr, st())),
             ('tg_true_fake_loss_k_f32', lambda: L.call('tg_true_fake_loss_k_f32', ptr(dev(z)), 1100, 2, ptr(dev(z)), 1100, 2, k, 1.0, 1.0, g.ptr,
                                                        1100, 0, g.ptr, 1100, 0, loss.ptr, st())),
             ('tg_c_loss_k_f32', lambda: L.call('tg_c_loss_k_f32', ptr(dev(z)), 1100, 1, 1, 0, 1, k, ptr(dev(y)), ptr(dev(y)), ptr(dev(z)), 1,
                                                ptr(dev(np.zeros(2, np.float32))), g.ptr, 1100, loss.ptr, st()))]
    for name, call in calls:
        with pytest.raises(L.TgError, match="1024"):
            call()


def test_ten_class_kernel_misses_hundred_class_data():
    """negative control: the K = 10 head on K = 100 logits (what a 100-class run got before the heads took K) is far outside the bound."""
    k, rng = 100, np.random.default_rng(5)
    n_real, n_unl, n_fake = 50, 50, 100
    z = logits(rng, n_real + 2 * n_unl + n_fake, k)
    z[:, k:] = 0.0                                       # the ten-class kernel reads its ten columns only; keep the rest finite
    y_real, y_fake = onehot(rng, n_real, k), onehot(rng, n_fake, k)
    d_unl = rng.standard_normal(n_unl).astype(np.float32)
    l64 = z[:, :k].astype(np.float64)
    o = np.cumsum([0, n_real, n_unl, n_unl, n_fake])
    ref_loss, _, ref_g = R.c_loss(l64[o[0]:o[1]], l64[o[1]:o[2]], l64[o[2]:o[3]], l64[o[3]:o[4]], y_real, y_fake, d_unl.astype(np.float64), W6)
    # the ten-class entry point reads labels as [n][10]: hand it the first ten columns so that only the class count is wrong
    loss, _, g = run_c_loss(True, k, z, n_real, n_unl, n_unl, n_fake, np.ascontiguousarray(y_real[:, :10]),
                            np.ascontiguousarray(y_fake[:, :10]), d_unl, W6, ten_class=True)
    err = np.abs(g[:, :k] - ref_g).max() / np.abs(ref_g).max()
    assert err > 1e-2 and abs(loss - ref_loss) > 1e-3 * abs(ref_loss), (err, loss, ref_loss)
    good = run_c_loss(True, k, z, n_real, n_unl, n_unl, n_fake, y_real, y_fake, d_unl, W6)
    close_grad(good[2][:, :k], ref_g, "gradient")
