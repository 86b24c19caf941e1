"""Per-kernel float64 tests of the parameter-side kernels of csrc/prep.hip: the weight-norm scale and gradient of conv / dense filters
(Model/nn.py:502,554) and of the transposed conv (NN_Base._WN_deconv2d, Model/modle_base.py:148), the filter re-layout with channel
padding, and their multi-job launches (tg_filter_prep_multi_f32: the forward preparation of a solver run, tg/runtime.py prep plans;
tg_filter_grad_tail_multi_f32: the deferred filter-gradient tails of Context.flush_tails).

Tolerance classes (tests/kernel_check.py):
  bit-exact   filter_prep / filter_prep_multi (a copy times at most two per-channel scales: fp32 products restated in NumPy's float32),
              the slab reduction of filter_grad_tail_multi (sum over the splits in slab order), both paths of tg_slab_reduce_f32 (the
              in-order restatements of tests/wgan_kernels_reference.py; also held in the reduction class), and the twin paths the code says give
              identical bits: wn_scale against the wn_scale_multi pass of filter_prep_multi, filter_prep against filter_prep_multi;
  reduction   wn_scale, wn_scale_tab: |got - ref| <= (TOL / 2 + 4u) |ref| (a sum of squares of one sign: its relative error TOL halves
              under the square root; rsqrtf and the product by g add 4u); wn_bwd, the WN tail of filter_grad_tail_multi, wn_bwd_tab:
              dg within TOL (sum|dw v| / ||v|| + |dg|), dv within TOL |g/||v||| (|dw| + |v| (2 |c1| + sum|dw v| / ||v||^2)), c1 = <dw,v>/||v||^2
              — the error of the two column reductions carried through the closed form.  Each holds a negative control: the same
              reference without the last filter row is rejected.

wn_bwd (tg_wn_bwd_f32, two accumulators per lane) and the WN tail of tg_filter_grad_tail_multi_f32 (one accumulator) add the rows of a
column in different orders, so they may differ in the last bits: both are held to the float64 reference here; DESIGN.md states why
they may differ and why no execution-mode bit-identity depends on it (a layer's tail path is fixed by its geometry)."""
import ctypes as C

import numpy as np
import pytest

import wgan_kernels_reference as WR
from kernel_check import TOL, U, assert_bits, close, dev, finish, guarded, lib, ptr, rejected, seq_sum32, st, worst
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

ROWS = [1, 31, 32, 97, 127, 128, 129, 1152]       # every tail of the unrolled row loops (4 x 32 and 2 x 32 lanes)


def wn_scale64(v, g, axes):
    ss = np.sum(np.square(v.astype(np.float64)), axis=axes)
    return g.astype(np.float64) / np.sqrt(np.maximum(ss, 1e-12))


def check_scale(got, ref, ref_short):
    lim = (TOL / 2 + 4 * U) * np.abs(ref)
    r = float((np.abs(got - ref) / lim).max())
    assert r <= 1.0, "weight-norm scale off by %.2f x its bound" % r
    if ref_short is not None:
        assert float((np.abs(got - ref_short) / lim).max()) > 10.0, "the bound does not reject a norm missing the last row"


def wn_bwd64(dw, v, g, axes, drop_last=None):
    """float64 dv, dg of W = g V/||V|| (oracle.tf_ops.wn_weight_bwd restated over `axes`) and the per-output sums |terms| of the bound;
    drop_last: leave the last row of the reductions out (negative control)."""
    dw, v, g = dw.astype(np.float64), v.astype(np.float64), g.astype(np.float64)
    vr, dr = (v, dw) if drop_last is None else drop_last(v, dw)
    ss = np.sum(vr * vr, axis=axes, keepdims=True)
    dot = np.sum(dr * vr, axis=axes, keepdims=True)
    sdot = np.sum(np.abs(dr * vr), axis=axes, keepdims=True)
    nrm = np.sqrt(ss)
    shp = [1] * v.ndim
    for a in range(v.ndim):
        if a not in axes:
            shp[a] = -1
    g = g.reshape(shp)
    c1 = dot / ss
    dv = (g / nrm) * (dw - v * c1)
    dg = dot / nrm
    s_dv = np.abs(g / nrm) * (np.abs(dw) + np.abs(v) * (2 * np.abs(c1) + sdot / ss))
    s_dg = sdot / nrm + np.abs(dg)
    return dv, dg.reshape(-1), s_dv, s_dg.reshape(-1)


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("c", [45, 128])
def test_wn_scale_and_its_multi_job_twin(r, c):
    """tg_wn_scale_f32 (tf.nn.l2_normalize(V,[0,1,2])*g, Model/nn.py:502; g/||V|| of dense_WN, :554) against float64, and the wn_scale_multi
    pass of tg_filter_prep_multi_f32 — "same summation order as wn_scale: both paths give identical bits" (prep.hip) — bit for bit."""
    L = lib()
    rng = np.random.default_rng(r * 3 + c)
    v = rng.standard_normal((r, c)).astype(np.float32)
    g = (rng.random(c) + 0.5).astype(np.float32)
    vd, gd = dev(v), dev(g)
    sc = guarded(c)
    L.call('tg_wn_scale_f32', ptr(vd), ptr(gd), r, c, sc.ptr, st())
    got = finish(sc)
    check_scale(got, wn_scale64(v, g, 0), wn_scale64(v[:-1], g, 0) if r > 1 else None)
    sc2, dst = guarded(c), guarded(r * c)
    job = L.PrepJob(vd.data_ptr(), gd.data_ptr(), sc2.t.data_ptr(), dst.t.data_ptr(), None, 0, 0, 1, r, c, r, c)
    L.call('tg_filter_prep_multi_f32', C.byref(job), 1, st())
    assert_bits(finish(sc2), got, "wn_scale_multi vs wn_scale")
    assert_bits(finish(dst, (r, c)), v * got[None, :], "filter_prep_multi of the scaled filter")


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("c", [45, 128])
def test_wn_bwd(r, c):
    """tg_wn_bwd_f32 (the weight-norm gradient optimizer.minimize emits for Model/nn.py:502,554; called from tg/ops.py filter_grad) against
    float64; coef is scratch, dv / dg fully written, nothing past them."""
    L = lib()
    rng = np.random.default_rng(r + 7 * c)
    v = rng.standard_normal((r, c)).astype(np.float32)
    dw = rng.standard_normal((r, c)).astype(np.float32)
    g = (rng.random(c) + 0.5).astype(np.float32)
    dv, dg, coef = guarded(r * c), guarded(c), guarded(2 * c)
    L.call('tg_wn_bwd_f32', ptr(dev(dw)), ptr(dev(v)), ptr(dev(g)), r, c, dv.ptr, dg.ptr, coef.ptr, st())
    finish(coef)
    got_dv, got_dg = finish(dv, (r, c)), finish(dg)
    ref_dv, ref_dg, s_dv, s_dg = wn_bwd64(dw, v, g, (0,))
    assert worst(got_dv, ref_dv, s_dv) <= 1.0 and worst(got_dg, ref_dg, s_dg) <= 1.0, (worst(got_dv, ref_dv, s_dv), worst(got_dg, ref_dg, s_dg))
    if r > 1:
        _, short_dg, _, _ = wn_bwd64(dw, v, g, (0,), drop_last=lambda a, b: (a[:-1], b[:-1]))
        assert worst(got_dg, short_dg, s_dg) > 10.0
    ref2, _ = T.wn_weight_bwd(v.astype(np.float64), g.astype(np.float64), dw.astype(np.float64), out_axis=-1)   # the oracle's statement
    np.testing.assert_allclose(ref_dv, ref2, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("b", [128, 7, 1])
def test_wn_scale_and_bwd_of_a_transposed_conv_filter(b):
    """tg_wn_scale_tab_f32 / tg_wn_bwd_tab_f32: weight norm of V[t][a][b] = [kh*kw][Cout][Cin] over (t, b) per output channel
    (Model/modle_base.py:148) at the image layer's t = 25, a = 3, with t*b = 3200, 175, 25 (none a multiple of the 256 lanes)."""
    L = lib()
    t, a = 25, 3
    rng = np.random.default_rng(b)
    v = rng.standard_normal((t, a, b)).astype(np.float32)
    dw = rng.standard_normal((t, a, b)).astype(np.float32)
    g = (rng.random(a) + 0.5).astype(np.float32)
    vd, gd = dev(v), dev(g)
    sc = guarded(a)
    L.call('tg_wn_scale_tab_f32', ptr(vd), ptr(gd), t, a, b, sc.ptr, st())
    check_scale(finish(sc), wn_scale64(v, g, (0, 2)), wn_scale64(v.reshape(t * a, b)[:-a].reshape(t - 1, a, b), g, (0, 2)) if t > 1 else None)
    dv, dg = guarded(t * a * b), guarded(a)
    L.call('tg_wn_bwd_tab_f32', ptr(dev(dw)), ptr(vd), ptr(gd), t, a, b, dv.ptr, dg.ptr, st())
    got_dv, got_dg = finish(dv, (t, a, b)), finish(dg)
    ref_dv, ref_dg, s_dv, s_dg = wn_bwd64(dw, v, g, (0, 2))
    assert worst(got_dv, ref_dv, s_dv) <= 1.0 and worst(got_dg, ref_dg, s_dg) <= 1.0
    _, short_dg, _, _ = wn_bwd64(dw, v, g, (0, 2), drop_last=lambda x, y: (x[:-1], y[:-1]))
    assert worst(got_dg, short_dg, s_dg) > 10.0
    ref2, ref2g = T.wn_weight_bwd(v.astype(np.float64), g.astype(np.float64), dw.astype(np.float64), out_axis=1)
    np.testing.assert_allclose(ref_dv, ref2, rtol=1e-9, atol=1e-12)


PREP_CASES = [  # t, a, b, a_pad, b_pad, scale, scale_a, same, tr
    (9, 3, 128, 32, 128, True, False, True, True),      # the discriminators' first conv, HWIO -> OTI and padded HWIO
    (25, 3, 128, 32, 128, False, True, True, True),     # the image layer's [kh,kw,Cout,Cin] filter with scale_a (weight norm over Cout)
    (1, 100, 250, 128, 256, True, True, True, False),   # a dense layer, only the padded copy
    (9, 45, 33, 64, 64, False, False, False, True),     # ragged tiles, only the transpose
    (1, 1, 1, 1, 1, True, True, True, True),
]


def prep_ref(src, scale, scale_a, a_pad, b_pad):
    t, a, b = src.shape
    v = src.copy()
    if scale is not None:
        v = v * scale[None, None, :]
    if scale_a is not None:
        v = v * scale_a[None, :, None]
    same = np.zeros((t, a_pad, b_pad), np.float32)
    same[:, :a, :b] = v
    return same, same.transpose(2, 0, 1).copy()          # OTI: dst_tr[b][t][a] with tr_sb = t*a_pad, tr_st = a_pad


@pytest.mark.parametrize("case", PREP_CASES, ids=lambda s: "x".join(map(str, s)))
def test_filter_prep(case):
    """tg_filter_prep_f32: re-layout with zero channel padding (bit-exact, padding exactly 0.0, every owned element written)."""
    L = lib()
    t, a, b, a_pad, b_pad, has_s, has_sa, same, tr = case
    rng = np.random.default_rng(t * a + b)
    src = rng.standard_normal((t, a, b)).astype(np.float32)
    scale = (rng.random(b) + 0.5).astype(np.float32) if has_s else None
    scale_a = (rng.random(a) + 0.5).astype(np.float32) if has_sa else None
    ds, dt = guarded(t * a_pad * b_pad), guarded(b_pad * t * a_pad)
    L.call('tg_filter_prep_f32', ptr(dev(src)), ptr(dev(scale)) if has_s else None, ptr(dev(scale_a)) if has_sa else None, t, a, b, a_pad, b_pad,
           ds.ptr if same else None, dt.ptr if tr else None, t * a_pad, a_pad, st())
    ref_same, ref_tr = prep_ref(src, scale, scale_a, a_pad, b_pad)
    if same:
        assert_bits(finish(ds, ref_same.shape), ref_same, "dst_same")
    else:
        ds.check_guard()
        assert np.isnan(ds.get()).all()
    if tr:
        assert_bits(finish(dt, ref_tr.shape), ref_tr, "dst_tr")
    else:
        dt.check_guard()
        assert np.isnan(dt.get()).all()


def test_filter_prep_multi_equals_the_single_launches():
    """tg_filter_prep_multi_f32 with 24 jobs of mixed shapes (weight-normalised or not, one or both layouts, one tile or many): the
    first_block prefix table sends every workgroup to its job — each job's outputs equal, bit for bit, tg_wn_scale_f32 +
    tg_filter_prep_f32 of that job alone."""
    L = lib()
    rng = np.random.default_rng(24)
    shapes = [(9, 3, 128, 32, 128), (9, 128, 128, 128, 128), (25, 3, 128, 32, 128), (1, 100, 250, 128, 256), (9, 45, 33, 64, 64),
              (1, 1, 1, 1, 1), (9, 256, 256, 256, 256), (1, 512, 10, 512, 32)]
    jobs = (L.PrepJob * 24)()
    keep, checks = [], []
    for i in range(24):
        t, a, b, a_pad, b_pad = shapes[i % len(shapes)]
        wn, same, tr = i % 3 != 2, i % 4 != 3, i % 4 != 1
        src = rng.standard_normal((t, a, b)).astype(np.float32)
        g = (rng.random(b) + 0.5).astype(np.float32)
        sd, gd = dev(src), dev(g)
        sc = guarded(b)
        ds, dt = guarded(t * a_pad * b_pad), guarded(b_pad * t * a_pad)
        keep.append((sd, gd))
        jobs[i] = L.PrepJob(sd.data_ptr(), gd.data_ptr() if wn else None, sc.t.data_ptr(), ds.t.data_ptr() if same else None,
                            dt.t.data_ptr() if tr else None, t * a_pad, a_pad, t, a, b, a_pad, b_pad)
        checks.append((sd, gd, sc, ds, dt, wn, same, tr, (t, a, b, a_pad, b_pad)))
    L.call('tg_filter_prep_multi_f32', C.cast(jobs, C.c_void_p), 24, st())
    for i, (sd, gd, sc, ds, dt, wn, same, tr, (t, a, b, a_pad, b_pad)) in enumerate(checks):
        scale = None
        if wn:
            s1 = guarded(b)
            L.call('tg_wn_scale_f32', ptr(sd), ptr(gd), t * a, b, s1.ptr, st())
            scale = finish(s1)
            assert_bits(finish(sc), scale, "job %d scale" % i)
        else:
            sc.check_guard()
            assert np.isnan(sc.get()).all(), "job %d without weight norm wrote its scale buffer" % i
        r_s, r_t = guarded(t * a_pad * b_pad), guarded(b_pad * t * a_pad)
        L.call('tg_filter_prep_f32', ptr(sd), ptr(dev(scale)) if wn else None, None, t, a, b, a_pad, b_pad, r_s.ptr, r_t.ptr, t * a_pad, a_pad, st())
        if same:
            assert_bits(finish(ds), finish(r_s), "job %d dst_same" % i)
        if tr:
            assert_bits(finish(dt), finish(r_t), "job %d dst_tr" % i)
        if not same:
            assert np.isnan(ds.get()).all()
        if not tr:
            assert np.isnan(dt.get()).all()
        ds.check_guard()
        dt.check_guard()


@pytest.fixture(scope="module")
def slabs():
    """the slabs of tests/wgan_kernels_reference.py's cases on the host and the device, built when first asked for and left unchanged."""
    made = {}

    def get(case):
        if case not in made:
            slab = WR.slab_case(case)
            made[case] = (slab, dev(slab))
        return made[case]
    return get


@pytest.mark.parametrize("case", WR.SLAB_CASES, ids=lambda s: "x".join(map(str, s)))
def test_slab_reduce(case, slabs):
    """tg_slab_reduce_f32, the kernel that finishes every split filter gradient: dst[t][c][n] = sum_s slab[s][t][c][n] with the slab padding
    (c >= c_dim, n >= n_dim) NaN and dst guarded.  Bit-exact against the in-order fp32 restatement of the path the case takes — one thread per
    output walking the slabs in order, or (n_split >= 32 and at most 65536 outputs) 8 lane groups with a contiguous range of slabs each,
    their partial sums added in index order — on both sides of the path switch (31 / 32 / 33 slabs, 65536 / 65792 outputs), with an empty
    trailing range (33 slabs) and past the 4096 x 256 outputs of one grid turn; and in the reduction class against float64 with the negative
    control that drops the last slab."""
    L = lib()
    n_split, t, c_pad, n_pad, c, n = case
    slab, sd = slabs(case)
    outs = []
    for _ in range(2):
        dst = guarded(t * c * n)
        L.call('tg_slab_reduce_f32', ptr(sd), n_split, t, c_pad, n_pad, c, n, dst.ptr, st())
        outs.append(finish(dst, (t, c, n)))
    got = outs[0]
    assert_bits(outs[1], got, "a second launch")
    assert_bits(got, WR.slab32(case, slab), "slab_reduce (%s path) vs its in-order fp32 restatement" % WR.slab_path(case))
    ref, sabs = WR.slab64(slab, c, n)
    close(got, ref, sabs, "slab sum")
    assert rejected(got, WR.slab64(slab, c, n, drop_last=True)[0], sabs), "the bound does not reject the sum without the last slab"


TAIL_JOBS = [  # n_split, t, c_in, c_pad, c_out, n_pad, weight-normalised
    (4, 9, 128, 128, 128, 128, True),        # 16-byte slab path, rows 1152
    (3, 1, 1, 32, 45, 64, True),             # rows 1, c_out % 4 != 0: scalar slab path
    (2, 1, 31, 32, 32, 32, True),
    (5, 1, 32, 32, 100, 128, True),
    (2, 1, 97, 128, 7, 32, True),
    (1, 1, 127, 128, 64, 64, True),
    (3, 1, 128, 128, 33, 64, True),
    (2, 1, 129, 160, 12, 32, True),
    (6, 25, 3, 32, 128, 128, False),         # no weight norm: dw is the final gradient
    (1, 9, 3, 32, 32, 32, False),
    (2, 9, 45, 64, 47, 64, True),
    (7, 1, 250, 256, 10, 32, True),
    (2, 1, 1, 32, 1, 32, False),
    (3, 4, 8, 32, 8, 32, True),
    (2, 9, 64, 64, 200, 224, True),
    (1, 1, 5, 32, 3, 32, True),
]


@pytest.mark.parametrize("n_jobs", [1, 16])
def test_filter_grad_tail_multi(n_jobs):
    """tg_filter_grad_tail_multi_f32 (Context.flush_tails): dw = sum_s slab in slab order (bit-exact; both the 16-byte and the scalar slab
    paths), and for weight-normalised jobs dv / dg from that dw held to float64 with the negative control; jobs without v leave dv, dg
    and coef untouched."""
    L = lib()
    rng = np.random.default_rng(n_jobs)
    specs = TAIL_JOBS if n_jobs == 16 else TAIL_JOBS[:1]
    jobs = (L.WnJob * n_jobs)()
    keep, outs = [], []
    for i, (ns, t, c_in, c_pad, c_out, n_pad, wn) in enumerate(specs):
        slab = rng.standard_normal((ns, t, c_pad, n_pad)).astype(np.float32)
        v = rng.standard_normal((t * c_in, c_out)).astype(np.float32)
        g = (rng.random(c_out) + 0.5).astype(np.float32)
        sd, vd, gd = dev(slab), dev(v), dev(g)
        dw, dv, dg, coef = guarded(t * c_in * c_out), guarded(t * c_in * c_out), guarded(c_out), guarded(2 * c_out)
        keep.append((sd, vd, gd))
        jobs[i] = L.WnJob(sd.data_ptr(), dw.t.data_ptr(), vd.data_ptr() if wn else None, gd.data_ptr() if wn else None, dv.t.data_ptr(),
                          dg.t.data_ptr(), coef.t.data_ptr(), ns, t, c_pad, n_pad, c_in, c_out)
        outs.append((slab, v, g, dw, dv, dg, coef, specs[i]))
    L.call('tg_filter_grad_tail_multi_f32', C.cast(jobs, C.c_void_p), n_jobs, st())
    for slab, v, g, dw, dv, dg, coef, (ns, t, c_in, c_pad, c_out, n_pad, wn) in outs:
        got_dw = finish(dw, (t * c_in, c_out))
        ref_dw = seq_sum32([slab[s, :, :c_in, :c_out] for s in range(ns)]).reshape(t * c_in, c_out)
        assert_bits(got_dw, ref_dw, "slab reduction %s" % ((ns, t, c_in, c_out),))
        if not wn:
            for o in (dv, dg, coef):
                o.check_guard()
                assert np.isnan(o.get()).all()
            continue
        finish(coef)
        got_dv, got_dg = finish(dv, (t * c_in, c_out)), finish(dg)
        ref_dv, ref_dg, s_dv, s_dg = wn_bwd64(got_dw, v, g, (0,))
        assert worst(got_dv, ref_dv, s_dv) <= 1.0 and worst(got_dg, ref_dg, s_dg) <= 1.0, (t * c_in, c_out)
        if t * c_in > 1:
            _, short_dg, _, _ = wn_bwd64(got_dw, v, g, (0,), drop_last=lambda a, b: (a[:-1], b[:-1]))
            assert worst(got_dg, short_dg, s_dg) > 10.0
        # the immediate path on the same dw: both within the bound; equal bits are not promised (module docstring)
        dv2, dg2, coef2 = guarded(t * c_in * c_out), guarded(c_out), guarded(2 * c_out)
        L.call('tg_wn_bwd_f32', ptr(dev(got_dw)), ptr(dev(v)), ptr(dev(g)), t * c_in, c_out, dv2.ptr, dg2.ptr, coef2.ptr, st())
        assert worst(finish(dv2, (t * c_in, c_out)), ref_dv, s_dv) <= 1.0 and worst(finish(dg2), ref_dg, s_dg) <= 1.0
