"""The float64 restatements of tests/ops_reference.py, checked without a GPU.

  * attainability: the same formulas evaluated in float32 (torch's own order of summation) stay inside the bound the float64 evaluation
    propagates, for every case of tests/launch_trace.py that has a reference and for every shape tests/test_gpu_ops_routes.py uses.  A
    correct fp32 implementation therefore passes the GPU test; a bound that is too tight here would be a derivation that misses a term.
    The float32 run plays the implementation under test: its stored forward outputs give the relu / lrelu masks of the reference's
    backward pass, as the device's do on the GPU.
  * pooling decisions: in every pooling window of every case the two largest reference values differ by more than four times their
    forward bound (the seeds in ops_reference.fill are the case names; a case that fails this gets another name suffix there, not an
    exclusion here).
  * negative controls: per family, a reference that is off by one tap / one slab / one segment row / one pixel exceeds the bound by more
    than 10x (kernel_check.rejected).
  * ragged shapes stay on their routes: every launch_trace.RAGGED shape runs through the Tracer and check_route.
  * coverage guard: every case of launch_trace.CASES has a reference or a stated exemption, never both.
  * the oracle's NumPy convolutions (oracle/tf_ops.py) and the torch restatement used here agree.

`python tests/test_ops_reference.py --profile [gpu_ratios.json]` writes profiles/ops_routes.txt."""
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == '__main__':
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "tensorflow-implementation-of-triple-gan_amd"), os.path.join(_root, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import kernel_check as KC
import launch_trace as LT
import ops_reference as R
from oracle import tf_ops as T

ITEMS = R.items(LT)
F32, F64 = torch.float32, torch.float64


def attain(name, shape, mp, ident=None):
    """-> ({key: worst ratio of the float32 evaluation}, pool margin of the reference)"""
    lo = R.run_reference(LT, name, mp, F32, None, shape, R.fill_key(name, ident))
    ref = R.run_reference(LT, name, mp, F64, lo.ystore, shape, R.fill_key(name, ident))
    want = R.expected(ref)
    got = {k: v[0] for k, v in R.expected(lo).items()}
    return R.ratios(got, want), ref.cx.pool_margin, got, want


@pytest.mark.parametrize('ident,name,shape', ITEMS, ids=[i[0] for i in ITEMS])
def test_float32_evaluation_stays_inside_the_bound(ident, name, shape, monkeypatch):
    rat, margin, got, want = attain(name, shape, monkeypatch, ident)
    assert margin > 1.0, "%s: a pooling window's two largest values are within 4x their bound (margin %.3g)" % (ident, margin)
    assert len(rat) >= 2
    for key, r in sorted(rat.items()):
        assert r <= 1.0, "%s: float32 evaluation at %.3g x the bound; %s" % (ident, r, R.worst_element(got, want, key))


@pytest.mark.parametrize('name', sorted(LT.RAGGED))
def test_ragged_shape_stays_on_its_route(name):
    shape = LT.RAGGED[name]
    variants = [n for n, c in LT.CASES.items() if c.fn.__name__ == name]
    assert variants
    for v in variants:
        with pytest.MonkeyPatch.context() as mp:
            LT.check_route(v, LT.run_case(v, mp, shape))


def test_every_case_has_a_reference_or_an_exemption():
    refs = R.register(LT)
    assert set(refs) | set(R.EXEMPT) == set(LT.CASES)
    assert not set(refs) & set(R.EXEMPT)
    assert all(len(reason) > 20 for reason in R.EXEMPT.values())
    assert set(LT.RAGGED) <= {c.fn.__name__ for c in LT.CASES.values()}
    # a single exempt shape: its case has a reference and is still held to float64 at its other shape
    held = {}
    for ident, name, _ in ITEMS:
        held.setdefault(name, []).append(ident)
    for ident, reason in R.EXEMPT_SHAPES.items():
        name = ident.split('@')[0]
        assert len(reason) > 20 and refs.get(name) in ('full', 'forward') and held.get(name) and ident not in held[name], ident
    assert {n for n in refs if refs[n] in ('full', 'forward')} == set(held)
    assert set(R.KERNEL_REFUSES) <= set(R.EXEMPT) | set(R.EXEMPT_SHAPES)


def test_undefined_tensors_belong_to_their_cases(monkeypatch):
    for name, keys in R.UNDEFINED.items():
        assert R.register(LT)[name] == 'full'
        want = R.expected(R.run_reference(LT, name, monkeypatch))
        assert set(keys) <= set(want), (name, sorted(set(keys) - set(want)))


# ------------------------------------------------------------------ the torch restatement against the oracle's NumPy one

@pytest.mark.parametrize('stride,padding,k', [(1, 'SAME', 3), (2, 'SAME', 3), (1, 'VALID', 3), (2, 'SAME', 5), (2, 'VALID', 3), (1, 'SAME', 1)])
def test_convolutions_agree_with_the_oracle(stride, padding, k):
    rng = np.random.default_rng(5)
    x, w = rng.standard_normal((3, 7, 6, 5)), rng.standard_normal((k, k, 5, 4))
    y = T.conv2d(x, w, (stride, stride), padding)
    dy = rng.standard_normal(y.shape)
    tx, tw, tdy = (torch.from_numpy(a) for a in (x, w, dy))
    np.testing.assert_allclose(R._conv_raw(tx, tw, stride, padding).numpy(), y, rtol=0, atol=1e-12)
    np.testing.assert_allclose(R._conv_dx_raw(tdy, tw, x.shape, stride, padding).numpy(), T.conv2d_bwd_input(x.shape, w, dy, (stride, stride), padding), rtol=0, atol=1e-12)
    np.testing.assert_allclose(R._conv_dw_raw(tx, tdy, w.shape, stride, padding).numpy(), T.conv2d_bwd_filter(x, dy, w.shape, (stride, stride), padding), rtol=0, atol=1e-12)


def test_deconv_and_weight_norm_agree_with_the_oracle():
    rng = np.random.default_rng(6)
    x, w, g = rng.standard_normal((2, 3, 5, 6)), rng.standard_normal((5, 5, 4, 6)), 1 + 0.1 * rng.standard_normal(4)
    V = lambda a: R.V(torch.from_numpy(np.asarray(a)))
    np.testing.assert_allclose(R.deconv_fwd(V(x), V(w)).v.numpy(), T.conv2d_transpose(x, w), rtol=0, atol=1e-12)
    np.testing.assert_allclose(R.wn_weight(V(w), V(g), 2).v.numpy(), T.wn_weight(w, g, 2), rtol=0, atol=1e-12)
    dw = rng.standard_normal(w.shape)
    dv, dg = R.wn_weight_bwd(V(w), V(g), V(dw), 2)
    rv, rg = T.wn_weight_bwd(w, g, dw, 2)
    np.testing.assert_allclose(dv.v.numpy(), rv, rtol=0, atol=1e-12)
    np.testing.assert_allclose(dg.v.numpy(), rg, rtol=0, atol=1e-12)


# ------------------------------------------------------------------ negative controls

def _V(a):
    return R.V(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(F64))


def _rejected(ctrl, ref):
    """the control (a V or tensor) lies more than 10x outside the bound of `ref`"""
    c = ctrl.v if isinstance(ctrl, R.V) else ctrl
    return KC.worst(c.numpy(), ref.v.numpy(), ref.e.numpy() / KC.TOL)


def controls():
    """{family: by how many bounds the off-by-one reference misses}"""
    rng = np.random.default_rng(11)
    n, h, w, ci, co = 3, 6, 10, 42, 48
    x, wt, dy = _V(rng.standard_normal((n, h, w, ci))), _V(0.1 * rng.standard_normal((3, 3, ci, co))), _V(rng.standard_normal((n, h, w, co)))
    g = _V(1 + 0.1 * rng.standard_normal(co))
    tap = R.V(wt.v.clone())
    tap.v[2, 2] = 0                                                           # one tap dropped
    out = {}
    out['conv forward, one tap'] = _rejected(R.conv_fwd(x, tap), R.conv_fwd(x, wt))
    out['input gradient, one tap'] = _rejected(R.conv_dx(dy, tap, x.shape), R.conv_dx(dy, wt, x.shape))
    slab = lambda a: R.V(torch.cat([a.v[:-1], torch.zeros_like(a.v[-1:])]))   # the last image's slab dropped
    full = R.wn_weight_bwd(wt, g, R.conv_dw(x, dy, wt.shape))
    part = R.wn_weight_bwd(wt, g, R.conv_dw(slab(x), dy, wt.shape))
    out['filter gradient with weight norm (dV), one slab'] = _rejected(part[0], full[0])
    out['filter gradient with weight norm (dg), one slab'] = _rejected(part[1], full[1])
    b, pop = _V(0.3 * rng.standard_normal(co)), _V(0.3 * rng.standard_normal(co))
    y, p1 = R.mobn_train(dy, b, pop, [1, 2])
    short = dy.v[1:].reshape(-1, co)[:-1].mean(0)                             # the last segment's mean without its final row
    ctrl = y.v.clone()
    ctrl[1:] = dy.v[1:] - short + b.v
    out['mean-only BN, one segment row'] = _rejected(ctrl, y)
    gam, bet = _V(1 + 0.1 * rng.standard_normal(co)), _V(0.3 * rng.standard_normal(co))
    yb, _, _, _ = R.batch_norm_train(dy, gam, bet, None, None, 1e-5, 0.9, [1, 2])
    rows = dy.v[1:].reshape(-1, co)[:-1]
    ctrl = yb.v.clone()
    ctrl[1:] = (dy.v[1:] - rows.mean(0)) / torch.sqrt(rows.var(0, unbiased=False) + 1e-5) * gam.v + bet.v
    out['batch norm, one segment row'] = _rejected(ctrl, yb)
    ym, _, _, _ = R.batch_norm_moments(dy, gam, bet, None, None, 1e-5, 0.9)
    rows = dy.v.reshape(-1, co)[:-1]
    out['batch norm from moments, one row'] = _rejected((dy.v - rows.mean(0)) / torch.sqrt(rows.var(0, unbiased=False) + 1e-5) * gam.v + bet.v, ym)
    pooled = R.maxpool2(dy)[0]
    out['max pool, window one pixel off'] = _rejected(R.maxpool2(R.V(torch.roll(dy.v, 1, 2)))[0], pooled)
    avg = R.global_avgpool(dy)
    out['global average pool, one pixel dropped'] = _rejected((dy.v.sum((1, 2), keepdim=True) - dy.v[:, -1:, -1:]) / (h * w), avg)
    cat = R.cond_concat(dy, _V(np.eye(10)[[1, 4, 7]]))
    lab = cat.v.clone()
    lab[..., co:] = torch.roll(lab[..., co:], 1, -1)                          # the labels one channel off
    out['label concat, one channel off'] = _rejected(lab, cat)
    xd, wd = _V(rng.standard_normal((2, 3, 5, ci))), _V(0.1 * rng.standard_normal((5, 5, co, ci)))
    tapd = R.V(wd.v.clone())
    tapd.v[4, 4] = 0
    out['deconv forward, one tap'] = _rejected(R.deconv_fwd(xd, tapd), R.deconv_fwd(xd, wd))
    out['deconv filter gradient, one tap'] = _rejected(R.V(R.deconv_dw(xd, R.deconv_fwd(xd, wd), wd.shape).v * (tapd.v != 0)), R.deconv_dw(xd, R.deconv_fwd(xd, wd), wd.shape))
    return out


def test_negative_controls_exceed_the_bound():
    for family, r in controls().items():
        assert r > 10.0, "%s: the off-by-one reference is only %.3g x the bound away" % (family, r)


# ------------------------------------------------------------------ profiles/ops_routes.txt

def write_profile(gpu_json=None):
    gpu = json.load(open(gpu_json)) if gpu_json else {}
    lines = ["Worst error-to-bound ratio per case and shape of tests/launch_trace.py (<= 1 passes; tests/ops_reference.py propagates the bound).",
             "fp32-cpu: the reference's formulas evaluated in torch float32 (tests/test_ops_reference.py); gpu: tg/ops.py on an MI355X",
             "(tests/test_gpu_ops_routes.py); '-': not measured.", "",
             "%-46s %10s %10s  %s" % ("case", "fp32-cpu", "gpu", "worst output (gpu, else fp32-cpu)")]
    for ident, name, shape in ITEMS:
        with pytest.MonkeyPatch.context() as mp:
            rat = attain(name, shape, mp, ident)[0]
        key = max(rat, key=rat.get)
        g = gpu.get(ident)
        gtxt, gkey = ("%10.3g" % g['worst'], g['key']) if g else ("%10s" % '-', key)
        lines.append("%-46s %10.3g %s  %s" % (ident, rat[key], gtxt, gkey))
    for ident in sorted(set(gpu) - {i[0] for i in ITEMS}):
        lines.append("%-46s %10s %10.3g  %s" % (ident, '-', gpu[ident]['worst'], gpu[ident]['key']))
    lines += ["", "No float64 check (ops_reference.EXEMPT, EXEMPT_SHAPES):"]
    lines += ["%-46s %s" % (k, 'the launch refuses the shape' if k in R.KERNEL_REFUSES else 'not a tg.ops route') for k in sorted(dict(R.EXEMPT, **R.EXEMPT_SHAPES))]
    lines += ["", "Negative controls (a reference off by one; > 10 is rejected):"]
    lines += ["%-56s %10.3g" % kv for kv in controls().items()]
    path = os.path.join(LT.ROOT, 'profiles', 'ops_routes.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print("wrote", path)


if __name__ == '__main__':
    if sys.argv[1:2] != ['--profile']:
        sys.exit("usage: python tests/test_ops_reference.py --profile [gpu_ratios.json]")
    write_profile(sys.argv[2] if len(sys.argv) > 2 else None)
