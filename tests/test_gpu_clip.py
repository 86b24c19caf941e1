"""GPU tests of config.CLIP_NORM: tg_grad_norm_clip_f32 and the tg_*_clip_f32 optimisers against the float64 restatement
(tests/clip_reference.py; its forms, bounds and negative controls are checked on the CPU by tests/test_clip_reference.py on the same
inputs), the clip inside the training step, bit-identical execution modes that follow set_clip_norm(), resume, two data-parallel ranks
and the summary files."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import step_cifar10 as S
from oracle import tf_ops as T
import clip_reference as CR
import gpu_common as G
import optimizer_reference as R
import test_gpu_optimizers as TO            # its trainers' helpers (_state, _expected_keys, _free_port, ...): they would belong in gpu_common.py,
                                            # but existing files under tests/ stay as they are in this change, so they are borrowed, not moved

pytestmark = pytest.mark.gpu
ROOT = TO.ROOT
SMALL, NETS = TO.SMALL, TO.NETS
_lib, _st, _dev, _host = TO._lib, TO._st, TO._dev, TO._host
GS = CR.GRAD_SCALE


# ------------------------------------------------------------------------------------------------------------- 3. the kernel, direct
def _norm_clip(g_dev, clip, grad_scale=GS, stream=None, extra_ws_bytes=0, fill=None):
    """one tg_grad_norm_clip_f32 launch -> (out2 host [2], workspace host)."""
    lib = _lib()
    n = g_dev.numel()
    need = lib.call('tg_grad_norm_workspace_bytes', n)
    ws = torch.zeros((need + extra_ws_bytes) // 4, device='cuda')
    if fill is not None:
        ws.fill_(fill)
    out2, thr = torch.full((2,), -7.0, device='cuda'), _dev([clip])
    torch.cuda.synchronize()
    lib.call('tg_grad_norm_clip_f32', lib.ptr(g_dev), n, grad_scale, lib.ptr(thr), lib.ptr(out2), lib.ptr(ws), need + extra_ws_bytes,
             _st() if stream is None else stream)
    torch.cuda.synchronize()
    return _host(out2), _host(ws)


@pytest.mark.parametrize("name", CR.NORM_CASES)
def test_norm_and_factor_match_the_restatement(name):
    """{norm, factor} within one float32 ulp (rtol 1.2e-7) of the float64 restatement on the same float32 inputs, factor exactly 1.0f
    when norm <= clip; grad_scale 0.5, thresholds below, equal to and above the norm; n = 10 007 (tail), 3, a store's size, and more
    chunks than workgroups."""
    g = CR.stored(CR.norm_case(name))
    gd = _dev(g)
    assert gd.numel() == g.size
    for clip in CR.thresholds(g):
        norm, factor, _, _ = CR.norm_and_factor(g, clip, GS)
        out, _ = _norm_clip(gd, clip)
        miss = (CR.out_close(out[0], norm), CR.out_close(out[1], factor))
        print('%s clip %.6g: norm %.9g (error / bound %.3f)  factor %.9g (error / bound %.3f)' % (name, clip, out[0], miss[0], out[1], miss[1]))
        assert miss[0] <= 1.0 and miss[1] <= 1.0
        if norm <= clip:
            assert out[1].tobytes() == np.float32(1.0).tobytes()
        else:
            assert out[1] < 1.0
    assert _host(gd).tobytes() == g.tobytes()                                       # the gradient is not written


def test_reruns_and_streams_agree_in_every_bit():
    for name in ('tail', 'store'):
        g = CR.stored(CR.norm_case(name))
        gd = _dev(g)
        clip = CR.thresholds(g)[0]
        first, _ = _norm_clip(gd, clip)
        for _ in range(5):
            assert _norm_clip(gd, clip)[0].tobytes() == first.tobytes()
        side = torch.cuda.Stream()
        import ctypes
        assert _norm_clip(gd, clip, stream=ctypes.c_void_p(side.cuda_stream))[0].tobytes() == first.tobytes()
        assert _norm_clip(gd, clip, fill=123.0)[0].tobytes() == first.tobytes()       # the workspace needs no initialisation


def test_non_finite_input_gives_a_nan_factor():
    g = CR.stored(CR.norm_case('tail')).copy()
    g[1234] = np.inf
    out, _ = _norm_clip(_dev(g), 1.0)
    assert np.isinf(out[0]) and np.isnan(out[1])
    g[1234] = np.nan
    out, _ = _norm_clip(_dev(g), 1.0)
    assert np.isnan(out[0]) and np.isnan(out[1])
    out, _ = _norm_clip(torch.zeros(64, device='cuda'), 1.0)                         # a zero gradient is not clipped
    assert out[0] == 0.0 and out[1] == 1.0


def test_nothing_is_written_past_the_workspace_size():
    for name in ('tail', 'n3', 'store'):
        g = CR.stored(CR.norm_case(name))
        need = _lib().call('tg_grad_norm_workspace_bytes', g.size)
        sentinel = np.float32(-1234.5)
        out, ws = _norm_clip(_dev(g), 1.0, extra_ws_bytes=64, fill=float(sentinel))
        assert ws.size == need // 4 + 16 and (ws[need // 4:] == sentinel).all(), name
        assert (ws[:need // 4] != sentinel).all() and np.isfinite(out).all(), name    # every partial sum was written


def test_bad_arguments_return_an_error_status():
    lib = _lib()
    h = lib.load()
    n = 64
    buf = [torch.zeros(n + 4, device='cuda') for _ in range(4)]
    ws, out2, thr, lr = torch.zeros(8, device='cuda'), torch.zeros(2, device='cuda'), torch.ones(1, device='cuda'), torch.zeros(1, device='cuda')
    step = torch.zeros(1, dtype=torch.int32, device='cuda')
    P = lib.ptr
    ok = [P(b) for b in buf]
    off = [P(b[1:]) for b in buf]
    assert h.tg_grad_norm_clip_f32(ok[0], n, 1.0, P(thr), P(out2), P(ws), 32, _st()) == 0
    assert h.tg_grad_norm_clip_f32(None, n, 1.0, P(thr), P(out2), P(ws), 32, _st()) != 0
    assert h.tg_grad_norm_clip_f32(ok[0], n, 1.0, None, P(out2), P(ws), 32, _st()) != 0
    assert h.tg_grad_norm_clip_f32(ok[0], n, 1.0, P(thr), None, P(ws), 32, _st()) != 0
    assert h.tg_grad_norm_clip_f32(ok[0], n, 1.0, P(thr), P(out2), None, 32, _st()) != 0
    assert h.tg_grad_norm_clip_f32(ok[0], 0, 1.0, P(thr), P(out2), P(ws), 32, _st()) != 0
    assert h.tg_grad_norm_clip_f32(ok[0], -3, 1.0, P(thr), P(out2), P(ws), 32, _st()) != 0
    assert h.tg_grad_norm_clip_f32(off[0], n, 1.0, P(thr), P(out2), P(ws), 32, _st()) != 0 and b'16-B aligned' in h.tg_last_error_string()
    assert h.tg_grad_norm_clip_f32(ok[0], n, 1.0, P(thr), P(out2), P(ws[1:]), 28, _st()) != 0 and b'16-B aligned' in h.tg_last_error_string()
    assert h.tg_grad_norm_clip_f32(ok[0], n, 1.0, P(thr), P(out2), P(ws), 4, _st()) != 0 and b'workspace' in h.tg_last_error_string()
    assert h.tg_momentum_clip_f32(ok[0], ok[1], ok[2], n, P(lr), 0.9, 1.0, P(out2), _st()) == 0
    assert h.tg_momentum_clip_f32(ok[0], ok[1], ok[2], n, P(lr), 0.9, 1.0, None, _st()) != 0
    assert h.tg_rmsprop_clip_f32(ok[0], ok[1], ok[2], ok[3], n, P(lr), 0.9, 0.0, 1e-10, 1.0, None, _st()) != 0
    assert h.tg_adam_clip_f32(ok[0], ok[1], ok[2], ok[3], n, P(lr), 0.5, 0.999, 1e-8, P(step), 1.0, None, _st()) != 0
    assert h.tg_adam_clip_f32(ok[0], ok[1], ok[2], ok[3], 0, P(lr), 0.5, 0.999, 1e-8, P(step), 1.0, P(out2), _st()) != 0
    for k in range(3):
        a = list(ok[:3])
        a[k] = off[k]
        assert h.tg_momentum_clip_f32(a[0], a[1], a[2], n, P(lr), 0.9, 1.0, P(out2), _st()) != 0
    for k in range(4):
        a = list(ok)
        a[k] = off[k]
        assert h.tg_rmsprop_clip_f32(a[0], a[1], a[2], a[3], n, P(lr), 0.9, 0.0, 1e-10, 1.0, P(out2), _st()) != 0
        assert h.tg_adam_clip_f32(a[0], a[1], a[2], a[3], n, P(lr), 0.5, 0.999, 1e-8, P(step), 1.0, P(out2), _st()) != 0
    with pytest.raises(lib.TgError, match='grad_norm_clip'):
        lib.call('tg_grad_norm_clip_f32', ok[0], -5, 1.0, P(thr), P(out2), P(ws), 32, _st())
    torch.cuda.synchronize()
    assert int(step.item()) == 0 and not any(b.any().item() for b in buf)           # the refusals launched nothing


# ------------------------------------------------------------------------------------------------------------- 4. the _clip_ optimisers
def _launch(kind, clip, h, p, gd, slots, lr, step, grad_scale, factor_dev):
    """one optimiser launch, clipped (factor_dev given) or its unclipped twin."""
    lib = _lib()
    P = lib.ptr
    n = p.numel()
    tail = (P(factor_dev), _st()) if clip else (_st(),)
    sfx = '_clip_f32' if clip else '_f32'
    if kind == 'adam':
        lib.call('tg_adam' + sfx, P(p), P(gd), P(slots['m']), P(slots['v']), n, P(lr), h['beta1'], h['beta2'], h['epsilon'], P(step), grad_scale, *tail)
    elif kind == 'momentum':
        lib.call('tg_momentum' + sfx, P(p), P(gd), P(slots['accum']), n, P(lr), h['momentum'], grad_scale, *tail)
    else:
        lib.call('tg_rmsprop' + sfx, P(p), P(gd), P(slots['rms']), P(slots['mom']), n, P(lr), h['decay'], h['momentum'], h['epsilon'], grad_scale, *tail)


def _run_clipped(kind, case, factor_override=None, clip=True):
    lib = _lib()
    h = case['hyper']
    p, lr = _dev(case['p0']), _dev([h['lr']])
    slots = {k: _dev(v) for k, v in case['slots0'].items()}
    step = torch.zeros(1, dtype=torch.int32, device='cuda')
    n = p.numel()
    need = lib.call('tg_grad_norm_workspace_bytes', n)
    ws, out2, thr = torch.zeros(need // 4, device='cuda'), torch.zeros(2, device='cuda'), _dev([case['clip']])
    factors = []
    for g in case['grads']:
        gd = _dev(CR.stored(g))
        lib.call('tg_grad_norm_clip_f32', lib.ptr(gd), n, GS, lib.ptr(thr), lib.ptr(out2), lib.ptr(ws), need, _st())
        if factor_override is not None:
            out2[1:2].fill_(factor_override)
        _launch(kind, clip, h, p, gd, slots, lr, step, GS, out2[1:2])
        factors.append(float(out2[1].item()))
    torch.cuda.synchronize()
    return dict({k: _host(v) for k, v in slots.items()}, p=_host(p), factors=factors, step=int(step.item()))


@pytest.mark.parametrize("kind", CR.OPT_KINDS)
def test_clipped_optimizers_match_the_restatement(kind):
    """three clipped steps on n = 10 007 against clip_reference.run_reference: the parameter bound of tests/test_gpu_optimizers.py and its
    slot bound with one more rounding per step (clip_reference.SLOT_RTOL, derived there).  With a factor of 1.0 the clipped kernel's
    results are its unclipped twin's bit for bit."""
    case = CR.optimizer_case(kind)
    ref = CR.run_reference(kind, case)
    got = _run_clipped(kind, case)
    assert all(CR.out_close(a, b) <= 1.0 for a, b in zip(got['factors'], ref['factors'])), (got['factors'], ref['factors'])
    assert got['step'] == (R.STEPS if kind == 'adam' else 0)
    miss, slot = CR.optimizer_miss(kind, got, ref)
    print('%s: parameter error / bound %.3f, slot error / bound %.3f, factors %s' % (kind, miss, slot, got['factors']))
    assert miss <= 1.0 and slot <= 1.0
    if kind != 'adam':                                                               # negative control (Adam divides the scale out again)
        wrong = CR.run_reference(kind, case, form='per_variable')
        assert np.abs(got['p'] - wrong['p']).max() / R.param_bound(ref, R.STEPS) > 100.0
    again = _run_clipped(kind, case)
    one, twin = _run_clipped(kind, case, factor_override=1.0), _run_clipped(kind, case, clip=False)
    for k in ref:
        if k in got and k != 'factors':
            assert got[k].tobytes() == again[k].tobytes(), k
            assert one[k].tobytes() == twin[k].tobytes(), k
    assert one['p'].tobytes() != got['p'].tobytes()


# ------------------------------------------------------------------------------------------------------------- 5. in the step
def _record(tr):
    """wrap Train._train_op and Train._train_op_w_grads: the network's buffers before and after each application, and {norm, factor}."""
    rec = []

    def wrap(orig, clipped):
        def wrapped(optimizer, store, grad_scale=1.0, clip=None):
            torch.cuda.synchronize()
            before = {k: _host(getattr(store, k)) for k in 'pgmv'}
            t0 = int(store.step.item())
            out = orig(optimizer, store, grad_scale, clip=clip) if clipped else orig(optimizer, store, grad_scale)
            torch.cuda.synchronize()
            r = dict(net=store.name, opt=optimizer, grad_scale=grad_scale, before=before, after={k: _host(getattr(store, k)) for k in 'pgmv'},
                     steps=(t0, int(store.step.item())), clipped=clipped, grads=out)
            if clipped:
                thr, out2 = tr._clip_state(store)
                r['clip'], r['out2'] = float(clip.item()), _host(out2)
                assert clip.data_ptr() == thr.data_ptr()
            rec.append(r)
            return out
        return wrapped
    tr._train_op, tr._train_op_w_grads = wrap(tr._train_op, False), wrap(tr._train_op_w_grads, True)
    return rec


def _close(got, ref, atol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (CR.SLOT_RTOL * np.abs(ref) + atol)).max())


def _check(r, lr):
    """one recorded application against the restatement applied to the values snapshotted before it.  Slots: clip_reference.SLOT_RTOL on
    the result plus an absolute part for the slots that are signed sums, which can cancel — derived per element from the standard model
    fl(x op y) = (x op y)(1 + d), |d| <= u, with g_used = fl(fl(g*grad_scale)*factor) carrying 2u (the restatement's g_used is exact):
      momentum  accum' = fl(fl(accum*mu) + g_used):  u|accum| for the product (the term tests/test_gpu_optimizers.py allows, there as
                u max|accum|) + 2u|g_used| for the two roundings of the gradient, which that test does not have (grad_scale 1, no factor)
      Adam m    m' = fl(m + fl(fl(g_used - m)*w)), w = 1 - beta1:  w*(2u|g_used| + u|g_used - m| + u|g_used - m|) <= w*u*(4|g_used| + 2|m|)
      Adam v    v' = fl(v + fl(fl(fl(g_used^2) - v)*w2)), w2 = 1 - beta2:  g_used^2 carries 5u, so w2*u*(7 g_used^2 + 2 v)
    The final addition's own rounding is relative to the result and inside SLOT_RTOL.  RMSProp keeps the bound of
    tests/test_gpu_optimizers.py (no absolute part beyond SLOT_ATOL): rms' >= 0.9 rms and rms' >= 0.1 g_used^2, so the same terms are
    below 8u of the result."""
    b, a, opt = r['before'], r['after'], r['opt']
    tag = (r['net'], opt.kind, r['clipped'])
    assert a['g'].tobytes() == b['g'].tobytes(), tag                                 # the stored gradient is not written
    if r['clipped']:
        norm, factor, _, _ = CR.norm_and_factor(b['g'], r['clip'], r['grad_scale'])
        assert CR.out_close(r['out2'][0], norm) <= 1.0 and CR.out_close(r['out2'][1], factor) <= 1.0, (tag, r['out2'], norm, factor)
        if norm <= r['clip']:
            assert r['out2'][1] == np.float32(1.0), tag
        gu = b['g'].astype(np.float64) * r['grad_scale'] * float(r['out2'][1])        # the factor the step computed, held to 1 ulp above
        assert set(r['grads'].keys()) == set(tr_names(r)) and all(v.numel() > 0 for v in r['grads'].values())
    else:
        gu = b['g'].astype(np.float64) * r['grad_scale']
    m0, v0 = b['m'].astype(np.float64), b['v'].astype(np.float64)
    if opt.kind == 'adam':
        assert r['steps'][1] == r['steps'][0] + 1, tag
        p, m, v = T.adam_update(b['p'].astype(np.float64), gu, b['m'].astype(np.float64), b['v'].astype(np.float64), r['steps'][1], lr,
                                opt.beta1, R.f32(opt.beta2), R.f32(opt.epsilon))
        w1, w2 = 1.0 - opt.beta1, 1.0 - R.f32(opt.beta2)
        assert _close(a['m'], m, R.SLOT_ATOL + w1 * CR.U * (4 * np.abs(gu) + 2 * np.abs(m0))) <= 1.0, tag
        assert _close(a['v'], v, R.SLOT_ATOL + w2 * CR.U * (7 * gu * gu + 2 * v0)) <= 1.0, tag
    elif opt.kind == 'momentum':
        assert r['steps'][1] == r['steps'][0], tag
        p, accum = R.momentum_step(b['p'], gu, b['m'], lr, R.f32(opt.momentum))
        assert _close(a['m'], accum, R.SLOT_ATOL + CR.U * (np.abs(m0) + 2 * np.abs(gu))) <= 1.0, tag
        assert a['v'].tobytes() == b['v'].tobytes(), tag
    else:
        assert r['steps'][1] == r['steps'][0], tag
        p, ms, mom = R.rmsprop_step(b['p'], gu, b['v'], b['m'], lr, R.f32(opt.decay), R.f32(opt.momentum), R.f32(opt.epsilon))
        assert _close(a['v'], ms, R.SLOT_ATOL) <= 1.0 and _close(a['m'], mom, R.SLOT_ATOL) <= 1.0, tag
    ref = dict(max_update=np.abs(p - b['p']).max(), max_p=np.abs(p).max())
    err = np.abs(a['p'].astype(np.float64) - p).max()
    assert err <= R.param_bound(ref, 1), (tag, err, R.param_bound(ref, 1))
    assert ref['max_update'] > 0 and a['p'].tobytes() != b['p'].tobytes() and np.isfinite(a['p']).all(), tag


def tr_names(r):
    return r['grads'].store.names(True)


@pytest.mark.parametrize("optimizer, loss", [('adam', 'GAN'), ('momentum', 'GAN'), ('rmsprop', 'WGAN_GP')])
def test_two_eager_iterations_clip_d_leave_g_and_do_not_touch_c(optimizer, loss):
    """CLIP_NORM = (1e-3, 1e30, None): D certainly clipped, G certainly not, C unclipped (through _train_op).  Under WGAN-GP the norm is
    taken after the penalty's gradient has been added."""
    cfg = G.make_config(SMALL, USE_HIP_GRAPH=False, EXEC_MODE='eager', SEED=2, OPTIMIZER=optimizer, LOSS=loss, CLIP_NORM=(1e-3, 1e30, None))
    tr = G.fresh_trainer(cfg)
    assert tr.clip_norms == (1e-3, 1e30, None) and set(tr._clip_views) == set(NETS[:2])
    tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
    lr, cla_lr = (float(v) for v in tr.hyper[:2].cpu().numpy())
    rec = _record(tr)
    pre_gp = []
    if loss == 'WGAN_GP':
        orig_add = tr._add_gp_slice

        def add(sl):
            torch.cuda.synchronize()
            pre_gp.append(_host(tr.cx.stores['discriminator'].g))
            orig_add(sl)
        tr._add_gp_slice = add
    full = dict(S.SIZES, **SMALL)
    for it in range(2):
        tr.feed(S.synth_batch(60 + it, full))
        tr.sample_latent()
        tr.train_iteration(use_graph=False)
        norms = tr.grad_norms()
        assert norms['c'] is None and norms['d'][1] < 1.0 and norms['g'][1] == 1.0 and norms['d'][0] > 1e-3 and norms['g'][0] > 0, norms
    torch.cuda.synchronize()
    assert [(r['net'], r['clipped']) for r in rec] == [(NETS[0], True), (NETS[1], True), (NETS[2], False)] * 2
    for r in rec:
        _check(r, cla_lr if r['net'] == 'classifier' else lr)
    d = [r for r in rec if r['net'] == 'discriminator']
    assert all(r['out2'][1] < 1.0 for r in d) and all(r['out2'][1] == 1.0 for r in rec if r['net'] == 'good_generator')
    assert (norms['d'][0], norms['d'][1]) == (float(d[-1]['out2'][0]), float(d[-1]['out2'][1]))
    assert all(np.isfinite(v) for v in tr.losses())
    if loss == 'WGAN_GP':
        assert len(pre_gp) == 2
        for r, g0 in zip(d, pre_gp):
            without = CR.global_norm(g0, r['grad_scale'])
            assert abs(float(r['out2'][0]) - without) > 1e-4 * without, (r['out2'], without)      # the penalty's gradient is in the norm
    with pytest.raises(_lib().TgError, match='unclipped'):
        tr.set_clip_norm(c=1.0)


def _run_philox(clip, iters=3, mode='plan', seed=3, optimizer='adam', new_d=None):
    tr = G.fresh_trainer(G.make_config(SMALL, USE_HIP_GRAPH=None, EXEC_MODE=mode, SEED=seed, OPTIMIZER=optimizer, CLIP_NORM=clip))
    tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
    tr.feed(S.synth_batch(7, dict(S.SIZES, **SMALL)))
    norms = []
    for it in range(iters):
        if new_d is not None and it == iters - 1:
            tr.set_clip_norm(d=new_d)
        tr.sample_latent()
        tr.train_iteration()
        norms.append(tr.grad_norms())
    torch.cuda.synchronize()
    state = {}
    for k, st in tr.cx.stores.items():
        for buf in ('p', 'm', 'v', 's'):
            state[k + '/' + buf] = _host(getattr(st, buf))
        if st.ema is not None:
            state[k + '/ema'] = _host(st.ema)
    return dict(state=state, norms=norms, losses=tr.losses())


def test_a_clip_that_never_bites_leaves_the_run_bit_identical():
    """(1e30, 1e30, 1e30): three Philox iterations leave weights, slots, EMA and running state as CLIP_NORM = None does."""
    a, b = _run_philox(None), _run_philox((1e30, 1e30, 1e30))
    assert a['norms'][-1] == dict(d=None, g=None, c=None)
    assert all(v[1] == 1.0 and v[0] > 0 for v in b['norms'][-1].values())
    assert a['losses'] == b['losses']
    for k in a['state']:
        assert a['state'][k].tobytes() == b['state'][k].tobytes(), k


def test_train_op_w_grads_stands_alone_with_a_number_and_without_a_clip():
    """Train_base._train_op_w_grads outside Train's wiring: clip as a plain number goes through the context's own {threshold, norm, factor}
    buffer and equals the device-threshold path bit for bit; clip = None is _train_op and still returns the gradient views."""
    from Training.train_base import GradViews
    lib = _lib()
    results = {}
    for how in ('number', 'tensor', 'none', 'train_op'):
        tr = G.fresh_trainer(G.make_config(SMALL, USE_HIP_GRAPH=False, EXEC_MODE='eager', SEED=4, OPTIMIZER='momentum'))
        assert tr._clip_views == {} and tr.clip_dev is None
        st = tr.cx.stores['classifier']
        st.g.copy_(torch.from_numpy(np.random.default_rng(41).standard_normal(st.n_p).astype(np.float32)))
        g0 = _host(st.g)
        if how == 'number':
            grads = tr._train_op_w_grads(tr.c_optimizer, st, 0.5, clip=0.25)
        elif how == 'tensor':
            grads = tr._train_op_w_grads(tr.c_optimizer, st, 0.5, clip=torch.full((1,), 0.25, device='cuda'))
        elif how == 'none':
            grads = tr._train_op_w_grads(tr.c_optimizer, st, 0.5)
        else:
            grads = tr._train_op(tr.c_optimizer, st, 0.5)
        torch.cuda.synchronize()
        results[how] = (_host(st.p), _host(st.m))
        assert _host(st.g).tobytes() == g0.tobytes()
        if how == 'train_op':
            assert grads is None
            continue
        assert isinstance(grads, GradViews) and list(grads.keys()) == st.names(True) and len(grads) == len(st.names(True))
        nm = st.names(True)[0]
        assert nm in grads and 'no_such_variable' not in grads and grads[nm].data_ptr() == st.grad(nm).data_ptr()
        assert np.array_equal(_host(grads[nm]), g0[st.offset(nm):st.offset(nm) + grads[nm].numel()])
        with pytest.raises(KeyError):
            grads['no_such_variable']
        if how != 'none':
            thr, out2 = tr._clip_state(st)
            norm, factor, _, _ = CR.norm_and_factor(g0, 0.25, 0.5)
            out = _host(out2)
            assert CR.out_close(out[0], norm) <= 1.0 and CR.out_close(out[1], factor) <= 1.0 and out[1] < 1.0
            if how == 'number':
                assert float(thr.item()) == 0.25
            for bad in (0.0, -1.0, float('nan'), float('inf')):
                with pytest.raises(lib.TgError, match='positive finite'):
                    tr._train_op_w_grads(tr.c_optimizer, st, 0.5, clip=bad)
            torch.cuda.synchronize()
            assert _host(st.p).tobytes() == results[how][0].tobytes()            # the refusals applied nothing
    for k in (0, 1):
        assert results['number'][k].tobytes() == results['tensor'][k].tobytes()
        assert results['none'][k].tobytes() == results['train_op'][k].tobytes()
        assert results['number'][k].tobytes() != results['none'][k].tobytes()


# ------------------------------------------------------------------------------------------------------------- 6. execution modes
def test_execution_modes_are_bit_identical_and_follow_set_clip_norm():
    """three Philox iterations with every network clipped, then set_clip_norm(d = 4x) and a fourth: a threshold passed by value into a
    recorded plan or graph would leave the replayed modes on the old one.  D runs first in an iteration, so both fourth iterations see
    the same D gradient: the factor scales by the ratio of the thresholds (4, a power of two) to one ulp."""
    clip = (1e-3, 1e-3, 1e-3)
    runs = {m: _run_philox(clip, iters=4, mode=m, optimizer='momentum', new_d=4e-3) for m in ('eager', 'overlap', 'plan', 'graph')}
    ref = runs['eager']
    assert all(v[1] < 1.0 for n in ref['norms'] for v in n.values()), ref['norms']            # an active clip, every network, every iteration
    for m, r in runs.items():
        assert r['norms'] == ref['norms'], (m, r['norms'], ref['norms'])
        assert r['losses'] == ref['losses'], m
        for k in ref['state']:
            assert r['state'][k].tobytes() == ref['state'][k].tobytes(), (m, k)
    old = _run_philox(clip, iters=4, mode='plan', optimizer='momentum')
    assert old['norms'][:3] == ref['norms'][:3]
    assert old['norms'][3]['d'][0] == ref['norms'][3]['d'][0]                                # the same D gradient
    ratio = ref['norms'][3]['d'][1] / old['norms'][3]['d'][1]
    assert abs(ratio - 4.0) <= 4.0 * CR.OUT_RTOL, ratio
    assert old['state']['discriminator/p'].tobytes() != ref['state']['discriminator/p'].tobytes()


# ------------------------------------------------------------------------------------------------------------- 7. resume
def test_resume_continues_bit_identically_and_the_checkpoint_gains_no_key(tmp_path):
    from Training.Saver import Saver
    kinds, clip = ('adam', 'momentum', 'rmsprop'), (1e-3, 1e-3, 2e-3)
    feeds = [S.synth_batch(40 + i, dict(S.SIZES, **SMALL)) for i in range(4)]

    def run(tr, its):
        for i in its:
            tr.feed(feeds[i])
            tr.sample_latent()
            tr.train_iteration()
        torch.cuda.synchronize()

    a = G.fresh_trainer(G.make_config(SMALL, SEED=9, USE_HIP_GRAPH=True, OPTIMIZER=kinds, CLIP_NORM=clip))
    a.set_hyper(lambda_1=0.3, lambda_2=0.5)
    run(a, [0, 1])
    saver = Saver(str(tmp_path))
    saver.set_save_path(comments='resume test')
    path = saver.save(a, 'model_0002.ckpt')
    with np.load(path) as z:
        assert set(z.files) == TO._expected_keys(a, kinds)                           # exactly an unclipped run's keys
    run(a, [2, 3])
    want, want_losses, want_norms = TO._state(a), a.losses(), a.grad_norms()
    assert all(v[1] < 1.0 for v in want_norms.values())
    b = G.fresh_trainer(G.make_config(SMALL, SEED=1234, USE_HIP_GRAPH=True, OPTIMIZER=kinds, CLIP_NORM=clip))
    b.set_hyper(lambda_1=0.3, lambda_2=0.5)
    assert Saver(str(tmp_path)).restore(b) == 2
    run(b, [2, 3])
    got = TO._state(b)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert b.losses() == want_losses and b.grad_norms() == want_norms
    c = G.fresh_trainer(G.make_config(SMALL, SEED=5, USE_HIP_GRAPH=True, OPTIMIZER=kinds))       # restoring works across CLIP_NORM settings
    assert Saver(str(tmp_path)).restore(c) == 2


# ------------------------------------------------------------------------------------------------------------- 8. data parallel
WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, os.path.join({root!r}, "tensorflow-implementation-of-triple-gan_amd"))
import torch
import gpu_common as G
from oracle import step_cifar10 as S
sizes = {sizes!r}
tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=None, EXEC_MODE='plan', SEED=5, OPTIMIZER={optimizer!r}, CLIP_NORM={clip!r}))
rank = tr.rank
tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
full = dict(S.SIZES, **sizes)
p0 = {{k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}}
norms = []
for it in range({iters}):
    tr.feed(S.synth_batch(1000 * rank + it, full))
    tr.sample_latent()
    tr.train_iteration()
    norms.append(tr.grad_norms())
torch.cuda.synchronize()
torch.save(dict(world=tr.world, rank=rank, norms=norms, losses=tr.losses(), p0=p0, p={{k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}}),
           {out!r} % rank)
torch.distributed.destroy_process_group()
'''


def _one_process_sum(sizes, p0, iters, optimizer, clip):
    """one process, no replicas: each shard's gradient (its own batch and Philox seed) is computed, the two are summed as the all-reduce does
    and the optimiser steps through _train_op_w_grads with grad_scale 1/2 and the network's device threshold."""
    tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=False, EXEC_MODE='eager', SEED=5, OPTIMIZER=optimizer, CLIP_NORM=clip))
    tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
    cx, st = tr.cx, tr.cx.stores
    for k, s in st.items():
        s.p.copy_(torch.from_numpy(p0[k]))
    st['classifier'].ema.copy_(st['classifier'].p)
    full = dict(S.SIZES, **sizes)
    phs = [tr.z_g_ph, tr.y_g_ph, tr.x_l_c_ph, tr.y_l_c_ph, tr.x_l_d_ph, tr.y_l_d_ph, tr.x_u_d_ph, tr.x_u_c_ph]
    rng = [torch.tensor([5 + 7919 * r, 0], dtype=torch.int64, device=cx.device) for r in range(2)]
    norms = []
    for it in range(iters):
        feeds = []
        for r in range(2):
            cx.rng.state.copy_(rng[r])
            tr.feed(S.synth_batch(1000 * r + it, full))
            tr.sample_latent()
            feeds.append([p.t.clone() for p in phs])

        def solver(fn, net, opt):
            g = []
            for r in range(2):
                cx.rng.state.copy_(rng[r])
                for p, v in zip(phs, feeds[r]):
                    p.t.copy_(v)
                tr._g_saved = None
                fn()
                g.append(st[net].g.clone())
            st[net].g.copy_(g[0] + g[1])
            tr._train_op_w_grads(opt, st[net], 0.5, clip=tr._clip_views[net][0])
        solver(tr._d_forward_backward, 'discriminator', tr.d_optimizer)
        solver(tr._g_forward_backward, 'good_generator', tr.g_optimizer)
        solver(tr._c_forward_backward, 'classifier', tr.c_optimizer)
        norms.append(tr.grad_norms())
        for r in range(2):
            cx.rng.state.copy_(rng[r])
            cx.rng.advance(cx)
            rng[r].copy_(cx.rng.state)
    torch.cuda.synchronize()
    return {k: s.p.cpu().numpy() for k, s in st.items()}, norms


def test_two_ranks_clip_like_one_process_on_the_summed_gradient(tmp_path):
    sizes, iters, optimizer, clip = SMALL, 2, ('momentum', 'adam', 'rmsprop'), (1e-3, 1e-3, 1e-3)
    port = TO._free_port()
    out = str(tmp_path / "r%d.pt")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, sizes=sizes, out=out, iters=iters, optimizer=optimizer, clip=clip))
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   TG_DIST_BACKEND="gloo", TG_DEVICE_INDEX="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-3000:]
    r = [torch.load(out % i, weights_only=False) for i in range(2)]
    assert r[0]['world'] == r[1]['world'] == 2
    assert r[0]['norms'] == r[1]['norms']                                            # the same {norm, factor} bits on both ranks
    assert all(v[1] < 1.0 for n in r[0]['norms'] for v in n.values())
    for k in r[0]['p']:
        np.testing.assert_array_equal(r[0]['p'][k], r[1]['p'][k])
    ref_p, ref_norms = _one_process_sum(sizes, r[0]['p0'], iters, optimizer, clip)
    assert ref_norms == r[0]['norms'], (ref_norms, r[0]['norms'])
    for k in ref_p:
        assert np.abs(ref_p[k] - r[0]['p'][k]).max() == 0.0, (k, np.abs(ref_p[k] - r[0]['p'][k]).max())
        assert np.abs(r[0]['p'][k] - r[0]['p0'][k]).max() > 0, k


# ------------------------------------------------------------------------------------------------------------- 9. summaries
def _one_epoch(tmp_path, monkeypatch, clip):
    from tg import runtime
    from Training import Train_goodGAN as TG
    runtime.set_context(None)

    class Flags(object):
        train_size = 4000 + 300
        sample_dir = None
        seed = 1
        clip_norm = clip
    monkeypatch.setattr(TG, "_root_dir", lambda: str(tmp_path))
    hist = TG._main_training_cifar10(Flags(), epochs=1)
    assert len(hist) == 1
    found = dict(hist=hist[0])
    for dirpath, _, files in os.walk(str(tmp_path)):
        for f in files:
            if os.sep + 'train' + os.sep in dirpath + os.sep and (f == 'history.csv' or f.startswith('events.out.tfevents')):
                found['csv' if f == 'history.csv' else 'events'] = open(os.path.join(dirpath, f), 'rb').read()
    return found


def test_summaries_carry_the_norms_only_with_a_clip(tmp_path, monkeypatch):
    tags = [b'd_grad_norm', b'g_grad_norm', b'c_grad_norm']
    plain = _one_epoch(tmp_path / 'plain', monkeypatch, None)
    lines = plain['csv'].decode().splitlines()
    h = plain['hist']                                                        # today's columns exactly, and the row Summary.write formats
    assert lines == ['step,g_loss,d_loss,c_loss', '%d,' % h['epoch'] + ','.join('%.6g' % h[k] for k in ('g_loss', 'd_loss', 'c_loss'))]
    again = _one_epoch(tmp_path / 'plain2', monkeypatch, None)               # the same seed: the same bytes
    assert again['csv'] == plain['csv']
    assert not any(t in plain['events'] for t in tags) and all(t in plain['events'] for t in (b'g_loss', b'd_loss', b'c_loss'))
    clipped = _one_epoch(tmp_path / 'clipped', monkeypatch, 1e-3)
    lines = clipped['csv'].decode().splitlines()
    assert lines[0] == 'step,g_loss,d_loss,c_loss,d_grad_norm,g_grad_norm,c_grad_norm' and len(lines) == 2
    vals = [float(v) for v in lines[1].split(',')]
    assert len(vals) == 7 and all(np.isfinite(vals)) and all(v > 1e-3 for v in vals[4:])
    assert all(clipped['events'].count(t) == 1 for t in tags)
