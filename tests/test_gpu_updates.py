"""The update kernels of csrc/optim.hip at the grid-stride wrap: tg_adam_f32, tg_momentum_f32, tg_rmsprop_f32, their _clip forms and
tg_ema_f32.  The launches cap their grid at 2 048 workgroups of 256 threads (ew_grid), which every real parameter buffer exceeds; the
other tests of these kernels stay far below it.

Sizes: n = 4 * 2048 * 256 + 4 * 37 + 3 for the four-wide kernels (every thread takes one 16-byte element, the first 37 a second one, and
three scalars remain for the tail loop); n = 2048 * 256 + 37 for tg_ema_f32 (one float per thread).

Two checks over two steps:
  (a) against the float64 restatements — oracle.tf_ops.adam_update / ema_update evaluated in float64 and tests/optimizer_reference.py, fed the
      hyper-parameters as the float32 values the kernels receive — with the bounds those kernels' tests already use: slots within
      SLOT_RTOL = 1e-6 (4 roundings per step), parameters within param_bound = 1e-6 max|update| steps + 2e-7 max|p|, the shadow within
      1e-6 |s| + 1e-7.  As in optimizer_reference.kernel_case the sign of an element's gradient is the same in both steps, so no slot
      cancels and a relative bound is meaningful; every 7th gradient is scaled by 1e-9 and every 11th is zero.
  (b) bit-identical to the same entry point called on consecutive pieces of at most 2^19 elements, each starting at a multiple of four
      elements (16 bytes) — launches that do not wrap (2^19 / 4 = 131 072 16-byte elements < 2 048 * 256 threads).  Adam's step counter is set
      to t - 1 in front of every piece so that both runs see the same t.  An element skipped or updated twice at the wrap cannot pass.
The _clip forms with the device factor 1.0f equal the plain forms bit for bit (include/tg_kernels.h).  p and every slot are followed by a
guard (tests/kernel_check.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from kernel_check import assert_bits, dev, finish, guarded, lib, ptr, st
from oracle import tf_ops as T
import optimizer_reference as R

pytestmark = pytest.mark.gpu

CAP = 2048 * 256
N4 = 4 * CAP + 4 * 37 + 3
N1 = CAP + 37
PIECE = 1 << 19
STEPS = 2
GRAD_SCALE = 0.5
HYPER = dict(lr=R.f32(3e-4), beta1=R.f32(0.5), beta2=R.f32(0.999), eps_adam=R.f32(1e-8), momentum=R.f32(0.9), decay=R.f32(0.9), eps_rms=R.f32(1e-10))
SLOTS = {'adam': ('m', 'v'), 'momentum': ('accum',), 'rmsprop': ('rms', 'mom')}
f8 = lambda a: np.asarray(a, np.float64)


def case(kind):
    rng = np.random.default_rng({'adam': 21, 'momentum': 22, 'rmsprop': 23}[kind])
    p0 = rng.standard_normal(N4).astype(np.float32)
    sign = np.where(rng.random(N4) < 0.5, -1.0, 1.0)
    grads = []
    for _ in range(STEPS):
        g = (np.abs(rng.standard_normal(N4)) * sign).astype(np.float32)
        g[::7] *= np.float32(1e-9)
        g[::11] = 0
        grads.append(g)
    slots0 = {s: (np.ones if s == 'rms' else np.zeros)(N4, np.float32) for s in SLOTS[kind]}
    return p0, slots0, grads


def pieces(n):
    return [(o, min(PIECE, n - o)) for o in range(0, n, PIECE)]


def launch(kind, clip, p, slots, g, n, lr, step, factor):
    """one call of the entry point on device pointers (ctypes) of p, the slots in SLOTS order and g"""
    L, h = lib(), HYPER
    tail = ([ptr(factor)] if clip else []) + [st()]
    if kind == 'adam':
        L.call('tg_adam_clip_f32' if clip else 'tg_adam_f32', p, g, slots[0], slots[1], n, ptr(lr), h['beta1'], h['beta2'], h['eps_adam'], ptr(step), GRAD_SCALE, *tail)
    elif kind == 'momentum':
        L.call('tg_momentum_clip_f32' if clip else 'tg_momentum_f32', p, g, slots[0], n, ptr(lr), h['momentum'], GRAD_SCALE, *tail)
    else:
        L.call('tg_rmsprop_clip_f32' if clip else 'tg_rmsprop_f32', p, g, slots[0], slots[1], n, ptr(lr), h['decay'], 0.0, h['eps_rms'], GRAD_SCALE, *tail)


def at(t, o):
    """pointer to element o of a float tensor the caller keeps alive"""
    return C.c_void_p(t.data_ptr() + 4 * o)


def run(kind, p0, slots0, grads, clip=False, in_pieces=False):
    """-> {'p': ..., slot: ...} after STEPS steps; whole-buffer launches on guarded buffers, or the same entry point piece by piece"""
    lr, factor = dev([HYPER['lr']]), dev([1.0])
    step = torch.zeros(1, dtype=torch.int32, device='cuda')
    bufs = [guarded(N4, fill=p0)] + [guarded(N4, fill=slots0[s]) for s in SLOTS[kind]]
    for t, g in enumerate(grads, 1):
        gd = dev(g / np.float32(GRAD_SCALE))                                # exact for 0.5
        if in_pieces:
            for o, m in pieces(N4):
                step.fill_(t - 1)
                launch(kind, clip, at(bufs[0].t, o), [at(b.t, o) for b in bufs[1:]], at(gd, o), m, lr, step, factor)
        else:
            launch(kind, clip, bufs[0].ptr, [b.ptr for b in bufs[1:]], ptr(gd), N4, lr, step, factor)
        torch.cuda.synchronize()
        assert gd.cpu().numpy().tobytes() == (g / np.float32(GRAD_SCALE)).tobytes(), "the gradient was written"
    if kind == 'adam':
        assert int(step.item()) == STEPS
    return dict(zip(('p',) + SLOTS[kind], [finish(b) for b in bufs]))


def reference(kind, p0, slots0, grads):
    h = HYPER
    p = f8(p0)
    s = {k: f8(v) for k, v in slots0.items()}
    max_update = 0.0
    for t, g in enumerate(grads, 1):
        if kind == 'adam':
            q, s['m'], s['v'] = T.adam_update(p, f8(g), s['m'], s['v'], t, h['lr'], h['beta1'], h['beta2'], h['eps_adam'])
        elif kind == 'momentum':
            q, s['accum'] = R.momentum_step(p, g, s['accum'], h['lr'], h['momentum'])
        else:
            q, s['rms'], s['mom'] = R.rmsprop_step(p, g, s['rms'], s['mom'], h['lr'], h['decay'], 0.0, h['eps_rms'])
        max_update, p = max(max_update, np.abs(q - p).max()), q
    return dict(s, p=p, max_update=max_update, max_p=np.abs(p).max())


@pytest.mark.parametrize("kind", ['adam', 'momentum', 'rmsprop'])
def test_update_kernels_at_the_wrap(kind):
    assert N4 // 4 > CAP and N4 % 4 == 3 and all(o % 4 == 0 and m <= PIECE and m // 4 + 1 <= CAP for o, m in pieces(N4))
    p0, slots0, grads = case(kind)
    got = run(kind, p0, slots0, grads)
    ref = reference(kind, p0, slots0, grads)
    miss = np.abs(f8(got['p']) - ref['p']).max() / R.param_bound(ref, STEPS)
    slot = {s: R.slots_close(got[s], ref[s]) for s in SLOTS[kind]}
    print('%s: parameter error / bound %.3f, slot error / bound %s' % (kind, miss, slot))
    assert miss <= 1.0 and all(v <= 1.0 for v in slot.values())
    assert ref['max_update'] > 0 and (got['p'] != p0).mean() > 0.7                      # the buffer moved (every 11th gradient is zero, every 7th tiny)
    split = run(kind, p0, slots0, grads, in_pieces=True)
    for k in got:
        assert_bits(split[k], got[k], "%s: %s of the whole buffer vs piece by piece" % (kind, k))
    clipped = run(kind, p0, slots0, grads, clip=True)
    for k in got:
        assert_bits(clipped[k], got[k], "%s: %s of the _clip form with factor 1" % (kind, k))


def test_ema_at_the_wrap():
    L = lib()
    assert N1 > CAP and [m for _, m in pieces(N1)] == [PIECE, 37]
    rng = np.random.default_rng(24)
    decay = R.f32(0.9999)
    s0 = rng.standard_normal(N1).astype(np.float32)
    ps = [(s0 + rng.standard_normal(N1) * (0.1 if t else 1.0)).astype(np.float32) for t in range(STEPS)]
    whole, split = guarded(N1, fill=s0), guarded(N1, fill=s0)
    ref = f8(s0)
    for p in ps:
        pd = dev(p)
        L.call('tg_ema_f32', whole.ptr, ptr(pd), N1, decay, st())
        for o, m in pieces(N1):
            L.call('tg_ema_f32', at(split.t, o), at(pd, o), m, decay, st())
        torch.cuda.synchronize()
        ref = T.ema_update(ref, f8(p), decay)
    got = finish(whole)
    assert (np.abs(f8(got) - ref) <= 1e-6 * np.abs(ref) + 1e-7).all()
    assert (got != s0).mean() > 0.9
    assert_bits(finish(split), got, "ema: the whole buffer vs piece by piece")
