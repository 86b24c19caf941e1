#!/usr/bin/env python3
"""The three optimiser launches alone (csrc/optim.hip; config.OPTIMIZER) on flat buffers the size of the CIFAR-10 networks'
parameter stores: tg_adam_f32 (28 B / parameter), tg_momentum_f32 (20 B), tg_rmsprop_f32 (28 B), each beside its clipped twin
tg_*_clip_f32 (config.CLIP_NORM, DESIGN §9.6: one more scalar load and one more multiply), and tg_grad_norm_clip_f32 alone (4 B / parameter
read; two launches).  All are timed alternately, --rounds times each, in one process; prints per network and kernel the fastest and the median round in us per launch, and the
algorithmic bytes over the fastest time in TB/s (HBM peak 8 TB/s)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-implementation-of-triple-gan_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tg import geom, lib  # noqa: E402
from Model.Good_GAN_cifar10 import Good_GAN_cifar10  # noqa: E402

BYTES = {'adam': 28.0, 'momentum': 20.0, 'rmsprop': 28.0, 'grad_norm': 4.0}


def store_sizes():
    """floats of each network's flat trainable buffer (ParamStore.n_p: every variable padded to 32 floats)."""
    return {net: sum(geom.pad32(int(np.prod(shape))) for _n, shape, trainable, _i in specs if trainable)
            for net, specs in Good_GAN_cifar10.param_specs().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=2000, help='launches per timed window')
    args = ap.parse_args()
    lib.load()
    st = lib.cur_stream()
    lr = torch.full((1,), 3e-4, device='cuda')
    step = torch.zeros(1, dtype=torch.int32, device='cuda')
    for net, n in store_sizes().items():
        p, g = torch.randn(n, device='cuda') * 0.05, torch.randn(n, device='cuda') * 1e-2
        m, v = torch.zeros(n, device='cuda'), torch.ones(n, device='cuda')
        P = lib.ptr
        need = lib.call('tg_grad_norm_workspace_bytes', n)
        ws, out2, thr = torch.zeros(need // 4, device='cuda'), torch.zeros(2, device='cuda'), torch.full((1,), 1.0, device='cuda')
        fac = out2[1:2]
        calls = {'adam': lambda: lib.call('tg_adam_f32', P(p), P(g), P(m), P(v), n, P(lr), 0.5, 0.999, 1e-8, P(step), 1.0, st),
                 'momentum': lambda: lib.call('tg_momentum_f32', P(p), P(g), P(m), n, P(lr), 0.9, 1.0, st),
                 'rmsprop': lambda: lib.call('tg_rmsprop_f32', P(p), P(g), P(v), P(m), n, P(lr), 0.9, 0.0, 1e-10, 1.0, st),
                 'grad_norm': lambda: lib.call('tg_grad_norm_clip_f32', P(g), n, 1.0, P(thr), P(out2), P(ws), need, st),
                 'adam_clip': lambda: lib.call('tg_adam_clip_f32', P(p), P(g), P(m), P(v), n, P(lr), 0.5, 0.999, 1e-8, P(step), 1.0, P(fac), st),
                 'momentum_clip': lambda: lib.call('tg_momentum_clip_f32', P(p), P(g), P(m), n, P(lr), 0.9, 1.0, P(fac), st),
                 'rmsprop_clip': lambda: lib.call('tg_rmsprop_clip_f32', P(p), P(g), P(v), P(m), n, P(lr), 0.9, 0.0, 1e-10, 1.0, P(fac), st)}
        times = {k: [] for k in calls}
        for fn in calls.values():
            for _ in range(50):
                fn()
        for _ in range(args.rounds):
            for k, fn in calls.items():
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    fn()
                b.record()
                torch.cuda.synchronize()
                times[k].append(a.elapsed_time(b) / args.iters * 1e3)
        for k, t in times.items():
            best = min(t)
            bpp = BYTES[k.replace('_clip', '')]
            print("%-14s %8d floats  %-13s fastest %7.2f us  median %7.2f us  %5.2f TB/s algorithmic (%.0f B/parameter)%s"
                  % (net, n, k, best, float(np.median(t)), bpp * n / best / 1e6, bpp,
                     "  [with its step-count launch]" if k.startswith('adam') else
                     "  [two launches]" if k == 'grad_norm' else ""), flush=True)


if __name__ == "__main__":
    main()
