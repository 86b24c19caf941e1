#!/usr/bin/env python3
"""Time the kernel-distance sums (tg_poly3_sums_f32) at the epoch tail's own shape: 10 000 real x 10 000 generated rows of the
CIFAR classifier's pooled feature (c = 128).

  1. whole set   the three one-segment calls of tg.metrics.kernel_distance — real x real and fake x fake without their diagonals,
                 real x fake — each timed alone (map copy, main launch, finishing launch): median of the timed repetitions, the achieved
                 fp64 FLOP/s at 2 c per pair, and the bytes of workspace;
  2. per class   the same three calls over 10 class segments of the rows gathered into class order;
  3. torch       ((a.double() @ b.double().T) / c + 1).pow(3).sum() on the same device, the straightforward alternative: it writes the
                 n x n fp64 matrix (800 MB at this shape, and once more for every elementwise step), its sum is not the kernel's bits, and
                 it goes through the vendor BLAS the package otherwise does not call.

    python tools/bench_kernel_distance.py [--n 10000] [--m 10000] [--c 128] [--classes 10] [--reps 10]

No fraction of a peak is printed: the fp64 MFMA's issue rate is not measured here.  Prints a table; the first run's output is
profiles/kernel_distance.txt."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tensorflow-implementation-of-triple-gan_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def features(rng, rows, c):
    return (np.maximum(0.7 * rng.standard_normal((rows, c)) + 0.4, 0.0) + 0.2 * rng.standard_normal((rows, c))).astype(np.float32)


def timed(fn, reps):
    """(median, min, max) ms of fn() over `reps` repetitions after 2 warm-up calls, by device events around the call."""
    import torch
    times = []
    for rep in range(reps + 2):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        if rep >= 2:
            times.append(start.elapsed_time(stop))
    return float(np.median(times)), min(times), max(times), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--m', type=int, default=10000, help='real rows')
    ap.add_argument('--n', type=int, default=10000, help='generated rows')
    ap.add_argument('--c', type=int, default=128, help="feature width (128: the CIFAR classifier's pooled feature)")
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    import ctypes as C
    import torch
    from tg import lib, metrics as tgm
    rng = np.random.default_rng(0)
    real_h, fake_h = features(rng, a.m, a.c), features(rng, a.n, a.c)
    lab_r, lab_f = rng.integers(0, a.classes, a.m), np.arange(a.n) % a.classes
    real, fake = torch.from_numpy(real_h).cuda(), torch.from_numpy(fake_h).cuda()
    (ord_r, off_r), (ord_f, off_f) = tgm.class_order(lab_r, a.classes), tgm.class_order(lab_f, a.classes)
    real_s, fake_s = real.index_select(0, torch.from_numpy(ord_r).cuda()), fake.index_select(0, torch.from_numpy(ord_f).cuda())
    whole_r, whole_f = np.array([0, a.m]), np.array([0, a.n])
    print("kernel-distance sums: %d real x %d generated rows, c %d, %d classes; %d timed repetitions after 2 warm-up calls"
          % (a.m, a.n, a.c, a.classes, a.reps))
    print("%-36s %9s %10s %10s %10s %12s %14s" % ('call', 'segments', 'median ms', 'min ms', 'max ms', 'fp64 TFLOP/s', 'workspace B'))
    sums, totals = {}, {}
    for group, (r, f, sr, sf) in (('whole', (real, fake, whole_r, whole_f)), ('per class', (real_s, fake_s, off_r, off_f))):
        total = 0.0
        for name, x, y, sx, sy, diag in (('real x real, no diagonal', r, r, sr, sr, True), ('fake x fake, no diagonal', f, f, sf, sf, True),
                                         ('real x fake', r, f, sr, sf, False)):
            nseg = len(sx) - 1
            need = lib.call('tg_poly3_sums_workspace_bytes', (C.c_int32 * (nseg + 1))(*sx.tolist()), (C.c_int32 * (nseg + 1))(*sy.tolist()), nseg)
            med, lo, hi, out = timed(lambda: tgm.poly3_sums(x, y, sx, sy, diag), a.reps)
            pairs = float((np.diff(sx) * np.diff(sy)).sum())
            print("%-36s %9d %10.3f %10.3f %10.3f %12.2f %14d" % ('%s: %s' % (group, name), nseg, med, lo, hi,
                                                                  2.0 * a.c * pairs / (med * 1e-3) / 1e12, need))
            sums[(group, name)] = out
            total += med
        totals[group] = total
        print("%-36s %9s %10.3f" % (group + ': the three calls', '', total))
    m_c, n_c = np.diff(off_r), np.diff(off_f)
    kid = tgm.kid_from_sums(sums[('whole', 'real x real, no diagonal')], sums[('whole', 'fake x fake, no diagonal')], sums[('whole', 'real x fake')],
                            a.m, a.n)
    per = tgm.kid_from_sums(sums[('per class', 'real x real, no diagonal')], sums[('per class', 'fake x fake, no diagonal')],
                            sums[('per class', 'real x fake')], m_c, n_c)
    print("kernel_distance %.6g; per class min %.6g max %.6g" % (kid[0], np.nanmin(per), np.nanmax(per)))
    # a second pass gives the same bits
    again = tgm.poly3_sums(real, fake, whole_r, whole_f, False)
    print("real x fake, repeated: bit-identical %s" % bool(again.tobytes() == sums[('whole', 'real x fake')].tobytes()))

    def torch_route(x, y):
        return (((x.double() @ y.double().T) / float(a.c) + 1.0).pow(3).sum()).item()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    med, lo, hi, val = timed(lambda: torch_route(real, fake), a.reps)
    peak = torch.cuda.max_memory_allocated() - before
    ours = sums[('whole', 'real x fake')][0]
    print("torch fp64 matmul route, real x fake: median %.3f ms (min %.3f, max %.3f), %.2f fp64 TFLOP/s, %.0f MB of temporaries at the peak"
          % (med, lo, hi, 2.0 * a.c * a.m * a.n / (med * 1e-3) / 1e12, peak / 1e6))
    print("    its sum %.17g, the kernel's %.17g (relative difference %.2e)" % (val, ours, abs(val - ours) / abs(ours)))
    whole_xy = timed(lambda: tgm.poly3_sums(real, fake, whole_r, whole_f, False), a.reps)[0]
    print("    the kernel's real x fake call takes %.2f x the torch route's time" % (whole_xy / med))


if __name__ == '__main__':
    main()
