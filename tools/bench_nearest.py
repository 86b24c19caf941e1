#!/usr/bin/env python3
"""Time the nearest-training-image search at the size of the CIFAR training split, 50 000 images of 3 072 bytes:

  1. decode + copy     every record of a TFRecord split decoded into pinned staging and copied to the device
                       (tg.metrics.PixelBank.add_records over Input_Pipeline.tfrecordDataset.training_chunks) — what a trainer pays once;
  2. the kernel        tg_nearest_u8_i32 (both launches) at m in {64, 1 000, 10 000} queries against the resident split, k = 3: median of
                       the timed repetitions, with the achieved int8 TOP/s (2 m n d operations) against the MFMA peak and two byte
                       rates against HBM — the bytes the workgroups request (every query tile reads the whole split) and the least any
                       schedule must move (both sets once);
  3. the host          the same answer from NumPy (float64 matrix products, exact at these magnitudes, then a lexsort of the best
                       candidates), compared with the kernel's for equality.

    python tools/bench_nearest.py [--n 50000] [--d 3072] [--k 3] [--m 64 1000 10000] [--host-m 64 1000] [--reps 10] [--dir DIR]

The split is random bytes written with tg.io.write_tfrecord under --dir (default: a temporary directory, removed afterwards).  Prints a
table; the first run's output is profiles/nearest_training.txt."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tensorflow-implementation-of-triple-gan_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_I8_TOPS = 5000.0        # v_mfma_i32_32x32x32_i8: twice the dense bf16 rate of about 2.5 PFLOP/s
PEAK_HBM_GBS = 8000.0        # HBM3E, specified (a float4 copy reaches about 6 300)


def write_split(root, n, shape, n_lab, seed=0):
    """CIFAR-10-named training TFRecords of random bytes under root/Tfrecord -> the training Dataset."""
    from tg import io as tgio
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    os.makedirs(os.path.join(root, 'Tfrecord'), exist_ok=True)
    rng = np.random.default_rng(seed)
    ds = cifar10Dataset(root, None, n_lab, 'train')
    for name, count in zip(ds.get_filenames(), (n_lab, n - n_lab)):
        for s in range(0, count, 10000):
            c = min(10000, count - s)
            tgio.write_tfrecord(name, rng.integers(0, 256, (c,) + shape, dtype=np.uint8), rng.integers(0, 10, c), append=s > 0)
    return ds


def host_nearest(q, r, k, block=8192):
    """the k best (d2, index) pairs of every row of q over the rows of r on the host: d2 = |q|^2 + |r|^2 - 2 q.r in float64 (every
    value is an integer below 2^53: exact), the k + ties smallest of every block kept, one lexsort at the end."""
    qf = q.astype(np.float64)
    qn = (qf * qf).sum(axis=1)
    best_d, best_i = [], []
    for s in range(0, r.shape[0], block):
        rf = r[s:s + block].astype(np.float64)
        d2 = qn[:, None] + (rf * rf).sum(axis=1)[None, :] - 2.0 * (qf @ rf.T)
        kk = min(k, d2.shape[1])
        kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1:kk]
        for i in range(q.shape[0]):
            j = np.nonzero(d2[i] <= kth[i])[0]
            best_d.append((i, d2[i, j], j + s))
    out_d = np.full((q.shape[0], k), 2 ** 31 - 1, np.int64)
    out_i = np.full((q.shape[0], k), -1, np.int64)
    rows = [[] for _ in range(q.shape[0])]
    for i, dv, jv in best_d:
        rows[i].append((dv, jv))
    for i, parts in enumerate(rows):
        dv, jv = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        order = np.lexsort((jv, dv))[:k]
        out_d[i, :len(order)], out_i[i, :len(order)] = dv[order].astype(np.int64), jv[order]
    return out_d.astype(np.int32), out_i.astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--n', type=int, default=50000)
    ap.add_argument('--d', type=int, default=3072, help='bytes per image: 3 h w with h = w (3072: CIFAR)')
    ap.add_argument('--k', type=int, default=3)
    ap.add_argument('--m', type=int, nargs='+', default=[64, 1000, 10000])
    ap.add_argument('--host-m', type=int, nargs='*', default=[64, 1000], help='the m at which NumPy computes the same answer')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dir', help='where the TFRecords are written (default: a temporary directory)')
    a = ap.parse_args()
    import torch
    from tg import lib, metrics as tgm
    from tg.runtime import Context, set_context
    from Input_Pipeline.tfrecordDataset import training_chunks
    side = int(round((a.d // 3) ** 0.5))
    assert 3 * side * side == a.d, "--d must be 3 h w with h = w"
    cx = set_context(Context('cuda:0'))
    root = a.dir or tempfile.mkdtemp(prefix='bench_nearest_')
    try:
        t0 = time.perf_counter()
        ds = write_split(root, a.n, (side, side, 3), min(4000, a.n // 2))
        print("split: %d images of %d bytes (%.1f MB), written in %.1f s" % (a.n, a.d, a.n * a.d / 1e6, time.perf_counter() - t0))
        for attempt in ('cold', 'warm'):                               # cold: first touch of the files and of the pinned allocation
            bank = tgm.PixelBank(a.d, cx.device)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bank.add_records(training_chunks(ds))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("decode + copy (%s): %.3f s  %.0f images/s  %.2f GB/s" % (attempt, dt, bank.n / dt, bank.n * a.d / dt / 1e9))
        assert bank.n == a.n
        r_host = bank.numpy()
    finally:
        if not a.dir:
            shutil.rmtree(root, ignore_errors=True)
    rng = np.random.default_rng(1)
    print("kernel: n %d, d %d, k %d, %d timed repetitions after 2 warm-up calls; peaks %.0f int8 TOP/s, %.0f GB/s"
          % (a.n, a.d, a.k, a.reps, PEAK_I8_TOPS, PEAK_HBM_GBS))
    print("%7s %7s %10s %10s %10s %9s %7s %12s %7s %12s" % ('m', 'ranges', 'median ms', 'min ms', 'max ms', 'TOP/s', '% peak', 'req. GB/s',
                                                            '% HBM', 'least GB/s'))
    for m in a.m:
        q_host = rng.integers(0, 256, (m, a.d), dtype=np.uint8)
        q_host[0] = r_host[a.n // 2]                                   # one query that is a training image
        q = tgm.PixelBank(a.d, cx.device).add_u8(q_host)
        times = []
        for rep in range(a.reps + 2):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            d2, idx = tgm.nearest_pixels(q, bank, a.k, cx.stream)
            stop.record()
            stop.synchronize()
            if rep >= 2:
                times.append(start.elapsed_time(stop))
        med = float(np.median(times))
        ops = 2.0 * m * a.n * a.d
        tiles = -(-m // 64)
        requested, least = float(tiles) * a.n * a.d + float(m) * a.d * -(-a.n // 64), float(a.n + m) * a.d
        tops, req = ops / (med * 1e-3) / 1e12, requested / (med * 1e-3) / 1e9
        print("%7d %7d %10.3f %10.3f %10.3f %9.1f %6.1f%% %12.0f %6.1f%% %12.0f" % (
            m, lib.call('tg_nearest_u8_ranges', m, a.n), med, min(times), max(times), tops, 100.0 * tops / PEAK_I8_TOPS, req,
            100.0 * req / PEAK_HBM_GBS, least / (med * 1e-3) / 1e9))
        got = d2.cpu().numpy(), idx.cpu().numpy()
        assert got[0][0, 0] == 0 and got[1][0, 0] == a.n // 2
        if m in a.host_m:
            t0 = time.perf_counter()
            want = host_nearest(q_host, r_host, a.k)
            dt = time.perf_counter() - t0
            same = bool((got[0] == want[0]).all() and (got[1] == want[1]).all())
            print("        host (NumPy float64, %d threads): %.2f s = %.0f x the kernel's median; same answer: %s"
                  % (torch.get_num_threads(), dt, dt / (med * 1e-3), same))
            assert same


if __name__ == '__main__':
    main()
