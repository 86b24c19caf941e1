#!/usr/bin/env python3
"""Measure the histogram summaries (config.SUMMARY_HISTOGRAM) on an MI355X at the CIFAR-10 stores' real segment tables,
after a few training iterations (so values and gradients are a run's, not the initialiser's):

  device route   tg_tf_histogram_f32 over store.p and store.g of the three networks (six launch sequences), timed with device events,
                 after warm-up, --repeats times: median / min / max
  host route     one device->host copy of the same six buffers + TensorFlow's binning in NumPy (searchsorted over the 1 551 limits,
                 bincount, min / max / sums) per variable, host clock, --host-repeats times
  epoch tail     the wall time Train.histograms('value') + Train.histograms('grad') add (launches, six result copies, dictionaries),
                 host clock around calls that end in a device synchronise

Both routes are checked to give the same counts before anything is timed.  Prints a text report (and writes it to --out).

    python tools/bench_summary.py [--repeats 30] [--host-repeats 5] [--out profiles/summary_histogram.txt]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
from bench_config import make_config  # noqa: E402  (puts the package on sys.path)

NETS = ('discriminator', 'good_generator', 'classifier')


def host_histograms(buf, segments, limits):
    """the host route on one flat buffer (a host array): per segment TensorFlow's counts and statistics in NumPy."""
    out = []
    for off, n in segments:
        x = buf[off:off + n]
        v = x[np.isfinite(x)].astype(np.float64)
        counts = np.bincount(np.searchsorted(limits, v, side='right'), minlength=limits.size)
        out.append((counts, v.min() if v.size else 0.0, v.max() if v.size else 0.0, v.size, v.sum(), np.dot(v, v)))
    return out


def spread(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return "median %.3f ms, min %.3f, max %.3f (%d runs)" % (np.median(a), a[0], a[-1], a.size)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--host-repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=4, help='training iterations before measuring')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from tg import summary as tgsum
    from Training.Train_goodGAN import Train
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10 as Model
    cfg = make_config('cifar10')
    cfg.EXEC_MODE = 'plan'
    q, _ = np.linalg.qr(np.random.default_rng(4321).standard_normal((3072, 3072)))
    cfg.ZCA = (np.zeros(3072, np.float32), q.astype(np.float32))
    tr = Train(cfg, None, None)
    tr._build_train_graph(Model)
    tr.set_hyper(lambda_1=cfg.FAKE_G_LAMBDA, lambda_2=0.5)
    rng = np.random.default_rng(1234)
    img = lambda n: rng.uniform(-1, 1, (n, 32, 32, 3)).astype(np.float32)
    oh = lambda n: np.eye(10, dtype=np.float32)[rng.integers(0, 10, n)]
    tr.feed(dict(x_l_c=img(cfg.BATCH_SIZE_L_C), y_l_c=oh(cfg.BATCH_SIZE_L_C), x_l_d=img(cfg.BATCH_SIZE_L_D), y_l_d=oh(cfg.BATCH_SIZE_L_D),
                 x_u_d=img(cfg.BATCH_SIZE_U_D), x_u_c=img(cfg.BATCH_SIZE_U_C)))
    for _ in range(args.iters):
        tr.sample_latent()
        tr.train_iteration()
    torch.cuda.synchronize()
    limits = np.array(tgsum.limits())
    stores = [tr.cx.stores[n] for n in NETS]
    tables = [[st.index[nm][1:3] for nm in st.names(True)] for st in stores]
    runs = [tgsum.StoreHistograms(t, tr.cx.device) for t in tables]
    elements = sum(n for t in tables for _, n in t)
    L = []
    say = lambda s: (L.append(s), print(s, flush=True))
    try:
        commit = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = 'unknown (not a git checkout)'
    say("command: python tools/bench_summary.py --repeats %d --host-repeats %d --iters %d" % (args.repeats, args.host_repeats, args.iters))
    say("commit: %s   device: %s   torch %s" % (commit, torch.cuda.get_device_name(0), torch.__version__))
    say("CIFAR-10 stores after %d iterations: %d trainable variables, %d elements per buffer set (%s), p and g binned = %d elements, %.1f MB read"
        % (args.iters, sum(len(t) for t in tables), elements, ' / '.join('%s %d vars %d' % (n[:4], len(t), sum(c for _, c in t)) for n, t in zip(NETS, tables)),
           2 * elements, 2 * elements * 4 / 1e6))

    # both routes agree before anything is timed
    for st, t, run in zip(stores, tables, runs):
        for buf in (st.p, st.g):
            counts, stats = run.run(buf, tr.cx.stream)
            ref = host_histograms(buf.detach().cpu().numpy(), t, limits)
            for k, (c, mn, mx, num, _s, _q) in enumerate(ref):
                assert (counts[k] == c).all() and stats[k][2] == num and (num == 0 or (stats[k][0] == mn and stats[k][1] == mx)), (st.name, k)
    say("device and host routes agree on every count, min, max and num")

    def device_once():
        for st, run in zip(stores, runs):
            run.launch(st.p, tr.cx.stream)
            run.launch(st.g, tr.cx.stream)            # (the result buffer is reused: this run measures, it does not fetch)

    for _ in range(3):
        device_once()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        device_once()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    say("device route (6 launch sequences, device events; includes the host-built chunk maps' copies): %s" % spread(ms))
    say("  = %.1f GB/s of parameters read at the median" % (2 * elements * 4 / 1e9 / (np.median(ms) / 1e3)))

    copy_ms, bin_ms = [], []
    for _ in range(args.host_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = [(st.p.detach().cpu().numpy(), st.g.detach().cpu().numpy()) for st in stores]
        t1 = time.perf_counter()
        for (p, g), t in zip(host, tables):
            host_histograms(p, t, limits)
            host_histograms(g, t, limits)
        t2 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        bin_ms.append((t2 - t1) * 1e3)
    say("host route, device->host copy of the 6 buffers: %s" % spread(copy_ms))
    say("host route, NumPy binning (%d threads visible to NumPy's BLAS; searchsorted / bincount are single-threaded): %s"
        % (os.cpu_count() or 0, spread(bin_ms)))
    say("host route, total: %s" % spread([c + b for c, b in zip(copy_ms, bin_ms)]))

    tail = []
    for _ in range(3):
        tr.histograms('value'), tr.histograms('grad')
    for _ in range(max(args.host_repeats, 10)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = tr.histograms('value')
        h.update(('gradients/' + k, v) for k, v in tr.histograms('grad').items())
        tail.append((time.perf_counter() - t0) * 1e3)
    say("epoch tail, Train.histograms('value') + ('grad') wall time (6 launch sequences, 6 result copies, %d dictionaries): %s" % (len(h), spread(tail)))
    from Training.Summary import encode_event
    t0 = time.perf_counter()
    ev = encode_event(0.0, step=1, histograms=h)
    say("epoch tail, compressing and encoding the %d histograms into one Event of %d bytes (host): %.1f ms" % (len(h), len(ev), (time.perf_counter() - t0) * 1e3))
    ratio = np.median([c + b for c, b in zip(copy_ms, bin_ms)]) / np.median(ms)
    say("host route / device route at the medians: %.0fx" % ratio)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write("\n".join(L) + "\n")


if __name__ == '__main__':
    main()
