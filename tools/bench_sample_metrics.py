#!/usr/bin/env python3
"""Wall time of the generated-sample metrics on an MI355X, two things:

  1. tg_feature_moments_f32 at n = 10 000, c = 128 (the classifier's pooled feature over a validation split) beside its host route —
     copy the [n, c] fp32 matrix to the host and form the sums and the Gram matrix in NumPy float64.  Device: HIP events around
     --repeats calls after a warm-up call, median; host route: the host clock around copy + NumPy, median.
  2. Train.sample_metrics on the CIFAR-10 configuration at the experiment's batch sizes (tools/bench_config.py, synthetic ZCA) with
     --val validation images and --samples generated samples, beside a plain Train.evaluate of the same split — both after one
     untimed pass (buffers, lazily loaded code objects), host clock around the call (each ends in a device->host copy), median of
     --repeats; raw weights and the EMA shadows.

And for the k-nearest-neighbour manifold metrics (--section manifold, report to --manifold-out):

  3. tg_knn_self_f32 and tg_manifold_query_f32 at n = m = 10 000, c = 128, k = --manifold-k (HIP events, median), each with the
     fraction of the fp32 vector peak its time corresponds to (3 operations per channel per pair), beside a host route for the same
     four numbers: blocked NumPy float64 distances (|a|^2 + |b|^2 - 2ab per block of 1 000 rows), two radius sweeps and two query
     sweeps; the four numbers of both routes are printed.
  4. Train.sample_metrics and Train.sample_manifold_metrics on the configuration of 2.

Epoch-tail work, stated for the record: no threshold.  Prints a text report and writes it to --out / --manifold-out.

    python tools/bench_sample_metrics.py [--repeats 5] [--val 10000] [--samples 10000] [--out profiles/sample_metrics.txt]
                                         [--section all|moments|manifold] [--manifold-k 3] [--manifold-out profiles/manifold_metrics.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
from bench_config import make_config  # noqa: E402  (puts the package on sys.path)


def bench_kernel(n, c, repeats):
    import torch
    from tg import lib
    rng = np.random.default_rng(0)
    f = torch.from_numpy((rng.standard_normal((n, c)) + 0.5).astype(np.float32)).cuda()
    acc = torch.zeros(c + c * c, dtype=torch.float64, device='cuda')
    need = lib.call('tg_feature_moments_workspace_bytes', n, c)
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device='cuda')
    call = lambda: lib.call('tg_feature_moments_f32', lib.ptr(f), c, n, c, lib.ptr(acc[:c]), lib.ptr(acc[c:]), lib.ptr(ws), need, lib.cur_stream())
    call()
    torch.cuda.synchronize()
    dev = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream())
        call()
        e1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        dev.append(e0.elapsed_time(e1))
    host = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = f.cpu().numpy().astype(np.float64)
        s, g = x.sum(axis=0), x.T @ x
        host.append(1e3 * (time.perf_counter() - t0))
    return dev, host[1:], need, (s, g)


PEAK_FP32_VECTOR = 157.3e12         # MI355X vector fp32 peak (FLOP/s, data sheet: counts fused and packed operations)


def device_ms(call, repeats):
    """HIP-event times of `call` on the current stream after one warm-up call."""
    import torch
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream())
        call()
        e1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def host_manifold(real, fake, k, block=1000):
    """the four numbers from float64 distances in NumPy, blocked so that no more than block x n distances exist at a time."""
    real, fake = real.astype(np.float64), fake.astype(np.float64)

    def sweep(q, r, fn, same=False):
        rr = (r * r).sum(axis=1)
        out = []
        for lo in range(0, q.shape[0], block):
            qb = q[lo:lo + block]
            d = np.maximum((qb * qb).sum(axis=1)[:, None] + rr[None, :] - 2.0 * (qb @ r.T), 0.0)
            if same:
                d[np.arange(d.shape[0]), lo + np.arange(d.shape[0])] = np.inf
            out.append(fn(d))
        return np.concatenate(out)

    kth = lambda d: np.partition(d, k - 1, axis=1)[:, k - 1]
    r2_real, r2_fake = sweep(real, real, kth, same=True), sweep(fake, fake, kth, same=True)
    count_fr = sweep(fake, real, lambda d: (d <= r2_real[None, :]).sum(axis=1))
    both = sweep(real, fake, lambda d: np.stack([(d <= r2_fake[None, :]).sum(axis=1), d.min(axis=1)], axis=1))
    count_rf, nn_rf = both[:, 0], both[:, 1]
    return dict(precision=float(np.mean(count_fr > 0)), recall=float(np.mean(count_rf > 0)),
                density=float(count_fr.sum() / (float(k) * fake.shape[0])), coverage=float(np.mean(nn_rf <= r2_real)))


def bench_manifold_kernels(n, c, k, repeats):
    import torch
    from tg import metrics as M
    rng = np.random.default_rng(0)
    real = np.maximum(rng.standard_normal((n, c)) + 0.5, 0.0).astype(np.float32)              # post-ReLU-like: a shared offset, exact zeros
    fake = np.maximum(rng.standard_normal((n, c)) * 0.9 + 0.6, 0.0).astype(np.float32)
    rd, fd = torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda()
    r2 = M.knn_self(rd, k)[:, k - 1].contiguous()
    t_self = device_ms(lambda: M.knn_self(rd, k), repeats)
    t_query = device_ms(lambda: M.manifold_query(fd, rd, r2), repeats)
    banks = []
    for x in (rd, fd):
        b = M.FeatureBank(c, x.device)
        b.buf, b.n = x.reshape(-1), n
        banks.append(b)
    torch.cuda.synchronize()
    t_all, t_host = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        dev = M.manifold_metrics(banks[0], banks[1], k)
        t_all.append(1e3 * (time.perf_counter() - t0))
    for _ in range(max(1, min(repeats, 2))):
        t0 = time.perf_counter()
        x, y = rd.cpu().numpy(), fd.cpu().numpy()
        host = host_manifold(x, y, k)
        t_host.append(1e3 * (time.perf_counter() - t0))
    return t_self, t_query, t_all, t_host, dev, host


def bench_manifold_pass(n_val, n_samples, k, repeats):
    import torch
    tr, val = _cifar_trainer(n_val)
    out = {}
    for name, fn in (('sample_metrics', lambda: tr.sample_metrics(val, n_samples)),
                     ('sample_manifold_metrics(k=%d)' % k, lambda: tr.sample_manifold_metrics(val, n_samples, k))):
        fn()
        ms = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        out[name] = (ms, res)
    return out, len(val) * tr.config.BATCH_SIZE


def manifold_report(a):
    import torch
    n, c, k = 10000, 128, a.manifold_k
    L = ["k-nearest-neighbour manifold metrics (DESIGN 9.11) on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), ""]
    t_self, t_query, t_all, t_host, dev, host = bench_manifold_kernels(n, c, k, a.repeats)
    ops = 3.0 * n * n * c
    frac = lambda ms: 100.0 * ops / (1e-3 * np.median(ms)) / PEAK_FP32_VECTOR
    L.append("3. n = m = %d rows of c = %d, k = %d: %.1f G fp32 operations per sweep (3 per channel per pair)" % (n, c, k, 1e-9 * ops))
    L.append("   tg_knn_self_f32 (device events)               %s = %.1f %% of the %.1f TFLOP/s fp32 vector peak" % (
        spread(t_self), frac(t_self), 1e-12 * PEAK_FP32_VECTOR))
    L.append("   tg_manifold_query_f32 (device events)         %s = %.1f %% of that peak" % (spread(t_query), frac(t_query)))
    L.append("   manifold_metrics: 2 + 2 launches, D2H (host)  %s" % spread(t_all))
    L.append("   D2H + blocked NumPy float64, 4 sweeps (host)   %s" % spread(t_host))
    L.append("   device %r" % (dev,))
    L.append("   host   %r   (float64 Gram-form distances: a pair on a ball's edge may fall on the other side)" % (host,))
    L.append("")
    res, n_val = bench_manifold_pass(a.val, a.samples, k, a.repeats)
    L.append("4. CIFAR-10 configuration, %d validation images in batches of 100, %d generated samples (host clock, one untimed pass first)" % (n_val, a.samples))
    for name, (ms, r) in res.items():
        L.append("   %-30s %s" % (name, spread(ms)))
    L.append("   an untrained model: the values below only show the pass ran")
    L.append("   %r" % (list(res.values())[-1][1],))
    text = "\n".join(L) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.manifold_out), exist_ok=True)
    open(a.manifold_out, 'w').write(text)


def spread(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return "median %.3f ms, min %.3f, max %.3f (%d runs)" % (np.median(a), a[0], a[-1], a.size)


def _cifar_trainer(n_val):
    """(trainer, validation batches) of the CIFAR-10 configuration at the experiment's batch sizes, untrained."""
    from tg import runtime
    from Training.Train_goodGAN import Train
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10
    cfg = make_config('cifar10')
    q, _ = np.linalg.qr(np.random.default_rng(4321).standard_normal((3072, 3072)))
    cfg.ZCA = (np.zeros(3072, np.float32), q.astype(np.float32))
    runtime.set_context(None)
    tr = Train(cfg, None, None)
    tr._build_train_graph(Good_GAN_cifar10)
    rng = np.random.default_rng(1)
    bs = cfg.BATCH_SIZE
    val = [(rng.uniform(-1, 1, (bs, 32, 32, 3)).astype(np.float32), np.eye(10, dtype=np.float32)[rng.integers(0, 10, bs)])
           for _ in range(max(1, n_val // bs))]
    return tr, val


def bench_pass(n_val, n_samples, repeats):
    import torch
    tr, val = _cifar_trainer(n_val)
    bs = tr.config.BATCH_SIZE
    out = {}
    for name, fn in (('evaluate', lambda: tr.evaluate(val)), ('evaluate(ema=True)', lambda: tr.evaluate(val, ema=True)),
                     ('sample_metrics', lambda: tr.sample_metrics(val, n_samples)),
                     ('sample_metrics(ema=True)', lambda: tr.sample_metrics(val, n_samples, ema=True))):
        fn()
        ms = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        out[name] = (ms, res)
    return out, len(val) * bs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--val', type=int, default=10000)
    ap.add_argument('--samples', type=int, default=10000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sample_metrics.txt'))
    ap.add_argument('--section', choices=('all', 'moments', 'manifold'), default='all')
    ap.add_argument('--manifold-k', type=int, default=3)
    ap.add_argument('--manifold-out', default=os.path.join(ROOT, 'profiles', 'manifold_metrics.txt'))
    a = ap.parse_args()
    if a.section in ('all', 'manifold'):
        manifold_report(a)
    if a.section == 'manifold':
        return
    import torch
    n, c = 10000, 128
    L = ["generated-sample metrics (DESIGN 9.10) on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), ""]
    dev, host, need, _ = bench_kernel(n, c, a.repeats)
    L.append("1. moments of an fp32 [%d, %d] feature matrix in fp64 (%.2f GFLOP, %.1f MB read, workspace %.1f MB)" % (
        n, c, 2e-9 * n * c * c, 4e-6 * n * c, 1e-6 * need))
    L.append("   tg_feature_moments_f32 (device events)        %s" % spread(dev))
    L.append("   D2H copy + NumPy float64 sums and x^T x (host) %s" % spread(host))
    L.append("")
    res, n_val = bench_pass(a.val, a.samples, a.repeats)
    L.append("2. CIFAR-10 configuration, %d validation images in batches of 100, %d generated samples (host clock, one untimed pass first)" % (n_val, a.samples))
    for name, (ms, r) in res.items():
        L.append("   %-26s %s" % (name, spread(ms)))
    base = np.median(res['evaluate'][0])
    L.append("   sample_metrics / evaluate = %.2f (raw), %.2f (shadows); an untrained model: the values below only show the pass ran" % (
        np.median(res['sample_metrics'][0]) / base, np.median(res['sample_metrics(ema=True)'][0]) / base))
    L.append("   %r" % (res['sample_metrics'][1],))
    text = "\n".join(L) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
