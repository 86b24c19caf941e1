#!/usr/bin/env python3
"""Wall time of the generated-sample metrics on an MI355X, two things:

  1. tg_feature_moments_f32 at n = 10 000, c = 128 (the classifier's pooled feature over a validation split) beside its host route —
     copy the [n, c] fp32 matrix to the host and form the sums and the Gram matrix in NumPy float64.  Device: HIP events around
     --repeats calls after a warm-up call, median; host route: the host clock around copy + NumPy, median.
  2. Train.sample_metrics on the CIFAR-10 configuration at the experiment's batch sizes (tools/bench_config.py, synthetic ZCA) with
     --val validation images and --samples generated samples, beside a plain Train.evaluate of the same split — both after one
     untimed pass (buffers, lazily loaded code objects), host clock around the call (each ends in a device->host copy), median of
     --repeats; raw weights and the EMA shadows.

Epoch-tail work, stated for the record: no threshold.  Prints a text report and writes it to --out.

    python tools/bench_sample_metrics.py [--repeats 5] [--val 10000] [--samples 10000] [--out profiles/sample_metrics.txt]"""
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


def spread(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return "median %.3f ms, min %.3f, max %.3f (%d runs)" % (np.median(a), a[0], a[-1], a.size)


def bench_pass(n_val, n_samples, repeats):
    import torch
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
    a = ap.parse_args()
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
