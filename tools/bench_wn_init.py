#!/usr/bin/env python3
"""Wall time of the data-dependent weight-norm initialisation pass (config.WN_INIT = 'data') on an MI355X, per
configuration at the experiments' batch sizes (tools/bench_config.py SHAPES): cifar10, svhn, mnist.

For each configuration --repeats FRESH trainers are built (the pass runs once per training run: there is no warm state to measure), a
synthetic batch is fed, latents are drawn, and Train.data_dependent_init() is bracketed by device events on the launch stream and by
the host clock (the call ends in no synchronisation of its own; the host figure is taken after one).  The first trainer of the process
also pays for lazily loaded code objects, so it is reported apart and left out of the median.  A one-time cost, stated for the record:
no threshold.  Prints a text report (and writes it to --out).

    python tools/bench_wn_init.py [--repeats 5] [--configs cifar10,svhn,mnist] [--out profiles/wn_init.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
from bench_config import make_config  # noqa: E402  (puts the package on sys.path)


_ZCA = []


def fresh_trainer(name):
    import torch
    from tg import runtime
    from Training.Train_goodGAN import Train
    cfg = make_config(name)
    if name == 'cifar10':
        from Model.Good_GAN_cifar10 import Good_GAN_cifar10 as Model
        if not _ZCA:                                    # the synthetic whitening of the benchmark workload: a fixed random rotation
            q, _ = np.linalg.qr(np.random.default_rng(4321).standard_normal((3072, 3072)))
            _ZCA.append((np.zeros(3072, np.float32), q.astype(np.float32)))
        cfg.ZCA = _ZCA[0]
    else:
        from Model.Good_GAN import Good_GAN as Model
    runtime.set_context(None)
    torch.cuda.empty_cache()
    tr = Train(cfg, None, None)
    tr._build_train_graph(Model)
    return tr, cfg


def feed(tr, cfg, seed):
    rng = np.random.default_rng(seed)
    lo = 0.0 if cfg.DATA_NAME == 'mnist' else -1.0
    img = lambda n: rng.uniform(lo, 1, [n] + list(cfg.IMAGE_DIM)).astype(np.float32)
    oh = lambda n: np.eye(cfg.NUM_CLASSES, dtype=np.float32)[rng.integers(0, cfg.NUM_CLASSES, n)]
    tr.feed(dict(x_l_c=img(cfg.BATCH_SIZE_L_C), y_l_c=oh(cfg.BATCH_SIZE_L_C), x_l_d=img(cfg.BATCH_SIZE_L_D), y_l_d=oh(cfg.BATCH_SIZE_L_D),
                 x_u_d=img(cfg.BATCH_SIZE_U_D), x_u_c=img(cfg.BATCH_SIZE_U_C)))
    tr.sample_latent()


def measure(name, repeats):
    import torch
    dev_ms, host_ms, counts = [], [], None
    for k in range(repeats + 1):                        # + the process's first trainer, reported apart
        tr, cfg = fresh_trainer(name)
        feed(tr, cfg, 100 + k)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(torch.cuda.current_stream())
        counts = tr.data_dependent_init()
        e1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        host_ms.append(1e3 * (time.perf_counter() - t0))
        dev_ms.append(e0.elapsed_time(e1))
    return dev_ms, host_ms, counts


def spread(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return "median %.3f ms, min %.3f, max %.3f (%d fresh trainers)" % (np.median(a), a[0], a[-1], a.size)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--configs', default='cifar10,svhn,mnist')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    L = []
    say = lambda s: (L.append(s), print(s, flush=True))
    say("Data-dependent weight-norm initialisation pass (config.WN_INIT = 'data', DESIGN 9.9): wall time per configuration, one MI355X")
    say("")
    say("command: python tools/bench_wn_init.py --repeats %d --configs %s" % (args.repeats, args.configs))
    say("device: %s   torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    first = True
    for name in args.configs.split(','):
        dev_ms, host_ms, counts = measure(name, args.repeats)
        cfg = make_config(name)
        say("%s (B_G %d, U_C %d, L_D + U_D %d): layers initialised %s" % (name, cfg.BATCH_SIZE_G, cfg.BATCH_SIZE_U_C,
                                                                         cfg.BATCH_SIZE_L_D + cfg.BATCH_SIZE_U_D, counts))
        say("  first trainer of %s: device %.3f ms, host %.3f ms" % ("the process (code objects load)" if first else "this configuration",
                                                                    dev_ms[0], host_ms[0]))
        say("  device events around the call: " + spread(dev_ms[1:]))
        say("  host clock, call + synchronise: " + spread(host_ms[1:]))
        first = False
    say("")
    say("notes: every figure is one Train.data_dependent_init() of a freshly built trainer (buffers of the pass are allocated inside it);")
    say("the pass runs once per training run, before the first iteration, and not at all after a restore.  No threshold.")
    if args.out:
        with open(args.out, 'w') as f:
            f.write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
