#!/usr/bin/env python3
"""Wall time of the classifier's evaluation report on an MI355X: over --val validation images of a configuration of
tools/bench_config.py at its batch size, three passes under the same synchronisation —

  evaluate            Train.evaluate alone: what an epoch tail without the report runs
  evaluate + report   Train.evaluate(report=ClassifierReport) and the one device->host copy of the counts: one more
                      tg_eval_report_f32 call (two launches) per batch
  host route          the same forward passes, each batch's logits copied to the host and the same counts formed there in vectorised
                      NumPy float64

Every pass ends in a device->host copy; the host clock runs from a device synchronise before the pass to the end of that copy.  One
untimed round of all three first (buffers, lazily loaded code objects), then --repeats rounds that alternate the three, so that a
drift of the shared host falls on all of them; median, minimum and maximum are printed, and the report's overhead as the difference
of the medians per batch.  Also the kernel alone at the pass's batch shape, HIP events around --repeats calls.  States what the time
is; asserts no threshold.  Prints a text report and writes it to --out.

    python tools/bench_eval_report.py [--config cifar10|cifar100|mnist] [--val 10000] [--repeats 7] [--out profiles/eval_report.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
from bench_config import make_config  # noqa: E402  (puts the package on sys.path)

RANKS, BINS = 16, 15


def trainer(name, n_val):
    """(trainer, validation batches) of configuration `name` at its batch size, untrained, synthetic images and labels."""
    from tg import runtime
    from Training.Train_goodGAN import Train
    cfg = make_config(name)
    if cfg.DATA_NAME in ('cifar10', 'cifar100'):
        from Model.Good_GAN_cifar10 import Good_GAN_cifar10 as Model
        q, _ = np.linalg.qr(np.random.default_rng(4321).standard_normal((3072, 3072)))
        cfg.ZCA = (np.zeros(3072, np.float32), q.astype(np.float32))
    else:
        from Model.Good_GAN import Good_GAN as Model
    runtime.set_context(None)
    tr = Train(cfg, None, None)
    tr._build_train_graph(Model)
    rng = np.random.default_rng(1)
    bs, k = cfg.BATCH_SIZE, cfg.NUM_CLASSES
    shape = (bs, cfg.IMAGE_HEIGHT, cfg.IMAGE_WIDTH, cfg.CHANNEL)
    val = [(rng.uniform(-1, 1, shape).astype(np.float32), np.eye(k, dtype=np.float32)[rng.integers(0, k, bs)])
           for _ in range(max(1, n_val // bs))]
    return tr, val


def host_counts(logits, labels, acc, nr, nb):
    """one batch into the host accumulators `acc`: the counts of tg_eval_report_f32 in vectorised NumPy (finite logits assumed)."""
    k = logits.shape[1]
    t, p = labels.argmax(axis=1), logits.argmax(axis=1)
    np.add.at(acc['confusion'], (t, p), 1)
    l = logits.astype(np.float64)
    rows = np.arange(l.shape[0])
    lt = logits[rows, t][:, None]
    rank = (logits > lt).sum(axis=1) + ((logits == lt) & (np.arange(k)[None, :] < t[:, None])).sum(axis=1)
    acc['rank_hist'] += np.bincount(np.minimum(rank, nr - 1), minlength=nr)
    m = l[rows, p]
    e = np.exp(l - m[:, None])
    s = e.sum(axis=1)
    conf = 1.0 / s
    pj = e / s[:, None]
    pj[rows, t] -= 1.0
    acc['sums'] += ((np.log(s) + (m - l[rows, t])).sum(), (pj * pj).sum())
    b = np.minimum(nb - 1, (conf * nb).astype(np.int64))
    acc['bin_count'] += np.bincount(b, minlength=nb)
    acc['bin_correct'] += np.bincount(b[p == t], minlength=nb)
    acc['bin_conf'] += np.bincount(b, weights=conf, minlength=nb)


def host_route(tr, val):
    """evaluate's forward passes with the report formed on the host -> the report_from_counts dict."""
    from tg import metrics as M
    cx, m = tr.cx, tr.model
    k = tr.options.num_classes
    nr = min(RANKS, k)
    acc = dict(confusion=np.zeros((k, k), np.int64), rank_hist=np.zeros(nr, np.int64), bin_count=np.zeros(BINS, np.int64),
               bin_correct=np.zeros(BINS, np.int64), bin_conf=np.zeros(BINS), sums=np.zeros(2), nonfinite=np.zeros(1, np.int64))
    for x, y in val:
        with cx.phase_scope('val', record=False):
            xa = cx.from_numpy(x, key='val:x')
            if m.zca() is not None:
                xa = m.zca().apply(m.as_image(xa))
            with cx.rng_scoped('val/C'):
                logits, _ = m.classifier(xa, False)
            host_counts(logits.numpy(), y, acc, nr, BINS)                 # (Act.numpy: a synchronising device->host copy)
    return M.report_from_counts(**acc)


def kernel_ms(n, k, repeats):
    """HIP-event times of one tg_eval_report_f32 call on an [n, k] batch after a warm-up call."""
    import torch
    from tg import lib
    from tg import metrics as M
    from tg.runtime import Act
    rng = np.random.default_rng(0)
    logits = torch.from_numpy((rng.standard_normal((n, k)) * 3).astype(np.float32)).cuda().reshape(-1)
    labels = torch.from_numpy(np.eye(k, dtype=np.float32)[rng.integers(0, k, n)]).cuda().reshape(-1)
    la, ya = Act(logits, n, 1, 1, k, k), Act(labels, n, 1, 1, k, k)
    rep = M.ClassifierReport(k, logits.device, RANKS, BINS)
    rep.add(ya, la, lib.cur_stream())
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream())
        rep.add(ya, la, lib.cur_stream())
        e1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def spread(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return "median %.3f ms, min %.3f, max %.3f (%d runs)" % (np.median(a), a[0], a[-1], a.size)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--config', choices=('cifar10', 'cifar100', 'mnist'), default='cifar10')
    ap.add_argument('--val', type=int, default=10000)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_report.txt'))
    a = ap.parse_args()
    import torch
    tr, val = trainer(a.config, a.val)
    bs, k = tr.config.BATCH_SIZE, tr.options.num_classes

    def with_report():
        rep = tr._new_report()
        tr.evaluate(val, report=rep)
        return rep.result()

    passes = (('evaluate', lambda: tr.evaluate(val)), ('evaluate + report', with_report), ('host route', lambda: host_route(tr, val)))
    results = {name: fn() for name, fn in passes}                         # the untimed round
    ms = {name: [] for name, _ in passes}
    for _ in range(a.repeats):
        for name, fn in passes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms[name].append(1e3 * (time.perf_counter() - t0))
    dev, host = results['evaluate + report'], results['host route']
    L = ["classifier evaluation report (DESIGN 9.12) on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), "",
         "%s configuration, %d classes: %d validation images in %d batches of %d (host clock, one untimed round first, the three passes"
         % (a.config, k, len(val) * bs, len(val), bs), "alternating)"]
    for name, _ in passes:
        L.append("   %-20s %s" % (name, spread(ms[name])))
    base, rep_ms, host_ms = (np.median(ms[name]) for name, _ in passes)
    L.append("   report - evaluate = %.3f ms per pass = %.1f us per batch (%.2f %% of evaluate); host route - evaluate = %.3f ms = %.1f us per batch"
             % (rep_ms - base, 1e3 * (rep_ms - base) / len(val), 100.0 * (rep_ms - base) / base, host_ms - base, 1e3 * (host_ms - base) / len(val)))
    L.append("   tg_eval_report_f32 alone on an [%d, %d] batch (device events, both launches): %s" % (bs, k, spread(kernel_ms(bs, k, a.repeats))))
    L.append("   an untrained model: the values below only show that both routes count the same rows")
    same = all((dev[key] == host[key]).all() for key in ('confusion', 'support', 'predicted')) and dev['accuracy'] == results['evaluate']
    L.append("   device accuracy %.4f nll %.6f ece %.6f | host accuracy %.4f nll %.6f ece %.6f | confusion matrices equal: %s"
             % (dev['accuracy'], dev['nll'], dev['ece'], host['accuracy'], host['nll'], host['ece'], same))
    text = "\n".join(L) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
