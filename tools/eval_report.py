#!/usr/bin/env python3
"""Restore a run's checkpoint and print its classifier's evaluation report over the validation split (Train.evaluate_report,
DESIGN §9.12): a per-class table (support, predicted, recall, precision, F1), the ten largest off-diagonal entries of the confusion
matrix, the reliability table behind the expected calibration error, then one JSON line of the scalars — with the raw weights, or with
the classifier's averaged weights (--ema).  With --samples N also the same for N generated samples, the class asked for as target:
which classes the generator fails to render, as judged by the checkpoint's own classifier.

    python tools/eval_report.py --experiment mnist [--weight-dir DIR] [--run Run_...] [--epoch N] [--ema] [--data-dir DIR]
                                [--samples N] [--out DIR]

--weight-dir, --run, --epoch and --data-dir as for tools/sample_metrics.py, whose `build` this tool uses; the note there on the
classifiers' input noise holds here too.  --out DIR writes confusion.npy (int64 [K, K]; g_confusion.npy with --samples) and report.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from sample_metrics import EXPERIMENTS, build  # noqa: E402  (puts the package on sys.path)


def scalars(rep):
    """the scalar entries of a report as JSON types (NaN -> None)."""
    from tg import metrics as M
    num = lambda v: None if isinstance(v, float) and v != v else v
    return {k: num(rep[k]) for k in M.REPORT_SCALARS}


def tables(rep, title):
    """the printed form of a report: per-class table, the ten largest confusions, the reliability table."""
    conf = rep['confusion']
    k = conf.shape[0]
    L = ["%s: %d rows (%d with a non-finite logit), accuracy %.4f, balanced %.4f, macro F1 %.4f, NLL %.4f, Brier %.4f, ECE %.4f" % (
        title, rep['n'], rep['n_nonfinite'], rep['accuracy'], rep['balanced_accuracy'], rep['macro_f1'], rep['nll'], rep['brier'], rep['ece']),
        "  class  support  predicted   recall  precision       F1"]
    for c in range(k):
        L.append("  %5d  %7d  %9d  %7.4f  %9.4f  %7.4f" % (c, rep['support'][c], rep['predicted'][c], rep['recall'][c], rep['precision'][c], rep['f1'][c]))
    off = conf - np.diag(np.diag(conf))
    order = np.argsort(-off, axis=None, kind='stable')[:10]
    L.append("  largest confusions (target -> prediction: rows)")
    for t, p in zip(*np.unravel_index(order, off.shape)):
        if off[t, p] > 0:
            L.append("  %5d -> %-5d %d" % (t, p, off[t, p]))
    L.append("  confidence bin      rows  mean confidence  accuracy")
    nb = rep['reliability'].shape[0]
    for b, (cnt, mc, acc) in enumerate(rep['reliability']):
        if cnt > 0:
            L.append("  [%.3f, %.3f%s  %6d  %15.4f  %8.4f" % (b / float(nb), (b + 1) / float(nb), "]" if b == nb - 1 else ")", cnt, mc, acc))
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--experiment', choices=EXPERIMENTS, required=True)
    ap.add_argument('--weight-dir', help="the directory that holds the run's Run_* directories (default: the experiment's WEIGHT_DIR)")
    ap.add_argument('--run', help='the Run_* directory to restore (default: the latest)')
    ap.add_argument('--epoch', type=int, help="the checkpoint's epoch (default: the run's last)")
    ap.add_argument('--ema', action='store_true', help="evaluate the classifier's averaged weights (the EMA shadows)")
    ap.add_argument('--data-dir', help="DATA_DIR of the experiment's TFRecords (default: the synthetic validation split)")
    ap.add_argument('--samples', type=int, help="also report on this many generated samples, the class asked for as target")
    ap.add_argument('--out', help='directory for confusion.npy (g_confusion.npy) and report.json')
    a = ap.parse_args()
    from Training.Saver import Saver
    tr, cfg, Dataset = build(a.experiment, a.weight_dir, a.data_dir)
    epoch = Saver(cfg.WEIGHT_DIR).restore(tr, dir_names=a.run, epoch=a.epoch)
    train = Dataset(cfg.DATA_DIR, cfg, cfg.NUM_LABEL, 'train', False)
    val = Dataset(cfg.DATA_DIR, cfg, cfg.NUM_LABEL, 'test', False)
    _, init_op_val, NNIO = train.inputpipline_train_val(val)
    init_op_val()
    if a.samples is None:
        reports = {'val': tr.evaluate_report(NNIO.val_batches(), ema=a.ema)}
    else:
        sm = tr.sample_metrics_report(NNIO.val_batches(), a.samples, ema=a.ema)
        reports = {'val': sm['val_report'], 'g': sm['g_report']}
    print(tables(reports['val'], "validation split"))
    if 'g' in reports:
        print(tables(reports['g'], "%d generated samples" % a.samples))
    out = dict(scalars(reports['val']), experiment=a.experiment, epoch=int(epoch), ema=bool(a.ema), weight_dir=cfg.WEIGHT_DIR, run=a.run)
    if 'g' in reports:
        out['generated'] = dict(scalars(reports['g']), samples=int(a.samples))
    print(json.dumps(out))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        np.save(os.path.join(a.out, 'confusion.npy'), reports['val']['confusion'])
        if 'g' in reports:
            np.save(os.path.join(a.out, 'g_confusion.npy'), reports['g']['confusion'])
        with open(os.path.join(a.out, 'report.json'), 'w') as f:
            json.dump(out, f)


if __name__ == '__main__':
    main()
