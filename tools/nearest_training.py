#!/usr/bin/env python3
"""Restore a run's checkpoint and show each generated sample's nearest training images (Train.nearest_training): are the
samples copies of training images?  In pixel space the samples — those tools/sample_metrics.py scores — are quantised back to the input
pipeline's bytes and searched against every training record with exact integer distances (tg_nearest_u8_i32); g_nn_rmse is read against
val_nn_rmse, the same statistic of held-out validation images: there is no threshold.  --space feature searches the classifier's pooled
features instead (k = 1).

    python tools/nearest_training.py --experiment mnist --data-dir DIR [--weight-dir DIR] [--run Run_...] [--epoch N] [--n 64] [--k 3]
                                     [--space pixel|feature] [--out PNG]

--data-dir is the DATA_DIR of the experiment's TFRecords: there is no synthetic training split to search.  --weight-dir, --run and
--epoch as in tools/sample_metrics.py.  --out (pixel space) writes one row per sample for the first 16: the sample, then its k nearest
training images.  Prints one JSON line: the four scalars, and per sample the training index, distance and label of its nearest image
(the training index counts records in file order: Input_Pipeline.tfrecordDataset.training_chunks)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sample_metrics as SM  # noqa: E402  (also puts the package on sys.path)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--experiment', choices=SM.EXPERIMENTS, required=True)
    ap.add_argument('--data-dir', required=True, help="DATA_DIR of the experiment's TFRecords")
    ap.add_argument('--weight-dir', help="the directory that holds the run's Run_* directories (default: the experiment's WEIGHT_DIR)")
    ap.add_argument('--run', help='the Run_* directory to restore (default: the latest)')
    ap.add_argument('--epoch', type=int, help="the checkpoint's epoch (default: the run's last)")
    ap.add_argument('--n', type=int, default=64, help='generated samples to look up')
    ap.add_argument('--k', type=int, default=3, help='nearest training images per sample (1..16; 1 with --space feature)')
    ap.add_argument('--space', choices=('pixel', 'feature'), default='pixel')
    ap.add_argument('--out', help='PNG to write the grid to (pixel space)')
    a = ap.parse_args()
    from Training.Saver import Saver
    from Training.epoch_tail import write_nearest_grid
    tr, cfg, Dataset = SM.build(a.experiment, a.weight_dir, a.data_dir)
    epoch = Saver(cfg.WEIGHT_DIR).restore(tr, dir_names=a.run, epoch=a.epoch)
    train = Dataset(cfg.DATA_DIR, cfg, cfg.NUM_LABEL, 'train', False)
    val = Dataset(cfg.DATA_DIR, cfg, cfg.NUM_LABEL, 'test', False)
    _, init_op_val, NNIO = train.inputpipline_train_val(val)
    init_op_val()
    out, (fake, bank) = tr.nearest_training(train, NNIO.val_batches(), a.n, a.k, space=a.space, return_banks=True)
    if a.out and a.space == 'pixel':
        write_nearest_grid(a.out, out['nn_idx'], fake, bank, cfg.IMAGE_DIM)
    line = {k: v for k, v in out.items() if not hasattr(v, 'shape')}
    line.update({k: out[k][:, 0].tolist() for k in ('nn_idx', 'nn_d2', 'nn_label') if k in out})
    print(json.dumps(dict(line, experiment=a.experiment, epoch=int(epoch), n=int(a.n), k=int(a.k), space=a.space, training_records=int(bank.n),
                          weight_dir=cfg.WEIGHT_DIR, run=a.run, out=a.out if a.space == 'pixel' else None)))


if __name__ == '__main__':
    main()
