#!/usr/bin/env python3
"""Fit the CIFAR ZCA whitening from the training TFRecords on the GPU and write DATA_DIR/<data>_zca_{mean,mat}.npy, the files the
reference loads (Model/Good_GAN_cifar10.py:289-290; here config.ZCA = 'fit').  Prints the wall time of each phase: decode,
host-to-device, Gram kernel, device-to-host, eigh, forming mat, write.  The device phases are synchronised one by one for the timing, so
they are measured back to back instead of overlapped as in Train.train.

    python tools/fit_zca.py --data cifar10 --data-dir DataSet/cifar_10 --num-label 4000
    python tools/fit_zca.py --synthetic 50000          # N random 32x32x3 records in a temporary DATA_DIR first
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-implementation-of-triple-gan_amd"))


def _synthetic(data_dir, Dataset, num_label, n, seed=0):
    """n random 32x32x3 records: num_label in the labelled file, the rest in the unlabelled one, and a small test file."""
    import numpy as np
    from tg import io as tgio
    os.makedirs(os.path.join(data_dir, 'Tfrecord'), exist_ok=True)
    rng = np.random.default_rng(seed)
    tr = Dataset(data_dir, None, num_label, 'train')
    te = Dataset(data_dir, None, num_label, 'test')
    for name, m in zip(tr.get_filenames() + te.get_filenames(), (num_label, n - num_label, 100)):
        for a in range(0, m, 10000):
            k = min(10000, m - a)
            tgio.write_tfrecord(name, rng.integers(0, 256, (k, 32, 32, 3), dtype=np.uint8), rng.integers(0, 10, k), append=a > 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--data', choices=('cifar10', 'cifar100'), default='cifar10')
    ap.add_argument('--data-dir', help='DATA_DIR: holds Tfrecord/<data>_train_*.tfrecords; receives the .npy files')
    ap.add_argument('--num-label', type=int, default=None, help='labelled records (default 4000 for CIFAR-10, 10000 for CIFAR-100)')
    ap.add_argument('--synthetic', type=int, metavar='N', help='write N random records to a temporary DATA_DIR and fit those')
    ap.add_argument('--eps', type=float, default=None, help='regularisation (default Model.zca.ZCA_EPS)')
    a = ap.parse_args()
    if (a.data_dir is None) == (a.synthetic is None):
        ap.error('give exactly one of --data-dir and --synthetic')
    import numpy as np
    import torch
    from tg import lib
    from tg.runtime import Context, set_context
    from Model.zca import ZCA_EPS, cifar10_ZCA, write_zca_files, zca_paths
    if a.data == 'cifar100':
        from Input_Pipeline.cifar100Dataset import cifar100Dataset as Dataset
    else:
        from Input_Pipeline.cifar10Dataset import cifar10Dataset as Dataset
    num_label = a.num_label if a.num_label is not None else (10000 if a.data == 'cifar100' else 4000)
    eps = ZCA_EPS if a.eps is None else a.eps
    if not torch.cuda.is_available():
        raise lib.TgError("fit_zca needs a GPU (the Gram matrix is computed by tg_gram_u8_i64)")
    tmp = None
    try:
        data_dir = a.data_dir
        if a.synthetic is not None:
            tmp = data_dir = tempfile.mkdtemp(prefix='fit_zca_')
            num_label = min(num_label, a.synthetic)
            _synthetic(data_dir, Dataset, num_label, a.synthetic)

        class C(object):
            DATA_NAME, DATA_DIR = a.data, data_dir
        set_context(Context('cuda:0'))
        ds = Dataset(data_dir, C, num_label, 'train')
        t = {}
        t0 = time.perf_counter()
        mean, mat = cifar10_ZCA.fit(ds, eps=eps, timings=t)
        t1 = time.perf_counter()
        write_zca_files(C, mean, mat)
        t['write'] = time.perf_counter() - t1
        n = sum(len(r) for r in ds.input_from_tfrecord_filename()[1:])
        phases = ('decode', 'h2d', 'gram', 'd2h', 'eigh', 'mat', 'write')
        for k in phases:
            print('%-7s %9.3f s' % (k, t.get(k, 0.0)))
        print('%-7s %9.3f s  (fit, phases one after the other)' % ('total', t1 - t0 + t['write']))
        print(json.dumps(dict(data=a.data, images=n, d=int(mean.size), eps=eps, files=list(zca_paths(C)) if tmp is None else None,
                              seconds={k: round(t.get(k, 0.0), 4) for k in phases})))
    finally:
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
