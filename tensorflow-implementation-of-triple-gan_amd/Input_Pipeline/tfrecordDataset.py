"""TFRecord input pipeline — MI355X-native counterpart of the reference's Input_Pipeline/{cifar10,svhn,mnist}Dataset.py
(same constructor, method names and file naming; line references are to Input_Pipeline/svhnDataset.py unless noted).

  reference (TensorFlow)                                   here
  tf.data.TFRecordDataset(name)             :33-42         tg.io.RecordFile: mmap + index + CRC check in C++ (csrc/tfrecord.cpp)
  .map(self.parser, num_parallel_calls)     :44-70         tg_ds_gather (threaded tf.Example decode into pinned uint8 staging),
                                                           then ON THE DEVICE: x/255*2-1 (MNIST x/255) and one_hot (tg_u8_affine_f32,
                                                           tg_onehot_i32_f32) — 4x fewer bytes over PCIe than float32 batches
  .shuffle(MIN_QUEUE_EXAMPLES + 30*BATCH_SIZE).repeat(n)   :76-82   ShuffleStream: the same streaming-buffer algorithm on record indices
  .batch(bs).prefetch(5*bs)                 :84-87         Batcher + a background thread that stays `PREFETCH` batches ahead
  iterators / initializers                  :96-137        init_op_train() / init_op_val() restart the streams
  .map(pre_processing) "do augmentation"    cifar10Dataset.py:72-74 (a no-op there)   config.AUGMENT: random shift (reflect padding)
                                                           and horizontal flip of every training batch, fused into the device tail
                                                           (tg_u8_augment_f32; augment_indices + _to_host: the same in NumPy)

Batch protocol (SURVEY §8a T1 — the reference's three pipelines disagree with its placeholders, the build fixes one):
three training streams — labelled for C (L_C), labelled for D (L_D), unlabelled (U_D + U_C, sliced as x_u[:U_D], x_u[U_D:]
Training/Train_goodGAN.py:255-256) — and the test split in batches of BATCH_SIZE.
"""
import os
import queue
import threading

import numpy as np

from tg import io as tgio


class ShuffleStream(object):
    """dataset.shuffle(buffer_size).repeat(count) on record indices 0..n-1: a buffer is filled with the next `buffer_size`
    indices in file order; every draw takes a uniformly random slot and refills it from the file; at the end of an epoch the
    buffer drains; `count` epochs (-1: endless)."""

    def __init__(self, n, buffer_size, repeat, seed):
        self.n, self.buffer_size, self.repeat = int(n), max(1, int(buffer_size)), repeat
        self.rng = np.random.default_rng(seed)

    def __iter__(self):
        epoch = 0
        while self.n > 0 and (self.repeat is None or self.repeat < 0 or epoch < self.repeat):
            nxt = min(self.buffer_size, self.n)
            buf = list(range(nxt))
            while buf:
                j = int(self.rng.integers(len(buf)))
                yield buf[j]
                if nxt < self.n:
                    buf[j] = nxt
                    nxt += 1
                else:
                    buf[j] = buf[-1]
                    buf.pop()
            epoch += 1


def philox4x32(ctr, key):
    """Philox4x32-10 (Random123; csrc/tg_device.h philox): ctr = four uint32 arrays (or ints) of one shape, key = two ints -> the four
    output words, uint64 arrays holding 32-bit values."""
    m = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & m for v in ctr)
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c0, c1, c2, c3


def augment_indices(n, h, w, max_shift, flip, seed, stream_id, count):
    """source rows [n, h] and columns [n, w] of the augmentation of a batch of n images (tg_u8_augment_f32): image i draws
    r = Philox4x32-10(counter (i, stream_id, lo32(count), hi32(count)), key (lo32(seed), hi32(seed))), is shifted by
    dy, dx = (r.x, r.y) * (2S+1) >> 32, minus S, with reflect padding, and flipped horizontally when flip and r.z >> 31."""
    seed, count = int(seed) & (2 ** 64 - 1), int(count) & (2 ** 64 - 1)
    i = np.arange(n, dtype=np.uint64)
    rx, ry, rz, _ = philox4x32((i, stream_id, count & 0xFFFFFFFF, count >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    span = np.uint64(2 * max_shift + 1)
    dy = ((rx * span) >> np.uint64(32)).astype(np.int64) - max_shift
    dx = ((ry * span) >> np.uint64(32)).astype(np.int64) - max_shift
    flipped = (rz >> np.uint64(31)).astype(bool) & bool(flip)

    def reflect(p, size):
        return np.where(p < 0, -p, np.where(p >= size, 2 * size - 2 - p, p))
    x = np.arange(w)
    return reflect(np.arange(h)[None, :] + dy[:, None], h), reflect(np.where(flipped[:, None], w - 1 - x, x) + dx[:, None], w)


def _batches(stream, batch_size):
    """dataset.batch(batch_size): consecutive groups; only the very last one may be short."""
    cur = []
    for i in stream:
        cur.append(i)
        if len(cur) == batch_size:
            yield np.asarray(cur, np.int64)
            cur = []
    if cur:
        yield np.asarray(cur, np.int64)


class _Slot(object):
    """one staging buffer of the prefetch ring: uint8 images + int32 labels in PINNED host memory when a GPU is present (so the
    host-to-device copy is asynchronous), and the event after which the buffer may be refilled."""

    def __init__(self, max_n, shape, pinned):
        h, w, c = shape
        self.t_img = self.t_lab = None
        if pinned:
            import torch
            self.t_img = torch.empty(max_n * h * w * c, dtype=torch.uint8).pin_memory()
            self.t_lab = torch.empty(max_n, dtype=torch.int32).pin_memory()
            self.img, self.lab = self.t_img.numpy(), self.t_lab.numpy()
        else:
            self.img, self.lab = np.empty(max_n * h * w * c, np.uint8), np.empty(max_n, np.int32)
        self.shape, self.n, self.event = shape, 0, None

    @property
    def images(self):
        h, w, c = self.shape
        return self.img[:self.n * h * w * c].reshape(self.n, h, w, c)

    @property
    def labels(self):
        return self.lab[:self.n]


class _Prefetcher(object):
    """background thread: index batches -> decoded uint8 / int32 batches, `depth` ahead (dataset.prefetch).  The ring has
    depth + 2 slots: up to `depth` queued, one being filled, one in the consumer's hands; a slot whose copy to the device is still
    in flight (the host runs ahead of the GPU) is not refilled before that copy's event has completed."""

    def __init__(self, rec, index_batches, depth, n_threads, max_batch, pinned):
        depth = max(1, depth)
        self.q = queue.Queue(maxsize=depth)
        self.stop = False
        ring = [_Slot(max_batch, rec.shape, pinned) for _ in range(depth + 2)] if len(rec) else []

        def run():
            try:
                k = 0
                for idx in index_batches:
                    if self.stop:
                        return
                    slot = ring[k % len(ring)]
                    k += 1
                    if slot.event is not None:
                        slot.event.synchronize()
                        slot.event = None
                    slot.n = len(idx)
                    rec.gather(idx, slot.img, slot.lab, n_threads=n_threads)
                    self.q.put(slot)
                self.q.put(None)
            except Exception as e:          # surfaced in the consumer
                self.q.put(e)
        self.t = threading.Thread(target=run, daemon=True)
        self.t.start()

    def get(self):
        item = self.q.get()
        if isinstance(item, Exception):
            raise item
        return item

    def close(self):
        self.stop = True
        try:
            while True:
                self.q.get_nowait()
        except queue.Empty:
            pass


TRAINING_CHUNK = 16384          # records per piece of training_chunks (50 MB of CIFAR bytes)


def training_files(dataset):
    """The record files of the training split of a tfrecordDataset (subset 'train'; MNIST's UNIT_RANGE scaling included), each once and
    in file order: input_from_tfrecord_filename() returns the labelled file twice ([labelled for D, labelled for C, unlabelled]).  The
    test split is not opened.  lib.TgError for any other Dataset or subset."""
    from tg import lib
    if not isinstance(dataset, tfrecordDataset):
        raise lib.TgError("the training records are those of a tfrecordDataset (such as cifar10Dataset); %s has none" % type(dataset).__name__)
    if dataset.subset != 'train':
        raise lib.TgError("the training records are read from the training split only, got subset %r" % (dataset.subset,))
    return each_once(dataset.input_from_tfrecord_filename())


def each_once(files):
    """the record files of a list, each once, in the order of first appearance."""
    out = []
    for rec in files:
        if all(rec is not r for r in out):
            out.append(rec)
    return out


def record_chunks(files, rows):
    """(RecordFile, record indices) pieces of at most `rows` records over the files given: file order, then record order."""
    for rec in files:
        for s in range(0, len(rec), rows):
            yield rec, np.arange(s, min(s + rows, len(rec)), dtype=np.int64)


def training_chunks(dataset, rows=TRAINING_CHUNK):
    """(RecordFile, record indices) pieces of at most `rows` records that cover every training record exactly once: file order, then
    record order.  That order defines the training index — the position of a record in the concatenation of the pieces — which
    Train.nearest_training's `nn_idx` refers to."""
    for piece in record_chunks(training_files(dataset), rows):
        yield piece


class _NNIO(object):
    """what Training/Train_goodGAN.py consumes: next() = the feed of one iteration, val_batches() = the test split."""

    def __init__(self, train, val):
        self.train, self.val = train, val

    def next(self):
        return self.train._next()

    def val_batches(self):
        return self.val._val_batches()


class tfrecordDataset(object):
    PREFIX = None
    TRAIN_SIZE = None
    CHANNELS = 3
    UNIT_RANGE = False          # True: x/255 (mnistDataset.py:65); False: x/255*2-1
    AUG_SHIFT = 2               # config.AUGMENT: random shift of every training image by up to this many pixels (reflect padding)
    AUG_FLIP = False            # config.AUGMENT: horizontal flip with probability 1/2 (natural images; not digits)
    PREFETCH = 5                # batches (the reference prefetches batch_size*5 elements, :86)
    DECODE_THREADS = 1          # one thread decodes ~0.9 M CIFAR records/s; spawning helpers only pays for large batches

    def __init__(self, data_dir, config, num_label=None, subset='train', use_augmentation=False, seed=None):
        self.data_dir = os.path.join(data_dir, "Tfrecord")                       # :16
        self.subset = subset
        self.use_augmentation = use_augmentation
        self.config = config
        self.num_label = num_label
        self.train_size = self.TRAIN_SIZE
        self.seed = (1234 if seed is None else seed) + 1000 * getattr(config, 'RANK', 0)
        self._streams = None
        self._aug_counts = [0, 0, 0, 0]      # batches augmented so far per stream id (0: records of the per-record parser path)

    # ---- files ----------------------------------------------------------------------------------
    def get_filenames(self):                                                     # :23-31
        assert self.subset in ['train', 'test'], 'Invalid data subset "%s"' % self.subset
        if self.subset == 'train':
            return [os.path.join(self.data_dir, '%s_%s_%s.tfrecords' % (self.PREFIX, self.subset, str(self.num_label).zfill(6))),
                    os.path.join(self.data_dir, '%s_%s_%s.tfrecords' % (self.PREFIX, self.subset,
                                                                       str(self.train_size - self.num_label).zfill(6)))]
        return [os.path.join(self.data_dir, '%s_%s.tfrecords' % (self.PREFIX, self.subset))]

    def input_from_tfrecord_filename(self):                                      # :33-42
        names = self.get_filenames()
        if self.subset == 'test':
            return [tgio.RecordFile(n) for n in names]
        lab = tgio.RecordFile(names[0])
        return [lab, lab, tgio.RecordFile(names[1])]                              # labelled for D, labelled for C, unlabelled

    # ---- per-record parser (API parity and tests; the batched path decodes in C++ and scales on the device) -------------
    def parser(self, serialized_example):                                        # :44-70
        img, label, h, w = tgio.parse_example(serialized_example)
        image = np.frombuffer(img, np.uint8).reshape(h, w, self.CHANNELS).astype(np.float32)
        image = image / 255 if self.UNIT_RANGE else image / 255 * 2 - 1
        onehot = np.eye(self.config.NUM_CLASSES, dtype=np.float32)[label]
        if self.use_augmentation:
            image, onehot = self.pre_processing(image, onehot)
        return image, onehot

    def pre_processing(self, image, label):                                      # :72-74 (a no-op in the reference)
        """config.AUGMENT: the training augmentation of one decoded record (a batch of one image of stream 0, counted per record)."""
        aug = self._aug_draw(0)
        if aug is None:
            return image, label
        h, w, _ = image.shape
        ys, xs = augment_indices(1, h, w, self.AUG_SHIFT, self.AUG_FLIP, self.seed, *aug)
        return image[ys[0][:, None], xs[0][None, :]], label

    def shuffle_and_repeat(self, dataset, repeat=1, seed=0):                     # :76-82
        return ShuffleStream(len(dataset), self.config.MIN_QUEUE_EXAMPLES + 30 * self.config.BATCH_SIZE, repeat, self.seed + seed)

    def batch(self, dataset, batch_size):                                        # :84-87
        return _batches(dataset, batch_size)

    # ---- augmentation (config.AUGMENT) -------------------------------------------------
    def _aug_draw(self, stream_id):
        """(stream_id, count) of the next batch of that stream when the training augmentation is on (config.AUGMENT on a Dataset built
        with use_augmentation), else None.  The count runs from the Dataset's creation, across epochs."""
        if not (self.use_augmentation and getattr(self.config, 'AUGMENT', False)):
            return None
        count = self._aug_counts[stream_id]
        self._aug_counts[stream_id] += 1
        return stream_id, count

    # ---- device tail ----------------------------------------------------------------------------
    def _to_device(self, images_u8, labels_i32, want_labels=True, slot=None, aug=None):
        """uint8 [n,H,W,C] / int32 [n] host arrays -> (Act float32 scaled, Act one-hot) on the GPU; aug = (stream_id, count): augmented
        (tg_u8_augment_f32) in the same pass."""
        import torch
        from tg import lib
        from tg.runtime import Act, ctx
        cx = ctx()
        n, h, w, c = images_u8.shape
        xu = torch.from_numpy(images_u8).to(cx.device, non_blocking=True)
        x = torch.empty(n * h * w * c, dtype=torch.float32, device=cx.device)
        scale, shift = (1.0, 0.0) if self.UNIT_RANGE else (2.0, -1.0)
        if aug is None:
            lib.call('tg_u8_affine_f32', lib.ptr(xu), lib.ptr(x), xu.numel(), scale, shift, cx.stream)
        else:
            lib.call('tg_u8_augment_f32', lib.ptr(xu), lib.ptr(x), n, h, w, c, scale, shift, self.AUG_SHIFT, int(self.AUG_FLIP),
                     self.seed & (2 ** 64 - 1), aug[0], aug[1] & (2 ** 64 - 1), cx.stream)
        xa, ya = Act(x, n, h, w, c, c), None
        if want_labels:
            k = self.config.NUM_CLASSES
            lu = torch.from_numpy(labels_i32).to(cx.device, non_blocking=True)
            y = torch.empty(n * k, dtype=torch.float32, device=cx.device)
            lib.call('tg_onehot_i32_f32', lib.ptr(lu), lib.ptr(y), n, k, cx.stream)
            ya = Act(y, n, 1, 1, k, k)
        if slot is not None:                 # the staging buffer may be refilled once these copies have run
            slot.event = torch.cuda.Event()
            slot.event.record(torch.cuda.current_stream(cx.device))
        return xa, ya

    def _to_host(self, images_u8, labels_i32, aug=None):
        """the same tail in NumPy (no GPU: tests, tools), bit for bit."""
        if aug is not None:
            n, h, w, _ = images_u8.shape
            ys, xs = augment_indices(n, h, w, self.AUG_SHIFT, self.AUG_FLIP, self.seed, *aug)
            images_u8 = images_u8[np.arange(n)[:, None, None], ys[:, :, None], xs[:, None, :]]
        x = images_u8.astype(np.float32)
        x = x / 255 if self.UNIT_RANGE else x / 255 * 2 - 1
        return x, np.eye(self.config.NUM_CLASSES, dtype=np.float32)[labels_i32]

    def _on_device(self):
        import torch
        return bool(getattr(self.config, 'PIPELINE_DEVICE', True)) and torch.cuda.is_available()

    def _finish(self, slot, stream_id, want_labels=True):
        aug = self._aug_draw(stream_id)
        if self._on_device():
            return self._to_device(slot.images, slot.labels, want_labels, slot, aug)
        return self._to_host(slot.images.copy(), slot.labels.copy(), aug)

    # ---- pipelines ------------------------------------------------------------------------------
    def _start_train(self):
        c = self.config
        lab_d, lab_c, unl = self._files
        if self._streams:
            for s in self._streams:
                s.close()
        mk = lambda rec, bs, repeat, seed: _Prefetcher(rec, self.batch(self.shuffle_and_repeat(rec, repeat, seed), bs), self.PREFETCH,
                                                       self.DECODE_THREADS, bs, self._on_device())
        self._streams = [mk(lab_c, c.BATCH_SIZE_L_C, -1, 1), mk(lab_d, c.BATCH_SIZE_L_D, -1, 2),
                         mk(unl, c.BATCH_SIZE_U_D + c.BATCH_SIZE_U_C, getattr(c, 'REPEAT', -1) or -1, 3)]
        self._epoch = getattr(self, '_epoch', 0) + 1

    def _next(self):
        c = self.config
        if self._streams is None:
            self._start_train()
        got = [s.get() for s in self._streams]
        if any(g is None for g in got) or got[2].n < c.BATCH_SIZE_U_D + c.BATCH_SIZE_U_C:
            raise StopIteration("unlabelled stream exhausted (config.REPEAT epochs)")
        b = {}
        b['x_l_c'], b['y_l_c'] = self._finish(got[0], 1)                          # stream ids: those of the shuffle seeds
        b['x_l_d'], b['y_l_d'] = self._finish(got[1], 2)
        xu, _ = self._finish(got[2], 3, want_labels=False)
        if isinstance(xu, np.ndarray):
            b['x_u_d'], b['x_u_c'] = xu[:c.BATCH_SIZE_U_D], xu[c.BATCH_SIZE_U_D:]
        else:
            b['x_u_d'], b['x_u_c'] = xu.view_rows(0, c.BATCH_SIZE_U_D), xu.view_rows(c.BATCH_SIZE_U_D, xu.n)
        return b

    def _val_batches(self):
        rec = self._files[0]
        stream = self.batch(self.shuffle_and_repeat(rec, 1, 99), self.config.BATCH_SIZE)
        pf = _Prefetcher(rec, stream, self.PREFETCH, self.DECODE_THREADS, self.config.BATCH_SIZE, False)
        while True:
            got = pf.get()
            if got is None:
                return
            yield self._to_host(got.images.copy(), got.labels.copy())          # Train.evaluate stages host arrays itself

    def inputpipline_train_val(self, other):                                     # :89-137
        self._files = self.input_from_tfrecord_filename()
        other._files = other.input_from_tfrecord_filename()

        def init_op_train():
            self._start_train()

        def init_op_val():
            pass
        return init_op_train, init_op_val, _NNIO(self, other)

    def inputpipline_testSet(self):                                              # :139-160 (cifar10Dataset.py)
        self._files = self.input_from_tfrecord_filename()
        return (lambda: None), self._val_batches()
