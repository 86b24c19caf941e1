"""Scalar, histogram and image summaries — counterpart of the reference's Training/Summary.py (:14-71): <log_dir>/<log_type>/Run_<timestamp>/
with Comments.txt and a TensorBoard event file.  tf.summary.FileWriter writes a TFRecord file of `Event` protos; the same bytes are
produced here (record framing by the C++ side, tg_record_append; the small protos encoded below):

    event.proto    Event   { double wall_time = 1; int64 step = 2; string file_version = 3; Summary summary = 5; }
    summary.proto  Summary { repeated Value value = 1; }
                   Value   { string tag = 1; float simple_value = 2; Image image = 4; HistogramProto histo = 5; }
                   Image   { int32 height = 1; int32 width = 2; int32 colorspace = 3; bytes encoded_image_string = 4; }
                   HistogramProto { double min = 1, max = 2, num = 3, sum = 4, sum_squares = 5;
                                    repeated double bucket_limit = 6 [packed], bucket = 7 [packed]; }

The three summary kinds of the reference (_scalar_summary, _histogram_summary, _image_summary, :49-62) are registered through
add_summary() and written as ONE Summary per step, as TensorFlow's merged summary is: scalars (config.SUMMARY_SCALAR), images
(config.SUMMARY_IMAGE: tf.summary.image's float normalisation, NormalizeFloatImage, on the host; PNG through utils.png_bytes) and
histograms (config.SUMMARY_HISTOGRAM: the statistics and bucket counts come from the device, Train.histograms / tg_tf_histogram_f32;
here they are compressed as Histogram::EncodeToProto does and encoded).  A histogram over a NaN or an infinity raises TgError, as
TensorFlow's op fails, before anything of that step is written.  A `history.csv` with the scalars is kept next to the event file.
The TensorFlow behaviour is restated from its sources; the bytes have not been opened in a TensorBoard.  [UNVERIFIED-TF]"""
import os
import socket
import struct
import time

import numpy as np

from Training.Saver import _eastern_now

DBL_MAX = 1.7976931348623157e308


def _varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _ld(field, payload):
    return _varint((field << 3) | 2) + _varint(len(payload)) + payload


def _double(field, v):
    return _varint((field << 3) | 1) + struct.pack('<d', float(v))


def compress_buckets(limits, counts):
    """Histogram::EncodeToProto(preserve_zero_buckets = false): a bucket with a count is kept as (limit, count); a run of empty buckets
    becomes ONE entry with the limit of the run's last bucket and count 0; (DBL_MAX, 0) when nothing was kept.  -> (bucket_limit, bucket)."""
    out_l, out_c = [], []
    i, n = 0, len(counts)
    while i < n:
        c, end = counts[i], limits[i]
        i += 1
        if c <= 0:
            while i < n and counts[i] <= 0:
                end = limits[i]
                i += 1
            c = 0
        out_l.append(float(end))
        out_c.append(float(c))
    if not out_l:
        out_l, out_c = [DBL_MAX], [0.0]
    return out_l, out_c


def encode_histogram(h):
    """HistogramProto of h = {min, max, num, sum, sum_squares, limits, counts} (limits / counts: the full table or an already compressed
    pair — compression leaves the latter as it is)."""
    limits, counts = compress_buckets(h['limits'], h['counts'])
    return (_double(1, h['min']) + _double(2, h['max']) + _double(3, h['num']) + _double(4, h['sum']) + _double(5, h['sum_squares']) +
            _ld(6, struct.pack('<%dd' % len(limits), *limits)) + _ld(7, struct.pack('<%dd' % len(counts), *counts)))


def encode_image(im):
    """Summary.Image of im = {height, width, colorspace, encoded} (encoded: PNG bytes)."""
    return (_varint((1 << 3) | 0) + _varint(int(im['height'])) + _varint((2 << 3) | 0) + _varint(int(im['width'])) +
            _varint((3 << 3) | 0) + _varint(int(im['colorspace'])) + _ld(4, bytes(im['encoded'])))


def encode_event(wall_time, step=None, file_version=None, scalars=None, histograms=None, images=None):
    """one Event; its Summary holds the scalars, then the images, then the histograms (the order the reference's add_summary registers
    them, :35-40) — {tag: value}, {tag: image dict of encode_image}, {tag: histogram dict of encode_histogram}."""
    ev = _varint((1 << 3) | 1) + struct.pack('<d', wall_time)
    if step is not None:
        ev += _varint((2 << 3) | 0) + _varint(int(step))
    if file_version is not None:
        ev += _ld(3, file_version.encode())
    vals = b''
    if scalars:
        vals += b''.join(_ld(1, _ld(1, tag.encode()) + _varint((2 << 3) | 5) + struct.pack('<f', float(v))) for tag, v in scalars.items())
    if images:
        vals += b''.join(_ld(1, _ld(1, tag.encode()) + _ld(4, encode_image(im))) for tag, im in images.items())
    if histograms:
        vals += b''.join(_ld(1, _ld(1, tag.encode()) + _ld(5, encode_histogram(h))) for tag, h in histograms.items())
    if vals:
        ev += _ld(5, vals)
    return ev


def normalize_float_image(img):
    """tf.summary.image on a float image (NormalizeFloatImage): img [H,W,C] -> uint8 [H,W,C].  A pixel is finite when all its channels are;
    over the finite pixels, min < 0: scale = 127 / max(|min|, |max|) (0 below 1e-6), offset 128; else scale = 255 / max (0 below 1e-6),
    offset 0; a finite pixel becomes uint8(v * scale + offset) — multiply, then add, in float32, truncated — and any other the bad colour
    (255, 0, 0), cut to the channel count."""
    v = np.ascontiguousarray(img, np.float32)
    assert v.ndim == 3, v.shape
    finite = np.isfinite(v).all(axis=2)
    if finite.any():
        image_min, image_max = np.float32(v[finite].min()), np.float32(v[finite].max())
    else:
        image_min, image_max = np.float32(np.inf), np.float32(-np.inf)
    eps = np.float32(1e-6)
    if image_min < 0:
        max_val = max(abs(image_min), abs(image_max))
        scale, offset = (np.float32(0) if max_val < eps else np.float32(127) / max_val), np.float32(128)
    else:
        scale, offset = (np.float32(0) if image_max < eps else np.float32(255) / image_max), np.float32(0)
    with np.errstate(invalid='ignore', over='ignore'):
        prod = (np.where(finite[:, :, None], v, np.float32(0)) * scale).astype(np.float32)
        out = np.trunc(prod + offset).astype(np.int32).astype(np.uint8)
    bad = np.array([255, 0, 0, 0], np.uint8)[:v.shape[2]] if v.shape[2] <= 4 else np.zeros(v.shape[2], np.uint8)
    out[~finite] = bad
    return out


def image_tag(name, i, max_outputs):
    """tf.summary.image's tags: '<name>/image' for max_outputs == 1, else '<name>/image/<i>'."""
    return '%s/image' % name if max_outputs == 1 else '%s/image/%d' % (name, i)


def image_values(name, batch, max_outputs):
    """{tag: image dict} of the first min(max_outputs, N) images of batch [N,H,W,C] (float)."""
    from utils import png_bytes
    batch = np.asarray(batch)
    assert batch.ndim == 4, batch.shape
    out = {}
    for i in range(min(int(max_outputs), batch.shape[0])):
        u8 = normalize_float_image(batch[i])
        out[image_tag(name, i, max_outputs)] = dict(height=u8.shape[0], width=u8.shape[1], colorspace=u8.shape[2], encoded=png_bytes(u8))
    return out


def check_histogram_finite(tag, h):
    """TensorFlow's histogram op fails on a non-finite value ("Nan in summary histogram for: <tag>"); so does this."""
    from tg.lib import TgError
    if h.get('nan', 0):
        raise TgError("Nan in summary histogram for: %s" % tag)
    if h.get('inf', 0):
        raise TgError("Infinity in summary histogram for: %s" % tag)


class _FileWriter(object):
    """tf.summary.FileWriter(log_dir): events.out.tfevents.<unix time>.<hostname>, first record = file_version 'brain.Event:2'."""

    def __init__(self, log_dir):
        from tg import io as tgio
        self._io = tgio
        os.makedirs(log_dir, exist_ok=True)
        self.path = os.path.join(log_dir, 'events.out.tfevents.%010d.%s' % (int(time.time()), socket.gethostname()))
        self._io.append_record(self.path, encode_event(time.time(), file_version='brain.Event:2'), append=False)

    def add_summary(self, scalars, global_step=None, histograms=None, images=None):
        self._io.append_record(self.path, encode_event(time.time(), step=global_step, scalars=scalars, histograms=histograms, images=images))

    def flush(self):
        pass                                                   # every record is written and closed immediately

    def close(self):
        pass


class Summary(object):
    def __init__(self, log_dir, config, **kwargs):                                    # :14-30
        self.config = config
        self.comments = kwargs.get('log_comments', '')
        if 'log_type' in kwargs:
            log_dir = os.path.join(log_dir, kwargs.get('log_type'))
        log_dir = os.path.join(log_dir, 'Run_' + _eastern_now().strftime("%Y-%m-%d_%H_%M_%S"))
        os.makedirs(log_dir, exist_ok=True)
        self.log_dir = log_dir
        self.summary_writer = _FileWriter(log_dir)
        self._write_comments()
        self._tags = []
        self._hist_tags = {}             # registered histogram name -> tag
        self._image_outputs = {}         # registered image name -> max_outputs

    def add_summary(self, summary_dict):                                              # :32-44 -> the "merged summary": tags to evaluate
        """summary_dict: {'scalar': {name: _}, 'image': {name: _}, 'histogram': {name: _}} — the names to write (the values are supplied to
        write(); a TF graph would hold the tensors).  Returns the scalar tags."""
        self._tags = self._scalar_summary(summary_dict['scalar']) if 'scalar' in summary_dict else []
        self._image_outputs = self._image_summary(summary_dict['image']) if 'image' in summary_dict else {}
        self._hist_tags = self._histogram_summary(summary_dict['histogram']) if 'histogram' in summary_dict else {}
        return self._tags

    def _scalar_summary(self, scalar_dict):                                           # :49-52
        return list(scalar_dict.keys())

    def _histogram_summary(self, histogram_dict):                                     # :54-57
        return {name: name.replace(':', '_') for name in histogram_dict}

    def _image_summary(self, image_dict, max_outputs=2):                              # :59-62
        return {name: int(max_outputs) for name in image_dict}

    def write(self, values, step, histograms=None, images=None):
        """summary_writer.add_summary(sess.run(merged_summary), step) of Train_goodGAN.py:293,346: one Event with the registered scalars
        of `values`, the registered images of `images` ({name: float batch [N,H,W,C]}) and the registered histograms of `histograms`
        ({name: histogram dict of Train.histograms}).  A histogram over a NaN / infinity raises TgError before anything is written."""
        scalars = {k: values[k] for k in (self._tags or values) if k in values}
        hist = {}
        for name, h in (histograms or {}).items():
            if self._hist_tags and name not in self._hist_tags:
                continue
            tag = self._hist_tags.get(name, name.replace(':', '_'))
            check_histogram_finite(tag, h)
            hist[tag] = h
        imgs = {}
        for name, batch in (images or {}).items():
            if self._image_outputs and name not in self._image_outputs:
                continue
            imgs.update(image_values(name, batch, self._image_outputs.get(name, 2)))
        self.summary_writer.add_summary(scalars, step, histograms=hist or None, images=imgs or None)
        csv = os.path.join(self.log_dir, 'history.csv')
        new = not os.path.exists(csv)
        with open(csv, 'a') as f:
            if new:
                f.write('step,' + ','.join(scalars) + '\n')
            f.write('%d,' % step + ','.join('%.6g' % float(v) for v in scalars.values()) + '\n')

    def _write_comments(self):                                                        # :63-65
        with open(os.path.join(self.log_dir, 'Comments.txt'), 'w') as txt_file:
            txt_file.write(self.comments)
