"""float64 / NumPy restatement of the TensorFlow summary behaviour that Training/Summary.py and csrc/summary.hip implement,
written from the TF 1.x sources (core/lib/histogram/histogram.cc, core/kernels/summary_op.cc, summary_image_op.cc) and independent of the
package: the bucket limits, Histogram::Add / EncodeToProto, the Event / Summary / HistogramProto / Image wire format (an encoder and a
decoder of its own) and NormalizeFloatImage.  The yardstick of tests/test_summary_reference.py and tests/test_gpu_summary.py.  The bytes
were never opened in a real TensorBoard (none is installed where this was written)."""
import math
import struct
import zlib

import numpy as np

DBL_MAX = 1.7976931348623157e308
N_LIMITS = 1551


def bucket_limits():
    """v = 1e-12; while v < 1e20: push v; v *= 1.1 (IEEE double, repeated multiplication) -> 774 values; then DBL_MAX; the table is the
    negated list reversed, 0.0, the list."""
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    pos.append(DBL_MAX)
    return np.array([-x for x in reversed(pos)] + [0.0] + pos, np.float64)


LIMITS = bucket_limits()


def bucket_of(x):
    """upper_bound(limits, (double)x) - limits for finite x (array or scalar)."""
    return np.searchsorted(LIMITS, np.asarray(x, np.float64), side='right')


def histogram(x):
    """what tensorflow::histogram::Histogram holds after Add(double(v)) for every finite v of x, plus the NaN / Inf counts the summary op
    trips over: {min, max, num, sum, sum_squares, counts int64 [1551], nan, inf}.  sum / sum_squares are math.fsum's (correctly rounded)."""
    x = np.asarray(x, np.float32).reshape(-1)
    nan = int(np.isnan(x).sum())
    inf = int(np.isinf(x).sum())
    v = x[np.isfinite(x)].astype(np.float64)
    counts = np.bincount(bucket_of(v), minlength=N_LIMITS).astype(np.int64) if v.size else np.zeros(N_LIMITS, np.int64)
    assert counts.size == N_LIMITS
    return dict(min=float(v.min()) if v.size else DBL_MAX, max=float(v.max()) if v.size else -DBL_MAX, num=float(v.size),
                sum=math.fsum(v.tolist()), sum_squares=fsum_squares(v),
                counts=counts, nan=nan, inf=inf, abs_sum=math.fsum(np.abs(v).tolist()))


def fsum_squares(v):
    """sum of the EXACT squares of float32-valued doubles: a float32 has 24 significant bits, so its square has at most 48 and v * v in
    double is exact; fsum then rounds the exact sum once."""
    return math.fsum((v * v).tolist())


def compress(limits, counts):
    """Histogram::EncodeToProto(preserve_zero_buckets = false) -> (bucket_limit, bucket) lists."""
    bl, b = [], []
    i = 0
    while i < len(counts):
        c, end = counts[i], limits[i]
        i += 1
        if c > 0:
            bl.append(float(end))
            b.append(float(c))
        else:
            while i < len(counts) and counts[i] <= 0:
                end = limits[i]
                i += 1
            bl.append(float(end))
            b.append(0.0)
    if not bl:
        bl, b = [DBL_MAX], [0.0]
    return bl, b


# ---- wire format ----------------------------------------------------------------------------------------------------------------------
def _varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(field, wire):
    return _varint(field << 3 | wire)


def _bytes_field(field, payload):
    return _key(field, 2) + _varint(len(payload)) + payload


def histogram_proto(h):
    bl, b = compress(h['limits'] if 'limits' in h else LIMITS, h['counts'])
    out = b''
    for field, k in ((1, 'min'), (2, 'max'), (3, 'num'), (4, 'sum'), (5, 'sum_squares')):
        out += _key(field, 1) + struct.pack('<d', h[k])
    return out + _bytes_field(6, np.asarray(bl, '<f8').tobytes()) + _bytes_field(7, np.asarray(b, '<f8').tobytes())


def image_proto(im):
    return (_key(1, 0) + _varint(im['height']) + _key(2, 0) + _varint(im['width']) + _key(3, 0) + _varint(im['colorspace']) +
            _bytes_field(4, im['encoded']))


def event_bytes(wall_time, step=None, file_version=None, scalars=None, histograms=None, images=None):
    ev = _key(1, 1) + struct.pack('<d', wall_time)
    if step is not None:
        ev += _key(2, 0) + _varint(step)
    if file_version is not None:
        ev += _bytes_field(3, file_version.encode())
    vals = b''
    for tag, v in (scalars or {}).items():
        vals += _bytes_field(1, _bytes_field(1, tag.encode()) + _key(2, 5) + struct.pack('<f', v))
    for tag, im in (images or {}).items():
        vals += _bytes_field(1, _bytes_field(1, tag.encode()) + _bytes_field(4, image_proto(im)))
    for tag, h in (histograms or {}).items():
        vals += _bytes_field(1, _bytes_field(1, tag.encode()) + _bytes_field(5, histogram_proto(h)))
    if vals:
        ev += _bytes_field(5, vals)
    return ev


def _read_varint(buf, pos):
    shift = v = 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        if not b & 0x80:
            return v, pos
        shift += 7


def fields(buf):
    """[(field, wire type, value)] of one message: varints as ints, 64- / 32-bit as raw bytes, length-delimited as bytes."""
    out, pos = [], 0
    while pos < len(buf):
        key, pos = _read_varint(buf, pos)
        field, wire = key >> 3, key & 7
        if wire == 0:
            v, pos = _read_varint(buf, pos)
        elif wire == 1:
            v, pos = buf[pos:pos + 8], pos + 8
        elif wire == 5:
            v, pos = buf[pos:pos + 4], pos + 4
        elif wire == 2:
            n, pos = _read_varint(buf, pos)
            v, pos = buf[pos:pos + n], pos + n
            assert len(v) == n
        else:
            raise ValueError("wire type %d" % wire)
        out.append((field, wire, v))
    assert pos == len(buf)
    return out


def decode_event(payload):
    """Event bytes -> {wall_time, step, file_version, scalars {tag: float}, histograms {tag: {min, max, num, sum, sum_squares,
    bucket_limit, bucket}}, images {tag: {height, width, colorspace, encoded}}, order [tags as written]} (absent parts left out)."""
    ev = {}
    for f, wt, v in fields(payload):
        if f == 1:
            ev['wall_time'] = struct.unpack('<d', v)[0]
        elif f == 2:
            ev['step'] = v
        elif f == 3:
            ev['file_version'] = v.decode()
        elif f == 5:
            ev.update(scalars={}, histograms={}, images={}, order=[])
            for f2, _, val in fields(v):
                assert f2 == 1
                tag = None
                for f3, wt3, vv in fields(val):
                    if f3 == 1:
                        tag = vv.decode()
                        ev['order'].append(tag)
                    elif f3 == 2:
                        ev['scalars'][tag] = struct.unpack('<f', vv)[0]
                    elif f3 == 4:
                        im = {}
                        for f4, _, x in fields(vv):
                            im[{1: 'height', 2: 'width', 3: 'colorspace', 4: 'encoded'}[f4]] = x
                        ev['images'][tag] = im
                    elif f3 == 5:
                        h = {}
                        for f4, wt4, x in fields(vv):
                            if f4 <= 5:
                                h[{1: 'min', 2: 'max', 3: 'num', 4: 'sum', 5: 'sum_squares'}[f4]] = struct.unpack('<d', x)[0]
                            else:
                                assert wt4 == 2 and len(x) % 8 == 0
                                h['bucket_limit' if f4 == 6 else 'bucket'] = list(struct.unpack('<%dd' % (len(x) // 8), x))
                        ev['histograms'][tag] = h
    return ev


# ---- images ----------------------------------------------------------------------------------------------------------------------------
def normalize_float_image(img):
    """NormalizeFloatImage of summary_image_op.cc on one [H,W,C] image, pixel by pixel in float32 (slow and plain on purpose)."""
    v = np.asarray(img, np.float32)
    h, w, c = v.shape
    f32 = np.float32
    image_min, image_max = f32(np.inf), f32(-np.inf)
    finite = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            if all(math.isfinite(float(t)) for t in v[y, x]):
                finite[y, x] = True
                image_min = min(image_min, v[y, x].min())
                image_max = max(image_max, v[y, x].max())
    if image_min < 0:
        max_val = max(abs(image_min), abs(image_max))
        scale, offset = (f32(0) if max_val < f32(1e-6) else f32(f32(127) / f32(max_val))), f32(128)
    else:
        scale, offset = (f32(0) if image_max < f32(1e-6) else f32(f32(255) / f32(image_max))), f32(0)
    bad = [255, 0, 0, 0][:c]
    out = np.zeros((h, w, c), np.uint8)
    for y in range(h):
        for x in range(w):
            if finite[y, x]:
                for k in range(c):
                    out[y, x, k] = int(f32(f32(v[y, x, k] * scale) + offset))
            else:
                out[y, x] = bad
    return out


def decode_png(data):
    """8-bit non-interlaced PNG (grey, RGB, RGBA; any of the five row filters) -> uint8 [H,W,C]; the chunk CRCs are checked."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, hdr = 8, b'', None
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, tag
        pos += 12 + n
        if tag == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat += body
        elif tag == b'IEND':
            break
    w, h, depth, color, comp, flt, lace = hdr
    assert depth == 8 and comp == 0 and flt == 0 and lace == 0
    c = {0: 1, 2: 3, 6: 4}[color]
    raw = zlib.decompress(idat)
    stride = w * c
    assert len(raw) == h * (stride + 1)
    out = np.zeros((h, stride), np.int32)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int32)
        up = out[y - 1] if y else np.zeros(stride, np.int32)
        if ft == 0:
            out[y] = line
        elif ft == 2:
            out[y] = (line + up) & 255
        else:
            for i in range(stride):
                a = out[y, i - c] if i >= c else 0
                b = up[i]
                cc = up[i - c] if i >= c else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) // 2
                else:
                    p = a + b - cc
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else cc)
                out[y, i] = (line[i] + pred) & 255
    return out.astype(np.uint8).reshape(h, w, c)
