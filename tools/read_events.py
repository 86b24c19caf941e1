#!/usr/bin/env python3
"""Print what a TensorBoard event file of Training/Summary.py holds: per event its step, scalars, histogram statistics (min, max, num, sum,
sum of squares, the number of encoded buckets and the fullest one) and image sizes; `--images DIR` also writes every PNG to
DIR/<step>_<tag>.png.  Pure Python (struct / zlib): the way to look at a run on a machine without TensorBoard, and the decoder the tests
use.  The record framing (length, masked CRC-32C of length and of data) is checked.

    python tools/read_events.py Training/Log_cifar10/train/Run_*/events.out.tfevents.* [--images DIR] [--buckets]"""
import argparse
import os
import struct
import sys
import zlib


def _crc32c_table():
    tab = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        tab.append(c)
    return tab


_TAB = _crc32c_table()


def masked_crc32c(data):
    c = 0xFFFFFFFF
    for b in data:
        c = _TAB[(c ^ b) & 0xFF] ^ (c >> 8)
    c ^= 0xFFFFFFFF
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def read_records(path):
    """the payloads of a TFRecord file; ValueError on a bad length / data CRC or a truncated record."""
    data, out, pos = open(path, 'rb').read(), [], 0
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError("%s: truncated record header at byte %d" % (path, pos))
        n, = struct.unpack('<Q', data[pos:pos + 8])
        if struct.unpack('<I', data[pos + 8:pos + 12])[0] != masked_crc32c(data[pos:pos + 8]):
            raise ValueError("%s: bad length CRC at byte %d" % (path, pos))
        body = data[pos + 12:pos + 12 + n]
        if len(body) != n or pos + 16 + n > len(data):
            raise ValueError("%s: truncated record at byte %d" % (path, pos))
        if struct.unpack('<I', data[pos + 12 + n:pos + 16 + n])[0] != masked_crc32c(body):
            raise ValueError("%s: bad data CRC at byte %d" % (path, pos))
        out.append(body)
        pos += 16 + n
    return out


def _fields(buf):
    pos = 0
    while pos < len(buf):
        key = shift = 0
        while True:
            b = buf[pos]
            pos += 1
            key |= (b & 0x7F) << shift
            shift += 7
            if b < 0x80:
                break
        field, wire = key >> 3, key & 7
        if wire == 0:
            v = shift = 0
            while True:
                b = buf[pos]
                pos += 1
                v |= (b & 0x7F) << shift
                shift += 7
                if b < 0x80:
                    break
        elif wire == 1:
            v, pos = buf[pos:pos + 8], pos + 8
        elif wire == 5:
            v, pos = buf[pos:pos + 4], pos + 4
        elif wire == 2:
            n = shift = 0
            while True:
                b = buf[pos]
                pos += 1
                n |= (b & 0x7F) << shift
                shift += 7
                if b < 0x80:
                    break
            v, pos = buf[pos:pos + n], pos + n
        else:
            raise ValueError("unsupported wire type %d" % wire)
        yield field, wire, v


_HIST = {1: 'min', 2: 'max', 3: 'num', 4: 'sum', 5: 'sum_squares'}
_IMG = {1: 'height', 2: 'width', 3: 'colorspace', 4: 'encoded'}


def decode_event(payload):
    """Event bytes -> dict(wall_time, step, file_version, scalars, histograms, images); histograms: {tag: {min, max, num, sum, sum_squares,
    bucket_limit [..], bucket [..]}}; images: {tag: {height, width, colorspace, encoded (PNG bytes)}}."""
    ev = dict(scalars={}, histograms={}, images={})
    for f, _w, v in _fields(payload):
        if f == 1:
            ev['wall_time'] = struct.unpack('<d', v)[0]
        elif f == 2:
            ev['step'] = v
        elif f == 3:
            ev['file_version'] = v.decode()
        elif f == 5:
            for f2, _w2, value in _fields(v):
                if f2 != 1:
                    continue
                tag = None
                for f3, _w3, x in _fields(value):
                    if f3 == 1:
                        tag = x.decode()
                    elif f3 == 2:
                        ev['scalars'][tag] = struct.unpack('<f', x)[0]
                    elif f3 == 4:
                        ev['images'][tag] = {_IMG[k]: y for k, _wk, y in _fields(x) if k in _IMG}
                    elif f3 == 5:
                        h = dict(bucket_limit=[], bucket=[])
                        for k, wk, y in _fields(x):
                            if k in _HIST:
                                h[_HIST[k]] = struct.unpack('<d', y)[0]
                            elif k in (6, 7):
                                vals = struct.unpack('<%dd' % (len(y) // 8), y) if wk == 2 else struct.unpack('<d', y)
                                h['bucket_limit' if k == 6 else 'bucket'].extend(vals)
                        ev['histograms'][tag] = h
    return ev


def read_events(path):
    return [decode_event(p) for p in read_records(path)]


def decode_png(data):
    """8-bit non-interlaced PNG whose rows use filter 0 (what utils.png_bytes writes) -> (height, width, channels, bytes of the pixels)."""
    if data[:8] != b'\x89PNG\r\n\x1a\n':
        raise ValueError("not a PNG")
    pos, idat, hdr = 8, b'', None
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(tag + body) & 0xffffffff:
            raise ValueError("PNG chunk %r: bad CRC" % tag)
        pos += 12 + n
        if tag == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat += body
    w, h, depth, color = hdr[:4]
    if depth != 8 or color not in (0, 2, 6) or hdr[6]:
        raise ValueError("PNG: only 8-bit non-interlaced grey / RGB / RGBA")
    c = {0: 1, 2: 3, 6: 4}[color]
    raw = zlib.decompress(idat)
    rows = []
    for y in range(h):
        line = raw[y * (w * c + 1):(y + 1) * (w * c + 1)]
        if line[0] != 0:
            raise ValueError("PNG row %d uses filter %d; this reader handles filter 0" % (y, line[0]))
        rows.append(line[1:])
    return h, w, c, b''.join(rows)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('event_file')
    ap.add_argument('--images', metavar='DIR', help='write every PNG to DIR/<step>_<tag>.png')
    ap.add_argument('--buckets', action='store_true', help='also print every encoded (limit, count) pair of every histogram')
    args = ap.parse_args(argv)
    for ev in read_events(args.event_file):
        if 'file_version' in ev:
            print("file_version %s" % ev['file_version'])
            continue
        print("step %s" % ev.get('step'))
        for tag, v in ev['scalars'].items():
            print("  scalar     %-60s %.6g" % (tag, v))
        for tag, h in ev['histograms'].items():
            top = max(range(len(h['bucket'])), key=lambda i: h['bucket'][i]) if h['bucket'] else None
            print("  histogram  %-60s num %d min %.6g max %.6g sum %.6g sum_squares %.6g buckets %d%s"
                  % (tag, h.get('num', 0), h.get('min', 0), h.get('max', 0), h.get('sum', 0), h.get('sum_squares', 0), len(h['bucket']),
                     "" if top is None else " fullest <%.6g: %d" % (h['bucket_limit'][top], h['bucket'][top])))
            if args.buckets:
                for lim, cnt in zip(h['bucket_limit'], h['bucket']):
                    print("      < %-24.17g %d" % (lim, cnt))
        for tag, im in ev['images'].items():
            print("  image      %-60s %dx%dx%d, %d bytes of PNG" % (tag, im.get('height', 0), im.get('width', 0), im.get('colorspace', 0),
                                                                     len(im.get('encoded', b''))))
            if args.images:
                os.makedirs(args.images, exist_ok=True)
                name = '%s_%s.png' % (ev.get('step', 0), tag.replace('/', '_'))
                with open(os.path.join(args.images, name), 'wb') as f:
                    f.write(im.get('encoded', b''))
    return 0


if __name__ == '__main__':
    sys.exit(main())
