"""CPU checks of the histogram / image summaries: the restatement of TensorFlow's behaviour (tests/summary_reference.py)
against the facts the issue pins, and Training/Summary.py, tg/summary.py's host entry point, utils.png_bytes and tools/read_events.py
against the restatement.  The kernel itself is held to it in tests/test_gpu_summary.py."""
import os
import sys

import numpy as np
import pytest

from oracle import tfrecord as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-implementation-of-triple-gan_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import summary_reference as R          # noqa: E402


# ------------------------------------------------------------------------------------------------------------- the bucket table
def test_the_limit_table():
    L = R.LIMITS
    assert L.size == 1551 and L.dtype == np.float64
    assert np.all(np.diff(L) > 0)
    assert L[775] == 0.0 and (L[:775] < 0).sum() == 775 and (L[776:] > 0).sum() == 775
    assert L[0] == -R.DBL_MAX and L[-1] == R.DBL_MAX
    pos = L[776:-1]
    assert pos.size == 774 and pos[0] == 1e-12 and pos[-1] < 1e20 <= pos[-1] * 1.1
    np.testing.assert_array_equal(L[:775], -L[776:][::-1])
    assert not any(float(np.float32(v)) == v for v in pos)            # no positive limit is a float32: x < limit has no tie to break


def test_the_library_builds_the_same_table_on_the_host():
    from tg import summary as tgsum
    got = tgsum.limits()
    assert got.dtype == np.float64 and got.tobytes() == R.LIMITS.tobytes()
    from tg import lib
    import ctypes as C
    with pytest.raises(lib.TgError, match='1551'):
        lib.call('tg_tf_histogram_limits', (C.c_double * 10)(), 10)


def test_pinned_bucket_indices():
    assert list(R.bucket_of([0.0, -0.0, 1e-12, 3e38, -3e38])) == [776, 776, 777, 1550, 1]
    fmax = float(np.finfo(np.float32).max)
    assert list(R.bucket_of([fmax, -fmax, 1e-45, -1e-45])) == [1550, 1, 776, 775]
    h = R.histogram(np.array([0.0, -0.0, np.nan, np.inf, 2.0], np.float32))
    assert h['num'] == 3 and h['nan'] == 1 and h['inf'] == 1 and h['counts'][776] == 2 and h['sum'] == 2.0 and h['sum_squares'] == 4.0
    e = R.histogram(np.zeros(0, np.float32))
    assert e['min'] == R.DBL_MAX and e['max'] == -R.DBL_MAX and e['num'] == 0 and not e['counts'].any()


# ------------------------------------------------------------------------------------------------------------- bucket compression
CASES = [
    ([0, 0, 0, 0, 0], [1., 2., 3., 4., 5.], ([5.], [0.])),                                  # all empty: ONE run, its last limit
    ([], [], ([R.DBL_MAX], [0.])),                                                          # nothing at all
    ([0, 0, 7, 0, 0], [1., 2., 3., 4., 5.], ([2., 3., 5.], [0., 7., 0.])),                  # one bucket, runs before and after
    ([4], [9.], ([9.], [4.])),
    ([1, 0, 0, 2, 3, 0, 4, 0], [1., 2., 3., 4., 5., 6., 7., 8.], ([1., 3., 4., 5., 6., 7., 8.], [1., 0., 2., 3., 0., 4., 0.])),
    ([0, 5], [1., 2.], ([1., 2.], [0., 5.])),
]


@pytest.mark.parametrize("counts,limits,want", CASES)
def test_compression_rule(counts, limits, want):
    from Training.Summary import compress_buckets
    assert R.compress(limits, counts) == want
    assert compress_buckets(limits, counts) == want
    assert compress_buckets(*want) == want                                                   # compressing twice changes nothing


def test_compression_of_a_real_histogram():
    from Training.Summary import compress_buckets
    x = (np.random.default_rng(0).standard_normal(5000) * 0.02).astype(np.float32)
    h = R.histogram(x)
    bl, b = R.compress(R.LIMITS, h['counts'])
    assert compress_buckets(R.LIMITS, h['counts']) == (bl, b)
    assert sum(b) == 5000 and len(bl) < 400 and b[0] == 0 and b[-1] == 0 and bl[-1] == R.DBL_MAX
    assert all(c > 0 or (i == 0 or b[i - 1] > 0) for i, c in enumerate(b))                  # never two empty entries in a row


# ------------------------------------------------------------------------------------------------------------- the wire format
def _sample_event_parts():
    from utils import png_bytes
    rng = np.random.default_rng(4)
    h = dict(R.histogram((rng.standard_normal(3000) * 3).astype(np.float32)), limits=R.LIMITS)
    u8 = rng.integers(0, 256, (6, 5, 3)).astype(np.uint8)
    im = dict(height=6, width=5, colorspace=3, encoded=png_bytes(u8))
    return h, im, u8


def test_scalar_only_events_are_the_bytes_they_were():
    """literal bytes of the previous encode_event (taken from that function before it learnt histograms and images)."""
    from Training.Summary import encode_event
    assert encode_event(1.5, step=3, scalars={'g_loss': 0.5, 'd_loss': 1.25}).hex() == \
        '09000000000000f83f10032a1e0a0d0a06675f6c6f7373150000003f0a0d0a06645f6c6f7373150000a03f'
    assert encode_event(2.0, file_version='brain.Event:2').hex() == '0900000000000000401a0d627261696e2e4576656e743a32'
    assert encode_event(0.25, step=300).hex() == '09000000000000d03f10ac02'
    assert encode_event(0.25, step=300, scalars={}, histograms={}, images={}).hex() == '09000000000000d03f10ac02'


def test_events_with_histograms_and_images_round_trip(tmp_path):
    from Training.Summary import encode_event
    from tg import io as tgio
    import read_events as RE
    h, im, u8 = _sample_event_parts()
    kw = dict(scalars={'g_loss': 0.5}, images={'generated/image/0': im}, histograms={'w': h, 'gradients/w': h})
    ev = encode_event(12.5, step=7, **kw)
    assert ev == R.event_bytes(12.5, step=7, **kw)                                           # the independent encoder: the same bytes
    path = str(tmp_path / 'events')
    tgio.append_record(path, encode_event(1.0, file_version='brain.Event:2'), append=False)
    tgio.append_record(path, ev)
    recs = O.read_tfrecord(path)                                                             # CRCs verified by the oracle's reader
    assert recs == RE.read_records(path) and recs[1] == ev
    for d in (R.decode_event(recs[1]), RE.decode_event(recs[1])):
        assert d['step'] == 7 and d['wall_time'] == 12.5 and d['scalars'] == {'g_loss': 0.5}
        assert list(d['histograms']) == ['w', 'gradients/w'] and list(d['images']) == ['generated/image/0']
        g = d['histograms']['w']
        assert (g['min'], g['max'], g['num'], g['sum'], g['sum_squares']) == (h['min'], h['max'], 3000.0, h['sum'], h['sum_squares'])
        assert (list(g['bucket_limit']), list(g['bucket'])) == R.compress(R.LIMITS, h['counts']) and sum(g['bucket']) == 3000
        i = d['images']['generated/image/0']
        assert (i['height'], i['width'], i['colorspace']) == (6, 5, 3) and i['encoded'] == im['encoded']
        np.testing.assert_array_equal(R.decode_png(i['encoded']), u8)
    assert R.decode_event(recs[1])['order'] == ['g_loss', 'generated/image/0', 'w', 'gradients/w']    # scalars, images, histograms
    hh, ww, cc, raw = RE.decode_png(im['encoded'])
    assert (hh, ww, cc) == (6, 5, 3) and raw == u8.tobytes()


def test_read_events_tool_prints_and_dumps(tmp_path, capsys):
    from Training.Summary import encode_event
    from tg import io as tgio
    import read_events as RE
    h, im, u8 = _sample_event_parts()
    path = str(tmp_path / 'events')
    tgio.append_record(path, encode_event(1.0, file_version='brain.Event:2'), append=False)
    tgio.append_record(path, encode_event(2.0, step=4, scalars={'d_loss': 1.25}, images={'generated/image/1': im}, histograms={'w': h}))
    assert RE.main([path, '--images', str(tmp_path / 'png'), '--buckets']) == 0
    out = capsys.readouterr().out
    assert 'file_version brain.Event:2' in out and 'step 4' in out and 'd_loss' in out and 'num 3000' in out and '6x5x3' in out
    assert open(str(tmp_path / 'png' / '4_generated_image_1.png'), 'rb').read() == im['encoded']
    bad = bytearray(open(path, 'rb').read())
    bad[-6] ^= 1
    open(path, 'wb').write(bytes(bad))
    with pytest.raises(ValueError, match='CRC'):
        RE.read_records(path)


def test_write_png_writes_the_bytes_it_wrote(tmp_path):
    """utils.write_png was split into png_bytes + the file write: the file is the encoder's bytes, and they decode to the rounding
    write_png has always applied."""
    from utils import png_bytes, write_png
    rng = np.random.default_rng(1)
    for shape in ((7, 9), (7, 9, 3)):
        img = rng.uniform(-0.1, 1.1, shape)
        p = str(tmp_path / ('a%d.png' % len(shape)))
        write_png(p, img)
        u8 = np.clip(img * 255.0 + 0.5, 0, 255).astype(np.uint8)
        data = open(p, 'rb').read()
        assert data == png_bytes(u8)
        np.testing.assert_array_equal(R.decode_png(data), u8.reshape(7, 9, -1))
    # the 2x2 grey image of the previous write_png, byte for byte
    write_png(str(tmp_path / 'lit.png'), np.array([[0.0, 1.0], [0.5, 0.25]]))
    assert open(str(tmp_path / 'lit.png'), 'rb').read().hex() == \
        '89504e470d0a1a0a0000000d494844520000000200000002080000000057dd52f80000000e49444154789c6360f8cfd0e00000054201c0703636d60000000049454e44ae426082'


# ------------------------------------------------------------------------------------------------------------- image normalisation
def _images():
    rng = np.random.default_rng(8)
    nan_one = rng.standard_normal((4, 5, 3)).astype(np.float32)
    nan_one[2, 3, 1] = np.nan
    inf_pos = np.abs(rng.standard_normal((4, 5, 3))).astype(np.float32)
    inf_pos[0, 0, 2] = np.inf
    return {
        'all-positive': np.abs(rng.standard_normal((6, 4, 3))).astype(np.float32) * 3,
        'mixed sign': rng.standard_normal((6, 4, 3)).astype(np.float32),
        'all-zero': np.zeros((3, 3, 3), np.float32),
        'under 1e-6 positive': np.full((2, 2, 3), 9.9e-7, np.float32),
        'over 1e-6 positive': np.full((2, 2, 3), 1.1e-6, np.float32),
        'under 1e-6 mixed': np.array([[[-9e-7], [5e-7]]], np.float32),
        'over 1e-6 mixed': np.array([[[-2e-6], [5e-7]]], np.float32),
        'nan in one channel': nan_one,
        'inf among positives': inf_pos,
        'one channel': rng.standard_normal((5, 5, 1)).astype(np.float32),
        'tanh range': np.tanh(rng.standard_normal((8, 8, 3)) * 2).astype(np.float32),
        'all nan': np.full((2, 2, 3), np.nan, np.float32),
    }


@pytest.mark.parametrize("name", sorted(_images()))
def test_image_normalisation(name):
    from Training.Summary import normalize_float_image
    img = _images()[name]
    got, want = normalize_float_image(img), R.normalize_float_image(img)
    assert got.dtype == np.uint8 and got.shape == img.shape
    np.testing.assert_array_equal(got, want)
    if name == 'all-positive':
        assert got.max() == 255 and got.min() < 128
    if name == 'mixed sign':
        assert got.max() <= 255 and got.min() >= 1 and (got.max() == 255 or got.min() == 1)
    if name in ('all-zero', 'under 1e-6 positive'):
        assert not got.any()
    if name == 'over 1e-6 positive':
        assert (got >= 254).all()
    if name == 'under 1e-6 mixed':
        assert (got == 128).all()
    if name == 'over 1e-6 mixed':
        assert got[0, 0, 0] == 1 and got[0, 1, 0] == 159
    if name == 'nan in one channel':
        assert list(got[2, 3]) == [255, 0, 0] and (np.argwhere((got == [255, 0, 0]).all(axis=2)) == [2, 3]).all()
    if name == 'inf among positives':
        assert list(got[0, 0]) == [255, 0, 0]
    if name == 'all nan':
        assert (got == [255, 0, 0]).all()


def test_image_tags_and_values():
    from Training.Summary import image_tag, image_values
    assert [image_tag('generated', i, 2) for i in range(2)] == ['generated/image/0', 'generated/image/1']
    assert image_tag('generated', 0, 1) == 'generated/image'
    batch = np.random.default_rng(2).standard_normal((5, 28, 28, 1)).astype(np.float32)
    v = image_values('g', batch, 3)
    assert list(v) == ['g/image/0', 'g/image/1', 'g/image/2']
    assert list(image_values('g', batch, 1)) == ['g/image'] and len(image_values('g', batch[:1], 4)) == 1
    for i, im in enumerate(v.values()):
        assert (im['height'], im['width'], im['colorspace']) == (28, 28, 1)
        np.testing.assert_array_equal(R.decode_png(im['encoded']), R.normalize_float_image(batch[i]))


# ------------------------------------------------------------------------------------------------------------- the public surface
def test_flags_reach_the_config():
    from config import Config
    from Training.Train_goodGAN import _customize_config

    class TempConfig(Config):
        BATCH_SIZE = 8
    c = TempConfig()
    assert c.SUMMARY_HISTOGRAM is False and c.SUMMARY_IMAGE is False and c.SUMMARY_IMAGE_MAX_OUTPUTS == 2

    class Flags(object):
        summary_histogram = True
        summary_image = True
        summary_image_max_outputs = 4
    _customize_config(c, Flags())
    assert c.SUMMARY_HISTOGRAM is True and c.SUMMARY_IMAGE is True and c.SUMMARY_IMAGE_MAX_OUTPUTS == 4


def test_summary_keeps_the_histogram_and_image_keys(tmp_path):
    from Training.Summary import Summary
    from tg import lib
    s = Summary(str(tmp_path), None, log_type='train', log_comments='c')
    tags = s.add_summary({'scalar': {'g_loss': None}, 'histogram': {'classifier/conv1_1/V:0': None, 'gradients/w': None},
                          'image': {'generated': None}})
    assert tags == ['g_loss']
    assert s._histogram_summary({'a:0': None, 'b': None}) == {'a:0': 'a_0', 'b': 'b'}       # reference :56
    assert s._image_summary({'x': None}) == {'x': 2} and s._image_summary({'x': None}, max_outputs=1) == {'x': 1}
    assert s._hist_tags == {'classifier/conv1_1/V:0': 'classifier/conv1_1/V_0', 'gradients/w': 'gradients/w'}
    assert s._image_outputs == {'generated': 2}
    rng = np.random.default_rng(6)
    x = rng.standard_normal(100).astype(np.float32)
    h = dict(R.histogram(x), limits=R.LIMITS)
    imgs = np.tanh(rng.standard_normal((3, 8, 8, 3))).astype(np.float32)
    s.write(dict(g_loss=0.5, other=1.0), 1, histograms={'classifier/conv1_1/V:0': h, 'gradients/w': h, 'unregistered': h},
            images={'generated': imgs})
    files = [f for f in os.listdir(s.log_dir) if f.startswith('events.out.tfevents.')]
    recs = O.read_tfrecord(os.path.join(s.log_dir, files[0]))
    assert len(recs) == 2                                                                    # file_version + ONE event for the step
    ev = R.decode_event(recs[1])
    assert ev['order'] == ['g_loss', 'generated/image/0', 'generated/image/1', 'classifier/conv1_1/V_0', 'gradients/w']
    assert ev['histograms']['gradients/w']['num'] == 100
    np.testing.assert_array_equal(R.decode_png(ev['images']['generated/image/1']['encoded']), R.normalize_float_image(imgs[1]))
    assert open(os.path.join(s.log_dir, 'history.csv')).read().splitlines() == ['step,g_loss', '1,0.5']     # scalars only
    # a non-finite histogram: TensorFlow's error, and nothing of the step is written
    for key, word in (('nan', 'Nan'), ('inf', 'Infinity')):
        with pytest.raises(lib.TgError, match="%s in summary histogram for: gradients/w" % word):
            s.write(dict(g_loss=0.25), 2, histograms={'gradients/w': dict(h, **{key: 3})})
    assert len(O.read_tfrecord(os.path.join(s.log_dir, files[0]))) == 2
    assert len(open(os.path.join(s.log_dir, 'history.csv')).read().splitlines()) == 2


def test_train_has_the_public_surface():
    import inspect
    from Training.Train_goodGAN import NETS, Train
    p = inspect.signature(Train.histograms).parameters
    assert list(p) == ['self', 'which', 'nets'] and p['which'].default == 'value' and p['nets'].default == NETS
    assert 'unscaled' in Train.histograms.__doc__ or 'before the 1/world scale' in Train.histograms.__doc__
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '9.8' in design and 'tg_tf_histogram_f32' in design and 'TensorBoard' in design
    assert 'tg_tf_histogram_f32' in open(os.path.join(ROOT, 'README.md')).read() or 'SUMMARY_HISTOGRAM' in open(os.path.join(ROOT, 'README.md')).read()
