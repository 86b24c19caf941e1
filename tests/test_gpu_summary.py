"""tg_tf_histogram_f32 (csrc/summary.hip) and the histogram / image summaries of the training loop (config.SUMMARY_HISTOGRAM,
config.SUMMARY_IMAGE) against tests/summary_reference.py.

Bucket counts, min, max, num and the NaN / Inf counts are integers or exact values: compared with ==.  sum and sum_squares are fp64 sums
of exactly representable terms ((double)x, and x*x of a float32 has at most 48 significant bits) taken in SOME order: any order of n
fp64 additions is within (n - 1) * 2^-53 * sum|term| * (1 + o(1)) of the exact sum, so the bound n * 2^-53 * sum|term| against
math.fsum needs no measured tolerance."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import gpu_common as G                 # noqa: E402
import summary_reference as R          # noqa: E402

NL, NS = 1551, 8
CHUNK = 16384                          # elements per workgroup of the chunk kernel (include/tg_kernels.h)
GUARD = 64
SMALL = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)


def _lib():
    from tg import lib
    return lib


_LIMITS_DEV = []


def _limits_dev():
    from tg import summary as tgsum
    if not _LIMITS_DEV:
        _LIMITS_DEV.append(torch.from_numpy(np.array(tgsum.limits())).cuda())
        torch.cuda.synchronize()
    return _LIMITS_DEV[0]


def _segs(segments):
    arr = (C.c_int64 * max(2 * len(segments), 2))()
    for k, (o, n) in enumerate(segments):
        arr[2 * k], arr[2 * k + 1] = o, n
    return arr


def run_kernel(x_dev, segments, stream=None, poison=0):
    """-> (counts [nseg,1551] int64, stats [nseg,8] float64, raw bytes of both); checks the guard regions behind the workspace and both
    outputs and that the input was not written."""
    lib = _lib()
    nseg = len(segments)
    segs = _segs(segments)
    need = lib.call('tg_tf_histogram_workspace_bytes', segs, nseg)
    assert need >= 16 and need % 8 == 0
    fill = {0: 0, 1: -1, 2: 0x7ff8dead}[poison]
    ws = torch.full((need // 8 + GUARD,), fill, dtype=torch.int64, device='cuda')
    ws[need // 8:] = 0x5a5a5a5a
    counts = torch.full((nseg * NL + GUARD,), 77 + poison, dtype=torch.int64, device='cuda')
    stats = torch.full((nseg * NS + GUARD,), -3.25, dtype=torch.float64, device='cuda')
    before = x_dev.clone()
    s = stream or torch.cuda.current_stream()
    lim = _limits_dev()
    s.wait_stream(torch.cuda.current_stream())             # the fills above ran on the current stream
    with torch.cuda.stream(s):
        lib.call('tg_tf_histogram_f32', lib.ptr(x_dev), x_dev.numel(), segs, nseg, lib.ptr(lim), lib.ptr(counts), lib.ptr(stats),
                 lib.ptr(ws), need, C.c_void_p(s.cuda_stream))
    s.synchronize()
    torch.cuda.synchronize()
    assert bool((ws[need // 8:] == 0x5a5a5a5a).all()), "written behind the workspace"
    assert bool((counts[nseg * NL:] == 77 + poison).all()), "written behind counts"
    assert bool((stats[nseg * NS:] == -3.25).all()), "written behind stats"
    assert torch.equal(before.view(torch.int32), x_dev.view(torch.int32)), "the input was written"
    c = counts[:nseg * NL].cpu().numpy().reshape(nseg, NL)
    st = stats[:nseg * NS].cpu().numpy().reshape(nseg, NS)
    return c, st, c.tobytes() + st.tobytes()


def check_segment(x_host, seg, c, st, what=''):
    off, n = seg
    ref = R.histogram(x_host[off:off + n])
    np.testing.assert_array_equal(c, ref['counts'], err_msg=what)
    assert st[0] == ref['min'] and st[1] == ref['max'] and st[2] == ref['num'], (what, st[:3], ref['min'], ref['max'], ref['num'])
    assert st[5] == ref['nan'] and st[6] == ref['inf'], (what, st[5:7], ref['nan'], ref['inf'])
    assert int(c.sum()) == int(ref['num'])
    v = x_host[off:off + n].astype(np.float64)
    v = v[np.isfinite(v)]
    nn = max(v.size, 1)
    tol_sum = nn * 2.0 ** -53 * ref['abs_sum']
    tol_sq = nn * 2.0 ** -53 * ref['sum_squares']
    print("%s n=%d sum err %.3g (allowed %.3g) sum_squares err %.3g (allowed %.3g)"
          % (what, n, abs(st[3] - ref['sum']), tol_sum, abs(st[4] - ref['sum_squares']), tol_sq))
    assert abs(st[3] - ref['sum']) <= tol_sum, (what, st[3], ref['sum'], tol_sum)
    assert abs(st[4] - ref['sum_squares']) <= tol_sq, (what, st[4], ref['sum_squares'], tol_sq)


def _mixed_buffer():
    """a flat buffer of many segments with poisoned gaps: sizes 1, 31, 33, 10 007, one of 2 chunks + 5, an all-zero one, an all-equal
    one, an empty one, +-0 / denormals / +-FLT_MAX, limit neighbours; NaN in every gap."""
    rng = np.random.default_rng(20)
    fmax = np.finfo(np.float32).max
    tiny = np.float32(1e-45)
    lim32 = []
    for i in (1, 100, 400, 700, 774, 776, 777, 900, 1100, 1300, 1500, 1549):        # a dozen limits across the table
        f = np.float32(R.LIMITS[i])
        lim32 += [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    parts = [
        rng.standard_normal(1).astype(np.float32),
        (rng.standard_normal(31) * 1e-3).astype(np.float32),
        (rng.standard_normal(33) * 50).astype(np.float32),
        (rng.standard_normal(10007) * np.exp(rng.uniform(-30, 30, 10007))).astype(np.float32),
        rng.standard_normal(2 * CHUNK + 5).astype(np.float32),
        np.zeros(700, np.float32),
        np.full(300, -0.0372, np.float32),
        np.zeros(0, np.float32),
        np.array([0.0, -0.0, tiny, -tiny, np.float32(1.1754942e-38), np.float32(-1.1754942e-38), fmax, -fmax, 1e-12, -1e-12], np.float32),
        np.array(lim32, np.float32),
        np.zeros(CHUNK, np.float32),                     # exactly one chunk of one bucket
        np.abs(rng.standard_normal(257)).astype(np.float32),
    ]
    segs, chunks, off = [], [], 0
    for p in parts:
        segs.append((off, p.size))
        pad = (-p.size) % 32 or 32                       # always a gap, as between the variables of a ParamStore (and then some)
        chunks += [p, np.full(pad, np.nan, np.float32)]
        off += p.size + pad
    return np.concatenate(chunks), segs


@pytest.fixture(scope='module')
def mixed():
    x, segs = _mixed_buffer()
    xd = torch.from_numpy(x).cuda()
    c, st, raw = run_kernel(xd, segs)
    return dict(x=x, xd=xd, segs=segs, c=c, st=st, raw=raw)


def test_every_segment_matches_the_restatement(mixed):
    assert len(mixed['segs']) == 12
    for k, seg in enumerate(mixed['segs']):
        check_segment(mixed['x'], seg, mixed['c'][k], mixed['st'][k], 'segment %d' % k)
    e = mixed['st'][7]                                    # the empty segment: TensorFlow's initial state
    assert e[0] == R.DBL_MAX and e[1] == -R.DBL_MAX and not e[2:].any() and not mixed['c'][7].any()
    assert mixed['st'][:, 5].sum() == 0                   # no NaN of the padding reached any result
    z = mixed['c'][5]
    assert z[776] == 700 and z.sum() == 700               # all zeros: one bucket
    edge = mixed['c'][8]
    assert edge[776] >= 2 and edge[1550] == 1 and edge[1] == 1


def test_widening_a_segment_into_the_padding_counts_its_nans(mixed):
    off, n = mixed['segs'][1]
    c, st, _ = run_kernel(mixed['xd'], [(off, n), (off, n + 1)])
    assert st[0][5] == 0 and st[1][5] == 1                # negative control: the poison is there, and only a wider segment sees it
    np.testing.assert_array_equal(c[0], c[1])
    assert st[1][2] == n and st[0][3] == st[1][3]


def test_reruns_streams_and_a_poisoned_workspace_give_identical_bytes(mixed):
    for k in range(5):
        assert run_kernel(mixed['xd'], mixed['segs'], poison=k % 3)[2] == mixed['raw'], k
    side = torch.cuda.Stream()
    assert run_kernel(mixed['xd'], mixed['segs'], stream=side, poison=2)[2] == mixed['raw']


def test_more_segments_than_workgroups_and_fewer():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(40 * 1000).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    many = [(i * 10, 7) for i in range(3000)]             # 3 000 segments of 7: far more workgroups than compute units
    c, st, _ = run_kernel(xd, many)
    for k in (0, 1, 1499, 2999):
        check_segment(x, many[k], c[k], st[k], 'many %d' % k)
    assert (c.sum(axis=1) == 7).all() and (st[:, 2] == 7).all()
    few = [(3, 39000)]                                    # one segment, three workgroups, an odd start
    c, st, _ = run_kernel(xd, few)
    check_segment(x, few[0], c[0], st[0], 'few')


def test_non_finite_values_are_counted_and_left_out():
    x = np.array([1.0, np.nan, 2.0, np.inf, -np.inf, -3.0, np.nan, np.nan] + [0.5] * 100, np.float32)
    c, st, _ = run_kernel(torch.from_numpy(x).cuda(), [(0, x.size)])
    check_segment(x, (0, x.size), c[0], st[0], 'non-finite')
    assert st[0][5] == 3 and st[0][6] == 2 and st[0][2] == 103 and st[0][0] == -3.0 and st[0][1] == 2.0
    assert math.isfinite(st[0][3]) and math.isfinite(st[0][4])


def test_no_segments_is_a_no_op_and_bad_tables_are_refused():
    lib = _lib()
    x = torch.zeros(64, device='cuda')
    out = torch.full((8,), 5, dtype=torch.int64, device='cuda')
    lib.call('tg_tf_histogram_f32', lib.ptr(x), 64, _segs([]), 0, None, None, None, None, 0, lib.cur_stream())
    torch.cuda.synchronize()
    assert bool((out == 5).all())
    assert lib.call('tg_tf_histogram_workspace_bytes', _segs([]), 0) >= 0
    ws = torch.zeros(1 << 12, dtype=torch.int64, device='cuda')
    cnt = torch.zeros(NL, dtype=torch.int64, device='cuda')
    st = torch.zeros(NS, dtype=torch.float64, device='cuda')
    for bad in ([(60, 5)], [(-1, 4)], [(0, 65)]):         # refused on the host, before anything is launched
        with pytest.raises(lib.TgError):
            lib.call('tg_tf_histogram_f32', lib.ptr(x), 64, _segs(bad), 1, lib.ptr(_limits_dev()), lib.ptr(cnt), lib.ptr(st), lib.ptr(ws),
                     ws.numel() * 8, lib.cur_stream())
    with pytest.raises(lib.TgError, match='workspace'):
        lib.call('tg_tf_histogram_f32', lib.ptr(x), 64, _segs([(0, 64)]), 1, lib.ptr(_limits_dev()), lib.ptr(cnt), lib.ptr(st), lib.ptr(ws),
                 8, lib.cur_stream())


# ------------------------------------------------------------------------------------------------------------- the training loop
def _train(tmp_path, hook=None, **over):
    from tg import runtime
    from Training.Train_goodGAN import Train
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10
    from Input_Pipeline.syntheticDataset import syntheticDataset
    runtime.set_context(None)
    torch.cuda.empty_cache()
    kw = dict(TRAIN_SIZE=8 * 3, EPOCHS=1, SAMPLE_DIR=None, SAMPLE_SIZE=16, USE_HIP_GRAPH=None, EXEC_MODE='plan', SUMMARY=True, NUM_LABEL=40,
              SEED=5)
    np.random.seed(11)                                     # Train.train draws sample_z from NumPy's global generator
    tr = Train(G.make_config(SMALL, **dict(kw, **over)), str(tmp_path / 'Log'), None, comments='summary')
    sample_y = np.eye(10, dtype=np.float32)[np.arange(16) % 10]
    if hook is not None:
        hook(tr)
    hist = tr.train(syntheticDataset, Good_GAN_cifar10, sample_y)
    return tr, hist, sample_y


def _train_run_dir(tmp_path):
    rd = os.path.join(str(tmp_path / 'Log'), 'train')
    return os.path.join(rd, os.listdir(rd)[0])


def _state(tr):
    out = {}
    for net, st in tr.cx.stores.items():
        for k in ('p', 'm', 'v', 's', 'g'):
            out[net + '/' + k] = getattr(st, k).detach().cpu().numpy().copy()
        if st.ema is not None:
            out[net + '/ema'] = st.ema.detach().cpu().numpy().copy()
        out[net + '/step'] = st.step.detach().cpu().numpy().copy()
    out['rng'] = tr.cx.rng.state.detach().cpu().numpy().copy()
    return out


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    on = tmp_path_factory.mktemp('on')
    drawn = []

    def keep_samples(tr):                                  # what Train.sample returned to the epoch tail
        orig = tr.sample
        tr.sample = lambda z, y: drawn.append(orig(z, y).copy()) or drawn[-1]

    tr, hist, sample_y = _train(on, hook=keep_samples, SUMMARY_HISTOGRAM=True, SUMMARY_IMAGE=True)
    assert len(drawn) == 1 and drawn[0].shape == (16, 32, 32, 3)
    samples = drawn[0]
    stores = {net: {nm: (st.get(nm), st.get(nm, 'grad')) for nm in st.names(True)} for net, st in tr.cx.stores.items()}
    state = _state(tr)
    off = tmp_path_factory.mktemp('off')
    tr2, hist2, _ = _train(off)
    return dict(on=on, off=off, hist=hist, hist2=hist2, stores=stores, samples=samples, state=state, state2=_state(tr2))


def test_one_epoch_writes_histograms_and_images_into_one_event(trained):
    import read_events as RE
    rdir = _train_run_dir(trained['on'])
    files = [f for f in os.listdir(rdir) if f.startswith('events.out.tfevents.')]
    assert len(files) == 1
    events = RE.read_events(os.path.join(rdir, files[0]))
    assert len(events) == 2 and events[0].get('file_version') == 'brain.Event:2'         # file_version + ONE event for the epoch
    ev = events[1]
    assert ev['step'] == 1 and set(ev['scalars']) == {'g_loss', 'd_loss', 'c_loss'}
    names = [nm for net in ('discriminator', 'good_generator', 'classifier') for nm in trained['stores'][net]]
    assert len(names) > 30
    assert set(ev['histograms']) == set(names) | {'gradients/' + nm for nm in names}
    flat = {nm: vg for net in trained['stores'].values() for nm, vg in net.items()}
    for nm in names:
        for tag, arr in ((nm, flat[nm][0]), ('gradients/' + nm, flat[nm][1])):
            h, ref = ev['histograms'][tag], R.histogram(arr)
            assert h['num'] == arr.size and sum(h['bucket']) == h['num'], tag
            bl, b = R.compress(R.LIMITS, ref['counts'])
            assert h['bucket_limit'] == bl and h['bucket'] == b, tag
            assert h['min'] == ref['min'] and h['max'] == ref['max'], tag
            n = arr.size
            assert abs(h['sum'] - ref['sum']) <= n * 2.0 ** -53 * ref['abs_sum'], tag
            assert abs(h['sum_squares'] - ref['sum_squares']) <= n * 2.0 ** -53 * ref['sum_squares'], tag
    assert any(flat[nm][1].any() for nm in names)                                        # the gradients are the last iteration's, not zeros
    assert set(ev['images']) == {'generated/image/0', 'generated/image/1'}
    for i in range(2):
        im = ev['images']['generated/image/%d' % i]
        assert (im['height'], im['width'], im['colorspace']) == (32, 32, 3)
        got = R.decode_png(im['encoded'])
        h, w, c, raw = RE.decode_png(im['encoded'])
        assert (h, w, c) == (32, 32, 3) and raw == got.tobytes()
        np.testing.assert_array_equal(got, R.normalize_float_image(trained['samples'][i]))
    lines = open(os.path.join(rdir, 'history.csv')).read().splitlines()
    assert lines[0] == 'step,g_loss,d_loss,c_loss' and len(lines) == 2 and len(lines[1].split(',')) == 4


def test_the_flags_change_nothing_the_run_computes(trained):
    """plan mode, same seed: weights, gradients, optimiser slots, running state, EMA, step counts and the Philox state are bit-identical with
    the summaries on and off — they only read, and no draw moves."""
    assert trained['hist'][0]['d_loss'] == trained['hist2'][0]['d_loss'] and trained['hist'][0]['c_loss'] == trained['hist2'][0]['c_loss']
    a, b = trained['state'], trained['state2']
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    import read_events as RE
    rdir = _train_run_dir(trained['off'])
    ev = RE.read_events(os.path.join(rdir, [f for f in os.listdir(rdir) if f.startswith('events')][0]))
    assert len(ev) == 2 and not ev[1]['histograms'] and not ev[1]['images'] and set(ev[1]['scalars']) == {'g_loss', 'd_loss', 'c_loss'}


def test_a_nan_in_a_weight_stops_the_epoch_before_its_event(tmp_path):
    lib = _lib()
    nm = 'good_generator/gg_h0_lin/gg_h0_lin/kernel'

    def poison_at_the_tail(tr):                            # sync_running_state runs in the epoch tail, before the summaries
        orig = tr.sync_running_state

        def poisoned():
            orig()
            tr.cx.stores['good_generator'].value(nm)[5] = float('nan')
        tr.sync_running_state = poisoned

    with pytest.raises(lib.TgError, match="Nan in summary histogram for: " + nm):
        _train(tmp_path, hook=poison_at_the_tail, SUMMARY_HISTOGRAM=True)
    import read_events as RE
    rdir = _train_run_dir(tmp_path)
    files = [f for f in os.listdir(rdir) if f.startswith('events')]
    ev = RE.read_events(os.path.join(rdir, files[0]))
    assert len(ev) == 1 and ev[0].get('file_version') == 'brain.Event:2'                # nothing was written for that epoch
    assert not os.path.exists(os.path.join(rdir, 'history.csv'))


def test_histograms_while_a_plan_is_held_and_non_finite_values(tmp_path):
    lib = _lib()
    tr = G.fresh_trainer(G.make_config(SMALL, USE_HIP_GRAPH=None, EXEC_MODE='plan', SEED=3))
    from oracle import step_cifar10 as S
    tr.feed(S.synth_batch(7, dict(S.SIZES, **SMALL)))
    for _ in range(3):
        tr.sample_latent()
        tr.train_iteration()
    h = tr.histograms('value')
    st = tr.cx.stores['classifier']
    nm = st.names(True)[0]
    np.testing.assert_array_equal(h[nm]['counts'], R.histogram(st.get(nm))['counts'])
    assert set(tr.histograms('ema')) == set(st.names(True))                            # only the classifier has shadows
    before = tr.cx.stores['discriminator'].p.clone()
    tr.sample_latent()
    tr.train_iteration()                                                               # the held plan still replays
    assert not torch.equal(before, tr.cx.stores['discriminator'].p)
    from Training.Summary import Summary
    s = Summary(str(tmp_path), None, log_type='train', log_comments='')
    s.add_summary({'histogram': dict.fromkeys(h)})
    st.value(nm)[1] = float('nan')
    bad = tr.histograms('value', nets=('classifier',))
    assert bad[nm]['nan'] == 1 and bad[nm]['num'] == st.value(nm).numel() - 1
    with pytest.raises(lib.TgError, match="Nan in summary histogram for: " + nm):
        s.write({}, 1, histograms=bad)
    st.value(nm)[1] = float('inf')
    with pytest.raises(lib.TgError, match="Infinity in summary histogram for: " + nm):
        s.write({}, 1, histograms=tr.histograms('value', nets=('classifier',)))
    import read_events as RE
    files = [f for f in os.listdir(s.log_dir) if f.startswith('events')]
    assert len(RE.read_events(os.path.join(s.log_dir, files[0]))) == 1                  # the file_version record only: no event was written
    assert not os.path.exists(os.path.join(s.log_dir, 'history.csv'))
