"""tf.summary.histogram on the device: the host side of tg_tf_histogram_f32 (include/tg_kernels.h, csrc/summary.hip).

One call bins every variable of one flat ParamStore buffer — a segment table of {element offset, count} pairs, so the 32-float alignment
padding between variables is never read — and ONE device->host copy brings back the bucket counts and statistics of all of them.  The
1 551 bucket limits are TensorFlow's, built once on the host by the library (tg_tf_histogram_limits) and kept on the device."""
import ctypes as C

import numpy as np

from . import lib

N_LIMITS = 1551
N_STATS = 8              # min, max, num, sum, sum_squares, #NaN, #Inf, 0

_LIMITS = None


def limits():
    """TensorFlow's bucket limits as a read-only float64 array [1551] (host; needs no GPU)."""
    global _LIMITS
    if _LIMITS is None:
        buf = (C.c_double * N_LIMITS)()
        lib.call('tg_tf_histogram_limits', buf, N_LIMITS)
        a = np.array(buf, np.float64)
        a.setflags(write=False)
        _LIMITS = a
    return _LIMITS


def segment_table(segments):
    """[(element offset, count)] -> the HOST int64 pair array tg_tf_histogram_f32 takes."""
    arr = (C.c_int64 * max(2 * len(segments), 2))()
    for k, (off, n) in enumerate(segments):
        arr[2 * k], arr[2 * k + 1] = int(off), int(n)
    return arr


def workspace_bytes(segs, nseg):
    return lib.call('tg_tf_histogram_workspace_bytes', segs, int(nseg))


class StoreHistograms(object):
    """the histograms of a fixed segment table over any flat fp32 device buffer that holds it (a store's p, g, ema): the table, the
    workspace and the result buffer are made once."""

    def __init__(self, segments, device):
        import torch
        self.nseg = len(segments)
        self.segs = segment_table(segments)
        self.extent = max([off + n for off, n in segments] + [0])
        self.device = device
        self.limits_dev = torch.from_numpy(np.array(limits())).to(device)
        need = workspace_bytes(self.segs, self.nseg)
        self.workspace_bytes = need
        self.workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=device)
        # counts [nseg][1551] int64, then stats [nseg][8] float64: one buffer, one copy to the host
        self.result = torch.empty(max(self.nseg, 1) * (N_LIMITS + N_STATS), dtype=torch.int64, device=device)

    def launch(self, buf, stream):
        """enqueue the launch sequence on `stream` (the results land in self.result)."""
        import torch
        if buf.dtype != torch.float32 or buf.numel() < self.extent:
            raise lib.TgError("histograms: a float32 buffer of at least %d elements is needed, got %s[%d]" % (self.extent, buf.dtype, buf.numel()))
        counts = self.result[:self.nseg * N_LIMITS]
        stats = self.result[self.nseg * N_LIMITS:]
        lib.call('tg_tf_histogram_f32', lib.ptr(buf), buf.numel(), self.segs, self.nseg, lib.ptr(self.limits_dev), lib.ptr(counts), lib.ptr(stats),
                 lib.ptr(self.workspace), self.workspace_bytes, stream)

    def fetch(self):
        """-> (counts int64 [nseg, 1551], stats float64 [nseg, 8]) on the host: ONE device->host copy (synchronises the current stream)."""
        host = self.result.cpu().numpy()
        counts = host[:self.nseg * N_LIMITS].reshape(self.nseg, N_LIMITS)
        stats = host[self.nseg * N_LIMITS:self.nseg * (N_LIMITS + N_STATS)].view(np.float64).reshape(self.nseg, N_STATS)
        return counts, stats

    def run(self, buf, stream):
        self.launch(buf, stream)
        return self.fetch()


def as_dicts(names, counts, stats):
    """{name: {min, max, num, sum, sum_squares, limits, counts, nan, inf}} of one StoreHistograms result (limits: the shared table)."""
    lim = limits()
    return {nm: dict(min=float(s[0]), max=float(s[1]), num=float(s[2]), sum=float(s[3]), sum_squares=float(s[4]), limits=lim, counts=c,
                     nan=int(s[5]), inf=int(s[6])) for nm, c, s in zip(names, counts, stats)}
