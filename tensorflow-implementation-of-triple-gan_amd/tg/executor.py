"""How one training iteration is launched, and the replay state that goes with it.  An iteration is a list of segments (Train._segments);
the same kernels on the same operands are issued 'eager' (one stream), with 'overlap' (Context.wgrad_on_side: a second stream), from a
native launch 'plan' recorded off the two-stream run (tg/plan.py) or as a replayed hip'graph' — resolve_launch says which, AutoMode
measures the last two for config.EXEC_MODE = 'auto', StepExecutor does it.  Host logic only: importable without a device."""
import contextlib
import ctypes as C
import gc
import os
import time

import torch

from . import dist as tgdist
from . import lib
from .plan import Plan


def resolve_launch(mode, use_graph, replayable, graphs_allowed, auto_pick):
    """(config.EXEC_MODE, train_iteration's use_graph merged with config.USE_HIP_GRAPH: None | False | True, the RNG is a PhiloxRNG,
    tg.dist.graphs_allowed(), callable -> 'plan' | 'graph') -> (how, graph_refused).  how: 'eager' | 'overlap' | 'plan' | 'graph'; the side
    stream is on for 'overlap' and 'plan'.  graph_refused: graphs were asked for beside a backend that forbids captures.  auto_pick is
    called (once) only where 'auto' may really choose; an unknown mode launches like 'eager'."""
    if mode == 'auto':
        if use_graph is None and replayable:
            mode = auto_pick() if graphs_allowed else 'plan'    # torch's RCCL process group forbids captures (tg/dist.py): plans are plain launches
        else:
            mode = 'graph' if use_graph else 'overlap'
    want_graph = bool(replayable and (mode == 'graph' if use_graph is None else use_graph))      # injected draws: nothing to replay
    if want_graph and graphs_allowed:
        return 'graph', False
    if mode == 'plan':
        return ('overlap' if want_graph or not replayable else 'plan'), want_graph
    return (mode if mode == 'overlap' else 'eager'), want_graph


# ---- EXEC_MODE = 'auto': which way of launching is faster for THIS workload on THIS host is measured, not assumed
AUTO_TIMED = 5                     # timed iterations per block
AUTO_SETTLE = 3                    # untimed iterations in front of each timed block (allocations, lazily loaded code objects, recorded launch plans)
AUTO_BLOCKS = 3                    # blocks per candidate, alternating: a candidate's time is its FASTEST block
AUTO_ITERS = 2 * AUTO_BLOCKS * (AUTO_SETTLE + AUTO_TIMED) + 1


def auto_schedule(n, settle, timed, blocks):
    """iteration n of the measurement -> (candidate it runs, a timing window opens at it, the previous block's window closes at it, it is
    the deciding iteration).  blocks x ['plan' block, 'graph' block], a block = settle untimed + timed timed iterations; the last window
    closes at the deciding iteration n = 2 * blocks * (settle + timed), whose candidate is void (the decision replaces it)."""
    b, k = divmod(n, settle + timed)
    return ('plan', 'graph')[b % 2], k == settle and b < 2 * blocks, k == 0 and b > 0, (b, k) == (2 * blocks, 0)


class AutoMode(object):
    """Both candidates compute the same numbers; which is faster depends on the workload: the CIFAR-10 / SVHN steps (15 ms of large
    kernels) gain 2.5 - 4 % from the second-stream overlap that only eager launches can have, the MNIST step (2.7 ms in ~300 launches of
    a few microseconds) is bound by the host's launch rate when launched eagerly (4.1 ms) and needs graph replay.  One per graph key,
    stepped by next() along auto_schedule (the first graph block captures); a candidate's time is its fastest block — the first block of a
    fresh process on a fresh machine measures page-ins of library code, not the candidate (seen: 28 ms for a 14.6 ms step) — then the
    faster candidate for good.  clock() (device synchronisation + host time) is called twice per block in the first AUTO_ITERS iterations,
    never afterwards; decide({candidate: seconds}) -> (pick, {candidate: seconds}) is tg.dist.decide_together."""

    def __init__(self, clock, decide):
        self.clock, self.decide = clock, decide
        self.n = 0                                  # iterations of the measurement so far
        self.t0 = None                              # clock() at the start of the open timing window
        self.times = {'plan': [], 'graph': []}      # seconds per iteration of each candidate's timed blocks
        self.pick = self.best = None                # the decision and the timings it was made from

    def next(self):
        """the candidate this iteration runs: 'plan' | 'graph'."""
        if self.pick is not None:
            return self.pick
        mode, opens, closes, decides = auto_schedule(self.n, AUTO_SETTLE, AUTO_TIMED, AUTO_BLOCKS)
        self.n += 1
        if closes:
            self.times['graph' if mode == 'plan' else 'plan'].append((self.clock() - self.t0) / AUTO_TIMED)
        if decides:
            # replicas decide together (every rank reaches this point in the same iteration): the slowest rank's time per candidate
            self.pick, self.best = self.decide({k: min(v) for k, v in self.times.items()})
            return self.pick
        if opens:
            self.t0 = self.clock()
        return mode

    def chosen(self):
        """(mode, {candidate: seconds per iteration}) once decided, else (None, partial timings)."""
        return self.pick, (dict(self.best) if self.best is not None else {k: min(v) for k, v in self.times.items() if v})


class Replay(object):
    """the replay state of one graph key: per segment the hipGraphExec handle and the launch plan (None until captured / recorded; sized by
    the first iteration), whether an iteration has run — graphs are captured from a mode's SECOND iteration on, the first one allocates its
    buffers eagerly — and whether a two-stream one has (its events and side-stream workspaces exist: plans may be recorded)."""

    def __init__(self, auto):
        self.graphs, self.plans = [], []
        self.ran = self.ran_two_stream = False
        self.auto = auto


class StepExecutor(object):
    def __init__(self, cx):
        self.cx = cx
        clock = lambda: (torch.cuda.synchronize(), time.perf_counter())[1]
        decide = lambda times: tgdist.decide_together(times, cx.device)
        self.replay = {key: Replay(AutoMode(clock, decide)) for key in ('full', 'pre')}
        self.exposed = None            # [(mark before, mark after)] of the waits for gradient buckets while measure_exposed(True)

    def run(self, segs, key, how):
        """one iteration: segs = Train._segments(), launched `how` resolve_launch said."""
        cx, st = self.cx, self.replay[key]
        if not st.graphs:
            st.graphs, st.plans = [None] * len(segs), [None] * len(segs)
        graphs, plans = (st.graphs if how == 'graph' else None), (st.plans if how == 'plan' else None)
        # a segment's plan is recorded while it runs eagerly in the SECOND two-stream iteration of its kind (the first one allocates the
        # buffers and records the multi-launch plans of the RNG / filter preparation / statistics arena) and replayed from then on
        plan_ready = plans is not None and st.ran_two_stream
        pending = []
        cx.prep_cache = {}                              # filter layouts stay valid between a network's optimiser steps
        cx.plan_tag = key
        # second-stream overlap (Context.wgrad_on_side): only beside eager launches — a captured graph with cross-stream edges replays slower
        # than the single chain on ROCm 7.2 (measured rounds 1 and 3), so graph replay stays one chain
        side_was = cx.wgrad_side
        cx.wgrad_side = on = how in ('overlap', 'plan')
        try:
            for i, (fn, grads, wait) in enumerate(segs):
                if wait:                                    # this segment opens with an optimiser step: its network's buckets must be in
                    mark = self._mark() if (self.exposed is not None and pending) else None
                    for wk in pending:
                        tgdist.wait_(wk)
                    if mark is not None:
                        self.exposed.append((mark, self._mark()))
                    pending = []
                if graphs is not None and graphs[i] is not None:
                    lib.call('tg_graph_launch', graphs[i], cx.stream)
                elif plans is not None and plans[i] is not None:
                    plans[i].replay()
                elif plan_ready:
                    plans[i] = self.record_plan(fn)
                else:
                    fn()
                if grads is not None and tgdist.active():
                    pending.append(tgdist.allreduce_sum_async_(grads))
        finally:
            cx.prep_cache = None
            cx.join_wgrad_side()
            cx.wgrad_side = side_was
        st.ran = True
        st.ran_two_stream |= on

    @contextlib.contextmanager
    def _frozen(self):
        """what a graph capture and a plan recording share: both keep device addresses, so no buffer may be born inside (cx.capturing)
        and ParamStore.extend must not re-allocate the stores from now on."""
        cx = self.cx
        for st in cx.stores.values():
            st.frozen = True
        was, cx.capturing = cx.capturing, True
        try:
            yield
        finally:
            cx.capturing = was

    def record_plan(self, fn):
        """run segment `fn` eagerly on the two streams while every launch and event operation is appended to a native launch plan
        (tg/plan.py, include/tg_plan.h); returns the plan."""
        plan = Plan([self.cx.torch_stream.cuda_stream, self.cx.side_stream.cuda_stream])
        with self._frozen(), plan.recording():
            fn()
        return plan

    def capture(self, segs, key):
        """Once an iteration of `key` has run: record every segment that has no hipGraph yet as one — all of them back to back, nothing
        launched and no collective issued in between.  Only reached when tg.dist.graphs_allowed(): the exchange backends used with graphs
        (rccl-direct, gloo) have no thread that touches HIP events behind the trainer's back, so a capture cannot be disturbed (tg/dist.py
        docstring)."""
        cx, st = self.cx, self.replay[key]
        if not st.ran or all(g is not None for g in st.graphs):
            return
        cx.prep_cache = {}
        cx.plan_tag = key
        # No garbage collection inside a capture window.  A collector pass can free a PINNED host tensor of an earlier owner (an input
        # pipeline's staging slots): torch's caching host allocator then records an event on every stream the tensor was copied on — torch
        # hands out streams from a pool of 32, so in a long-lived process that can be THIS trainer's capturing stream — and its next query of
        # that captured event fails with "operation not permitted when stream is capturing", which invalidates the capture (every later
        # launch: "operation failed due to a previous error during capture").  Seen once in a full test session (round 4); mechanism
        # reproduced in tools/micro/capture_pinned_free.py.
        gc_was = gc.isenabled()
        if not os.environ.get('TG_DEBUG_CAPTURE_GC'):      # (test hook: leave the collector running, to show what the guard is for)
            gc.collect()
            gc.disable()
        try:
            for i, (fn, _grads, _wait) in enumerate(segs):
                if st.graphs[i] is not None:
                    continue
                lib.call('tg_graph_begin_capture', cx.stream)
                try:
                    with self._frozen():
                        if os.environ.get('TG_DEBUG_CAPTURE_SLEEP'):          # test hook: widen the capture window
                            time.sleep(float(os.environ['TG_DEBUG_CAPTURE_SLEEP']))
                        fn()
                finally:
                    h = C.c_void_p()
                    lib.call('tg_graph_end_capture', cx.stream, C.byref(h))
                st.graphs[i] = h
        finally:
            cx.prep_cache = None
            if gc_was:
                gc.enable()

    # ---- how much of the gradient exchange is NOT hidden behind the backward pass (bench.py `exchange_exposed_ms`)
    def _mark(self):
        """a point of the launch stream's timeline: a timing event on a GPU (the waits are stream-side, the host does not block),
        the host clock otherwise (gloo's wait blocks the host)."""
        if self.cx.device.type == 'cuda':
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream())
            return e
        return time.perf_counter()

    def measure_exposed(self, on=True):
        """start (or stop) bracketing every wait for a network's gradient buckets in run()."""
        self.exposed = [] if on else None

    def exposed_ms(self):
        """total time the launch stream spent stalled in those waits since measure_exposed(True) — the exchange time the backward
        pass did not hide.  Synchronises the device."""
        if not self.exposed:
            return 0.0
        if isinstance(self.exposed[0][0], float):
            return 1e3 * sum(b - a for a, b in self.exposed)
        torch.cuda.synchronize()
        return float(sum(a.elapsed_time(b) for a, b in self.exposed))
