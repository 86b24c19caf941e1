"""Launch traces of tg/ops.py without a GPU (helper of tests/test_ops_launch_trace.py).

libtg_hip.so loads on a machine without a device and its host-side queries answer there (descriptor builders, tg_*_supported,
tg_*_workspace_bytes, tg_wgrad_splits, tg_plan_signature).  `Tracer` runs the ops on a Context whose buffers are CPU tensors and
replaces tg.lib.call: every launch entry point (tg.plan.signature(name) is not None) is RECORDED instead of issued, every query goes to
the library.  A recorded launch is [name, argument, ...] without the stream: scalars as they are, descriptors / segment tables / job
structs field by field, and every pointer as '<buffer>+<byte offset>' where <buffer> is the workspace key of Context.buffers that holds
it ('<phase>/<tag><call-site number>'), 'zarena:<phase>' (the fp64 accumulator arena of a phase), or the label of a tensor the case
made itself (kernel, bias, kernel_grad, ...).  The buffer names pin the call-site counter order a captured graph or launch plan relies on.

CASES maps a case name to its Case; `python tests/launch_trace.py --record` rewrites tests/golden/ops_launch_traces.json from the
package in the tree (a deliberate change of route, argument or launch order: say so in the commit message)."""
import contextlib
import ctypes as C
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tensorflow-implementation-of-triple-gan_amd")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ops_launch_traces.json")
if __name__ == '__main__':
    for _p in (ROOT, PKG):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from tg import geom, grad_penalty, lib, ops, plan, runtime      # noqa: E402
from tg.runtime import Act, Context, InjectedRNG, ParamStore, pad32      # noqa: E402

# the MFMA launches Context.mfma_dtype = 'bf16' switches to their bf16-operand entry points (a case states the f32 names)
BF16_OF = {n: n[:-3] + 'bf16' for n in ('tg_igemm_f32', 'tg_igemm_multi_f32', 'tg_igemm_colsum_f32', 'tg_igemm_actsum_f32', 'tg_igemm_bnstat_f32',
                                        'tg_igemm_bnbwdstat_f32', 'tg_wgrad_f32', 'tg_igemm_labels_f32')}


class TraceContext(Context):
    """Context without a device: CPU buffers, a null stream, and markers in the trace where the second stream would be entered / joined."""

    def __init__(self, trace, mfma_dtype='f32', act_dtype='f32', wgrad_side=False):      # Context.__init__ minus the device setup
        self.trace = trace
        self.device = torch.device('cpu')
        self.wgrad_side, self._wgrad_side_pending = wgrad_side, False
        self.plan_tag, self.prep_plans, self._planned, self._prep_rec = None, {}, set(), None
        self.tail_jobs, self.prep_cache, self.state_replay = [], None, None
        self._zarena, self._events, self._side_depth, self._phase_depth = {}, {}, 0, 0
        self.buffers, self.stores, self.tape, self.phase, self.counter = {}, {}, None, 'init', 0
        self.scopes, self.rng_scope, self.rng_counters = [], '', {}
        self.rng = InjectedRNG({}, self.device)
        self.train_nets = set()
        self.mfma_dtype, self.act_dtype, self.bf16_act_layers = mfma_dtype, act_dtype, set()

    @property
    def stream(self):
        return C.c_void_p(0)

    @contextlib.contextmanager
    def wgrad_on_side(self):
        if not self.wgrad_side or self._side_depth or not self._phase_depth:
            yield
            return
        self.trace.append('side-begin')
        self._side_depth += 1
        try:
            yield
        finally:
            self._side_depth -= 1
            self._wgrad_side_pending = True
            self.trace.append('side-end')

    def join_wgrad_side(self):
        if self._wgrad_side_pending:
            self.trace.append('join')
            self._wgrad_side_pending = False


class Tracer(object):
    launches = True            # False on a runner that computes the case without launches (tests/ops_reference.py): no trace to assert on
    names_buffers = True       # False on a runner whose trace holds every pointer as an opaque '<ptr>' (tests/test_gpu_ops_routes.py)

    def __init__(self, **ctx_kw):
        self.trace = []
        self.cx = TraceContext(self.trace, **ctx_kw)
        self.labels = {}
        self._real_call = None

    # ---- installation ----------------------------------------------------------------------------
    def install(self, monkeypatch):
        """replace tg.lib.call and the current context until `monkeypatch` is undone (pytest's fixture, or pytest.MonkeyPatch.context())."""
        plan.signature('tg_fill_f32')                      # binds the library through the real lib.call path first
        self._real_call = lib.call
        monkeypatch.setattr(lib, 'call', self.call)
        monkeypatch.setattr(runtime, '_CTX', self.cx)
        return self

    def call(self, name, *args):
        kinds = plan.signature(name)
        if kinds is None:
            return self._real_call(name, *args)            # a host-side query: the library answers
        assert len(args) == len(kinds) + 1, (name, len(args), len(kinds) + 1)
        self.trace.append([name] + [self._arg(k, a) for k, a in zip(kinds, args)])
        return 0

    # ---- the case's own tensors ------------------------------------------------------------------
    def t(self, label, numel, dtype=torch.float32):
        assert label not in self.labels, label
        self.labels[label] = torch.zeros(max(int(numel), 1), dtype=dtype)
        return self.labels[label][:int(numel)]

    def mark(self, text):
        self.trace.append(text)

    @contextlib.contextmanager
    def phase(self, name='p', train=True, record=True):
        """one solver run training the network 'net' (or only applying it)."""
        with self.cx.phase_scope(name, train_nets=('net',) if train else (), record=record), self.cx.variable_scope('net'):
            yield self.cx

    def x(self, n, h, w, c, requires_grad=True, dtype='f32'):
        return self.cx.new_act(n, h, w, c, pad32(c), requires_grad=requires_grad, tag='x', dtype=dtype)

    def seed(self, y, ld=None):
        """the loss head's write into y's gradient buffer (ld: a channel stride other than y's, the padded dlogits of a narrow logit)."""
        if ld is None:
            return self.cx.grad_of(y)
        y.grad = Act(self.cx.scratch('dlogits', y.rows * ld), y.n, y.h, y.w, y.c, ld)
        y.grad.contribs = 1
        return y.grad

    # ---- encoding --------------------------------------------------------------------------------
    def _regions(self):
        for key, t in self.cx.buffers.items():
            yield key, t
        for ph, za in self.cx._zarena.items():
            if za['buf'] is not None:
                yield 'zarena:' + ph, za['buf']
        for key, t in self.labels.items():
            yield key, t
        for sname, st in self.cx.stores.items():
            for k, t in st._full.items():
                yield 'store:%s.%s' % (sname, k), t

    def _ptr(self, p):
        p = getattr(p, 'value', p)
        if p is None:
            return None
        for key, t in self._regions():
            lo = t.data_ptr()
            if lo <= p < lo + t.numel() * t.element_size():
                return '%s+%d' % (key, p - lo)
        raise AssertionError("launch argument %#x lies in no workspace buffer and no labelled tensor of the case" % p)

    def _struct(self, s):
        out = {}
        for fname, ftype in s._fields_:
            v = getattr(s, fname)
            if ftype is C.c_void_p:
                out[fname] = self._ptr(v)
            elif isinstance(v, C.Array):
                out[fname] = list(v)
            else:
                out[fname] = v
        return out

    def _arg(self, kind, v):
        if kind == 'f':
            return float(getattr(v, 'value', v))
        if kind == 'i':
            return int(getattr(v, 'value', v))
        if isinstance(v, C.Structure):
            return self._struct(v)
        if isinstance(v, C.Array):
            return [self._struct(e) if isinstance(e, C.Structure) else int(e) for e in v]
        return self._ptr(v)


class Case(object):
    def __init__(self, fn, expect, absent, ctx_kw):
        self.fn, self.ctx_kw = fn, ctx_kw
        bf16 = ctx_kw.get('mfma_dtype') == 'bf16'
        self.expect = [BF16_OF.get(n, n) if bf16 else n for n in expect]
        self.absent = list(absent)


CASES = {}


def case(expect=(), absent=(), variants=None):
    """register fn(tr) under its name (+ suffix per variant: {suffix: TraceContext keywords}).  expect / absent: launch names the route
    must / must not issue (f32 names: a bf16-MFMA variant expects the bf16 entry points)."""
    def deco(fn):
        for sfx, kw in (variants or {'': {}}).items():
            CASES[fn.__name__ + sfx] = Case(fn, expect, absent, kw)
        return fn
    return deco


BOTH_MFMA = {'': {}, '_bf16mfma': dict(mfma_dtype='bf16')}
BOTH_SIDE = {'': {}, '_side': dict(wgrad_side=True)}

# A second, ragged shape per case body (odd n, h != w, unequal segments, channel counts that are no multiple of the tile where the route
# admits them): the bodies below take it as an optional argument, the default is the recorded shape.  tests/test_ops_reference.py runs
# every entry through the Tracer and check_route (a shape that falls off its route fails there, without a GPU), tests/test_gpu_ops_routes.py
# holds the numbers of both shapes to float64.  Keys are the bodies' names: every variant of a body takes the same second shape.
RAGGED = {}


def ragged(*shape):
    def deco(fn):
        RAGGED[fn.__name__] = shape
        return fn
    return deco


def names(trace):
    return [e if isinstance(e, str) else e[0] for e in trace]


# ================================================================== layer arguments

def conv_kw(tr, c_in, c_out, k, p='', bias=True, wn=False, mobn=False, grads=True, bias_grad=True):
    """(kernel, bias, keywords) of one ops.conv2d layer with labelled variables '<p>kernel', '<p>bias', ..."""
    t = k * k
    kernel = tr.t(p + 'kernel', t * c_in * c_out)
    b = tr.t(p + 'bias', c_out) if (bias and not mobn) else None
    kw = {}
    if grads:
        kw['kernel_grad'] = tr.t(p + 'kernel_grad', t * c_in * c_out)
        if b is not None and bias_grad:
            kw['bias_grad'] = tr.t(p + 'bias_grad', c_out)
    if wn:
        kw['wn'] = (tr.t(p + 'g', c_out), tr.t(p + 'g_grad', c_out) if grads else None)
    if mobn:
        kw['mobn'] = (tr.t(p + 'b', c_out), tr.t(p + 'b_grad', c_out) if grads else None, tr.t(p + 'pop_mean', c_out))
    return kernel, b, kw


def conv(tr, x, c_out, k=3, stride=1, padding='SAME', p='', bias=True, wn=False, mobn=False, grads=True, bias_grad=True, **kw):
    kernel, b, lkw = conv_kw(tr, x.c, c_out, k, p, bias, wn, mobn, grads, bias_grad)
    lkw.update(kw)
    return ops.conv2d(x, kernel, b, c_out, k, stride, padding, **lkw)


def bn(tr, x, p='bn.', grads=True, **kw):
    c = x.c
    return ops.batch_norm_train(x, tr.t(p + 'gamma', c), tr.t(p + 'beta', c), tr.t(p + 'mm', c), tr.t(p + 'mv', c), 1e-5, 0.9,
                                gamma_grad=tr.t(p + 'gamma_grad', c) if grads else None, beta_grad=tr.t(p + 'beta_grad', c) if grads else None, **kw)


def fwd_bwd(tr, build, seed_ld=None):
    """one training solver run: y = build(), the loss head's gradient into y, the backward pass."""
    with tr.phase() as cx:
        y = build()
        tr.seed(y, seed_ld)
        cx.backward()


# ================================================================== conv2d: forward routes (each with its backward)

@case(expect=['tg_filter_prep_f32', 'tg_igemm_f32', 'tg_actgrad_bias_f32', 'tg_wgrad_f32', 'tg_igemm_multi_f32', 'tg_filter_grad_tail_multi_f32'],
      absent=['tg_wn_scale_f32', 'tg_actgrad_f32'], variants=BOTH_MFMA)
@ragged(3, 6, 10, 42, 138)
def conv_plain(tr, shape=(4, 8, 8, 32, 64)):
    fwd_bwd(tr, lambda: conv(tr, tr.x(*shape[:4]), shape[4], act='lrelu'))


@case(expect=['tg_wn_scale_f32', 'tg_filter_prep_f32', 'tg_igemm_f32', 'tg_actgrad_bias_f32', 'tg_wgrad_f32', 'tg_filter_grad_tail_multi_f32'])
@ragged(5, 7, 9, 74, 48)
def conv_wn_bias(tr, shape=(4, 8, 8, 32, 64)):
    fwd_bwd(tr, lambda: conv(tr, tr.x(*shape[:4]), shape[4], wn=True, act='lrelu'))


@case(expect=['tg_filter_prep_f32', 'tg_igemm_f32', 'tg_actgrad_bias_f32', 'tg_wgrad_f32', 'tg_igemm_multi_f32'])
@ragged(5, 1, 1, 74, 48)
def conv_dense(tr, shape=(4, 1, 1, 64, 32)):
    fwd_bwd(tr, lambda: conv(tr, tr.x(*shape[:4]), shape[4], k=1, act='relu'))


@case(expect=['tg_igemm_f32', 'tg_colstats_f32', 'tg_wgrad_f32', 'tg_igemm_multi_f32'], absent=['tg_actgrad_f32', 'tg_actgrad_bias_f32'])
def conv_narrow_logit_padded_dlogits(tr):
    """D's logit: one stored column (n_store_ld); the loss head writes dlogits with the padded channel stride and the backward uses it in place."""
    def build():
        y = conv(tr, tr.x(4, 1, 1, 64), 1, k=1, n_store_ld=(1, 1))
        assert (y.c, y.ld) == (1, 1)
        return y
    fwd_bwd(tr, build, seed_ld=32)


def _packed_shape():
    """the smallest (n, h, w, c_in, c_out) tg_conv3x3_packed_supported accepts"""
    for h in range(1, 9):
        for w in range(1, 33):
            if lib.call('tg_conv3x3_packed_supported', 2, h, w, 3, 32):
                return 2, h, w, 3, 32
    raise AssertionError("no packed shape")


@case(expect=['tg_conv3x3_packed_fwd_f32', 'tg_actgrad_bias_f32', 'tg_conv3x3_packed_wgrad_f32', 'tg_igemm_multi_f32'],
      absent=['tg_igemm_f32', 'tg_wgrad_f32', 'tg_igemm_labels_f32'], variants=BOTH_SIDE)
def conv_packed(tr):
    n, h, w, ci, co = _packed_shape()
    fwd_bwd(tr, lambda: conv(tr, tr.x(n, h, w, ci), co, act='lrelu'))


@case(expect=['tg_conv3x3_packed_fwd_f32', 'tg_conv3x3_packed_wgrad_f32'], absent=['tg_igemm_f32', 'tg_igemm_labels_f32', 'tg_cond_concat_f32'])
def conv_packed_concat(tr):
    n, h, w, ci, co = _packed_shape()
    lab = tr.t('labels', n * 10)

    def build():
        y = conv(tr, tr.x(n, h, w, ci), co, act='lrelu', concat=(lab, 10))
        assert y.labels is not None and y.ld == 64
        return ops.cond_concat(y, lab, 10)
    fwd_bwd(tr, build)


@case(expect=['tg_igemm_labels_f32', 'tg_actgrad_bias_f32', 'tg_wgrad_f32'], absent=['tg_igemm_f32', 'tg_cond_concat_f32'], variants=BOTH_MFMA)
@ragged(3, 6, 10, 42, 96)
def conv_labels(tr, shape=(4, 8, 8, 32, 64)):
    lab = tr.t('labels', shape[0] * 10)
    fwd_bwd(tr, lambda: ops.cond_concat(conv(tr, tr.x(*shape[:4]), shape[4], act='lrelu', concat=(lab, 10)), lab, 10))


@case(expect=['tg_igemm_f32', 'tg_cond_concat_f32'], absent=['tg_igemm_labels_f32'])
@ragged(3, 5, 7, 74, 138)
def conv_concat_not_fused(tr, shape=(4, 8, 8, 32, 48)):
    """c_out is no multiple of 32: the convolution cannot append the label channels, cond_concat runs its own launch"""
    lab = tr.t('labels', shape[0] * 10)
    fwd_bwd(tr, lambda: ops.cond_concat(conv(tr, tr.x(*shape[:4]), shape[4], act='lrelu', concat=(lab, 10)), lab, 10))


@case(expect=['tg_igemm_bnstat_f32', 'tg_bn_train_apply_f32', 'tg_bn_train_bwd_act_f32', 'tg_wgrad_f32', 'tg_igemm_multi_f32'],
      absent=['tg_igemm_f32', 'tg_bn_train_f32', 'tg_actgrad_f32', 'tg_actgrad_bias_f32', 'tg_bn_train_bwd_f32'], variants=BOTH_MFMA)
@ragged(4, 8, 16, 42, 64, (1, 3))
def conv_bnstat_into_batch_norm(tr, shape=(4, 8, 8, 32, 64, (2, 2))):
    """conv2d(bn_stats) -> batch_norm_train through bn_sums; backward: the batch norm folds act' and the bias gradient (the convolution's
    BiasSums offer), the convolution takes its gradient as the pre-activation gradient (what the batch norm left in Act.taken)"""
    segs = list(shape[5])
    fwd_bwd(tr, lambda: bn(tr, conv(tr, tr.x(*shape[:4]), shape[4], act='relu', bn_stats=True, segments=segs), segments=segs))


@case(expect=['tg_igemm_f32', 'tg_bn_train_f32', 'tg_bn_train_bwd_act_f32'], absent=['tg_igemm_bnstat_f32', 'tg_bn_train_apply_f32'])
def conv_bnstat_falls_back(tr):
    """16-row segments: tg_igemm_colsum_supported says no"""
    def build():
        x = tr.x(2, 4, 4, 32)
        assert not geom.colsum_supported(geom.conv_fwd(2, 4, 4, 32, 64, 3, 1, 'SAME'), [16, 16])
        return bn(tr, conv(tr, x, 64, act='relu', bn_stats=True, segments=[1, 1]), segments=[1, 1])
    fwd_bwd(tr, build)


BF16_STORE = {'': dict(mfma_dtype='bf16', act_dtype='bf16')}


@case(expect=['tg_bn_train_bf16', 'tg_igemm_bf16in_bf16', 'tg_wgrad_bf16in_bf16', 'tg_igemm_bnbwdstat_bf16'], absent=['tg_igemm_bf16', 'tg_wgrad_bf16'],
      variants=BF16_STORE)
@ragged(3, 8, 32, 64, 128)
def conv_bf16_input_plain(tr, shape=(4, 8, 8, 32, 64)):
    def build():
        h = bn(tr, tr.x(*shape[:4]), out_bf16=True)
        assert h.dtype == 'bf16'
        return conv(tr, h, shape[4], act='relu')
    fwd_bwd(tr, build)


@case(expect=['tg_igemm_bnstat_bf16', 'tg_bn_train_apply_bf16', 'tg_igemm_bnstat_bf16in_bf16', 'tg_bn_train_apply_f32', 'tg_wgrad_bf16in_bf16',
              'tg_igemm_bnbwdstat_bf16'], variants=BF16_STORE)
@ragged(3, 8, 32, 32, 64, 128)
def conv_bf16_input_bnstat(tr, shape=(4, 8, 8, 32, 32, 64)):
    def build():
        h = bn(tr, conv(tr, tr.x(*shape[:4]), shape[4], p='l1.', act='relu', bn_stats=True), p='bn1.', out_bf16=True)
        assert h.dtype == 'bf16'
        return bn(tr, conv(tr, h, shape[5], p='l2.', act='relu', bn_stats=True), p='bn2.')
    fwd_bwd(tr, build)


# ---- mean-only batch norm

@case(expect=['tg_wn_scale_f32', 'tg_igemm_colsum_f32', 'tg_mobn_apply_f32', 'tg_mobn_bwd_f32', 'tg_wgrad_f32', 'tg_igemm_multi_f32'],
      absent=['tg_igemm_f32', 'tg_mobn_finalize_f32', 'tg_mobn_center_f32'], variants=BOTH_MFMA)
@ragged(4, 8, 16, 42, 64, (1, 3))
def mobn_fused(tr, shape=(4, 8, 8, 32, 32, (2, 2))):
    fwd_bwd(tr, lambda: conv(tr, tr.x(*shape[:4]), shape[4], wn=True, mobn=True, act='lrelu', segments=list(shape[5])))


@case(expect=['tg_igemm_colsum_f32', 'tg_mobn_apply_pool_f32', 'tg_maxpool2_bwd_actsum_f32', 'tg_mobn_center_f32'],
      absent=['tg_mobn_apply_f32', 'tg_maxpool2_fwd_f32', 'tg_mobn_bwd_f32'])
@ragged(3, 4, 12, 42, 32)
def mobn_fused_pool(tr, shape=(4, 8, 8, 32, 32)):
    n, h, w, _, co = shape
    mask = tr.t('keep', n * (h // 2) * (w // 2) * co)
    fwd_bwd(tr, lambda: conv(tr, tr.x(*shape[:4]), co, wn=True, mobn=True, act='lrelu', pool=(mask, 1.25)))


@case(expect=['tg_igemm_colsum_f32', 'tg_mobn_apply_f32', 'tg_maxpool2_fwd_f32', 'tg_maxpool2_bwd_actsum_f32', 'tg_mobn_center_f32'],
      absent=['tg_mobn_apply_pool_f32'])
def mobn_pool_odd_map(tr, shape=(4, 7, 7, 32, 32)):
    n, h, w, _, co = shape
    mask = tr.t('keep', n * (h // 2) * (w // 2) * co)
    fwd_bwd(tr, lambda: conv(tr, tr.x(*shape[:4]), co, wn=True, mobn=True, act='lrelu', pool=(mask, 1.25)))


@case(expect=['tg_igemm_colsum_f32', 'tg_mobn_apply_f32', 'tg_igemm_actsum_f32', 'tg_mobn_center_f32', 'tg_mobn_bwd_f32'], variants=BOTH_MFMA)
@ragged(3, 8, 16, 42, 64, 32)
def mobn_two_layers_grad_fused(tr, shape=(4, 8, 8, 32, 32, 64)):
    """the second layer's input-gradient launch applies the first layer's act' and sums the columns (ActSums in Act.taken -> tg_mobn_center_f32)"""
    def build():
        h = conv(tr, tr.x(*shape[:4]), shape[4], p='l1.', wn=True, mobn=True, act='lrelu')
        return conv(tr, h, shape[5], p='l2.', wn=True, mobn=True, act='lrelu')
    fwd_bwd(tr, build)


@case(expect=['tg_igemm_f32', 'tg_colstats_f32', 'tg_mobn_finalize_f32', 'tg_seg_scale_shift_act_f32', 'tg_mobn_bwd_f32', 'tg_igemm_multi_f32'],
      absent=['tg_igemm_colsum_f32'])
@ragged(3, 6, 10, 42, 64)
def mobn_unfused_stride2(tr, shape=(4, 8, 8, 32, 32)):
    """stride 2: no fused statistics; the input gradient is one launch over the four parity descriptors"""
    fwd_bwd(tr, lambda: conv(tr, tr.x(*shape[:4]), shape[4], stride=2, wn=True, mobn=True, act='lrelu'))
    multi = [e for e in tr.trace if e[0] == 'tg_igemm_multi_f32']
    assert not tr.launches or (len(multi) == 1 and multi[0][2] == 4 and len(multi[0][1]) == 4)


@case(expect=['tg_igemm_f32', 'tg_mobn_finalize_f32', 'tg_seg_scale_shift_act_f32', 'tg_mobn_bwd_finalize_f32', 'tg_seg_actgrad_shift_f32'],
      absent=['tg_igemm_colsum_f32', 'tg_mobn_bwd_f32'])
@ragged(3, 6, 10, 42, 138, (1, 2))
def mobn_unfused_c48(tr, shape=(4, 8, 8, 32, 48, (4,))):
    fwd_bwd(tr, lambda: conv(tr, tr.x(*shape[:4]), shape[4], wn=True, mobn=True, act='lrelu', segments=list(shape[5]) if len(shape[5]) > 1 else None))


@case(expect=['tg_igemm_f32', 'tg_mobn_finalize_f32', 'tg_mobn_bwd_finalize_f32', 'tg_seg_actgrad_shift_f32'], absent=['tg_igemm_colsum_f32', 'tg_mobn_bwd_f32'])
def mobn_generic_backward_c544(tr):
    fwd_bwd(tr, lambda: conv(tr, tr.x(64, 1, 1, 32), 544, k=1, wn=True, mobn=True, act='lrelu'))


@case(expect=['tg_igemm_f32', 'tg_mobn_finalize_f32', 'tg_seg_scale_shift_act_f32'], absent=['tg_igemm_colsum_f32', 'tg_colstats_f32'])
def mobn_eval(tr):
    with tr.phase(train=False, record=False):
        conv(tr, tr.x(4, 8, 8, 32, requires_grad=False), 32, wn=True, mobn=True, grads=False, act='lrelu', train=False)


@case(expect=['tg_igemm_colsum_f32', 'tg_mobn_apply_f32', 'tg_mobn_bwd_f32'])
def mobn_zarena_replay(tr):
    """the same solver run twice: the second takes its fp64 accumulators from the phase's arena at the same call-site numbers"""
    for k in (1, 2):
        tr.mark('pass %d' % k)
        kernel, b, kw = conv_kw(tr, 32, 32, 3, p='r%d.' % k, wn=True, mobn=True)
        with tr.phase() as cx:
            y = ops.conv2d(tr.x(4, 8, 8, 32), kernel, b, 32, 3, 1, 'SAME', act='lrelu', **kw)
            tr.seed(y)
            cx.backward()


# ================================================================== conv2d: the remaining backward routes

@case(expect=['tg_actgrad_f32', 'tg_colstats_f32', 'tg_wgrad_f32'], absent=['tg_actgrad_bias_f32'])
def bwd_actgrad_colstats_wide(tr):
    fwd_bwd(tr, lambda: conv(tr, tr.x(4, 1, 1, 32), 1056, k=1, act='lrelu'))


@case(expect=['tg_actgrad_f32', 'tg_wgrad_f32'], absent=['tg_actgrad_bias_f32', 'tg_colstats_f32'])
@ragged(3, 6, 10, 42, 138)
def bwd_actgrad_no_bias_gradient(tr, shape=(4, 8, 8, 32, 64)):
    fwd_bwd(tr, lambda: conv(tr, tr.x(*shape[:4]), shape[4], act='lrelu', bias_grad=False))


def _bn_then(tr, consumers, shape=(4, 8, 8, 32, 64)):
    def build():
        h = bn(tr, tr.x(*shape[:4]))
        ys = [conv(tr, h, shape[4], p='c%d.' % k, act='lrelu') for k in range(consumers)]
        for y in ys[:-1]:
            tr.seed(y)
        return ys[-1]
    return build


@case(expect=['tg_bn_train_f32', 'tg_igemm_bnbwdstat_f32', 'tg_bn_train_bwd_f32'], absent=['tg_igemm_multi_f32'], variants=BOTH_MFMA)
@ragged(3, 8, 16, 64, 138)
def bwd_bnbwdstat(tr, shape=(4, 8, 8, 32, 64)):
    fwd_bwd(tr, _bn_then(tr, 1, shape))
    assert not tr.launches or [e[15] for e in tr.trace if e[0] == 'tg_bn_train_bwd_f32'] == [2]             # the epilogue's sums, marked as taken


@case(expect=['tg_igemm_bnbwdstat_f32', 'tg_igemm_multi_f32', 'tg_bn_train_bwd_f32'])
def bwd_bnbwdstat_invalidated(tr):
    """a second consumer adds to the batch norm's output gradient: the first launch's sums are dropped, the batch norm takes its own"""
    fwd_bwd(tr, _bn_then(tr, 2))
    assert not tr.launches or [e[15] for e in tr.trace if e[0] == 'tg_bn_train_bwd_f32'] == [0]


@case(expect=['tg_igemm_actsum_f32', 'tg_igemm_multi_f32', 'refused'], absent=['tg_mobn_center_f32'])
def bwd_single_consumer_refusal(tr):
    def build():
        h = conv(tr, tr.x(4, 8, 8, 32), 32, p='l1.', wn=True, mobn=True, act='lrelu')
        ya = conv(tr, h, 64, p='a.', act='lrelu')
        tr.seed(ya)
        return conv(tr, h, 64, p='b.', act='lrelu')
    try:
        fwd_bwd(tr, build)
    except lib.TgError as e:
        assert 'written by 2 consumers' in str(e)
        tr.mark('refused')


# ================================================================== filter_grad

def _fg(tr, shape, wn, defer=True, in_phase=True):
    n, h, w, ci, co, k = shape
    cx = tr.cx
    desc = geom.conv_wgrad(n, h, w, ci, co, k, 1, 'SAME')
    x, dpre = tr.t('x', n * h * w * ci), tr.t('dpre', n * h * w * co)
    dst = tr.t('dst', k * k * ci * co)
    w4 = (tr.t('v', k * k * ci * co), tr.t('g', co), tr.t('dv', k * k * ci * co), tr.t('dg', co)) if wn else None
    if not in_phase:
        ops.filter_grad(desc, x, dpre, k * k, ci, co, dst, wn=w4, defer=defer)
        return desc
    with tr.phase():
        ops.filter_grad(desc, x, dpre, k * k, ci, co, dst, wn=w4, defer=defer)
        cx.flush_tails()
    return desc


FG_VARIANTS = {s + w: dict(wgrad_side=bool(s)) for s in ('', '_side') for w in ('_plain', '_wn')}


@case(expect=['tg_wgrad_f32', 'tg_filter_grad_tail_multi_f32'], absent=['tg_slab_reduce_f32', 'tg_wn_bwd_f32'], variants=FG_VARIANTS)
@ragged(3, 6, 10, 64, 96, 3)
def filter_grad_deferred(tr, shape=(4, 8, 8, 32, 64, 3)):
    _fg(tr, shape, wn=_wn_variant(tr))


@case(expect=['tg_wgrad_f32', 'tg_slab_reduce_f32'], absent=['tg_filter_grad_tail_multi_f32'], variants=FG_VARIANTS)
def filter_grad_wide(tr):
    d = _fg(tr, (64, 8, 8, 32, 32, 3), wn=_wn_variant(tr))
    assert geom.wgrad_splits(d) >= 32


@case(expect=['tg_wgrad_f32', 'tg_slab_reduce_f32'], absent=['tg_filter_grad_tail_multi_f32', 'side-begin'], variants=FG_VARIANTS)
@ragged(5, 7, 9, 32, 160, 3)
def filter_grad_immediate(tr, shape=(4, 8, 8, 32, 64, 3)):
    _fg(tr, shape, wn=_wn_variant(tr), defer=False)


@case(expect=['tg_wgrad_f32', 'tg_slab_reduce_f32'], absent=['tg_filter_grad_tail_multi_f32', 'side-begin'], variants=FG_VARIANTS)
def filter_grad_no_phase(tr):
    _fg(tr, (4, 8, 8, 32, 64, 3), wn=_wn_variant(tr), in_phase=False)


@case(expect=['tg_wgrad_f32', 'tg_filter_grad_tail_multi_f32'], absent=['tg_slab_reduce_f32'], variants=BOTH_SIDE)
def filter_grad_large(tr):
    """>= 2^34 multiply-adds: beside the input-gradient chain only when the second stream is on"""
    _fg(tr, (512, 8, 8, 256, 256, 3), wn=False)


def _wn_variant(tr):
    return '_wn' in tr.variant                             # the case's name as registered (run_case)


# ================================================================== deconv2d

def deconv(tr, x, c_out, p='', wn=False, grads=True, **kw):
    kernel, bias = tr.t(p + 'kernel', 25 * c_out * x.c), tr.t(p + 'bias', c_out)
    if grads:
        kw.update(kernel_grad=tr.t(p + 'kernel_grad', 25 * c_out * x.c), bias_grad=tr.t(p + 'bias_grad', c_out))
    if wn:
        kw['wn'] = (tr.t(p + 'g', c_out), tr.t(p + 'g_grad', c_out) if grads else None)
    return ops.deconv2d(x, kernel, bias, c_out, **kw)


@case(expect=['tg_deconv_merge_prep_f32', 'tg_filter_prep_f32', 'tg_igemm_f32', 'tg_actgrad_bias_f32', 'tg_wgrad_f32', 'tg_filter_grad_tail_multi_f32'],
      absent=['tg_igemm_multi_f32', 'tg_deconv5x5s2_narrow_wgrad_f32', 'tg_deconv5x5s2_narrow_dgrad_f32'])
@ragged(3, 3, 5, 42, 5)
def deconv_merged(tr, shape=(2, 4, 4, 32, 3)):
    fwd_bwd(tr, lambda: deconv(tr, tr.x(*shape[:4]), shape[4], act='tanh'))


@case(expect=['tg_deconv_merge_prep_f32', 'tg_igemm_f32', 'tg_actgrad_bias_f32', 'tg_wgrad_f32'], absent=['tg_igemm_multi_f32'])
def deconv_merged_narrow_out(tr):
    def build():
        y = deconv(tr, tr.x(2, 4, 4, 32), 3, act='tanh', narrow_out=True)
        assert y.ld == 3
        return y
    fwd_bwd(tr, build)


@case(expect=['tg_deconv_merge_prep_f32', 'tg_igemm_f32', 'tg_deconv5x5s2_narrow_wgrad_f32', 'tg_deconv5x5s2_narrow_dgrad_f32'],
      absent=['tg_wgrad_f32', 'tg_filter_prep_f32'], variants={'': {}, '_side': dict(wgrad_side=True), '_wn': {}, '_wn_side': dict(wgrad_side=True)})
def deconv_narrow_backward(tr):
    assert lib.call('tg_deconv5x5s2_narrow_supported', 2, 4, 16, 3, 32) and not lib.call('tg_deconv5x5s2_narrow_supported', 2, 3, 16, 3, 32)
    fwd_bwd(tr, lambda: deconv(tr, tr.x(2, 4, 16, 32), 3, act='tanh', narrow_out=True, wn=_wn_variant(tr)))


@case(expect=['tg_filter_prep_f32', 'tg_igemm_multi_f32', 'tg_actgrad_bias_f32', 'tg_wgrad_f32', 'tg_igemm_f32', 'tg_filter_grad_tail_multi_f32'],
      absent=['tg_deconv_merge_prep_f32'], variants=BOTH_MFMA)
@ragged(3, 3, 5, 42, 48)
def deconv_unmerged(tr, shape=(2, 4, 4, 64, 32)):
    fwd_bwd(tr, lambda: deconv(tr, tr.x(*shape[:4]), shape[4], act='relu'))


@case(expect=['tg_wn_scale_tab_f32', 'tg_filter_prep_f32', 'tg_igemm_multi_f32', 'tg_wgrad_f32', 'tg_slab_reduce_f32', 'tg_wn_bwd_tab_f32'],
      absent=['tg_filter_grad_tail_multi_f32'])
@ragged(3, 5, 3, 74, 48)
def deconv_weight_normalised(tr, shape=(2, 4, 4, 64, 32)):
    fwd_bwd(tr, lambda: deconv(tr, tr.x(*shape[:4]), shape[4], act='relu', wn=True))


@case(expect=['tg_igemm_multi_f32', 'tg_bn_train_f32', 'tg_bn_train_bwd_act_f32', 'tg_wgrad_f32'], absent=['tg_actgrad_bias_f32', 'tg_actgrad_f32'])
@ragged(3, 3, 5, 42, 64)
def deconv_into_batch_norm(tr, shape=(2, 4, 4, 64, 32)):
    fwd_bwd(tr, lambda: bn(tr, deconv(tr, tr.x(*shape[:4]), shape[4], act='relu')))


@case(expect=['tg_actgrad_f32', 'tg_igemm_f32'], absent=['tg_actgrad_bias_f32', 'tg_wgrad_f32'])
def deconv_applied_only(tr):
    """the network is applied, not trained: an input gradient without filter or bias gradients"""
    with tr.phase(train=False) as cx:
        y = deconv(tr, tr.x(2, 4, 4, 64), 32, act='relu', grads=False)
        tr.seed(y)
        cx.backward()


# ================================================================== filter prep: cache and plan

@case(expect=['tg_filter_prep_f32', 'tg_wn_scale_f32', 'tg_filter_prep_multi_f32', 'tg_igemm_f32'])
def filter_prep_plan(tr):
    """one two-layer solver run (its first layer applied twice) three times inside a training step: the recording pass, the
    tg_filter_prep_multi_f32 pass, and one more"""
    cx = tr.cx
    cx.plan_tag = 'full'
    k1, b1, kw1 = conv_kw(tr, 32, 64, 3, p='l1.', wn=True, bias_grad=False)      # no bias gradient: no fp64 accumulator, whose buffer is the
    k2, b2, kw2 = conv_kw(tr, 64, 32, 3, p='l2.', bias_grad=False)               # phase's arena from the second pass on (mobn_zarena_replay)
    for k in (1, 2, 3):
        tr.mark('pass %d' % k)
        cx.prep_cache = {}
        with tr.phase() as _:
            x = tr.x(4, 8, 8, 32)
            h = ops.conv2d(x, k1, b1, 64, 3, 1, 'SAME', act='lrelu', **kw1)
            y = ops.conv2d(h, k2, b2, 32, 3, 1, 'SAME', act='lrelu', **kw2)
            tr.seed(ops.conv2d(x, k1, b1, 64, 3, 1, 'SAME', act='lrelu', **kw1))
            tr.seed(y)
            cx.backward()
    cx.prep_cache = None


# ================================================================== grad_penalty's shared pieces

@case(expect=['tg_wn_scale_f32', 'tg_filter_prep_f32', 'tg_wgrad_f32', 'tg_slab_reduce_f32', 'tg_wn_bwd_f32', 'tg_colstats_f32'])
def grad_penalty_rows(tr):
    cx = tr.cx
    rows = [grad_penalty.weight_normed('wnrow', 64), grad_penalty.plain('plainrow', 64)]
    heads = [grad_penalty.weight_normed('wnhead', 1), grad_penalty.plain('plainhead', 1)]
    specs = []
    for r, shape in [(r, (3, 3, 32, 64)) for r in rows] + [(r, (64, 1)) for r in heads]:
        specs += [(r.w, shape, True), (r.b, (r.cout,), True)] + ([(r.g, (r.cout,), True)] if r.g else [])
    st = cx.stores['discriminator'] = ParamStore('discriminator', specs, cx.device)
    grad = tr.t('gpgrad', st.n_p)
    with cx.phase_scope('wgan_gp', record=False):
        t_in, dpre, tp = cx.new_act(4, 8, 8, 32, 32), cx.new_act(4, 8, 8, 64, 64), cx.new_act(4, 1, 1, 64, 64)
        desc = geom.conv_wgrad(4, 8, 8, 32, 64, 3, 1, 'SAME')
        for r in rows:
            tr.mark(r.w)
            grad_penalty._filter_prep(cx, st, r, 9, 32)
            grad_penalty._filter_grad(cx, st, grad, r, desc, t_in, dpre, 9, 32)
        for r in heads:
            tr.mark(r.w)
            grad_penalty._filter_prep(cx, st, r, 1, 64)
            grad_penalty._filter_grad(cx, st, grad, r, None, tp, None, 1, 64)


# ================================================================== the remaining ops

@case(expect=['tg_colstats_f32', 'tg_mobn_finalize_f32', 'tg_seg_scale_shift_act_f32', 'tg_mobn_bwd_finalize_f32', 'tg_seg_actgrad_shift_f32', 'tg_actgrad_f32'])
@ragged(5, 3, 7, 42)
def op_mean_only_batch_norm(tr, shape=(4, 4, 4, 32)):
    for train in (True, False):
        tr.mark('train %s' % train)
        p = 't%d.' % train
        c = shape[3]
        fwd_bwd(tr, lambda: ops.mean_only_batch_norm(tr.x(*shape), tr.t(p + 'pop', c), tr.t(p + 'b', c), tr.t(p + 'b_grad', c), train=train))


@case(expect=['tg_bn_eval_finalize_f32', 'tg_seg_scale_shift_act_f32'])
def op_batch_norm_eval(tr):
    with tr.phase(train=False, record=False):
        ops.batch_norm_eval(tr.x(4, 4, 4, 32), tr.t('gamma', 32), tr.t('beta', 32), tr.t('mm', 32), tr.t('mv', 32), 1e-5)


@case(expect=['tg_bn_train_f32', 'tg_bn_moving_update_f32', 'tg_bn_train_bwd_f32'])
@ragged(5, 3, 7, 42, (2, 3))
def op_batch_norm_train(tr, shape=(4, 4, 4, 32, (2, 2))):
    """stand-alone (its own statistics launch), relu_input, in a kept forward pass whose moving-statistics update is replayed"""
    with tr.phase() as cx:
        replay = []
        with cx.sub_tape(('net',), replay=replay) as tape:
            y = bn(tr, tr.x(*shape[:4]), relu_input=True, segments=list(shape[4]))
        for fn in replay:
            fn()
        tr.seed(y)
        cx.run_tape(tape)


@case(expect=['tg_actgrad_f32', 'tg_cond_concat_f32'])
def op_scale_mask_cond_concat(tr):
    """dropout as its own launch; dropout deferred into cond_concat; cond_concat alone, its gradient aliased or copied"""
    lab = tr.t('labels', 4 * 10)
    for k, (defer, second) in enumerate([(False, False), (True, False), (None, False), (None, True)]):
        tr.mark('variant %d' % k)
        mask = tr.t('keep%d' % k, 4 * 4 * 4 * 32)
        with tr.phase() as cx:
            x = tr.x(4, 4, 4, 32)
            h = ops.activation(x, 'lrelu')
            if second:
                tr.seed(h)                                                  # another consumer wrote h's gradient first: no alias
            out = ops.cond_concat(h if defer is None else ops.scale_mask(h, mask, 1.25, defer=defer), lab, 10)
            tr.seed(out)
            cx.backward()


@case(expect=['tg_pad_add_f32', 'tg_im2col3x3_add_f32', 'tg_argmax_onehot_f32', 'tg_copy2d_f32', 'tg_copy_multi_f32', 'tg_fill_f32', 'tg_bn_finalize_f32'])
def op_forward_only(tr):
    with tr.phase(train=False, record=False) as cx:
        x = cx.new_act(4, 4, 4, 3, 3, tag='x')
        ops.pad_add(x, tr.t('noise', 4 * 4 * 4 * 3), 32)
        ops.im2col3x3_add(x, tr.t('noise2', 4 * 4 * 4 * 3))
        ops.argmax_onehot(tr.x(4, 1, 1, 10, requires_grad=False), 10)
        a, b = tr.t('a', 256), tr.t('b', 256)
        ops.copy2d(a, 32, 8, b, 16, 4, 16)
        ops.copy_rows(a, 64, b, 100)
        ops.copy_many([(a, 0, b, 10), (a, 16, b, 0), (a, 32, b, 20)])
        ops.moments_normalize(tr.x(4, 4, 4, 32, requires_grad=False), 1e-8, 2.0)
        ops.batch_norm_moments(tr.x(4, 4, 4, 32, requires_grad=False), tr.t('scale', 32), tr.t('beta', 32), tr.t('pm', 32), tr.t('pv', 32), 1e-5, 0.9, False)


@case(expect=['tg_maxpool2_fwd_f32', 'tg_maxpool2_bwd_f32', 'tg_gmaxpool_fwd_f32', 'tg_gmaxpool_bwd_f32', 'tg_gavgpool_concat_f32', 'tg_gavgpool_bwd_f32',
              'tg_act_f32', 'tg_actgrad_f32', 'tg_pad_add_f32'])
def op_pooling_pointwise(tr):
    lab = tr.t('labels', 4 * 10)
    for k, build in enumerate([lambda x: ops.maxpool2_dropout(x, tr.t('keep', 4 * 2 * 2 * 32), 1.25), ops.global_maxpool,
                               lambda x: ops.global_avgpool_concat(x, lab, 10), ops.global_avgpool, lambda x: ops.activation(x, 'tanh'),
                               lambda x: ops.add_noise(x, tr.t('noise', 4 * 4 * 4 * 32)),
                               lambda x: ops.view(ops.reshape(ops.global_avgpool(x), 1, 1, 1, 4 * 32), 2, 2, 32),
                               lambda x: ops.concat_batch([ops.activation(x, 'relu'), ops.activation(x, 'sigmoid')])]):
        tr.mark('op %d' % k)
        fwd_bwd(tr, lambda: build(tr.x(4, 4, 4, 32)))


@case(expect=['tg_colstats_f32', 'tg_bn_finalize_f32', 'tg_seg_scale_shift_act_f32', 'tg_bn_bwd_finalize_f32', 'tg_bn_bwd_apply_f32'])
@ragged(5, 3, 7, 42)
def op_batch_norm_moments(tr, shape=(4, 4, 4, 32)):
    c = shape[3]
    for k, grads in enumerate((True, False)):
        tr.mark('grads %s' % grads)
        p = 'm%d.' % k
        fwd_bwd(tr, lambda: ops.batch_norm_moments(tr.x(*shape), tr.t(p + 'scale', c), tr.t(p + 'beta', c), tr.t(p + 'pm', c), tr.t(p + 'pv', c),
                                                   1e-5, 0.9, True, scale_grad=tr.t(p + 'sg', c) if grads else None,
                                                   beta_grad=tr.t(p + 'bg', c) if grads else None))


@case(expect=['tg_igemm_f32', 'tg_minibatch_disc_fwd_f32', 'tg_minibatch_disc_bwd_f32', 'tg_pad_add_f32', 'tg_wgrad_f32'])
def op_minibatch_discrimination(tr):
    for k, cat in enumerate((True, False)):
        tr.mark('concat_input %s' % cat)
        p = 'm%d.' % k
        fwd_bwd(tr, lambda: ops.minibatch_discrimination(tr.x(4, 1, 1, 64), tr.t(p + 'w', 64 * 8 * 4), tr.t(p + 'b', 8), 8, 4, w_grad=tr.t(p + 'w_grad', 64 * 8 * 4),
                                                         b_grad=tr.t(p + 'b_grad', 8), concat_input=cat))


@case(expect=['tg_colstats_f32'])
def op_colstats(tr):
    with tr.phase(train=False, record=False):
        a, b = tr.t('a', 64 * 32), tr.t('b', 64 * 32)
        ops.colstats(1, a, 32, None, 0, 64, 32, [32, 32])
        ops.colstats(3, a, 32, b, 32, 64, 32, [64], act='lrelu', s1=tr.t('s1', 36), s2=tr.t('s2', 36))


# ================================================================== a second writer of one gradient (ops._write_grad)

def second_writer(tr, name, build, launch=None, via=None, shape=(2, 4, 4, 32)):
    """One solver run `name`: h = x (or via(x)) feeds the op under test, build(h) -> its output[s], and an activation recorded AFTER it, whose
    backward therefore runs first and is the first writer of h's gradient.  The op's own backward launch (`launch`) must then name a
    scratch buffer, not the gradient buffer, and tg_add_f32 add that scratch to the gradient; launch None: an alias of the same channel
    stride, added from where it lies in the consumer's gradient buffer."""
    tr.mark(name)
    start = len(tr.trace)
    with tr.phase(name) as cx:
        x = tr.x(*shape)
        h = x if via is None else via(x)
        outs = build(h)
        tr.seed(ops.activation(h, 'lrelu'))
        for o in outs if isinstance(outs, (list, tuple)) else [outs]:
            tr.seed(o)
        cx.backward()
    if tr.launches and tr.names_buffers:
        seg = [e for e in tr.trace[start:] if not isinstance(e, str)]
        gbuf = [e[8] for e in seg if e[0] == 'tg_actgrad_f32' and re.match(r'%s/g\d+\+0$' % name, e[8])][0]      # the first writer's destination
        add = [e for e in seg if e[0] == 'tg_add_f32'][-1]
        assert add[1] == add[2] == gbuf and add[3] != gbuf, add
        if launch is None:
            assert re.match(r'%s/g\d+\+0$' % name, add[3]), add
        else:
            own = [e for e in seg if e[0] == launch and add[3] in e[1:]]      # the one launch that names the scratch buffer
            assert add[3].startswith(name + '/gxp') and len(own) == 1 and gbuf not in own[0][1:], (own, add)


@case(expect=['tg_act_f32', 'tg_actgrad_f32', 'tg_add_f32'])
def second_writer_pointwise(tr, shape=(2, 4, 4, 32)):
    second_writer(tr, 'activation', lambda x: ops.activation(x, 'tanh'), 'tg_actgrad_f32', shape=shape)
    second_writer(tr, 'scale_mask', lambda x: ops.scale_mask(x, tr.t('keep', x.rows * x.c), 1.25), 'tg_actgrad_f32', shape=shape)


@case(expect=['tg_act_f32', 'tg_actgrad_f32', 'tg_add_f32'])
def second_writer_pointwise_c48(tr):
    """48 channels in a channel stride of 64: the scratch buffer and the sum carry the zero padding"""
    second_writer_pointwise(tr, (2, 4, 4, 48))


@case(expect=['tg_maxpool2_bwd_f32', 'tg_gmaxpool_bwd_f32', 'tg_gavgpool_bwd_f32', 'tg_add_f32'], absent=['tg_maxpool2_bwd_actsum_f32'])
def second_writer_pooling(tr):
    second_writer(tr, 'maxpool2', lambda x: ops.maxpool2_dropout(x, tr.t('keep', 2 * 2 * 2 * 32), 1.25), 'tg_maxpool2_bwd_f32')
    second_writer(tr, 'gmaxpool', ops.global_maxpool, 'tg_gmaxpool_bwd_f32')
    second_writer(tr, 'gavgpool', lambda x: ops.global_avgpool_concat(x, tr.t('labels', 2 * 10), 10), 'tg_gavgpool_bwd_f32')


@case(expect=['tg_seg_actgrad_shift_f32', 'tg_bn_train_bwd_f32', 'tg_bn_bwd_apply_f32', 'tg_add_f32'], absent=['tg_bn_train_bwd_act_f32'])
def second_writer_norms(tr):
    second_writer(tr, 'mobn', lambda x: ops.mean_only_batch_norm(x, tr.t('pop', 32), tr.t('b', 32), tr.t('b_grad', 32)), 'tg_seg_actgrad_shift_f32')
    second_writer(tr, 'bn', lambda x: bn(tr, x), 'tg_bn_train_bwd_f32')
    second_writer(tr, 'moments', lambda x: ops.batch_norm_moments(x, tr.t('m.scale', 32), tr.t('m.beta', 32), tr.t('m.pm', 32), tr.t('m.pv', 32), 1e-5, 0.9,
                                                                  True, scale_grad=tr.t('m.sg', 32), beta_grad=tr.t('m.bg', 32)), 'tg_bn_bwd_apply_f32')


@case(expect=['tg_igemm_multi_f32', 'tg_igemm_f32', 'tg_deconv5x5s2_narrow_dgrad_f32', 'tg_add_f32'])
def second_writer_deconv(tr):
    """the generic input gradient (tg_igemm_f32 on the transposed filter) and the K-packed one of the 3-channel image layer, whose smallest map is 4x16"""
    second_writer(tr, 'generic', lambda x: deconv(tr, x, 32, p='g.', act='relu'), 'tg_igemm_f32')
    second_writer(tr, 'narrow', lambda x: deconv(tr, x, 3, p='n.', act='tanh', narrow_out=True), 'tg_deconv5x5s2_narrow_dgrad_f32', shape=(2, 4, 16, 32))


@case(expect=['tg_igemm_labels_f32', 'tg_cond_concat_f32', 'tg_actgrad_f32', 'tg_add_f32'])
def second_writer_aliases(tr):
    """the closures whose contribution is a view of the consumer's gradient buffer: added from where it lies, or, where the channel strides
    differ (cond_concat behind an op that reads its gradient through a stride), copied into scratch first; and cond_concat's copying paths"""
    lab = tr.t('labels', 2 * 10)
    second_writer(tr, 'reshape', lambda x: ops.reshape(x, 2, 1, 1, 4 * 4 * 32))
    second_writer(tr, 'add_noise', lambda x: ops.add_noise(x, tr.t('noise', x.rows * x.c)))
    second_writer(tr, 'concat_batch', lambda x: ops.concat_batch([x, tr.x(3, 4, 4, 32)]))
    second_writer(tr, 'concat_alias', lambda h: ops.cond_concat(h, lab, 10), via=lambda x: conv(tr, x, 32, p='a.', act='lrelu', concat=(lab, 10)))
    second_writer(tr, 'concat_strided', lambda h: ops.cond_concat(h, lab, 10), 'tg_actgrad_f32', via=lambda x: ops.activation(x, 'relu'))
    second_writer(tr, 'concat_copy', lambda x: ops.cond_concat(x, lab, 10), 'tg_actgrad_f32')
    second_writer(tr, 'concat_dropout', lambda x: ops.cond_concat(ops.scale_mask(x, tr.t('keep', x.rows * x.c), 1.25, defer=True), lab, 10),
                  'tg_actgrad_f32')


# ================================================================== recording

def run_all():
    import pytest
    out = {}
    for name in CASES:
        with pytest.MonkeyPatch.context() as mp:
            out[name] = run_case(name, mp)
    return out


def run_case(name, monkeypatch, shape=None):
    c = CASES[name]
    tr = Tracer(**c.ctx_kw).install(monkeypatch)
    tr.variant = name
    if shape is None:
        c.fn(tr)
    else:
        c.fn(tr, shape)
    return json.loads(json.dumps(tr.trace))                # what the fixture holds: lists, dicts, numbers, strings


def check_route(name, trace):
    got = set(names(trace))
    c = CASES[name]
    missing, unexpected = [n for n in c.expect if n not in got], [n for n in c.absent if n in got]
    assert not missing and not unexpected, "%s took another route: missing %s, unexpected %s; issued %s" % (name, missing, unexpected, names(trace))


def dump(traces):
    """one launch per line, so that a deliberate change shows as a readable diff"""
    parts = []
    for name in sorted(traces):
        parts.append('%s: [\n%s\n]' % (json.dumps(name), ',\n'.join(json.dumps(e, separators=(',', ':')) for e in traces[name])))
    return '{\n' + ',\n'.join(parts) + '\n}\n'


def launch_literals(path=os.path.join(PKG, 'tg', 'ops.py')):
    """every quoted tg_* name in tg/ops.py that is a launch entry point; a literal ending in '_' is the stem of names completed with a
    dtype suffix ('tg_bn_train_' + 'f32' | 'bf16') and stands for both"""
    found = set(re.findall(r"""['"](tg_[a-z0-9_]+)['"]""", open(path).read()))
    out = set()
    for n in found:
        out.update([n + 'f32', n + 'bf16'] if n.endswith('_') else [n])
    return {n for n in out if plan.signature(n) is not None}


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit("usage: python tests/launch_trace.py --record    (rewrites %s)" % os.path.relpath(FIXTURE, ROOT))
    traces = run_all()
    for nm, trc in traces.items():
        check_route(nm, trc)
    with open(FIXTURE, 'w') as f:
        f.write(dump(traces))
    print("recorded %d cases, %d launches -> %s" % (len(traces), sum(len(t) for t in traces.values()), FIXTURE))
