"""Every launch route of tg/ops.py held to float64 on the GPU: the case bodies of tests/launch_trace.py (the routes of conv2d, deconv2d,
filter_grad, the batch norms, mean-only BN and the small ops around them) run for real on a runtime.Context, and what they leave behind is
compared, element by element, with tests/ops_reference.py: a float64 restatement of the same ops and the error bound it propagates
(tests/test_ops_reference.py shows on the CPU that a correct fp32 evaluation stays inside that bound, and that an off-by-one does not).

The runner (`GpuRunner`) has the Tracer's interface.  Inputs are drawn by the role of their label (ops_reference.fill: kernels N(0, 0.1),
gains 1 + 0.1 N, biases and population statistics 0.3 N, variances positive, keep masks 0 / 1, labels one-hot, data N(0, 1)).  Every
labelled tensor and every workspace buffer of the Context is a kernel_check.guarded allocation.  Gradient destinations start as NaN:
tg/ops.py OVERWRITES every variable gradient it is given (tg_slab_reduce_f32 / tg_filter_grad_tail_multi_f32 write dw, tg_wn_bwd[_tab]_f32
dv and dg, tg_actgrad_bias_f32 / tg_colstats_f32 the bias gradient, the mean-only-BN and batch-norm backward launches db, dgamma, dbeta);
none accumulates, so a NaN left behind is an element that was never written.  The logical channels of every activation an op makes and of
every activation-gradient buffer Context.grad_of hands out start as NaN as well (their padding as the zeros a workspace buffer is born
with): the backward launches overwrite those too.  tg.lib.call records [name, scalar arguments...] (pointers opaque)
and then issues the launch, so the assertions of the case bodies on the trace hold here too and launch_trace.check_route ties each
numeric check to the route it claims.  tg_conv3x3_policy stays at its default.

Per case and shape (the recorded shape, and the ragged one of launch_trace.RAGGED):
  * before any launch: in the reference, the two largest values of every pooling window differ by more than 4x their bound;
  * the route is the recorded one;
  * every forward output (of every op call of the body), every input gradient, every *_grad tensor and the updated pop_mean / mm / mv lie
    within the propagated bound; tensors the ops only read are unchanged bit for bit; relu / lrelu masks of the reference's backward pass
    come from the forward outputs the device stored (which are held to the bound themselves);
  * channel padding of outputs and input gradients is exactly 0.0, every guard is intact, no owned element is still NaN;
  * a second run is bit-identical;
  * a '_side' variant (filter gradients on the second stream) is bit-identical to the variant without it.
'_bf16mfma' variants and the bf16-stored cases run against the reference with bf16-rounded MFMA operands (ops_reference.bf16q).
bwd_single_consumer_refusal asserts the refusal.  ops_reference.EXEMPT and EXEMPT_SHAPES list what has no float64 check and why (shapes
the launch itself refuses: asserted here), ops_reference.UNDEFINED the tensors whose content tg/ops.py does not define.

Set TG_OPS_ROUTES_DUMP to a path to get the worst ratio per case as JSON (profiles/ops_routes.txt is written from it)."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import kernel_check as KC
import launch_trace as LT
import ops_reference as R
from tg import lib, plan, runtime
from tg.runtime import Act, Context

pytestmark = pytest.mark.gpu

ITEMS = R.items(LT)
RATIOS = {}


class GpuContext(Context):
    """a real Context whose workspace buffers are guarded allocations"""

    def __init__(self, runner, mfma_dtype='f32', act_dtype='f32', wgrad_side=False):
        self.runner, self.guards = runner, {}
        Context.__init__(self)
        self.mfma_dtype, self.act_dtype, self.wgrad_side = mfma_dtype, act_dtype, wgrad_side

    def ws(self, key, numel, zero=False):
        t = self.buffers.get(key)
        if t is None or t.numel() < numel:
            g = KC.guarded(max(int(numel), 1))
            g.t.zero_()                                   # a workspace buffer is born zeroed (Context.ws)
            self.guards[key], self.buffers[key], t = g, g.t, g.t
        elif zero:
            lib.call('tg_fill_f32', lib.ptr(t), 0.0, int(numel), self.stream)
        return t[:numel]

    def new_act(self, n, h, w, c, ld=None, requires_grad=False, tag='a', dtype='f32'):
        a = Context.new_act(self, n, h, w, c, ld, requires_grad, tag, dtype)
        if tag == 'x':
            self.runner.fill_x(a)
        else:
            if dtype == 'f32':
                a.t.view(a.rows, a.ld)[:, :c] = float('nan')
            self.runner.made.append(a)
        return a

    def grad_of(self, a):
        fresh = a.grad is None
        g = Context.grad_of(self, a)
        if fresh:                                         # every backward launch overwrites its destination: a NaN left is an element never written
            g.t.view(g.rows, g.ld)[:, :g.c] = float('nan')
        return g


def snap(a):
    """a device copy of an activation (taken on the launch stream, where its producer ran)"""
    own = a.c + (a.labels.ncls if a.labels is not None else 0)     # a convolution that appends the label channels owns them too
    return dict(t=a.t.detach().float().clone(), rows=a.rows, ld=a.ld, shape=(a.n, a.h, a.w, a.c), own=own)


def logical(s):
    return s['t'].cpu().numpy().reshape(s['rows'], s['ld'])[:, :s['shape'][3]].reshape(s['shape'])


def padding(s):
    return s['t'].cpu().numpy().reshape(s['rows'], s['ld'])[:, s['own']:]


class GpuRunner(LT.Tracer):
    names_buffers = False      # pointers are opaque in this trace

    def __init__(self, name, ident, **ctx_kw):
        self.trace, self.labels, self.label_guards, self._real_call = [], {}, {}, None
        self.variant, self.key = name, R.fill_key(name, ident)
        self.xs, self.dx, self.outs, self.stored, self.made, self.n_seeds, self.n_calls, self.depth = [], {}, [], {}, [], 0, 0, 0
        self.cx = GpuContext(self, **ctx_kw)

    # ---- launches: recorded, then issued
    def _ptr(self, p):
        return None if getattr(p, 'value', p) is None else '<ptr>'

    def call(self, name, *args):
        kinds = plan.signature(name)
        if kinds is not None:
            assert len(args) == len(kinds) + 1, (name, len(args), len(kinds) + 1)
            self.trace.append([name] + [self._arg(k, a) for k, a in zip(kinds, args)])
        return self._real_call(name, *args)

    # ---- the case's tensors
    def t(self, label, numel, dtype=torch.float32):
        assert label not in self.labels, label
        g = KC.guarded(max(int(numel), 1), fill=R.fill(self.key, label, max(int(numel), 1)))
        self.label_guards[label], self.labels[label] = g, g.t
        return g.t[:int(numel)]

    def _put(self, a, vals):
        v = a.t.view(a.rows, a.ld)
        v.zero_()
        v[:, :a.c] = torch.from_numpy(vals.reshape(a.rows, a.c)).to(v.device)

    def fill_x(self, a):
        self._put(a, R.fill_x(self.key, len(self.xs), (a.n, a.h, a.w, a.c)))
        self.xs.append(a)

    def seed(self, y, ld=None):
        g = LT.Tracer.seed(self, y, ld)
        self._put(g, R.fill_seed(self.key, self.n_seeds, (g.n, g.h, g.w, g.c)))
        self.n_seeds += 1
        return g

    @contextlib.contextmanager
    def phase(self, name='p', train=True, record=True):
        with LT.Tracer.phase(self, name, train, record) as cx:
            yield cx
        for i, x in enumerate(self.xs):                   # before a later solver run reuses the call-site buffers
            if i not in self.dx and x.grad is not None:
                self.dx[i] = snap(Act(x.grad.t, x.n, x.h, x.w, x.c, x.grad.ld))

    def wrap(self, name, fn):
        def call(*a, **kw):
            if self.depth:
                return fn(*a, **kw)
            k, self.n_calls, self.depth, self.made = self.n_calls, self.n_calls + 1, 1, []
            try:
                r = fn(*a, **kw)
            finally:
                self.depth = 0
            if isinstance(r, Act):
                self.outs.append((k, None if r.t is None else snap(r)))
                src = self.made[0] if (name == 'conv2d' and self.made) else r      # conv2d's y, also where a pool follows inside the call
                self.stored[k] = None if src.t is None else snap(src)
            elif torch.is_tensor(r):
                self.outs.append((k, r.detach().clone()))
            return r
        return call

    # ---- what the case left behind
    def finish(self):
        torch.cuda.synchronize()
        for g in list(self.cx.guards.values()) + list(self.label_guards.values()):
            g.check_guard()
        got, pads = {}, {}
        for label, g in self.label_guards.items():
            got['label:' + label] = g.get()
        for k, s in self.outs:
            if s is None:
                continue
            if isinstance(s, dict):
                got['out:%d' % k], pads['out:%d' % k] = logical(s), padding(s)
            else:
                got['out:%d' % k] = s.cpu().numpy()
        for i, s in self.dx.items():
            got['dx:%d' % i], pads['dx:%d' % i] = logical(s), padding(s)
        self.got, self.pads = got, pads
        self.stored = {k: (None if s is None else logical(s)) for k, s in self.stored.items()}
        return self


class OpsProxy(object):
    def __init__(self, runner, ops):
        for n in R.OPS_API:
            setattr(self, n, runner.wrap(n, getattr(ops, n)))


def gpu_run(ident, name, shape):
    c = LT.CASES[name]
    default = torch.cuda.current_stream()
    with pytest.MonkeyPatch.context() as mp:
        tr = GpuRunner(name, ident, **c.ctx_kw)
        try:
            tr.install(mp)
            mp.setattr(LT, 'ops', OpsProxy(tr, LT.ops))
            if shape is None:
                c.fn(tr)
            else:
                c.fn(tr, shape)
            return tr.finish()
        except Exception as e:
            if 'illegal memory access' in str(e) or 'HIP error' in str(e) or 'hipError' in str(e):
                pytest.exit("GPU fault in %s: %s (nothing more is started on the device)" % (ident, e), returncode=3)
            raise
        finally:
            torch.cuda.synchronize()
            torch.cuda.set_stream(default)


def same_bits(a, b, what):
    assert set(a) == set(b), what
    for key in sorted(a):
        x, y = np.ascontiguousarray(a[key], np.float32).view(np.int32), np.ascontiguousarray(b[key], np.float32).view(np.int32)
        assert x.shape == y.shape and (x == y).all(), "%s: %s differs in %d elements" % (what, key, int((x != y).sum()))


@pytest.fixture(scope='module', autouse=True)
def dump_ratios():
    yield
    path = os.environ.get('TG_OPS_ROUTES_DUMP')
    if path:
        with open(path, 'w') as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


@pytest.mark.parametrize('ident,name,shape', ITEMS, ids=[i[0] for i in ITEMS])
def test_route_is_held_to_float64(ident, name, shape):
    with pytest.MonkeyPatch.context() as mp:              # before any launch: no pooling decision within reach of rounding
        pre = R.run_reference(LT, name, mp, torch.float64, None, shape, R.fill_key(name, ident))
    assert pre.cx.pool_margin > 1.0, "%s: a pooling window's two largest values are within 4x their bound" % ident
    run = gpu_run(ident, name, shape)
    LT.check_route(name, run.trace)
    with pytest.MonkeyPatch.context() as mp:
        ref = R.run_reference(LT, name, mp, torch.float64, run.stored, shape, R.fill_key(name, ident))
    want = R.expected(ref)
    for key in R.UNDEFINED.get(name, ()):
        assert key in want and key in run.got, key
        for d in (want, run.got, run.pads):
            d.pop(key, None)
    rat = R.ratios(run.got, want)
    worst = max(rat, key=rat.get)
    RATIOS[ident] = dict(worst=rat[worst], key=worst)
    print("%s: %s" % (ident, ', '.join('%s %.3g' % kv for kv in sorted(rat.items()))))
    bad = [R.worst_element(run.got, want, k) for k in sorted(rat) if not rat[k] <= 1.0]
    assert not bad, "%s: beyond the float64 bound (ratio %s):\n  %s" % (ident, ', '.join('%.3g' % rat[k] for k in sorted(rat) if not rat[k] <= 1.0), '\n  '.join(bad))
    for key, p in run.pads.items():
        assert (p == 0).all(), "%s: %s has %d non-zero padding elements" % (ident, key, int((p != 0).sum()))
    again = gpu_run(ident, name, shape)
    for key in R.UNDEFINED.get(name, ()):
        again.got.pop(key)
    same_bits(run.got, again.got, "%s: second run" % ident)
    if '_side' in name:
        base = gpu_run(ident.replace('_side', ''), name.replace('_side', ''), shape)
        same_bits(run.got, base.got, "%s against the variant without the second stream" % ident)


@pytest.mark.parametrize('name', R.ON_DEVICE)
def test_large_filter_gradient_against_float64_on_the_device(name):
    """filter_grad_large: 512 x 8 x 8 x 256 -> 256, the one route defined by its size (>= 2^34 multiply-adds: its launch goes beside the
    input-gradient chain only when the second stream is on, and its tail is deferred to flush_tails, which has to join that stream first).
    The reference is the same sum in float64 on the device, tap by tap; x and dpre are exact inputs, so the bound is the reduction
    stage's alone: TOL * sum |x| |dpre|."""
    R.register(LT)
    assert R.REFS[name] == 'device'
    run = gpu_run(name, name, None)
    LT.check_route(name, run.trace)
    n, h, w, ci, co = 512, 8, 8, 256, 256
    x = run.labels['x'].double().view(n, h, w, ci)
    dy = run.labels['dpre'].double().view(n * h * w, co)
    xp = torch.zeros(n, h + 2, w + 2, ci, dtype=torch.float64, device=x.device)
    xp[:, 1:-1, 1:-1] = x
    ref, sabs = torch.empty(9, ci, co, dtype=torch.float64, device=x.device), torch.empty(9, ci, co, dtype=torch.float64, device=x.device)
    for t in range(9):
        xs = xp[:, t // 3:t // 3 + h, t % 3:t % 3 + w].reshape(n * h * w, ci)
        ref[t], sabs[t] = xs.T @ dy, xs.abs().T @ dy.abs()
    got = run.got['label:dst'].reshape(9, ci, co)
    r = KC.worst(got, ref.cpu().numpy(), sabs.cpu().numpy())
    RATIOS[name] = dict(worst=r, key='label:dst')
    print("%s: label:dst %.3g" % (name, r))
    assert r <= 1.0, "%s: the filter gradient is at %.3g x the reduction bound" % (name, r)
    ctrl = ref.clone()                                     # negative control: the last image's share of one tap dropped
    ctrl[8] -= xp[-1:, 2:2 + h, 2:2 + w].reshape(h * w, ci).T @ dy[-h * w:]
    assert KC.rejected(ctrl.cpu().numpy(), ref.cpu().numpy(), sabs.cpu().numpy())
    again = gpu_run(name, name, None)
    same_bits(run.got, again.got, "%s: second run" % name)
    if '_side' in name:
        base = gpu_run(name.replace('_side', ''), name.replace('_side', ''), None)
        same_bits(run.got, base.got, "%s against the variant without the second stream" % name)


@pytest.mark.parametrize('ident', sorted(R.KERNEL_REFUSES))
def test_an_exempt_shape_is_one_the_launch_refuses(ident):
    """ops_reference.EXEMPT / EXEMPT_SHAPES: the host code routes these shapes (the trace fixture pins it) and the launch refuses them,
    loudly and before it computes anything.  Asserted so that the exemption cannot outlive its reason."""
    name = ident.split('@')[0]
    assert ident in R.EXEMPT or ident in R.EXEMPT_SHAPES
    with pytest.raises(lib.TgError, match=R.KERNEL_REFUSES[ident]):
        gpu_run(ident, name, LT.RAGGED[LT.CASES[name].fn.__name__] if '@' in ident else None)


def test_the_fused_backward_refuses_a_second_consumer():
    run = gpu_run('bwd_single_consumer_refusal', 'bwd_single_consumer_refusal', None)
    assert 'refused' in run.trace
    LT.check_route('bwd_single_consumer_refusal', run.trace)
