"""Kernel-level building blocks (forward + recorded backward) that Model/nn.py and
Model/model_base.py compose.  Every function launches tg_* kernels through the C ABI on the
context's stream and, when a tape is active, records a closure producing the input / variable
gradients.  Gradient of an activation `a` lives in `a.grad` (an Act of identical layout)."""
import collections
import contextlib
import ctypes as C
import types

import torch

from . import geom, lib
from .lib import ACT
from .runtime import Act, ctx, pad32, seg_array

_BF16_ENTRY = {'tg_igemm_f32': 'tg_igemm_bf16', 'tg_igemm_multi_f32': 'tg_igemm_multi_bf16', 'tg_igemm_colsum_f32': 'tg_igemm_colsum_bf16',
               'tg_igemm_actsum_f32': 'tg_igemm_actsum_bf16', 'tg_igemm_bnstat_f32': 'tg_igemm_bnstat_bf16',
               'tg_igemm_bnbwdstat_f32': 'tg_igemm_bnbwdstat_bf16', 'tg_igemm_labels_f32': 'tg_igemm_labels_bf16', 'tg_wgrad_f32': 'tg_wgrad_bf16'}
_TAKES_SCRATCH = {n for n in list(_BF16_ENTRY) + list(_BF16_ENTRY.values()) + ['tg_igemm_bf16in_bf16', 'tg_igemm_bnstat_bf16in_bf16'] if 'igemm' in n}


def _call(name, *args):
    """lib.call; the MFMA launches switch to their bf16-operand variants when the context asks for the "bf16 MFMA conv path"
    (Context.mfma_dtype = 'bf16', BASELINE.json configs[3]).  The igemm entry points take caller-owned scratch (include/tg_kernels.h):
    sized by tg_igemm_workspace_bytes — the partial sums of tiles the schedule cuts along K, the packed bf16 filter of the 3x3 kernel —
    one buffer per call site like every other workspace; callers here pass the arguments WITHOUT it."""
    cx = ctx()
    if cx.mfma_dtype == 'bf16':
        name = _BF16_ENTRY.get(name, name)
    if name in _TAKES_SCRATCH:
        args = igemm_scratch(cx, name, args, cx.mfma_dtype == 'bf16')
    return lib.call(name, *args)


def igemm_scratch(cx, name, args, bf16):
    """insert (scratch, scratch_bytes) in front of the stream argument of a tg_igemm_* call."""
    need = lib.igemm_workspace_bytes(name, args)
    buf = cx.scratch('igws', (need + 3) // 4) if need > 0 else None
    return args[:-1] + (_p(buf), need, args[-1])


def _p(t):
    if t is not None and t.dtype == torch.bfloat16:
        raise lib.TgError("a bf16-stored tensor was handed to a launch that reads fp32")
    return C.c_void_p(t.data_ptr()) if t is not None else None


STATS_REPLICAS = 8          # replicas of an fp64 statistics accumulator = tg_stats_replicas() (csrc/norm.hip REPL; tests/test_cabi.py)


def _sums64(cx, tag, nseg, c, pair=False, replicas=True):
    """(tensor, zeroed) of Context.zscratch for the fp64 accumulators [replicas][nseg][2 if pair][c] of a statistics launch: one sum per
    (segment, column), or a pair (S0, S1: batch norm); replicas=False: the single copy an igemm epilogue adds to."""
    doubles = (STATS_REPLICAS if replicas else 1) * nseg * (2 if pair else 1) * c
    return cx.zscratch(tag, 2 * doubles)


def fill(t, value):
    """t[:] = value on the context's stream."""
    _call('tg_fill_f32', _p(t), float(value), t.numel(), ctx().stream)


def require_f32(x, op):
    """refuse a bf16-stored activation (Act.dtype, config.ACT_DTYPE) in an op that has no bf16 reader — never reinterpret its bytes."""
    for a in (x if isinstance(x, (list, tuple)) else (x,)):
        if getattr(a, 'dtype', 'f32') != 'f32':
            raise lib.TgError("ops.%s: the %dx%dx%dx%d input is stored as %s; this op reads fp32 activations only (a bf16-stored activation "
                              "may feed conv2d only)" % (op, a.n, a.h, a.w, a.c, a.dtype))


# Hand-offs of the fused backward paths (Act.offer / Act.taken, protocol in runtime.Act), one record type per kind: the producer offers it
# with the result fields empty, the consumer that takes it fills them in (`_replace`) and leaves it in Act.taken.
#   ActSums     a mean-only-BN layer's output: the taker stores dy*act'(y) in .grad and the column sums per application in `sums` (fp64, `replicas` copies)
#   BiasSums    conv / deconv + bias + relu-like activation: the taker (a batch norm's backward) stores the PRE-activation gradient, writes bias_grad
#   BnBwdStats  a training-mode batch norm of input x: the taker leaves sum dy, sum dy*x in `sums`; `grad` is the gradient handle it wrote
# and the forward notes BnSums (Act.bn_sums), Labels (Act.labels), Pending (Act.pending) an op leaves for the op that follows directly.
ActSums, BiasSums = collections.namedtuple('ActSums', 'act alpha seg_rows sums replicas'), collections.namedtuple('BiasSums', 'act alpha bias_grad')
BnBwdStats, BnSums = collections.namedtuple('BnBwdStats', 'x seg_rows sums grad'), collections.namedtuple('BnSums', 'sums seg_rows')
Labels, Pending = collections.namedtuple('Labels', 'address ncls'), collections.namedtuple('Pending', 'x mask scale')


def _offer(y, record):
    assert y.offer is None, "a producer makes at most one offer (Act.offer)"
    y.offer = record


def _trusted(y, gy):
    """y.taken if y's producer may trust it, given y's gradient handle gy, else None: what a taker left is valid only while the taker is the ONE
    writer of the gradient.  A batch norm then takes its own statistics; a gradient ALREADY multiplied by act'(y) (ActSums, BiasSums) cannot
    be told apart from a second consumer's raw contribution in the same buffer: refuse instead of training on it."""
    t = y.taken
    if t is None:
        return None
    if isinstance(t, BnBwdStats):
        return t if (t.grad is gy and gy.contribs == 1) else None
    if gy.contribs > 1:
        raise lib.TgError("fused backward: the gradient of a %dx%dx%dx%d activation was written by %d consumers, but one of them already folded "
                          "the activation derivative into it" % (y.n, y.h, y.w, y.c, gy.contribs))
    return t


def _write_grad(cx, x, store=None, alias=None):
    """THE way a backward closure contributes to x.grad.  store(dst): issue the closure's launch(es), which OVERWRITE dst, an Act of the
    layout of x's gradient.  The first writer (x.grad is None) stores into the buffer of Context.grad_of; a later writer stores into a
    scratch Act and tg_add_f32 adds that to the gradient (one more fp32 rounding), so no contribution is lost, whichever order the tape runs
    the consumers in.  alias (instead of store): the contribution IS already in memory, as a fresh Act view of a consumer's gradient buffer
    with x's logical shape: the first writer adopts it without a launch (every reader of a gradient goes through (pointer, channel stride));
    a later one adds it, through a tg_actgrad_f32 copy into scratch where the channel strides differ.
    -> (gradient handle, whether this was the first writer); handle.contribs counts the writers."""
    first = x.grad is None
    if first and alias is not None:
        x.grad = alias
    gx = cx.grad_of(x)
    if first:
        if alias is None:
            store(gx)
        return gx, first
    part = alias
    if alias is None or alias.ld != gx.ld:
        part = Act(cx.scratch('gxp', gx.rows * gx.ld), gx.n, gx.h, gx.w, gx.c, gx.ld)
        if alias is None:
            store(part)
        else:
            _call('tg_actgrad_f32', alias.ptr, alias.ld, None, 0, None, 0, 1.0, part.ptr, part.ld, x.rows, x.c, 0, 0.0, cx.stream)
    _call('tg_add_f32', gx.ptr, gx.ptr, part.ptr, gx.rows * gx.ld, cx.stream)
    return gx, first


def _segs(x, segments):
    """per-application image counts -> row counts of the batched activation."""
    segments = [x.n] if segments is None else segments
    assert sum(segments) == x.n, (segments, x.n)
    per = x.h * x.w
    return [s * per for s in segments]


# ------------------------------------------------------------------ statistics helpers

def colstats(mode, a_t, ld_a, b_t, ld_b, rows, c, seg_rows, act=None, alpha=0.2, s1=None, s2=None):
    cx = ctx()
    nseg = len(seg_rows)
    wsn = _call('tg_colstats_workspace_floats', rows, nseg, c)
    work = cx.scratch('cs', wsn)
    if s1 is None:
        s1 = cx.scratch('s1_', nseg * c + 4)          # +4: mode 4 reads its per-channel input in 16-B groups
    if s2 is None and mode in (1, 3):
        s2 = cx.scratch('s2_', nseg * c + 4)
    _call('tg_colstats_f32', mode, _p(a_t), ld_a, _p(b_t), ld_b, rows, c, seg_array(seg_rows), nseg, ACT[act], alpha,
          _p(work), _p(s1), _p(s2), cx.stream)
    return s1, s2


# ------------------------------------------------------------------ filter preparation (MFMA layouts + weight-norm scale)

def prep_filter(cx, kernel, g, scale, w_oti, w_hwio, t, c_in, c_out, ci_p, co_p):
    """[scale = g/||V||, then] the [scaled] filter as OTI [co_p][t][ci_p] and HWIO [t][ci_p][co_p] (or None) into the caller's buffers, uncached."""
    if g is not None:
        _call('tg_wn_scale_f32', _p(kernel), _p(g), t * c_in, c_out, _p(scale), cx.stream)
    _call('tg_filter_prep_f32', _p(kernel), _p(scale), None, t, c_in, c_out, ci_p, co_p, _p(w_hwio), _p(w_oti), t * ci_p, ci_p, cx.stream)


def _run_prep_plan(cx, plan):
    """tg_filter_prep_multi_f32 for the recorded layers that are not prepared yet; every result goes into the cache tagged with the
    scratch count its layer would have consumed, so that call-site numbering stays what it was in the recording pass."""
    todo = [j for j in plan if j['key'] not in cx.prep_cache]
    for k in range(0, len(todo), 24):
        part = todo[k:k + 24]
        arr = (lib.PrepJob * len(part))(*[
            lib.PrepJob(j['kernel'].data_ptr(), j['g'].data_ptr() if j['g'] is not None else None, j['scale'].data_ptr() if j['g'] is not None else None,
                        j['w_hwio'].data_ptr(), j['w_oti'].data_ptr(), j['t'] * j['a_pad'], j['a_pad'], j['t'], j['a'], j['b'], j['a_pad'], j['b_pad'])
            for j in part])
        lib.call('tg_filter_prep_multi_f32', arr, len(part), cx.stream)
    for j in todo:
        cx.prep_cache[j['key']] = (j['scale'], j['w_oti'], j['w_hwio'], j['bump'], cx.phase)


def _prepared_filter(cx, kernel, g, t, c_in, c_out, ci_p, co_p, needs_x):
    """(scale, w_oti, w_hwio) of a convolution's filter.  Inside Train.train_iteration the result is kept per variable until that network's
    optimiser step: the classifier is prepared once for the D-update's forward passes and the C-update, the discriminator once for the
    G- and C-updates (Context.prep_cache; None outside train_iteration: no caching); a recorded sequence is prepared by its first layer."""
    cache = cx.prep_cache
    key = ('conv', kernel.data_ptr(), g.data_ptr() if g is not None else 0, t, c_in, c_out, ci_p, co_p)
    ent = cache.get(key) if cache is not None else None
    if ent is None and cache is not None:
        plan = cx.prep_plans.get((cx.plan_tag, cx.phase, key))
        if plan is not None:                               # this layer opens a recorded sequence: prepare all of its layers now
            _run_prep_plan(cx, plan)
            ent = cache.get(key)
    if ent is not None and (ent[2] is not None or not needs_x):
        if len(ent) > 3:                                   # produced by a plan in this phase: keep the call-site numbering of the
            if ent[4] == cx.phase:                         # recording pass, in which this layer allocated its own buffers here
                cx.counter += ent[3]
            cache[key] = ent[:3]
        return ent[:3]
    c_before = cx.counter
    w_oti = cx.scratch('woti', co_p * t * ci_p)
    w_hwio = cx.scratch('whwio', t * ci_p * co_p) if (needs_x or cache is not None) else None
    scale = cx.scratch('wns', c_out) if g is not None else None
    prep_filter(cx, kernel, g, scale, w_oti, w_hwio, t, c_in, c_out, ci_p, co_p)
    if cache is not None:
        cache[key] = (scale, w_oti, w_hwio)
        if cx._prep_rec is not None and w_hwio is not None:
            cx._prep_rec.append(dict(key=key, kernel=kernel, g=g, scale=scale, w_oti=w_oti, w_hwio=w_hwio,
                                     t=t, a=c_in, b=c_out, a_pad=ci_p, b_pad=co_p, bump=cx.counter - c_before))
    return scale, w_oti, w_hwio


# ------------------------------------------------------------------ filter gradient

def filter_grad_tail(cx, dst, t, c_dim, n_dim, wn, slab=None, ns=0, desc=None):
    """finish a filter gradient NOW: sum the `ns` slabs into dst (slab None: dst holds the sum), then, wn=(v, g, dv, dg), the variables' gradient."""
    if slab is not None:
        _call('tg_slab_reduce_f32', _p(slab), ns, t, desc.ld_in, desc.c_out, c_dim, n_dim, _p(dst), cx.stream)
    if wn is not None:
        coef = cx.scratch('coef', 2 * n_dim)
        _call('tg_wn_bwd_f32', _p(dst), _p(wn[0]), _p(wn[1]), t * c_dim, n_dim, _p(wn[2]), _p(wn[3]), _p(coef), cx.stream)


def filter_grad(desc, in_act_t, dout_t, t, c_dim, n_dim, dst, wn=None, defer=True, in16=False):
    """dst[t][c_dim][n_dim] = filter gradient via tg_wgrad_f32 slabs + deterministic reduce.
    wn=(v, g, dv, dg): weight-normalised layer — dst is the gradient of the effective filter (scratch), dv / dg the variables'.
    The tail (slab reduction [+ weight-norm gradient]) is DEFERRED to Context.flush_tails (end of the backward pass / bucket
    boundary), where the tails of all layers go out as three launches; the 512-split first convolution keeps its own reduce.
    in16: in_act_t is a bf16-stored activation (tg_wgrad_bf16in_bf16)."""
    cx = ctx()
    ns = geom.wgrad_splits(desc, cx.mfma_dtype == 'bf16')      # pixel split and slab size: the library's rule (tg_wgrad_splits[_bf16])
    slab = cx.scratch('slab', geom.wgrad_slab_floats(desc, ns))
    deferred = defer and (cx.tape is not None or cx._phase_depth > 0)
    small = desc.n_img * desc.h_v * desc.w_v * desc.ld_in * desc.c_out * desc.n_taps < (1 << 34)      # < 34 GFLOP: the generic kernel's launches
    wide = ns >= 32 and t * c_dim * n_dim <= 65536
    side = deferred and (small if wide else (small or cx.wgrad_side))      # beside the input-gradient chain (Context.wgrad_on_side; joined in flush_tails)
    with cx.wgrad_on_side() if side else contextlib.nullcontext():
        src = C.c_void_p(in_act_t.data_ptr()) if in16 else _p(in_act_t)
        _call('tg_wgrad_bf16in_bf16' if in16 else 'tg_wgrad_f32', desc, src, _p(dout_t), _p(slab), ns, cx.stream)
        if side and wide:
            # many splits of a small filter (the discriminator's first layers, the classifier's first): the launch AND its own reduction go to
            # the second stream, so the input-gradient chain does not wait for them (round 4: they were 0.18 ms of the D-update's launch stream)
            return filter_grad_tail(cx, dst, t, c_dim, n_dim, wn, slab, ns, desc)
    if not (deferred and not wide):
        return filter_grad_tail(cx, dst, t, c_dim, n_dim, wn, slab, ns, desc)
    coef = cx.scratch('coef', 2 * n_dim) if wn is not None else None
    cx.tail_jobs.append(lib.WnJob(slab.data_ptr(), dst.data_ptr(), wn[0].data_ptr() if wn else None, wn[1].data_ptr() if wn else None,
                                  wn[2].data_ptr() if wn else None, wn[3].data_ptr() if wn else None, coef.data_ptr() if wn else None,
                                  ns, t, desc.ld_in, desc.c_out, c_dim, n_dim))


# ------------------------------------------------------------------ conv / dense (plain and weight-normalised)

def _conv_route(cx, L, bn_stats, n_store_ld):
    """the forward route (_fwd_*) of a conv2d layer: the eligibility predicates, evaluated once (the backward reads L.packed, L.narrow_mobn)"""
    simple_act = L.act in (None, 'relu', 'lrelu')
    L.packed = (cx.mfma_dtype != 'bf16' and L.k == 3 and L.stride == 1 and L.padding == 'SAME' and L.wn is None and L.mobn is None and not bn_stats
                and n_store_ld is None and L.c_out == L.co_p and simple_act and L.c_in <= 16
                and bool(_call('tg_conv3x3_packed_supported', L.x.n, L.x.h, L.x.w, L.c_in, L.c_out)))
    if L.narrow_mobn and L.train and L.stride == 1 and geom.colsum_supported(L.d, L.seg_rows):
        return _fwd_colsum
    if (bn_stats and L.mobn is None and simple_act and L.c_out == L.co_p == L.ld_out and len(L.seg_rows) <= 8
            and geom.colsum_supported(L.d, L.seg_rows)):
        return _fwd_bnstat
    return _fwd_packed if L.packed else _fwd_labels if L.fuse_cat else _fwd_plain


def _fwd_colsum(cx, L):
    """convolution + per-(application, channel) sums in one launch, then ONE apply pass (mean, +b, activation, pop_mean [, 2x2 pool: returned])"""
    x, y, seg_rows, c_out = L.x, L.y, L.seg_rows, L.c_out
    b, b_grad, pop = L.mobn
    sums, zd = _sums64(cx, 'cs64', len(seg_rows), c_out, replicas=False)
    _call('tg_igemm_colsum_f32', L.d, x.ptr, _p(L.w_oti), y.ptr, seg_array(seg_rows), len(seg_rows), _p(sums), zd, cx.stream)
    if L.pool is not None and y.h % 2 == 0 and y.w % 2 == 0 and all(r % (y.h * y.w) == 0 for r in seg_rows):
        pooled = cx.new_act(y.n, y.h // 2, y.w // 2, c_out, L.co_p, requires_grad=L.needs_w or L.needs_x)
        _call('tg_mobn_apply_pool_f32', y.ptr, y.ld, y.n, y.h, y.w, c_out, seg_array(seg_rows), len(seg_rows), _p(sums), _p(b), _p(pop), 0.9, ACT[L.act],
              L.alpha, pooled.ptr, pooled.ld, _p(L.pool[0]), c_out, L.pool[1], cx.stream)
        return pooled
    _call('tg_mobn_apply_f32', y.ptr, y.ld, y.rows, c_out, seg_array(seg_rows), len(seg_rows), _p(sums), _p(b), _p(pop), 0.9, ACT[L.act],
          L.alpha, cx.stream)


def _fwd_bnstat(cx, L):
    seg_rows = L.seg_rows
    bsum, zd = _sums64(cx, 'bn64', len(seg_rows), L.c_out, pair=True)     # the batch norm's buffer
    _call('tg_igemm_bnstat_bf16in_bf16' if L.x16 else 'tg_igemm_bnstat_f32', L.d, L.x.ptr, _p(L.w_oti), _p(L.bias), L.y.ptr, seg_array(seg_rows),
          len(seg_rows), _p(bsum), zd, cx.stream)
    L.y.bn_sums = BnSums(bsum, tuple(seg_rows))


def _fwd_packed(cx, L):
    """K-packed products straight from the [3,3,Cin,Cout] variable (csrc/packed_conv.hip); with concat the label channels ride along"""
    x, lab = L.x, L.concat if L.fuse_cat else (None, 0)
    _call('tg_conv3x3_packed_fwd_f32', x.ptr, x.ld, L.c_in, _p(L.kernel), _p(L.bias), ACT[L.act], L.alpha, _p(lab[0]), lab[1], L.y.ptr, L.ld_out,
          x.n, x.h, x.w, L.c_out, cx.stream)


def _fwd_labels(cx, L):
    _call('tg_igemm_labels_f32', L.d, L.x.ptr, _p(L.w_oti), _p(L.bias), _p(L.concat[0]), L.concat[1], L.y.ptr, cx.stream)


def _fwd_plain(cx, L):
    _call('tg_igemm_bf16in_bf16' if L.x16 else 'tg_igemm_f32', L.d, L.x.ptr, _p(L.w_oti), (_p(L.bias) if L.mobn is None else None), L.y.ptr, cx.stream)


def _mobn_unfused(cx, src, dst, c, seg_rows, b, pop, decay, train, act=None, alpha=0.0):
    """dst = act(src - mean_seg + b) (training: statistics pass, pop updated) or act(src - pop + b): shift, then one apply pass"""
    sums = None
    if train:
        sums, _ = colstats(0, src.t, src.ld, None, 0, src.rows, c, seg_rows)
    shift = cx.scratch('shift', len(seg_rows) * c)
    _call('tg_mobn_finalize_f32', _p(sums), seg_array(seg_rows), len(seg_rows), src.rows, c, _p(b), _p(pop), decay, 1 if train else 0, _p(shift), cx.stream)
    _call('tg_seg_scale_shift_act_f32', src.ptr, src.ld, dst.ptr, dst.ld, src.rows, c, c, seg_array(seg_rows), len(seg_rows),
          None, _p(shift), ACT[act], alpha, cx.stream)


def _dpre_plain(cx, y, gy, act, alpha, c_out, co_p, bias_grad, head=False):
    """pre-activation gradient [rows][co_p] of y = act(pre + bias) from gy = y.grad, and the bias gradient (None: not wanted).  gy itself where a
    batch norm behind the layer already made it that (it took the layer's BiasSums offer) or — head: conv2d only — the loss head wrote a padded
    dlogits."""
    taken = _trusted(y, gy)
    if head and act is None and gy.ld == co_p:
        if bias_grad is not None:
            colstats(0, gy.t, co_p, None, 0, y.rows, c_out, [y.rows], s1=bias_grad)
        return gy.t
    if isinstance(taken, BiasSums) and gy.ld == co_p:
        return gy.t
    dpre = cx.scratch('dpre', y.rows * co_p)
    if bias_grad is not None and co_p <= 1024:
        zs, zd = _sums64(cx, 'ab64', 1, c_out)
        _call('tg_actgrad_bias_f32', gy.ptr, gy.ld, y.ptr if act else None, y.ld, _p(dpre), co_p, y.rows, c_out, ACT[act], alpha,
              _p(zs), zd, _p(bias_grad), cx.stream)
    else:
        _call('tg_actgrad_f32', gy.ptr, gy.ld, y.ptr if act else None, y.ld, None, 0, 1.0, _p(dpre), co_p, y.rows, c_out,
              ACT[act], alpha, cx.stream)
        if bias_grad is not None:
            colstats(0, dpre, co_p, None, 0, y.rows, c_out, [y.rows], s1=bias_grad)
    return dpre


def _dpre_mobn(cx, L, gy):
    y, seg_rows, c_out, co_p = L.y, L.seg_rows, L.c_out, L.co_p
    nseg = len(seg_rows)
    taken = _trusted(y, gy)
    dpre = cx.scratch('dpre', y.rows * co_p)
    if taken is not None:
        # the consumer's backward launch already stored t = dy*act'(y) in y.grad and summed its columns per application (ActSums)
        db = L.mobn[1] if L.needs_w else cx.scratch('db', c_out)
        _call('tg_mobn_center_f32', gy.ptr, gy.ld, _p(dpre), co_p, y.rows, c_out, seg_array(seg_rows), nseg, _p(taken.sums),
              taken.replicas, _p(db), cx.stream)
    elif L.narrow_mobn:
        db = L.mobn[1] if L.needs_w else cx.scratch('db', c_out)
        sums64, zd = _sums64(cx, 'bs64', nseg, c_out)
        _call('tg_mobn_bwd_f32', gy.ptr, gy.ld, y.ptr, y.ld, _p(dpre), co_p, y.rows, c_out, seg_array(seg_rows), nseg,
              ACT[L.act], L.alpha, _p(sums64), zd, _p(db), cx.stream)
    else:
        sums, _ = colstats(2, gy.t, gy.ld, y.t, y.ld, y.rows, c_out, seg_rows, L.act, L.alpha)
        sh = cx.scratch('bshift', nseg * c_out)
        db = L.mobn[1] if L.needs_w else cx.scratch('db', c_out)
        _call('tg_mobn_bwd_finalize_f32', _p(sums), seg_array(seg_rows), nseg, y.rows, c_out, _p(sh), _p(db), cx.stream)
        _call('tg_seg_actgrad_shift_f32', gy.ptr, gy.ld, y.ptr, y.ld, _p(dpre), co_p, y.rows, c_out, seg_array(seg_rows),
              nseg, _p(sh), ACT[L.act], L.alpha, cx.stream)
    return dpre


def _input_grad(cx, L, dpre):
    x, ci_p = L.x, L.ci_p
    first = x.grad is None

    def store(gx):
        dlist = geom.conv_dgrad(x.n, x.h, x.w, ci_p, L.co_p, L.k, L.stride, L.padding, ld_out=gx.ld, n_store=ci_p)
        takes_over = first and len(dlist) == 1 and x.c == ci_p == gx.ld == x.ld
        o = x.offer
        if isinstance(o, ActSums) and takes_over and sum(o.seg_rows) == x.rows and geom.colsum_supported(dlist[0], o.seg_rows):
            # x is the output of a mean-only-BN layer: this launch also applies that layer's activation derivative and sums the
            # columns per application, so its backward pass needs no statistics pass of its own (tg_mobn_center_f32)
            nsg = len(o.seg_rows)
            gsum, zd = _sums64(cx, 'gs64', nsg, ci_p, replicas=False)
            _call('tg_igemm_actsum_f32', dlist[0], _p(dpre), _p(L.w_hwio), x.ptr, ACT[o.act], o.alpha, gx.ptr, seg_array(o.seg_rows), nsg,
                  _p(gsum), zd, cx.stream)
            x.taken = o._replace(sums=gsum, replicas=1)
        elif (isinstance(o, BnBwdStats) and takes_over and o.x.ld == gx.ld and len(o.seg_rows) <= 8 and sum(o.seg_rows) == x.rows
              and geom.colsum_supported(dlist[0], o.seg_rows)):
            # x is a training-mode batch norm's output and this launch is the first to write its gradient: the batch norm's backward
            # statistics (sum dy, sum dy * its input) are taken in this epilogue
            segs = o.seg_rows
            bsums, zdb = _sums64(cx, 'bnb64', len(segs), ci_p, pair=True)
            _call('tg_igemm_bnbwdstat_f32', dlist[0], _p(dpre), _p(L.w_hwio), o.x.ptr, gx.ptr, seg_array(segs), len(segs), _p(bsums), zdb, cx.stream)
            x.taken = o._replace(sums=bsums, grad=gx)
        else:
            dds = lib.desc_array(dlist)
            _call('tg_igemm_multi_f32', dds, len(dds), _p(dpre), _p(L.w_hwio), None, gx.ptr, cx.stream)

    _write_grad(cx, x, store)


def conv2d(x, kernel, bias, c_out, k, stride, padding, act=None, alpha=0.2, wn=None, mobn=None, segments=None,
           train=True, kernel_grad=None, bias_grad=None, n_store_ld=None, bn_stats=False, concat=None, pool=None):
    """y = act(conv(x, W) + bias)   or, with wn=(g, g_grad) and mobn=(b, b_grad, pop_mean):
       W = g V/||V||; y = act(conv(x, W) - mean_seg + b)            (Model/nn.py:469-520,525-589).
    kernel: HWIO tensor [k,k,c_in,c_out] (flat).  Dense layers are k = 1 on [n,1,1,c].
    n_store_ld: (n_store, ld_out) override for narrow outputs (D's logit).
    bn_stats: a training-mode batch norm over `segments` follows directly — its sum / sum-of-squares pass is taken in this launch's
    epilogue (tg_igemm_bnstat_*) and left in y.bn_sums for batch_norm_train.
    concat: (label tensor [n, ncls], ncls) — a cond_concat with these labels follows directly (the discriminators' conv -> leaky relu -> concat
    pairs): the launch writes into the concatenated tensor's buffer and appends the label channels itself (tg_igemm_labels_*); the handle
    returned still describes the c_out convolution channels, y.labels tells cond_concat that its work is done.
    pool: (keep-mask tensor or None, 1/keep) — tf.nn.max_pool 2x2 + dropout follow directly (the classifier's conv1_3 / conv2_3): returns the POOLED
    activation; on the fused mean-only-BN path the apply pass and the pooling are one launch (tg_mobn_apply_pool_f32)."""
    cx = ctx()
    assert x.ld % 32 == 0, "conv input must be channel-padded to 32"
    x16 = x.dtype == 'bf16'                # a bf16-stored input (config.ACT_DTYPE): the *_bf16in_bf16 launches read it as it is
    if x16 and not (cx.mfma_dtype == 'bf16' and k == 3 and stride == 1 and padding == 'SAME' and wn is None and mobn is None and concat is None
                    and n_store_ld is None and pool is None):
        raise lib.TgError("conv2d: a bf16-stored input is read by the bf16-operand 3x3 / stride-1 / SAME convolution without weight norm, "
                          "mean-only BN, concat or pooling only (MFMA_DTYPE %r)" % (cx.mfma_dtype,))
    co_p = pad32(c_out)
    needs_w = cx.trains() and kernel_grad is not None
    needs_x = cx.tape is not None and x.requires_grad
    L = types.SimpleNamespace(x=x, x16=x16, kernel=kernel, bias=bias, c_in=x.c, ci_p=x.ld, c_out=c_out, co_p=co_p, k=k, t=k * k, stride=stride,
                              padding=padding, act=act, alpha=alpha, wn=wn, mobn=mobn, train=train, kernel_grad=kernel_grad, concat=concat,
                              pool=pool, needs_w=needs_w, needs_x=needs_x)
    _, L.w_oti, L.w_hwio = _prepared_filter(cx, kernel, wn[0] if wn is not None else None, L.t, L.c_in, c_out, L.ci_p, co_p, needs_x)
    L.fuse_cat = (concat is not None and mobn is None and not bn_stats and n_store_ld is None and c_out == co_p)
    n_store, ld_out = (c_out, pad32(c_out + concat[1])) if L.fuse_cat else n_store_ld if n_store_ld is not None else (c_out, co_p)
    L.ld_out = ld_out
    L.d = geom.conv_fwd(x.n, x.h, x.w, L.ci_p, co_p, k, stride, padding, ld_out=ld_out, n_store=n_store, act=act if mobn is None else None, alpha=alpha)
    y = L.y = cx.new_act(x.n, L.d.h_out, L.d.w_out, c_out, ld_out, requires_grad=needs_w or needs_x)
    y.strided_grad_ok = True
    L.seg_rows = _segs(y, segments)
    # a mean-only-BN layer the fused kernels serve (statistics in an epilogue, one-pass backward)
    L.narrow_mobn = mobn is not None and c_out == co_p and c_out <= 512 and len(L.seg_rows) <= 8
    fwd = _conv_route(cx, L, bn_stats, n_store_ld)
    pooled = fwd(cx, L)
    if L.fuse_cat:
        y.labels = Labels(concat[0].data_ptr(), concat[1])
    if mobn is not None and fwd is not _fwd_colsum:
        _mobn_unfused(cx, y, y, c_out, L.seg_rows, mobn[0], mobn[2], 0.9, train, act, alpha)
    if not (needs_w or needs_x):
        return _pool_after(cx, y, pooled, pool)
    if L.narrow_mobn and train and act is not None and ld_out == co_p:
        _offer(y, ActSums(act, alpha, tuple(L.seg_rows), None, 0))
    if mobn is None and act in ('relu', 'lrelu') and needs_w and bias_grad is not None and c_out == co_p == ld_out:
        _offer(y, BiasSums(act, alpha, bias_grad))       # a batch norm behind this layer may fold act' and the bias gradient into its backward

    def bwd():
        gy = y.grad
        assert gy is not None, "conv2d backward: no gradient reached the output"
        if mobn is not None:
            dpre = _dpre_mobn(cx, L, gy)
        else:
            dpre = _dpre_plain(cx, y, gy, act, alpha, c_out, co_p, bias_grad if needs_w else None, head=True)
        if needs_w and L.packed:
            pws = cx.scratch('pkws', _call('tg_conv3x3_packed_wgrad_workspace_bytes', x.n, x.h, x.w, x.c, c_out) // 4)
            with cx.wgrad_on_side():                      # beside the input-gradient chain; joined in flush_tails
                _call('tg_conv3x3_packed_wgrad_f32', x.ptr, x.ld, x.c, _p(dpre), co_p, x.n, x.h, x.w, c_out, _p(pws), _p(kernel_grad), cx.stream)
        elif needs_w:
            dw = kernel_grad if wn is None else cx.scratch('dw', L.t * x.c * c_out)
            filter_grad(geom.conv_wgrad(x.n, x.h, x.w, x.ld, co_p, k, stride, padding), x.t, dpre, L.t, x.c, c_out, dw, in16=x16,
                        wn=None if wn is None else (kernel, wn[0], kernel_grad, wn[1]))
        if needs_x:
            _input_grad(cx, L, dpre)

    cx.record(bwd)
    return _pool_after(cx, y, pooled, pool)


def _pool_after(cx, y, pooled, pool):
    """what conv2d returns: y, or — conv2d(pool=...) — the max-pooled, dropped-out activation: made by the fused apply launch (`pooled`) or by the
    stand-alone pooling op; its backward closure goes on the tape behind the convolution's."""
    if pool is None:
        return y
    if pooled is None:
        return maxpool2_dropout(y, pool[0], pool[1])
    _record_maxpool_bwd(cx, y, pooled, pool[0], pool[1])
    return pooled


def deconv2d(x, kernel, bias, c_out, act=None, kernel_grad=None, bias_grad=None, narrow_out=False, wn=None):
    """tf.layers.conv2d_transpose 5x5 s2 'same' + bias + act (Model/modle_base.py:246-259);
    kernel [5,5,c_out,c_in].  narrow_out: store only the logical channels (generator output).
    wn=(g, g_grad): W = g * l2_normalize(V,[0,1,3]) (NN_Base._WN_deconv2d, Model/modle_base.py:130-155)."""
    require_f32(x, 'deconv2d')
    cx = ctx()
    assert x.ld % 32 == 0
    c_in, ci_p, co_p = x.c, x.ld, pad32(c_out)
    needs_w = cx.trains() and kernel_grad is not None
    needs_x = cx.tape is not None and x.requires_grad
    scale_a = None
    ld_out = c_out if narrow_out else co_p
    # Narrow outputs (the 3-channel image layer) run the forward as ONE 3x3 problem over (output parity, channel) columns
    # (geom.deconv_fwd_merged): the four parities share one 32-column tile instead of padding 3 -> 32 four times (0.118 -> 0.050 ms).
    # Measured on the 128-channel layer the merged form is slower (0.19 -> 0.22 ms: 36/25 of the arithmetic outweighs the balance).
    merged = pad32(4 * c_out) < 4 * co_p and pad32(4 * c_out) <= 128
    if wn is not None:
        scale_a = cx.scratch('wnsa', c_out)
        _call('tg_wn_scale_tab_f32', _p(kernel), _p(wn[0]), 25, c_out, c_in, _p(scale_a), cx.stream)
    # the 3-channel image layer's backward runs as K-packed products straight from the [5,5,Cout,Cin] variable (csrc/narrow.hip): no transposed copy
    narrow = x.ld == ci_p and bool(lib.call('tg_deconv5x5s2_narrow_supported', x.n, x.h, x.w, c_out, ci_p))
    w_tr = cx.scratch('wtr', 25 * ci_p * co_p) if (needs_x and not narrow) else None
    if merged:
        d, ng, tapmap = geom.deconv_fwd_merged(x.n, x.h, x.w, ci_p, c_out, ld_out, n_store=c_out, act=act)
        w_m = cx.scratch('wmrg', d.c_out * 9 * ci_p)
        _call('tg_deconv_merge_prep_f32', _p(kernel), _p(scale_a), c_out, c_in, ng, d.c_out, ci_p, (C.c_int32 * 36)(*tapmap), _p(w_m), cx.stream)
        if w_tr is not None:
            _call('tg_filter_prep_f32', _p(kernel), None, _p(scale_a), 25, c_out, c_in, co_p, ci_p, None, _p(w_tr), co_p, ci_p * co_p, cx.stream)
    else:
        w_pad = cx.scratch('wpad', 25 * co_p * ci_p)
        _call('tg_filter_prep_f32', _p(kernel), None, _p(scale_a), 25, c_out, c_in, co_p, ci_p, _p(w_pad), _p(w_tr), co_p, ci_p * co_p, cx.stream)
    y = cx.new_act(x.n, 2 * x.h, 2 * x.w, c_out, ld_out, requires_grad=needs_w or needs_x)
    y.strided_grad_ok = True
    if act in ('relu', 'lrelu') and needs_w and bias_grad is not None and c_out == co_p == ld_out:
        _offer(y, BiasSums(act, 0.2, bias_grad))         # see conv2d
    if merged:
        _call('tg_igemm_f32', d, x.ptr, _p(w_m), _p(bias), y.ptr, cx.stream)
    else:
        dds = lib.desc_array(geom.deconv_fwd(x.n, x.h, x.w, ci_p, co_p, ld_out=ld_out, n_store=c_out, act=act))
        _call('tg_igemm_multi_f32', dds, len(dds), x.ptr, _p(w_pad), _p(bias), y.ptr, cx.stream)
    if not (needs_w or needs_x):
        return y

    def bwd():
        gy = y.grad
        assert gy is not None
        dpre = _dpre_plain(cx, y, gy, act, 0.2, c_out, co_p, bias_grad if needs_w else None)
        # the 3-channel image layer: both gradients as K-packed products (csrc/narrow.hip) — the generic tiles would pad 3 channels to 32
        if needs_w:
            dw = kernel_grad if wn is None else cx.scratch('dw', 25 * c_out * c_in)
            if narrow:
                nws = cx.scratch('nwws', lib.call('tg_deconv5x5s2_narrow_wgrad_workspace_bytes', x.n, x.h, x.w, c_out, ci_p) // 4)
                # a vector-ALU kernel: beside the input-gradient chain like the other filter gradients, unless tg_wn_bwd_tab_f32 consumes it right below
                with cx.wgrad_on_side() if wn is None else contextlib.nullcontext():
                    _call('tg_deconv5x5s2_narrow_wgrad_f32', _p(dpre), co_p, x.ptr, x.ld, x.n, x.h, x.w, c_out, c_in, ci_p, _p(nws), _p(dw), cx.stream)
            else:                                        # a weight-normalised layer's dw is consumed right below: no deferred tail
                filter_grad(geom.deconv_wgrad(x.n, x.h, x.w, co_p, ci_p), dpre, x.t, 25, c_out, c_in, dw, defer=wn is None)
            if wn is not None:
                _call('tg_wn_bwd_tab_f32', _p(dw), _p(kernel), _p(wn[0]), 25, c_out, c_in, _p(kernel_grad), _p(wn[1]), cx.stream)

        def store(gx):
            if narrow and gx.ld >= ci_p:
                _call('tg_deconv5x5s2_narrow_dgrad_f32', _p(dpre), co_p, _p(kernel), _p(scale_a), x.n, x.h, x.w, c_out, c_in, ci_p, gx.ptr, gx.ld, cx.stream)
            else:
                assert w_tr is not None, "deconv2d backward: the transposed filter was not prepared (gradient buffer narrower than the input's channel stride)"
                _call('tg_igemm_f32', geom.deconv_dgrad(x.n, x.h, x.w, ci_p, co_p, ld_out=gx.ld, n_store=ci_p), _p(dpre), _p(w_tr), None,
                      gx.ptr, cx.stream)
        if needs_x:
            _write_grad(cx, x, store)

    cx.record(bwd)
    return y


def mean_only_batch_norm(x, pop_mean, b, b_grad=None, train=True, decay=0.9, segments=None):
    """x - mean + b (training, pop_mean updated) or x - pop_mean + b (Model/nn.py:147-187) as a stand-alone op on an activation
    (the layers of the models use the version fused into the convolution, conv2d(mobn=...))."""
    require_f32(x, 'mean_only_batch_norm')
    cx = ctx()
    c = x.c
    seg_rows = _segs(x, segments)
    nseg = len(seg_rows)
    needs = cx.tape is not None and (x.requires_grad or (cx.trains() and b_grad is not None))
    y = cx.new_act(x.n, x.h, x.w, c, x.ld, requires_grad=needs)
    y.strided_grad_ok = True
    _mobn_unfused(cx, x, y, c, seg_rows, b, pop_mean, decay, train)
    if not needs:
        return y
    want_b = cx.trains() and b_grad is not None

    def bwd():
        gy = y.grad
        assert gy is not None

        def store(gx):
            if train:
                s1, _ = colstats(0, gy.t, gy.ld, None, 0, x.rows, c, seg_rows)
                sh = cx.scratch('bshift', nseg * c)
                db = b_grad if want_b else cx.scratch('db', c)
                _call('tg_mobn_bwd_finalize_f32', _p(s1), seg_array(seg_rows), nseg, x.rows, c, _p(sh), _p(db), cx.stream)
                _call('tg_seg_actgrad_shift_f32', gy.ptr, gy.ld, gy.ptr, gy.ld, gx.ptr, gx.ld, x.rows, c, seg_array(seg_rows), nseg, _p(sh), 0, 0.0,
                      cx.stream)
            else:
                _call('tg_actgrad_f32', gy.ptr, gy.ld, None, 0, None, 0, 1.0, gx.ptr, gx.ld, x.rows, c, 0, 0.0, cx.stream)
                if want_b:
                    colstats(0, gy.t, gy.ld, None, 0, x.rows, c, [x.rows], s1=b_grad)
        _write_grad(cx, x, store)

    cx.record(bwd)
    return y


# ------------------------------------------------------------------ batch norm (tf.contrib.layers.batch_norm, training mode)

def batch_norm_eval(x, gamma, beta, mm, mv, eps):
    """contrib batch_norm with is_training=False: y = gamma*(x-moving_mean)/sqrt(moving_var+eps)+beta (no tape: evaluation only)."""
    require_f32(x, 'batch_norm_eval')
    cx = ctx()
    c = x.c
    scale, shift = cx.scratch('bnsc', c), cx.scratch('bnsh', c)
    _call('tg_bn_eval_finalize_f32', c, _p(gamma), _p(beta), _p(mm), _p(mv), eps, _p(scale), _p(shift), cx.stream)
    y = cx.new_act(x.n, x.h, x.w, c, x.ld)
    _call('tg_seg_scale_shift_act_f32', x.ptr, x.ld, y.ptr, y.ld, x.rows, c, c, seg_array([x.rows]), 1, _p(scale), _p(shift), 0, 0.0,
          cx.stream)
    return y


def batch_norm_train(x, gamma, beta, mm, mv, eps, decay, gamma_grad=None, beta_grad=None, relu_input=False, segments=None, out_bf16=False):
    """y = gamma*(x-mu)/sqrt(var+eps)+beta over all rows (Model/modle_base.py:229-237); with `segments` (image counts of the
    applications batched into x) the statistics are per application and the moving statistics are updated application by
    application.  Fused: one statistics launch (fp64 atomics) + one apply launch per direction.
    relu_input: x is the output of a fused ReLU; the backward then also masks by x > 0 and the
    gradient it produces is wrt the PRE-ReLU value (consumed by the producing conv's backward).
    out_bf16: the caller's promise that y is read ONLY by bf16-operand 3x3 convolutions (conv2d) — with Context.act_dtype 'bf16' y is then
    stored as bf16 (tg_bn_train[_apply]_bf16), the bits those convolutions would have rounded it to; the backward pass reads x and dy only."""
    require_f32(x, 'batch_norm_train')
    cx = ctx()
    c = x.c
    trains = cx.trains()
    needs = cx.tape is not None and (x.requires_grad or trains)
    seg_rows = _segs(x, segments)
    nseg = len(seg_rows)
    mean_inv = cx.scratch('bnmi', 2 * nseg * c)
    y16 = out_bf16 and cx.act_dtype == 'bf16'
    if y16 and cx.mfma_dtype != 'bf16':
        raise lib.TgError("batch_norm_train: a bf16-stored output needs the bf16 MFMA path (MFMA_DTYPE 'bf16') behind it")
    y = cx.new_act(x.n, x.h, x.w, c, x.ld, requires_grad=needs, dtype='bf16' if y16 else 'f32')
    sfx = 'bf16' if y16 else 'f32'
    if y16:
        cx.bf16_act_layers.add(cx.scope_name())
    if x.bn_sums is not None and x.bn_sums.seg_rows == tuple(seg_rows):
        sums = x.bn_sums.sums                                # the producing convolution took the statistics in its epilogue (conv2d(bn_stats=True))
        _call('tg_bn_train_apply_' + sfx, x.ptr, x.ld, y.ptr, y.ld, x.rows, c, seg_array(seg_rows), nseg, _p(gamma), _p(beta), eps, decay, _p(mm), _p(mv),
              _p(sums), _p(mean_inv), cx.stream)
    else:
        sums, zd = _sums64(cx, 'bn64', nseg, c, pair=True)
        _call('tg_bn_train_' + sfx, x.ptr, x.ld, y.ptr, y.ld, x.rows, c, seg_array(seg_rows), nseg, _p(gamma), _p(beta), eps, decay, _p(mm), _p(mv),
              _p(sums), zd, _p(mean_inv), cx.stream)
    if cx.state_replay is not None and mm is not None:
        # this forward pass is being KEPT for a later solver run that TensorFlow would re-execute (Context.sub_tape(replay=...)): the
        # re-execution's only lasting effect is one more moving-statistics update from the same batch sums
        rows_total = x.rows
        cx.state_replay.append(lambda: _call('tg_bn_moving_update_f32', _p(sums), rows_total, c, seg_array(seg_rows), nseg, decay, _p(mm), _p(mv),
                                             cx.stream))
    if not needs:
        return y
    if x.ld == y.ld and nseg <= 8:
        _offer(y, BnBwdStats(x, tuple(seg_rows), None, None))

    def bwd():
        gy = y.grad
        assert gy is not None
        want = trains and gamma_grad is not None
        taken = _trusted(y, gy)

        def store(gx):
            if taken is not None:
                bsums, zdb = taken.sums, 2                  # the launch that produced gy took the statistics in its epilogue (tg_igemm_bnbwdstat_*)
            else:
                bsums, zdb = _sums64(cx, 'bnb64', nseg, c, pair=True)
            o = x.offer
            if isinstance(o, BiasSums) and x.ld == gx.ld and c % 4 == 0 and (c <= 256 and 256 % (c // 4) == 0 or c % 256 == 0):
                # x = act(conv + bias) of the layer in front: this pass also multiplies by act'(x) and sums the columns — what it stores IS
                # that layer's pre-activation gradient and its bias gradient is done (no tg_actgrad_bias_f32 pass over the activation)
                dsum, zds = _sums64(cx, 'bnd64', 1, c)
                _call('tg_bn_train_bwd_act_f32', gy.ptr, gy.ld, x.ptr, x.ld, gx.ptr, gx.ld, x.rows, c, seg_array(seg_rows), nseg, _p(gamma), _p(mean_inv),
                      ACT[o.act], o.alpha, _p(bsums), zdb, _p(gamma_grad) if want else None, _p(beta_grad) if want else None, _p(dsum), zds,
                      _p(o.bias_grad), cx.stream)
                x.taken = o
                return
            _call('tg_bn_train_bwd_f32', gy.ptr, gy.ld, x.ptr, x.ld, gx.ptr, gx.ld, x.rows, c, seg_array(seg_rows), nseg, _p(gamma), _p(mean_inv),
                  1 if relu_input else 0, _p(bsums), zdb, _p(gamma_grad) if want else None, _p(beta_grad) if want else None, cx.stream)
        _write_grad(cx, x, store)

    cx.record(bwd)
    return y


# ------------------------------------------------------------------ pointwise / pooling / concat

def scale_mask(x, mask_t, mscale, defer=False):
    """y = x*mask*mscale (inverted dropout, Model/modle_base.py:190-191).  defer: return a handle WITHOUT storage whose dropout the next
    op applies inside its own launch — only cond_concat does (the discriminator's dropout -> concat pairs, Good_GAN_cifar10.py:63-65,
    73-75); anything else touching the handle fails loudly on its missing buffer."""
    require_f32(x, 'scale_mask')
    cx = ctx()
    if defer:
        y = Act(None, x.n, x.h, x.w, x.c, x.ld, requires_grad=x.requires_grad)
        y.pending = Pending(x, mask_t, mscale)
        return y
    y = cx.new_act(x.n, x.h, x.w, x.c, x.ld, requires_grad=x.requires_grad)
    _call('tg_actgrad_f32', x.ptr, x.ld, None, 0, _p(mask_t), x.c, mscale, y.ptr, y.ld, x.rows, x.c, 0, 0.0, cx.stream)
    if cx.tape is not None and x.requires_grad:
        cx.record(lambda: _write_grad(cx, x, lambda gx: _call('tg_actgrad_f32', y.grad.ptr, y.grad.ld, None, 0, _p(mask_t), x.c, mscale, gx.ptr,
                                                              gx.ld, x.rows, x.c, 0, 0.0, cx.stream)))
    return y


def cond_concat(x, y_onehot_t, ncls):
    """concat([x, y*ones], 3), output channel-padded to 32 (Model/modle_base.py:239-244)."""
    require_f32(x, 'cond_concat')
    cx = ctx()
    ld = pad32(x.c + ncls)
    if x.labels == Labels(y_onehot_t.data_ptr(), ncls) and x.ld == ld and x.pending is None:
        # the producing convolution already wrote this concatenation into its own (wide) buffer: the same storage, seen with the label channels
        out = Act(x.t, x.n, x.h, x.w, x.c + ncls, ld, requires_grad=x.requires_grad)
        if cx.tape is not None and x.requires_grad:
            # the convolution's backward reads its gradient through (pointer, channel stride): no copy
            cx.record(lambda: _write_grad(cx, x, alias=Act(out.grad.t, x.n, x.h, x.w, x.c, out.grad.ld)))
        return out
    mask_t, mscale = None, 1.0
    if x.pending is not None:                    # a deferred dropout in front (scale_mask(defer=True)): one launch for both
        x, mask_t, mscale = x.pending
    out = cx.new_act(x.n, x.h, x.w, x.c + ncls, ld, requires_grad=x.requires_grad)
    _call('tg_cond_concat_f32', x.ptr, x.ld, x.c, _p(mask_t), x.c, mscale, _p(y_onehot_t), ncls, out.ptr, ld, x.n, x.h * x.w, cx.stream)
    if cx.tape is not None and x.requires_grad:
        def bwd():   # gradient of the first x.c channels; the label channels are constants
            g = out.grad
            if mask_t is None and x.strided_grad_ok:
                # no copy: x's gradient IS the leading channels of the concatenated gradient
                return _write_grad(cx, x, alias=Act(g.t, x.n, x.h, x.w, x.c, g.ld))
            _write_grad(cx, x, lambda gx: _call('tg_actgrad_f32', g.ptr, g.ld, None, 0, _p(mask_t), x.c if mask_t is not None else 0, mscale, gx.ptr,
                                                gx.ld, x.rows, x.c, 0, 0.0, cx.stream))
        cx.record(bwd)
    return out


def pad_add(x, add_t, ld_out):
    """x + noise, channel-padded (classifier input; no gradient is ever needed upstream)."""
    require_f32(x, 'pad_add')
    cx = ctx()
    out = cx.new_act(x.n, x.h, x.w, x.c, ld_out)
    _call('tg_pad_add_f32', x.ptr, x.ld, x.c, _p(add_t), x.c, out.ptr, ld_out, x.rows, cx.stream)
    return out


def im2col3x3_add(x, add_t):
    """3x3 SAME patches of (x + noise) as a [n,h,w,9*c] activation (channel stride padded to 32): the classifier's
    first conv then runs as a 1x1 product over K = 27 instead of K = 9*32 (no gradient is needed upstream)."""
    require_f32(x, 'im2col3x3_add')
    cx = ctx()
    assert x.ld == x.c
    out = cx.new_act(x.n, x.h, x.w, 9 * x.c, pad32(9 * x.c))
    _call('tg_im2col3x3_add_f32', x.ptr, _p(add_t), x.n, x.h, x.w, x.c, out.ptr, out.ld, cx.stream)
    return out


def maxpool2_dropout(y, mask_t, mscale):
    """tf.nn.max_pool 2x2 + tf.layers.dropout (Model/Good_GAN_cifar10.py:123-124)."""
    require_f32(y, 'maxpool2_dropout')
    cx = ctx()
    out = cx.new_act(y.n, y.h // 2, y.w // 2, y.c, y.ld, requires_grad=y.requires_grad)
    _call('tg_maxpool2_fwd_f32', y.ptr, y.ld, out.ptr, out.ld, _p(mask_t), y.c, mscale, y.n, y.h, y.w, y.c, cx.stream)
    _record_maxpool_bwd(cx, y, out, mask_t, mscale)
    return out


def _record_maxpool_bwd(cx, y, out, mask_t, mscale):
    """backward closure of max-pool 2x2 + dropout from y to out (shared by maxpool2_dropout and the fused apply + pool launch of conv2d)."""
    if cx.tape is not None and y.requires_grad:
        def bwd():
            first, o = y.grad is None, y.offer

            def store(gy):
                if (isinstance(o, ActSums) and first and y.c % 4 == 0 and y.c <= 512 and sum(o.seg_rows) == y.rows
                        and all(r % (y.h * y.w) == 0 for r in o.seg_rows)):
                    # y is the output of a mean-only-BN layer: route, multiply by its activation derivative and sum the columns in one pass
                    nsg = len(o.seg_rows)
                    gsum, zd = _sums64(cx, 'ps64', nsg, y.c)
                    _call('tg_maxpool2_bwd_actsum_f32', out.grad.ptr, out.grad.ld, _p(mask_t), y.c, mscale, y.ptr, y.ld, gy.ptr, gy.ld, y.n, y.h, y.w,
                          y.c, seg_array(o.seg_rows), nsg, ACT[o.act], o.alpha, _p(gsum), zd, cx.stream)
                    y.taken = o._replace(sums=gsum, replicas=STATS_REPLICAS)
                else:
                    _call('tg_maxpool2_bwd_f32', out.grad.ptr, out.grad.ld, _p(mask_t), y.c, mscale, y.ptr, y.ld, gy.ptr, gy.ld, y.n, y.h, y.w,
                          y.c, cx.stream)
            _write_grad(cx, y, store)
        cx.record(bwd)


def global_maxpool(x):
    require_f32(x, 'global_maxpool')
    cx = ctx()
    out = cx.new_act(x.n, 1, 1, x.c, pad32(x.c), requires_grad=x.requires_grad)
    _call('tg_gmaxpool_fwd_f32', x.ptr, x.ld, out.ptr, out.ld, x.n, x.h * x.w, x.c, cx.stream)
    if cx.tape is not None and x.requires_grad:
        cx.record(lambda: _write_grad(cx, x, lambda gx: _call('tg_gmaxpool_bwd_f32', out.grad.ptr, out.grad.ld, x.ptr, x.ld, gx.ptr, gx.ld, x.n,
                                                              x.h * x.w, x.c, cx.stream)))
    return out


def global_avgpool_concat(x, y_onehot_t, ncls):
    """average_pooling2d over the whole map + squeeze + concat([h, y], 1) (Good_GAN_cifar10.py:94-96)."""
    require_f32(x, 'global_avgpool_concat')
    cx = ctx()
    out = cx.new_act(x.n, 1, 1, x.c + ncls, pad32(x.c + ncls), requires_grad=x.requires_grad)
    _call('tg_gavgpool_concat_f32', x.ptr, x.ld, x.c, _p(y_onehot_t), ncls, out.ptr, out.ld, x.n, x.h * x.w, cx.stream)
    if cx.tape is not None and x.requires_grad:
        cx.record(lambda: _write_grad(cx, x, lambda gx: _call('tg_gavgpool_bwd_f32', out.grad.ptr, out.grad.ld, x.ptr, x.ld, gx.ptr, gx.ld, x.n,
                                                              x.h * x.w, x.c, 0, 0.0, cx.stream)))
    return out


def global_avgpool(x):
    """tf.reduce_mean(x, axis=[1,2]) (Model/Good_GAN.py:198,346) -> [N,C]: global_avgpool_concat without labels."""
    require_f32(x, 'global_avgpool')
    return global_avgpool_concat(x, None, 0)


def minibatch_discrimination(x, w, b, num_kernels, dim, w_grad=None, b_grad=None, concat_input=False):
    """NN_Base._minibatch_discrimination (Model/modle_base.py:110-128) on a dense [n, c] activation: A = x @ W (a 1-tap MFMA product),
    f[i,k] = sum_j exp(-|A[i,k,:] - A[j,k,:]|_1) + b[k].  Returns f, or concat([x, f], 1) when concat_input (what the SVHN
    discriminator does with it, Model/Good_GAN.py:160-161)."""
    require_f32(x, 'minibatch_discrimination')
    cx = ctx()
    holder = {}
    skip = concat_input and cx.tape is not None and x.requires_grad
    if skip:
        def bwd_skip():      # recorded BEFORE the product, so it runs after the product's input gradient has been written to x.grad
            g, gx = holder['g'], cx.grad_of(x)
            _call('tg_pad_add_f32', gx.ptr, gx.ld, x.c, g.ptr, g.ld, gx.ptr, gx.ld, x.rows, cx.stream)
        cx.record(bwd_skip)
    a = conv2d(x, w, None, num_kernels * dim, 1, 1, 'SAME', kernel_grad=w_grad)
    c0 = x.c if concat_input else 0
    out = cx.new_act(x.n, 1, 1, c0 + num_kernels, pad32(c0 + num_kernels), requires_grad=a.requires_grad)
    _call('tg_minibatch_disc_fwd_f32', a.ptr, a.ld, x.ptr, x.ld, c0, _p(b), out.ptr, out.ld, x.n, num_kernels, dim, cx.stream)
    if cx.tape is not None and a.requires_grad:
        def bwd():
            g = out.grad
            holder['g'] = g
            _write_grad(cx, a, lambda ga: _call('tg_minibatch_disc_bwd_f32', a.ptr, a.ld, C.c_void_p(g.t.data_ptr() + 4 * c0), g.ld, ga.ptr, ga.ld,
                                                _p(b_grad), x.n, num_kernels, dim, cx.stream))
        cx.record(bwd)
    return out


def argmax_onehot(logits, k):
    require_f32(logits, 'argmax_onehot')
    cx = ctx()
    out = cx.scratch('oh', logits.n * k)
    _call('tg_argmax_onehot_f32', logits.ptr, logits.ld, logits.n, k, _p(out), cx.stream)
    return out


def copy2d(dst_t, ld_d, dst_col, src_t, ld_s, rows, c):
    """dst[r][dst_col : dst_col+c] = src[r][:c] (strided device copy)."""
    cx = ctx()
    _call('tg_copy2d_f32', C.c_void_p(src_t.data_ptr()), ld_s, C.c_void_p(dst_t.data_ptr() + 4 * dst_col), ld_d, rows, c, cx.stream)


def copy_rows(dst_t, dst_off, src_t, numel):
    """contiguous device copy (batch concatenation along N)."""
    copy2d(dst_t, int(numel), int(dst_off), src_t, int(numel), 1, int(numel))


def copy_many(jobs):
    """[(dst tensor, dst element offset, src tensor, numel)] as contiguous device copies, 16 per launch (tg_copy_multi_f32)."""
    cx = ctx()
    jobs = [j for j in jobs if j[3] > 0]
    for k in range(0, len(jobs), 16):
        part = jobs[k:k + 16]
        arr = (lib.CopyJob * len(part))(*[lib.CopyJob(s.data_ptr(), d.data_ptr() + 4 * int(off), int(n)) for d, off, s, n in part])
        _call('tg_copy_multi_f32', arr, len(part), cx.stream)


def reshape(x, n, h, w, c):
    """view change of a dense (ld == c) buffer, e.g. [N,8192] -> [N,4,4,512]; gradients share storage."""
    require_f32(x, 'reshape')
    cx = ctx()
    assert x.ld == x.c and n * h * w * c == x.rows * x.c
    y = Act(x.t, n, h, w, c, c, x.requires_grad)
    if cx.tape is not None and x.requires_grad:
        cx.record(lambda: _write_grad(cx, x, alias=Act(y.grad.t, x.n, x.h, x.w, x.c, x.c)))
    return y


def add_noise(x, noise_t):
    """x + noise on a dense activation (NN_Base._add_noise, Model/modle_base.py:193-202); the gradient passes through."""
    require_f32(x, 'add_noise')
    cx = ctx()
    y = cx.new_act(x.n, x.h, x.w, x.c, x.ld, requires_grad=x.requires_grad)
    _call('tg_pad_add_f32', x.ptr, x.ld, x.c, _p(noise_t), x.c, y.ptr, y.ld, x.rows, cx.stream)
    if cx.tape is not None and x.requires_grad:
        cx.record(lambda: _write_grad(cx, x, alias=Act(y.grad.t, x.n, x.h, x.w, x.c, y.grad.ld)))
    return y


def view(x, h, w, c):
    """reinterpret a dense activation's per-image shape (tf.reshape), gradients share storage."""
    return reshape(x, x.n, h, w, c)


def concat_batch(acts):
    """tf.concat(acts, 0) of network OUTPUTS: the parts receive views of the concatenated gradient."""
    require_f32(acts, 'concat_batch')
    from .batching import concat_acts
    cx = ctx()
    out = concat_acts(acts)
    out.requires_grad = any(a.requires_grad for a in acts)
    if cx.tape is not None and out.requires_grad:
        def bwd():
            if out.grad is None:          # e.g. the concatenated features: no loss term of Train_goodGAN.py uses them
                return
            off = 0
            for a in acts:
                _write_grad(cx, a, alias=out.grad.view_rows(off, off + a.n))
                off += a.n
        cx.record(bwd)
    return out


# ------------------------------------------------------------------ stand-alone activation / batch norm of the reference's free functions

def activation(x, act, alpha=0.2):
    """y = act(x) as its own launch (an activation CALLED on a tensor, e.g. Good_GAN_cifar10.leakyReLu(x), NN_Base._relu(x)); the models
    pass their activations as `nonlinearity=` / `activation=` instead and get them fused into the producing kernel's epilogue."""
    require_f32(x, 'activation')
    cx = ctx()
    y = cx.new_act(x.n, x.h, x.w, x.c, x.ld, requires_grad=x.requires_grad)
    y.strided_grad_ok = True
    _call('tg_act_f32', x.ptr, x.ld, y.ptr, y.ld, x.rows, x.c, ACT[act], alpha, cx.stream)
    if cx.tape is not None and x.requires_grad:
        cx.record(lambda: _write_grad(cx, x, lambda gx: _call('tg_actgrad_f32', y.grad.ptr, y.grad.ld, y.ptr, y.ld, None, 0, 1.0, gx.ptr, gx.ld, x.rows,
                                                              x.c, ACT[act], alpha, cx.stream)))
    return y


def batch_norm_moments(x, scale, beta, pop_mean, pop_var, eps, decay, train, scale_grad=None, beta_grad=None):
    """nn.batch_norm_impl (Model/nn.py:192-217): tf.nn.moments + tf.nn.batch_normalization with the running statistics updated
    as pop <- pop*decay + batch*(1-decay) from the BIASED batch variance (tf.nn.moments; contrib's fused batch_norm — ops.batch_norm_train —
    feeds the unbiased one), or, train=False, normalisation by the running statistics.  Two-pass centred variance as tf.nn.moments."""
    require_f32(x, 'batch_norm_moments')
    cx = ctx()
    c = x.c
    if not train:
        return batch_norm_eval(x, scale, beta, pop_mean, pop_var, eps)
    trains = cx.trains()
    needs = cx.tape is not None and (x.requires_grad or trains)
    s1, _ = colstats(0, x.t, x.ld, None, 0, x.rows, c, [x.rows])
    s2, _ = colstats(4, x.t, x.ld, s1, 0, x.rows, c, [x.rows], alpha=1.0 / x.rows)
    sc, sh, mean_inv = cx.scratch('bnsc', c), cx.scratch('bnsh', c), cx.scratch('bnmi', 2 * c)
    _call('tg_bn_finalize_f32', _p(s1), _p(s2), x.rows, c, _p(scale), _p(beta), eps, _p(sc), _p(sh), _p(mean_inv), _p(pop_mean), _p(pop_var), decay, 0,
          cx.stream)
    y = cx.new_act(x.n, x.h, x.w, c, x.ld, requires_grad=needs)
    _call('tg_seg_scale_shift_act_f32', x.ptr, x.ld, y.ptr, y.ld, x.rows, c, c, seg_array([x.rows]), 1, _p(sc), _p(sh), 0, 0.0, cx.stream)
    if not needs:
        return y

    def bwd():
        gy = y.grad
        assert gy is not None

        def store(gx):
            d1, d2 = colstats(3, gy.t, gy.ld, x.t, x.ld, x.rows, c, [x.rows])
            abc = cx.scratch('bnabc', 3 * c)
            want = trains and scale_grad is not None
            dg = scale_grad if want else cx.scratch('bndg', c)
            db = beta_grad if want else cx.scratch('bndb', c)
            _call('tg_bn_bwd_finalize_f32', _p(d1), _p(d2), x.rows, c, _p(scale), _p(mean_inv), _p(abc), _p(dg), _p(db), cx.stream)
            _call('tg_bn_bwd_apply_f32', gy.ptr, gy.ld, x.ptr, x.ld, gx.ptr, gx.ld, x.rows, c, _p(abc), 0, cx.stream)
        _write_grad(cx, x, store)

    cx.record(bwd)
    return y


def moments_normalize(x, eps, init_scale=1.0):
    """scale_init * (x - m_init) with m, v = tf.nn.moments(x, all axes but the last), scale_init = init_scale / sqrt(v + eps): the value
    the data-dependent-initialisation branch (init=True) of the Salimans layers returns (Model/nn.py:230-243,263-277,302-316).
    Forward only (the reference never differentiates that branch: its models call it once to create variables)."""
    require_f32(x, 'moments_normalize')
    cx = ctx()
    c = x.c
    s1, _ = colstats(0, x.t, x.ld, None, 0, x.rows, c, [x.rows])
    s2, _ = colstats(4, x.t, x.ld, s1, 0, x.rows, c, [x.rows], alpha=1.0 / x.rows)
    sc, sh, mi = cx.scratch('bnsc', c), cx.scratch('bnsh', c), cx.scratch('bnmi', 2 * c)
    g, b = cx.ws('const:init_scale%g' % init_scale, c), cx.ws('const:zeros', max(c, 1024))
    fill(g, init_scale)
    _call('tg_bn_finalize_f32', _p(s1), _p(s2), x.rows, c, _p(g), _p(b), eps, _p(sc), _p(sh), _p(mi), None, None, 0.0, 0, cx.stream)
    y = cx.new_act(x.n, x.h, x.w, c, x.ld)
    _call('tg_seg_scale_shift_act_f32', x.ptr, x.ld, y.ptr, y.ld, x.rows, c, c, seg_array([x.rows]), 1, _p(sc), _p(sh), 0, 0.0, cx.stream)
    return y


def wn_data_init(t, g, b, eps, init_scale, act=None, alpha=0.0):
    """Data-dependent initialisation of a weight-normalised layer (Salimans & Kingma 2016; Model/nn.py:492-500, Model/modle_base.py:68-71)
    from its unit-gain pre-activation t = conv(x, V/||V||) (the layer's ordinary launch with wn=(ones, None)): with m, v the moments of t
    over all axes but the last (biased variance, two passes in fp64),  g <- init_scale / sqrt(v + eps),  b <- -m * g  are WRITTEN into the
    variables' tensors `g`, `b` ([t.c] each), and act(g*t + b) - what the layer evaluates from then on - is returned.  Forward only, recorded
    nowhere, refused inside a hipGraph capture / launch-plan recording: it runs once, before a step exists.  The launch is tg/wn_init.py's:
    this module's launches are the ones a recorded step replays (tests/launch_trace.py pins them), and this one never is."""
    from . import wn_init
    return wn_init.data_init(t, g, b, eps, init_scale, act, alpha)
