"""Float64 restatements of tg/ops.py with a propagated error bound (helper of tests/test_ops_reference.py and tests/test_gpu_ops_routes.py).

Every quantity is a `V`: a torch tensor `v` and, element by element, a bound `e` on |what a correct fp32 implementation holds - v|.  The
bound is first-order propagation in the manner of tests/kernel_check.py, built stage by stage by the primitives below, so a formula
written with them carries its own bound and no constant is chosen by eye:
  reduction   (rsum, bilin: a convolution or its two gradients)   TOL * (the operator applied to |operands|), TOL = kernel_check.TOL;
  pointwise   (add, sub, mul, scale, div, rsqrt, vexp, act)       K u |value|, u = 2^-24, K written beside each primitive;
  incoming    a bound passes through a stage by the stage's absolute-value operator (|a| e_b + |b| e_a for a product, the magnitude of
              the derivative for division, rsqrt, exp and the activations, the same selection for data movement);
  bf16        an MFMA operand the route rounds to bf16 is rounded with oracle.tf_ops.bf16_round, an activation stored as bf16 with
              kernel_check.bf16_rne_bits.  Rounding is monotone: a device value within e of v rounds into [rne(v - e), rne(v + e)], so the
              bound of the rounded value is its distance to the farther end of that interval - 0 (bit for bit) wherever v - e and v + e
              round to the same bf16 number, in particular for every exact operand (e = 0: an input, a variable), one bf16 step where a
              rounding boundary lies within e of v.
The functions work in the dtype of the tensors they are given: tests/test_ops_reference.py evaluates them in float32 and shows that such
an evaluation stays inside the bound of the float64 one.

Decisions that are not differentiable: relu / lrelu masks in a backward pass come from the STORED forward output of the implementation
under test (`stored`, what its backward kernels read; the forward output is held to float64 on its own); the arg-max of a pooling window
is the reference's own, and `pool_margin` records the smallest (gap between the two largest values) / (4 x their forward bound) so that a
test can assert, before any launch, that no window's decision is within reach of rounding.

`RefOps` gives these functions the call signatures of tg.ops and `RefRunner` the interface of launch_trace.Tracer, so that the case bodies
of tests/launch_trace.py run on them unchanged: whatever route tg/ops.py takes for a case, this is the number it has to produce."""
import contextlib
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import kernel_check as KC
from oracle import tf_ops as T
from tg.ops import Labels, Pending

U, TOL = KC.U, KC.TOL
F64 = torch.float64
ALPHA = float(KC.ALPHA)


def f32c(x):
    """a Python constant as the fp32 number the kernels receive"""
    return float(np.float32(x))


class V(object):
    """value and bound"""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros(v.shape, dtype=F64) if e is None else e

    @property
    def shape(self):
        return tuple(self.v.shape)

    def map(self, fn):
        """data movement / selection: the same on the value and on the bound"""
        return V(fn(self.v), fn(self.e))

    def reshape(self, *s):
        return self.map(lambda t: t.reshape(*s))


def _a(t):
    return t.detach().abs().to(F64)


def const(x, like):
    return V(torch.as_tensor(x, dtype=like.v.dtype))


def _rounded(v, e, k=1):
    return V(v, e + k * U * _a(v))


def add(a, b):                       # K = 1
    return _rounded(a.v + b.v, a.e + b.e)


def sub(a, b):                       # K = 1
    return _rounded(a.v - b.v, a.e + b.e)


def mul(a, b):                       # K = 1
    return _rounded(a.v * b.v, _a(a.v) * b.e + _a(b.v) * a.e)


def scale(a, s):                     # K = 1; s an fp32 constant
    return _rounded(a.v * s, abs(s) * a.e)


def div(a, b):                       # K = 1; |d/da| = 1/|b|, |d/db| = |a/b|/|b|
    v = a.v / b.v
    return _rounded(v, a.e / _a(b.v) + _a(v) / _a(b.v) * b.e)


def rsqrt(a):                        # K = 2 (square root, reciprocal); |d/da| = |v| / (2 |a|)
    v = a.v.rsqrt()
    return _rounded(v, 0.5 * _a(v) / _a(a.v) * a.e, 2)


def vexp(a):                         # K = 4 (expf within 2 ulp, 1 ulp <= 2u: tests/test_gpu_elementwise.py); |d/da| = v
    v = a.v.exp()
    return _rounded(v, _a(v) * a.e, 4)


def addn(*terms):
    """t0 + t1 + ... in whatever order and grouping: each of the n - 1 roundings is of a partial sum no larger than sum |t_i|
    (K = n - 1 on that magnitude; x - mean + b is evaluated by the kernels as x + (b - mean))"""
    v = sum(t.v for t in terms[1:]) + terms[0].v
    mag = sum(_a(t.v) for t in terms[1:]) + _a(terms[0].v)
    return V(v, sum(t.e for t in terms[1:]) + terms[0].e + (len(terms) - 1) * U * mag)


def neg(a):
    return V(-a.v, a.e)


def rsum(a, dims, keepdim=False):
    """sum over `dims`: a reduction stage"""
    return V(a.v.sum(dims, keepdim=keepdim), a.e.sum(dims, keepdim=keepdim) + TOL * _a(a.v).sum(dims, keepdim=keepdim))


def bilin(fn, a, b):
    """fn(a, b) bilinear (a convolution, one of its gradients, a matrix product): a reduction stage"""
    A, B = _a(a.v), _a(b.v)
    return V(fn(a.v, b.v), fn(A, b.e) + fn(a.e, B) + TOL * fn(A, B))


def vcat(parts, dim=0):
    return V(torch.cat([p.v for p in parts], dim), torch.cat([p.e for p in parts], dim))


def _rne_stored(x):
    """fp32 -> the bf16 number kernel_check.bf16_rne_bits stores, as fp32"""
    return (KC.bf16_rne_bits(x).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16q(a, rne=T.bf16_round):
    """an MFMA operand of the bf16 path (see the module docstring)"""
    x, e = a.v.detach().to(F64).numpy(), a.e.numpy()
    mid, lo, hi = (np.asarray(rne(np.ascontiguousarray(t, np.float32)), np.float64) for t in (x, x - e, x + e))
    return V(torch.from_numpy(mid).to(a.v.dtype), torch.from_numpy(np.maximum(hi - mid, mid - lo)))


def bf16_store(a):
    """an activation stored as bf16: round to nearest even of the fp32 value"""
    return bf16q(a, _rne_stored)


# ------------------------------------------------------------------ activations

ACT_K = {None: 0, 'none': 0, 'relu': 1, 'lrelu': 1, 'tanh': 4, 'sigmoid': 6, 'softplus': 6}       # tests/test_gpu_elementwise.py


def act(x, kind, alpha=ALPHA):
    """act(x); the derivative's magnitude is at most 1 for every kind here (a relu-family mask may differ where |x| <= e: slope <= 1)"""
    v = x.v
    if kind in (None, 'none'):
        return x
    if kind == 'relu':
        y = torch.where(v > 0, v, torch.zeros_like(v))
    elif kind == 'lrelu':
        y = torch.where(v > 0, v, alpha * v)
    elif kind == 'tanh':
        y = torch.tanh(v)
    elif kind == 'sigmoid':
        y = torch.sigmoid(v)
    elif kind == 'softplus':
        y = F.softplus(v)
    else:
        raise ValueError(kind)
    return _rounded(y, x.e, ACT_K[kind])


def act_bwd(gy, y, kind, alpha=ALPHA, stored=None):
    """gy * act'(y) through the activation OUTPUT; relu / lrelu take the mask from `stored` (the implementation's forward output)"""
    if kind in (None, 'none'):
        return gy
    if kind in ('relu', 'lrelu'):
        src = y.v if stored is None else stored
        one = torch.ones_like(y.v)
        return mul(gy, V(torch.where(src > 0, one, (alpha if kind == 'lrelu' else 0.0) * one)))
    one = const(1.0, y)
    if kind == 'tanh':
        return mul(gy, sub(one, mul(y, y)))
    if kind == 'sigmoid':
        return mul(gy, mul(y, sub(one, y)))
    if kind == 'softplus':
        return mul(gy, sub(one, vexp(neg(y))))
    raise ValueError(kind)


# ------------------------------------------------------------------ convolutions (NHWC activations, HWIO filters)

def _conv_raw(x, w, stride, padding):
    k = w.shape[0]
    _, _, pt, pb, pl, pr = T._out_and_pad(x.shape[1], x.shape[2], k, k, stride, stride, padding)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, w.permute(3, 2, 0, 1), stride=stride).permute(0, 2, 3, 1)


def _conv_dx_raw(dy, w, xshape, stride, padding):
    x0 = torch.zeros(xshape, dtype=dy.dtype, requires_grad=True)
    return torch.autograd.grad(_conv_raw(x0, w, stride, padding), x0, dy)[0]


def _conv_dw_raw(x, dy, wshape, stride, padding):
    w0 = torch.zeros(wshape, dtype=dy.dtype, requires_grad=True)
    return torch.autograd.grad(_conv_raw(x, w0, stride, padding), w0, dy)[0]


def conv_fwd(x, w, stride=1, padding='SAME'):
    """tf.nn.conv2d"""
    return bilin(lambda a, b: _conv_raw(a, b, stride, padding), x, w)


def conv_dx(dy, w, xshape, stride=1, padding='SAME'):
    return bilin(lambda a, b: _conv_dx_raw(a, b, xshape, stride, padding), dy, w)


def conv_dw(x, dy, wshape, stride=1, padding='SAME'):
    return bilin(lambda a, b: _conv_dw_raw(a, b, wshape, stride, padding), x, dy)


def deconv_fwd(x, w):
    """tf conv2d_transpose 5x5 stride 2 'same', filter [5,5,c_out,c_in]: the input gradient of the stride-2 convolution c_out -> c_in"""
    n, h, wd, _ = x.shape
    return conv_dx(x, w, (n, 2 * h, 2 * wd, w.shape[2]), 2, 'SAME')


def deconv_dx(dy, w):
    return conv_fwd(dy, w, 2, 'SAME')


def deconv_dw(x, dy, wshape):
    return conv_dw(dy, x, wshape, 2, 'SAME')


# ------------------------------------------------------------------ weight norm

def wn_weight(v, g, out_axis=-1):
    """W = g V / ||V||, the norm over every axis but `out_axis` (conv: the last; the transposed-conv table [5,5,c_out,c_in]: axis 2)"""
    out_axis %= v.v.dim()
    axes = tuple(a for a in range(v.v.dim()) if a != out_axis)
    shp = [1] * v.v.dim()
    shp[out_axis] = -1
    inv = rsqrt(rsum(mul(v, v), axes, keepdim=True))
    return mul(v, mul(g.reshape(shp), inv))


def wn_weight_bwd(v, g, dw, out_axis=-1):
    """(dV, dg) of W = g V/||V||"""
    out_axis %= v.v.dim()
    axes = tuple(a for a in range(v.v.dim()) if a != out_axis)
    shp = [1] * v.v.dim()
    shp[out_axis] = -1
    inv = rsqrt(rsum(mul(v, v), axes, keepdim=True))
    vhat = mul(v, inv)
    dot = rsum(mul(dw, vhat), axes, keepdim=True)
    dv = mul(mul(g.reshape(shp), inv), sub(dw, mul(vhat, dot)))
    return dv, dot.reshape(-1)


# ------------------------------------------------------------------ segments, mean-only BN, batch norm

def seg_bounds(n, segments):
    segments = [n] if segments is None else list(segments)
    assert sum(segments) == n, (segments, n)
    out, a = [], 0
    for s in segments:
        out.append((a, a + s))
        a += s
    return out


def _rows_of(x):
    return x.shape[0] * x.shape[1] * x.shape[2]


def col_mean(x):
    return scale(rsum(x, (0, 1, 2)), 1.0 / _rows_of(x))


def mobn_train(x, b, pop, segments=None, decay=0.9):
    """x - mean_seg + b per application segment; pop <- decay pop + (1 - decay) mean_seg, segment after segment.  -> (y, pop)"""
    d = f32c(decay)
    parts = []
    for lo, hi in seg_bounds(x.shape[0], segments):
        xs = x.map(lambda t: t[lo:hi])
        m = col_mean(xs)
        parts.append(addn(xs, neg(m), b))
        pop = add(scale(pop, d), scale(m, 1.0 - d))
    return vcat(parts), pop


def mobn_eval(x, b, pop):
    return addn(x, neg(pop), b)


def seg_center(g, segments=None):
    """g - mean_seg(g): the backward of the mean subtraction"""
    parts = []
    for lo, hi in seg_bounds(g.shape[0], segments):
        gs = g.map(lambda t: t[lo:hi])
        parts.append(sub(gs, col_mean(gs)))
    return vcat(parts)


def _moments(xs):
    """(mean, biased variance, x - mean) over all axes but the last"""
    m = col_mean(xs)
    xc = sub(xs, m)
    return m, scale(rsum(mul(xc, xc), (0, 1, 2)), 1.0 / _rows_of(xs)), xc


def batch_norm_train(x, gamma, beta, mm, mv, eps, decay, segments=None):
    """contrib batch_norm, training mode, per application segment; the moving statistics take the unbiased variance, segment after
    segment.  -> (y, mm, mv, cache for the backward)"""
    d, eps = f32c(decay), f32c(eps)
    parts, cache = [], []
    for lo, hi in seg_bounds(x.shape[0], segments):
        xs = x.map(lambda t: t[lo:hi])
        m, var, xc = _moments(xs)
        inv = rsqrt(add(var, const(eps, var)))
        xhat = mul(xc, inv)
        parts.append(add(mul(xhat, gamma), beta))
        cache.append((lo, hi, xhat, inv))
        if mm is not None:
            mm, mv = bn_moving_update(mm, mv, m, var, _rows_of(xs), d, bessel=True)
    return vcat(parts), mm, mv, cache


def bn_moving_update(mm, mv, m, var, rows, d, bessel):
    v = scale(var, rows / float(max(rows - 1, 1))) if bessel else var
    return add(scale(mm, d), scale(m, 1.0 - d)), add(scale(mv, d), scale(v, 1.0 - d))


def batch_norm_train_bwd(gy, gamma, cache, relu_mask=None):
    """-> (dx, dgamma, dbeta); relu_mask: the stored input > 0 (relu_input: the gradient is then at the pre-ReLU value)"""
    parts, dgam, dbet = [], None, None
    for lo, hi, xhat, inv in cache:
        gs = gy.map(lambda t: t[lo:hi])
        rows = _rows_of(gs)
        db = rsum(gs, (0, 1, 2))
        dg = rsum(mul(gs, xhat), (0, 1, 2))
        t = sub(sub(gs, scale(db, 1.0 / rows)), mul(xhat, scale(dg, 1.0 / rows)))
        parts.append(mul(mul(gamma, inv), t))
        dgam = dg if dgam is None else add(dgam, dg)
        dbet = db if dbet is None else add(dbet, db)
    dx = vcat(parts)
    if relu_mask is not None:
        dx = mul(dx, V(relu_mask.to(dx.v.dtype)))
    return dx, dgam, dbet


def batch_norm_eval(x, gamma, beta, mm, mv, eps):
    sc = mul(gamma, rsqrt(add(mv, const(f32c(eps), mv))))
    return add(mul(x, sc), sub(beta, mul(mm, sc)))


def batch_norm_moments(x, gamma, beta, pm, pv, eps, decay):
    """tf.nn.moments + tf.nn.batch_normalization, one segment; the running statistics take the BIASED variance.  -> (y, pm, pv, cache)"""
    m, var, xc = _moments(x)
    inv = rsqrt(add(var, const(f32c(eps), var)))
    xhat = mul(xc, inv)
    y = add(mul(xhat, gamma), beta)
    if pm is not None:
        pm, pv = bn_moving_update(pm, pv, m, var, _rows_of(x), f32c(decay), bessel=False)
    return y, pm, pv, [(0, x.shape[0], xhat, inv)]


def moments_normalize(x, eps, init_scale=1.0):
    m, var, xc = _moments(x)
    return mul(xc, scale(rsqrt(add(var, const(f32c(eps), var))), f32c(init_scale)))


# ------------------------------------------------------------------ dropout, pooling, concat

def dropout(x, mask, mscale):
    """x * mask * mscale (inverted dropout; mask [n,h,w,c] of 0 / 1)"""
    return x if mask is None else mul(x, scale(mask, f32c(mscale)))


def _windows(t):
    """[n,h,w,c] -> [n,h/2,w/2,c,4] (floor: tf.nn.max_pool 2x2 stride 2 VALID)"""
    n, h, w, c = t.shape
    t = t[:, :h // 2 * 2, :w // 2 * 2]
    return t.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)


def _margin(vals, errs, dim):
    """min over the windows of (largest - second largest) / (4 x the larger of their two bounds)"""
    top, idx = vals.to(F64).topk(2, dim)
    e = errs.gather(dim, idx).amax(dim)
    return float(((top.select(dim, 0) - top.select(dim, 1)) / (4 * e + 1e-300)).min())


def maxpool2(x):
    """-> (pooled, arg-max index [n,h/2,w/2,c], margin)"""
    wv, we = _windows(x.v), _windows(x.e)
    idx = wv.argmax(-1, keepdim=True)
    return V(wv.gather(-1, idx)[..., 0], we.gather(-1, idx)[..., 0]), idx, _margin(wv, we, -1)


def maxpool2_bwd(g, idx, xshape):
    n, h, w, c = xshape

    def route(t):
        z = torch.zeros(n, h // 2, w // 2, c, 4, dtype=t.dtype).scatter_(-1, idx, t[..., None])
        full = torch.zeros(xshape, dtype=t.dtype)
        full[:, :h // 2 * 2, :w // 2 * 2] = z.reshape(n, h // 2, w // 2, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n, h // 2 * 2, w // 2 * 2, c)
        return full
    return g.map(route)


def global_maxpool(x):
    n, h, w, c = x.shape
    fv, fe = x.v.reshape(n, h * w, c), x.e.reshape(n, h * w, c)
    idx = fv.argmax(1, keepdim=True)
    return V(fv.gather(1, idx).reshape(n, 1, 1, c), fe.gather(1, idx).reshape(n, 1, 1, c)), idx, (_margin(fv, fe, 1) if h * w > 1 else float('inf'))


def global_maxpool_bwd(g, idx, xshape):
    n, h, w, c = xshape
    return g.map(lambda t: torch.zeros(n, h * w, c, dtype=t.dtype).scatter_(1, idx, t.reshape(n, 1, c)).reshape(xshape))


def global_avgpool(x):
    return scale(rsum(x, (1, 2), keepdim=True), 1.0 / (x.shape[1] * x.shape[2]))


def global_avgpool_bwd(g, xshape):
    return scale(g, 1.0 / (xshape[1] * xshape[2])).map(lambda t: t.expand(xshape).clone())


def cond_concat(x, labels):
    """concat([x, y * ones], 3); labels [n, ncls]"""
    n, h, w, _ = x.shape
    return x.map(lambda t: t) if labels is None else vcat([x, labels.map(lambda t: t.reshape(n, 1, 1, -1).expand(n, h, w, -1))], 3)


def im2col3x3(x):
    """3x3 SAME stride-1 patches [n,h,w,9c], tap-major (t*c + k), zero outside the image"""
    def f(t):
        n, h, w, c = t.shape
        p = F.pad(t, (0, 0, 1, 1, 1, 1))
        return torch.cat([p[:, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], 3)
    return x.map(f)


def minibatch_disc(a, b, num_kernels, dim):
    """f[i,k] = sum_j exp(-|A[i,k,:] - A[j,k,:]|_1) + b[k] from A [n, num_kernels*dim].  -> (f [n, num_kernels], cache)"""
    n = a.shape[0]
    A = a.reshape(n, num_kernels, dim)
    D = sub(A.map(lambda t: t[:, None]), A.map(lambda t: t[None]))          # [i, j, k, d]
    E = vexp(neg(rsum(D.map(torch.abs), 3)))                                # [i, j, k]
    return add(rsum(E, 1), b), (D, E)


def minibatch_disc_bwd(gf, cache):
    """-> (dA [n, num_kernels*dim], db)"""
    D, E = cache
    n = gf.shape[0]
    t = mul(gf.map(lambda x: x[:, None]), E)                                # d f[i,k] / d(-L1[i,j,k]) * gf[i,k]
    sgn = V(torch.sign(D.v))
    s = mul(neg(t).map(lambda x: x[..., None]), sgn)                        # gradient at D[i,j,k,d]
    dA = sub(rsum(s, 1), rsum(s, 0))                                        # D = A_i - A_j
    return dA.reshape(n, -1), rsum(gf, 0)


# ================================================================== the tg.ops signatures on these functions

def pad32(c):
    return (c + 31) // 32 * 32


class RT(object):
    """a labelled flat tensor of a case (a variable, a gradient destination, a mask, ...)"""

    def __init__(self, label, val):
        self.label, self.val, self.written = label, val, False

    def set(self, val):
        assert val.v.numel() == self.val.v.numel(), (self.label, val.shape, self.val.shape)
        self.val, self.written = val.reshape(-1), True

    def numel(self):
        return self.val.v.numel()


class RAct(object):
    """an activation [n,h,w,c]; ld / labels / dtype only mirror what the case bodies assert on"""

    def __init__(self, v, requires_grad=False, ld=None, k=None):
        self.v, self.requires_grad, self.grad = v, requires_grad, None
        self.n, self.h, self.w, self.c = v.shape
        self.ld = pad32(self.c) if ld is None else ld
        self.k, self.labels, self.pending, self.dtype = k, None, None, 'f32'

    @property
    def rows(self):
        return self.n * self.h * self.w


def _val(t):
    return None if t is None else t.val


class RefOps(object):
    def __init__(self, cx):
        self.cx = cx

    # ---- helpers
    def _q(self, v):
        return bf16q(v) if self.cx.mfma_dtype == 'bf16' else v

    def _out(self, v, requires_grad, ld=None):
        k = self.cx.call_k
        self.cx.runner.ystore.setdefault(k, v.v.detach())      # the first activation a top-level call makes: conv2d's y (before a pool)
        return RAct(v, requires_grad, ld, k)

    # ---- conv / deconv / filter gradient
    def conv2d(self, x, kernel, bias, c_out, k, stride, padding, act=None, alpha=0.2, wn=None, mobn=None, segments=None, train=True,
               kernel_grad=None, bias_grad=None, n_store_ld=None, bn_stats=False, concat=None, pool=None):
        cx, alpha = self.cx, f32c(alpha)
        wshape = (k, k, x.c, c_out)
        vk = kernel.val.reshape(wshape)
        w = wn_weight(vk, wn[0].val) if wn is not None else vk
        needs_w = cx.trains() and kernel_grad is not None
        needs_x = cx.tape is not None and x.requires_grad
        xq, wq = self._q(x.v), self._q(w)
        pre = conv_fwd(xq, wq, stride, padding)
        if mobn is None and bias is not None:
            pre = add(pre, bias.val)
        if mobn is not None:
            if train:
                pre, pop = mobn_train(pre, mobn[0].val, mobn[2].val, segments, 0.9)
                mobn[2].set(pop)
            else:
                pre = mobn_eval(pre, mobn[0].val, mobn[2].val)
        fuse_cat = concat is not None and mobn is None and not bn_stats and n_store_ld is None and c_out == pad32(c_out)
        ld = pad32(c_out + concat[1]) if fuse_cat else n_store_ld[1] if n_store_ld is not None else None
        y = self._out(act_fn(pre, act, alpha), needs_w or needs_x, ld)
        if fuse_cat:
            y.labels = Labels(concat[0], concat[1])
        if needs_w or needs_x:
            def bwd():
                assert y.grad is not None, "conv2d backward: no gradient reached the output"
                dpre = act_bwd(y.grad, y.v, act, alpha, cx.mask_of(y))
                if mobn is not None:
                    if needs_w and mobn[1] is not None:
                        mobn[1].set(rsum(dpre, (0, 1, 2)))
                    if train:
                        dpre = seg_center(dpre, segments)
                elif needs_w and bias_grad is not None:
                    bias_grad.set(rsum(dpre, (0, 1, 2)))
                dq = self._q(dpre)
                if needs_w:
                    dw = conv_dw(xq, dq, wshape, stride, padding)
                    if wn is not None:
                        dv, dg = wn_weight_bwd(vk, wn[0].val, dw)
                        kernel_grad.set(dv)
                        if wn[1] is not None:
                            wn[1].set(dg)
                    else:
                        kernel_grad.set(dw)
                if needs_x:
                    cx.add_grad(x, conv_dx(dq, wq, x.v.shape, stride, padding))
            cx.record(bwd)
        return y if pool is None else self.maxpool2_dropout(y, pool[0], pool[1])

    def deconv2d(self, x, kernel, bias, c_out, act=None, kernel_grad=None, bias_grad=None, narrow_out=False, wn=None):
        cx = self.cx
        wshape = (5, 5, c_out, x.c)
        vk = kernel.val.reshape(wshape)
        w = wn_weight(vk, wn[0].val, 2) if wn is not None else vk
        needs_w = cx.trains() and kernel_grad is not None
        needs_x = cx.tape is not None and x.requires_grad
        xq, wq = self._q(x.v), self._q(w)
        y = self._out(act_fn(add(deconv_fwd(xq, wq), bias.val), act, ALPHA), needs_w or needs_x, c_out if narrow_out else None)
        if needs_w or needs_x:
            def bwd():
                dpre = act_bwd(y.grad, y.v, act, ALPHA, cx.mask_of(y))
                if needs_w and bias_grad is not None:
                    bias_grad.set(rsum(dpre, (0, 1, 2)))
                dq = self._q(dpre)
                if needs_w:
                    dw = deconv_dw(xq, dq, wshape)
                    if wn is not None:
                        dv, dg = wn_weight_bwd(vk, wn[0].val, dw, 2)
                        kernel_grad.set(dv)
                        wn[1].set(dg)
                    else:
                        kernel_grad.set(dw)
                if needs_x:
                    cx.add_grad(x, deconv_dx(dq, wq))
            cx.record(bwd)
        return y

    def filter_grad(self, desc, in_act_t, dout_t, t, c_dim, n_dim, dst, wn=None, defer=True, in16=False):
        k = int(round(t ** 0.5))
        n, h, w = desc.n_img, desc.h_in, desc.w_in
        x, dy = in_act_t.val.reshape(n, h, w, c_dim), dout_t.val.reshape(n, h, w, n_dim)
        dw = conv_dw(self._q(x), self._q(dy), (k, k, c_dim, n_dim), 1, 'SAME')
        dst.set(dw)
        if wn is not None:
            dv, dg = wn_weight_bwd(wn[0].val.reshape(k, k, c_dim, n_dim), wn[1].val, dw)
            wn[2].set(dv)
            wn[3].set(dg)

    # ---- normalisation
    def mean_only_batch_norm(self, x, pop_mean, b, b_grad=None, train=True, decay=0.9, segments=None):
        cx = self.cx
        needs = cx.tape is not None and (x.requires_grad or (cx.trains() and b_grad is not None))
        if train:
            yv, pop = mobn_train(x.v, b.val, pop_mean.val, segments, decay)
            pop_mean.set(pop)
        else:
            yv = mobn_eval(x.v, b.val, pop_mean.val)
        y = self._out(yv, needs, x.ld)
        if needs:
            def bwd():
                if cx.trains() and b_grad is not None:
                    b_grad.set(rsum(y.grad, (0, 1, 2)))
                cx.add_grad(x, seg_center(y.grad, segments) if train else y.grad)
            cx.record(bwd)
        return y

    def batch_norm_eval(self, x, gamma, beta, mm, mv, eps):
        return self._out(batch_norm_eval(x.v, gamma.val, beta.val, mm.val, mv.val, eps), False, x.ld)

    def batch_norm_train(self, x, gamma, beta, mm, mv, eps, decay, gamma_grad=None, beta_grad=None, relu_input=False, segments=None, out_bf16=False):
        cx = self.cx
        trains = cx.trains()
        needs = cx.tape is not None and (x.requires_grad or trains)
        yv, m1, v1, cache = batch_norm_train(x.v, gamma.val, beta.val, _val(mm), _val(mv), eps, decay, segments)
        if mm is not None:
            mm.set(m1)
            mv.set(v1)
            if cx.state_replay is not None:
                def again():
                    _, m2, v2, _ = batch_norm_train(x.v, gamma.val, beta.val, mm.val, mv.val, eps, decay, segments)
                    mm.set(m2)
                    mv.set(v2)
                cx.state_replay.append(again)
        y16 = out_bf16 and cx.act_dtype == 'bf16'
        if y16:
            yv = bf16_store(yv)
        y = self._out(yv, needs, x.ld)
        y.dtype = 'bf16' if y16 else 'f32'
        if needs:
            def bwd():
                mask = (cx.mask_of(x) if cx.mask_of(x) is not None else x.v.v) > 0 if relu_input else None
                dx, dg, db = batch_norm_train_bwd(y.grad, gamma.val, cache, mask)
                if trains and gamma_grad is not None:
                    gamma_grad.set(dg)
                    beta_grad.set(db)
                cx.add_grad(x, dx)
            cx.record(bwd)
        return y

    def batch_norm_moments(self, x, scale_t, beta, pop_mean, pop_var, eps, decay, train, scale_grad=None, beta_grad=None):
        cx = self.cx
        if not train:
            return self.batch_norm_eval(x, scale_t, beta, pop_mean, pop_var, eps)
        trains = cx.trains()
        needs = cx.tape is not None and (x.requires_grad or trains)
        yv, pm, pv, cache = batch_norm_moments(x.v, scale_t.val, beta.val, pop_mean.val, pop_var.val, eps, decay)
        pop_mean.set(pm)
        pop_var.set(pv)
        y = self._out(yv, needs, x.ld)
        if needs:
            def bwd():
                dx, dg, db = batch_norm_train_bwd(y.grad, scale_t.val, cache)
                if trains and scale_grad is not None:
                    scale_grad.set(dg)
                    beta_grad.set(db)
                cx.add_grad(x, dx)
            cx.record(bwd)
        return y

    def moments_normalize(self, x, eps, init_scale=1.0):
        return self._out(moments_normalize(x.v, eps, init_scale), False, x.ld)

    def colstats(self, mode, a_t, ld_a, b_t, ld_b, rows, c, seg_rows, act=None, alpha=0.2, s1=None, s2=None):
        assert mode in (0, 1, 3), mode
        a = a_t.val.reshape(rows, ld_a).map(lambda t: t[:, :c])
        b = b_t.val.reshape(rows, ld_b).map(lambda t: t[:, :c]) if b_t is not None else None
        o1, o2, lo = [], [], 0
        for r in seg_rows:
            sa = a.map(lambda t: t[lo:lo + r])
            o1.append(rsum(sa, 0))
            if mode != 0:
                o2.append(rsum(mul(sa, sa if mode == 1 else b.map(lambda t: t[lo:lo + r])), 0))
            lo += r
        for dst, parts in ((s1, o1), (s2, o2)):
            if dst is not None and parts:
                full = vcat(parts)
                dst.val = vcat([full, dst.val.map(lambda t: t[full.v.numel():])])
                dst.written = True
        return s1, s2

    # ---- pointwise / pooling / concat
    def activation(self, x, kind, alpha=0.2):
        cx, alpha = self.cx, f32c(alpha)
        y = self._out(act_fn(x.v, kind, alpha), x.requires_grad, x.ld)
        if cx.tape is not None and x.requires_grad:
            cx.record(lambda: cx.add_grad(x, act_bwd(y.grad, y.v, kind, alpha, cx.mask_of(y))))
        return y

    def scale_mask(self, x, mask_t, mscale, defer=False):
        cx = self.cx
        if defer:
            y = RAct(x.v, x.requires_grad, x.ld)
            y.pending = Pending(x, mask_t, mscale)
            return y
        m = mask_t.val.reshape(x.v.shape)
        y = self._out(dropout(x.v, m, mscale), x.requires_grad, x.ld)
        if cx.tape is not None and x.requires_grad:
            cx.record(lambda: cx.add_grad(x, dropout(y.grad, m, mscale)))
        return y

    def cond_concat(self, x, y_onehot_t, ncls):
        cx = self.cx
        m, mscale = None, 1.0
        if x.pending is not None:
            x, mask_t, mscale = x.pending
            m = mask_t.val.reshape(x.v.shape)
        c = x.c
        lab = y_onehot_t.val.reshape(x.n, ncls)
        out = self._out(cond_concat(dropout(x.v, m, mscale), lab), x.requires_grad, pad32(c + ncls))
        if cx.tape is not None and x.requires_grad:
            cx.record(lambda: cx.add_grad(x, dropout(out.grad.map(lambda t: t[..., :c]), m, mscale)))
        return out

    def pad_add(self, x, add_t, ld_out):
        return self._out(x.v if add_t is None else add(x.v, add_t.val.reshape(x.v.shape)), False, ld_out)

    def im2col3x3_add(self, x, add_t):
        return self._out(im2col3x3(add(x.v, add_t.val.reshape(x.v.shape))), False)

    def add_noise(self, x, noise_t):
        cx = self.cx
        y = self._out(add(x.v, noise_t.val.reshape(x.v.shape)), x.requires_grad, x.ld)
        if cx.tape is not None and x.requires_grad:
            cx.record(lambda: cx.add_grad(x, y.grad))
        return y

    def maxpool2_dropout(self, y, mask_t, mscale):
        cx = self.cx
        pooled, idx, margin = maxpool2(y.v)
        cx.pool_margin = min(cx.pool_margin, margin)
        m = mask_t.val.reshape(pooled.shape) if mask_t is not None else None
        out = self._out(dropout(pooled, m, mscale), y.requires_grad, y.ld)
        if cx.tape is not None and y.requires_grad:
            cx.record(lambda: cx.add_grad(y, maxpool2_bwd(dropout(out.grad, m, mscale), idx, y.v.shape)))
        return out

    def global_maxpool(self, x):
        cx = self.cx
        pooled, idx, margin = global_maxpool(x.v)
        cx.pool_margin = min(cx.pool_margin, margin)
        out = self._out(pooled, x.requires_grad)
        if cx.tape is not None and x.requires_grad:
            cx.record(lambda: cx.add_grad(x, global_maxpool_bwd(out.grad, idx, x.v.shape)))
        return out

    def global_avgpool_concat(self, x, y_onehot_t, ncls):
        cx = self.cx
        c = x.c
        lab = y_onehot_t.val.reshape(x.n, ncls) if y_onehot_t is not None else None
        out = self._out(cond_concat(global_avgpool(x.v), lab), x.requires_grad)
        if cx.tape is not None and x.requires_grad:
            cx.record(lambda: cx.add_grad(x, global_avgpool_bwd(out.grad.map(lambda t: t[..., :c]), x.v.shape)))
        return out

    def global_avgpool(self, x):
        return self.global_avgpool_concat(x, None, 0)

    def minibatch_discrimination(self, x, w, b, num_kernels, dim, w_grad=None, b_grad=None, concat_input=False):
        cx = self.cx
        holder = {}
        if concat_input and cx.tape is not None and x.requires_grad:
            def bwd_skip():      # the one gradient tg/ops.py ADDS (tg_pad_add_f32 in place): the skip path, after the product's input gradient
                x.grad = add(x.grad, holder['g'].map(lambda t: t[..., :x.c]))
            cx.record(bwd_skip)
        k0 = cx.call_k
        a = self.conv2d(x, w, None, num_kernels * dim, 1, 1, 'SAME', kernel_grad=w_grad)
        f, cache = minibatch_disc(a.v.reshape(x.n, -1), b.val, num_kernels, dim)
        f = f.reshape(x.n, 1, 1, num_kernels)
        c0 = x.c if concat_input else 0
        out = self._out(vcat([x.v, f], 3) if concat_input else f, a.requires_grad)
        out.k = k0
        if cx.tape is not None and a.requires_grad:
            def bwd():
                holder['g'] = out.grad
                da, db = minibatch_disc_bwd(out.grad.map(lambda t: t[..., c0:]).reshape(x.n, num_kernels), cache)
                if b_grad is not None:
                    b_grad.set(db)
                cx.add_grad(a, da.reshape(a.v.shape))
            cx.record(bwd)
        return out

    def argmax_onehot(self, logits, k):
        v = logits.v.v.reshape(logits.n, -1)[:, :k]
        return F.one_hot(v.argmax(1), k).to(v.dtype).reshape(-1)

    # ---- copies and views
    def copy2d(self, dst_t, ld_d, dst_col, src_t, ld_s, rows, c):
        def f(d, s):
            d = d.clone()
            for r in range(rows):
                d[r * ld_d + dst_col:r * ld_d + dst_col + c] = s[r * ld_s:r * ld_s + c]
            return d
        dst_t.val = V(f(dst_t.val.v, src_t.val.v), f(dst_t.val.e, src_t.val.e))
        dst_t.written = True

    def copy_rows(self, dst_t, dst_off, src_t, numel):
        self.copy2d(dst_t, int(numel), int(dst_off), src_t, int(numel), 1, int(numel))

    def copy_many(self, jobs):
        for d, off, s, n in jobs:
            if n > 0:
                self.copy_rows(d, off, s, n)

    def reshape(self, x, n, h, w, c):
        cx = self.cx
        assert x.ld == x.c and n * h * w * c == x.rows * x.c
        y = RAct(x.v.reshape(n, h, w, c), x.requires_grad, c, x.k)
        if cx.tape is not None and x.requires_grad:
            cx.record(lambda: cx.add_grad(x, y.grad.reshape(x.v.shape)))
        return y

    def view(self, x, h, w, c):
        return self.reshape(x, x.n, h, w, c)

    def concat_batch(self, acts):
        cx = self.cx
        out = self._out(vcat([a.v for a in acts]), any(a.requires_grad for a in acts), acts[0].ld)
        if cx.tape is not None and out.requires_grad:
            def bwd():
                if out.grad is None:
                    return
                off = 0
                for a in acts:
                    lo, hi = off, off + a.n
                    cx.add_grad(a, out.grad.map(lambda t: t[lo:hi]))
                    off = hi
            cx.record(bwd)
        return out


def act_fn(x, kind, alpha):
    return act(x, kind, alpha)


# ================================================================== input fill by the role of a label

def role(label):
    """what a labelled tensor of a case is, from its name: decides the fill (and, for 'out', that the op writes it)"""
    leaf = label.split('.')[-1]
    if leaf.endswith('_grad') or leaf in ('dst', 'dv', 'dg', 'sg', 'bg', 's1', 's2', 'gpgrad'):
        return 'out'
    if leaf in ('kernel', 'w', 'v'):
        return 'kernel'
    if leaf in ('g', 'gamma', 'scale'):
        return 'gain'
    if leaf in ('bias', 'b', 'beta', 'pop', 'pop_mean', 'mm', 'pm'):
        return 'bias'
    if leaf in ('mv', 'pv'):
        return 'var'
    if leaf.startswith('keep'):
        return 'mask'
    if leaf == 'labels':
        return 'labels'
    return 'data'


def fill(seed, label, numel):
    """the fp32 values of the labelled tensor `label` of the case seeded `seed` (None for a gradient destination)"""
    rng = np.random.default_rng(zlib.crc32(('%s/%s' % (seed, label)).encode()))
    r = role(label)
    if r == 'out':
        return None
    if r == 'kernel':
        a = 0.1 * rng.standard_normal(numel)
    elif r == 'gain':
        a = 1 + 0.1 * rng.standard_normal(numel)
    elif r == 'bias':
        a = 0.3 * rng.standard_normal(numel)
    elif r == 'var':
        a = 0.5 + rng.random(numel)
    elif r == 'mask':
        a = (rng.random(numel) < 0.8).astype(np.float64)
    elif r == 'labels':
        a = np.zeros((numel // 10, 10))
        a[np.arange(numel // 10), rng.integers(0, 10, numel // 10)] = 1
    else:
        a = rng.standard_normal(numel)
    return np.ascontiguousarray(a.reshape(-1), np.float32)


def fill_x(seed, k, shape):
    """the k-th input activation of a case, logical [n,h,w,c]"""
    return fill(seed, 'x#%d' % k, int(np.prod(shape))).reshape(shape)


def fill_seed(seed, k, shape):
    """the k-th gradient a loss head writes"""
    return fill(seed, 'dy#%d' % k, int(np.prod(shape))).reshape(shape)


# ================================================================== the runner (launch_trace.Tracer's interface)

class RefContext(object):
    """what the case bodies and RefOps ask of a Context"""

    def __init__(self, runner, mfma_dtype='f32', act_dtype='f32', wgrad_side=False):
        self.runner, self.mfma_dtype, self.act_dtype, self.wgrad_side = runner, mfma_dtype, act_dtype, wgrad_side
        self.tape, self.train, self.state_replay, self.call_k, self.pool_margin = None, False, None, None, float('inf')
        self.plan_tag, self.prep_cache, self.stores = None, None, {}

    def trains(self):
        return self.tape is not None and self.train

    def record(self, fn):
        if self.tape is not None:
            self.tape.append(fn)

    def add_grad(self, a, g):
        """a backward closure writes g as its contribution to the gradient of `a` (ops._write_grad).  The first writer's launch stores, and an
        alias adopts the consumer's buffer: g as it is.  Every later writer ADDS: its launch stores into a scratch buffer (an alias is
        already in memory) and tg_add_f32 adds that to the gradient, one more float32 rounding.  minibatch_discrimination's skip path adds
        in place (tg_pad_add_f32) and states that itself.  The fused paths that cannot tolerate a second writer refuse it
        (bwd_single_consumer_refusal)."""
        a.grad = g if a.grad is None else add(a.grad, g)

    def mask_of(self, a):
        """the stored forward output of the implementation under test for activation `a` (None: the reference's own)"""
        st = self.runner.stored
        if st is None or a.k is None or st.get(a.k) is None or int(np.prod(np.shape(st[a.k]))) != a.v.v.numel():
            return None
        return torch.as_tensor(st[a.k]).reshape(a.v.shape)

    def new_act(self, n, h, w, c, ld=None, requires_grad=False, tag='a', dtype='f32'):
        assert tag == 'x', "only input activations are made by a case"
        return self.runner.make_x(n, h, w, c, ld, requires_grad)

    def _run(self, tape):
        for fn in reversed(tape):
            fn()

    def backward(self):
        tape, self.tape = self.tape, []
        self._run(tape)

    def run_tape(self, tape):
        self._run(tape)
        del tape[:]

    @contextlib.contextmanager
    def sub_tape(self, train_nets, replay=None):
        prev = (self.tape, self.train, self.state_replay)
        tape = []
        self.tape, self.train, self.state_replay = tape, 'net' in train_nets, replay
        try:
            yield tape
        finally:
            self.tape, self.train, self.state_replay = prev

    def flush_tails(self):
        pass

    def grad_of(self, a):
        return a.grad


class RefRunner(object):
    """runs a case body of tests/launch_trace.py on RefOps.  dtype float64: the reference and its bounds; float32: the attainability run.
    stored: {call number: forward output [n,h,w,c]} of the implementation under test (relu / lrelu masks), or None.
    After run(): labels {label: RT}, outs [(call number, V or exact tensor or None)], xs [RAct] (inputs; .grad), seeds [RAct]."""
    launches = False

    def __init__(self, name, dtype=F64, stored=None, seed=None, **ctx_kw):
        self.variant, self.dtype, self.stored = name, dtype, stored
        self.fill_seed = name if seed is None else seed
        self.cx = RefContext(self, **ctx_kw)
        self.ops = RefOps(self.cx)
        self.labels, self.outs, self.xs, self.seeds, self.trace, self.n_calls, self.ystore = {}, [], [], [], [], 0, {}

    def _tensor(self, a):
        return torch.from_numpy(np.asarray(a, np.float32)).to(self.dtype)

    def t(self, label, numel, dtype=None):
        assert label not in self.labels, label
        a = fill(self.fill_seed, label, int(numel))
        self.labels[label] = RT(label, V(self._tensor(np.full(int(numel), np.nan, np.float32) if a is None else a)))
        return self.labels[label]

    def make_x(self, n, h, w, c, ld=None, requires_grad=True):
        x = RAct(V(self._tensor(fill_x(self.fill_seed, len(self.xs), (n, h, w, c)))), requires_grad, ld)
        self.xs.append(x)
        return x

    def x(self, n, h, w, c, requires_grad=True, dtype='f32'):
        return self.make_x(n, h, w, c, None, requires_grad)

    def seed(self, y, ld=None):
        g = V(self._tensor(fill_seed(self.fill_seed, len(self.seeds), y.v.shape)))
        self.seeds.append(y)
        y.grad = g                                         # the loss head's write: an assignment, as Tracer.seed
        return y.grad

    def mark(self, text):
        self.trace.append(text)

    @contextlib.contextmanager
    def phase(self, name='p', train=True, record=True):
        cx = self.cx
        prev = (cx.tape, cx.train)
        cx.tape, cx.train = ([] if record else None), train
        try:
            yield cx
        finally:
            cx.tape, cx.train = prev

    def wrap(self, fn_name):
        """the op `fn_name` as the case body calls it: top-level calls are numbered and their results kept"""
        fn = getattr(self.ops, fn_name)

        def call(*a, **kw):
            cx = self.cx
            if cx.call_k is not None:
                return fn(*a, **kw)
            cx.call_k = k = self.n_calls
            self.n_calls += 1
            try:
                r = fn(*a, **kw)
            finally:
                cx.call_k = None
            if isinstance(r, RAct):
                self.outs.append((k, None if r.pending is not None else r.v))
            elif torch.is_tensor(r):
                self.outs.append((k, r))
            return r
        return call


OPS_API = ['conv2d', 'deconv2d', 'filter_grad', 'mean_only_batch_norm', 'batch_norm_eval', 'batch_norm_train', 'batch_norm_moments',
           'moments_normalize', 'colstats', 'activation', 'scale_mask', 'cond_concat', 'pad_add', 'im2col3x3_add', 'add_noise',
           'maxpool2_dropout', 'global_maxpool', 'global_avgpool_concat', 'global_avgpool', 'minibatch_discrimination', 'argmax_onehot',
           'copy2d', 'copy_rows', 'copy_many', 'reshape', 'view', 'concat_batch']


class OpsShim(object):
    """stands in for the module tg.ops inside tests/launch_trace.py while a case runs on a runner"""

    def __init__(self, runner):
        for n in OPS_API:
            setattr(self, n, runner.wrap(n))


def run_reference(LT, name, monkeypatch, dtype=F64, stored=None, shape=None, seed=None):
    """the case `name` of launch_trace (module LT) on the reference.  -> RefRunner"""
    c = LT.CASES[name]
    kw = {k: v for k, v in c.ctx_kw.items()}
    r = RefRunner(name, dtype, stored, seed=seed, **kw)
    monkeypatch.setattr(LT, 'ops', OpsShim(r))
    if shape is None:
        c.fn(r)
    else:
        c.fn(r, shape)
    return r


# ================================================================== which case is held to what

# 'full': forward outputs, input gradients, variable gradients and updated statistics; 'forward': the case has no backward pass;
# 'refusal': the case asserts that tg/ops.py refuses (nothing to compute); 'device': the float64 restatement runs on the GPU (ON_DEVICE)
REFS = {}
EXEMPT = {
    'grad_penalty_rows': "drives tg/grad_penalty.py's private helpers on a ParamStore, not the tg.ops signatures this module restates; the penalty's "
                         "numbers are held to float64 by tests/test_gpu_wgan_gp.py",
    'mobn_pool_odd_map': "conv2d(pool=...) routes a 7x7 map to tg_maxpool2_fwd_f32 / tg_maxpool2_bwd_actsum_f32, which take even maps only: the "
                         "forward launch refuses (TgError) and nothing is computed.  tests/golden/ops_launch_traces.json pins those launches, so "
                         "the route stays recorded; no network pools an odd map",
}
# A case in REFS of which ONE shape has no float64 check (the case keeps its check at its other shape; the coverage guard of
# tests/test_ops_reference.py holds that).  Keys are the ids of items(): the case name is the recorded shape, name@ragged the second one.
_BF16_IN = ("the recorded 4x8x8x32 shape is routed to tg_igemm_*_bf16in_bf16, whose launcher serves a bf16-stored input at w in {16, 32, 64}, "
            "256 | h*w, 64 | ld_in, 128 | c_out only and refuses this one (TgError, nothing is computed); tests/golden/ops_launch_traces.json "
            "pins those launches, so the admission stays where it is and the case is held to float64 at its second shape, 3x8x32")
EXEMPT_SHAPES = {'conv_bf16_input_plain': _BF16_IN, 'conv_bf16_input_bnstat': _BF16_IN}
# What the launch says when it refuses an exempt case or shape: tests/test_gpu_ops_routes.py asserts it, so an exemption ends the day
# the kernel takes the shape.
KERNEL_REFUSES = {
    'conv_bf16_input_plain': 'a bf16-stored input is served for 3x3 / stride-1 / SAME layers of width 16 / 32 / 64',
    'conv_bf16_input_bnstat': 'a bf16-stored input is served for 3x3 / stride-1 / SAME layers of width 16 / 32 / 64',
    'mobn_pool_odd_map': 'maxpool2_fwd: bad args',
}
# Tensors of a case in REFS whose content tg/ops.py does not define (left out of the numeric, padding and rerun checks; the guard holds
# that each names a tensor of its case).  filter_prep_plan applies its first layer twice in one backward pass with the same variable-
# gradient destinations: the two tail jobs of the one tg_filter_grad_tail_multi_f32 launch both write them, in no defined order.
UNDEFINED = {'filter_prep_plan': ('label:l1.kernel_grad', 'label:l1.g_grad')}
# 2^34 multiply-adds: minutes of float64 on the CPU; tests/test_gpu_ops_routes.py restates this one in float64 on the device
ON_DEVICE = ('filter_grad_large', 'filter_grad_large_side')
FORWARD_ONLY = ('mobn_eval', 'op_batch_norm_eval', 'op_forward_only', 'op_colstats')


def register(LT):
    """fill REFS from launch_trace's CASES (every case that is not exempt has a reference: the bodies run on RefOps)"""
    for name in LT.CASES:
        if name not in EXEMPT:
            REFS[name] = ('refusal' if name == 'bwd_single_consumer_refusal' else 'device' if name in ON_DEVICE else
                          'forward' if name in FORWARD_ONLY else 'full')
    return REFS


# Seeds.  The inputs of a case are drawn from its name; an entry here appends a salt, chosen on the CPU so that in every pooling window of
# the case the two largest reference values differ by more than four times their bound (tests/test_ops_reference.py asserts it).
SALT = {}


def fill_key(name, ident=None):
    """the seed of a case's inputs: a '_side' variant gets the inputs of the variant without the second stream (they are compared bit for bit)"""
    ident = (ident or name).replace('_side', '')
    return ident + ('#%d' % SALT[ident] if ident in SALT else '')


def items(LT):
    """[(id, case name, shape or None)]: every case with a reference at its recorded shape and, where it has one, at its ragged shape"""
    out = []
    for name in sorted(register(LT)):
        if REFS[name] in ('refusal', 'device'):
            continue
        if name not in EXEMPT_SHAPES:
            out.append((name, name, None))
        shp = LT.RAGGED.get(LT.CASES[name].fn.__name__)
        if shp is not None and name + '@ragged' not in EXEMPT_SHAPES:
            out.append((name + '@ragged', name, shp))
    return out


def expected(ref):
    """{key: (float64 value, bound or None = exact)} of everything a run of the case leaves behind"""
    out = {}
    for label, rt in ref.labels.items():
        out['label:' + label] = (rt.val.v.detach().to(F64).numpy(), rt.val.e.numpy() if rt.written else None)
    for k, v in ref.outs:
        if v is None:
            continue
        out['out:%d' % k] = (v.v.detach().to(F64).numpy(), v.e.numpy()) if isinstance(v, V) else (v.detach().to(F64).numpy(), None)
    for i, x in enumerate(ref.xs):
        if x.grad is not None:
            out['dx:%d' % i] = (x.grad.v.detach().to(F64).numpy(), x.grad.e.numpy())
    return out


def ratios(got, want):
    """{key: worst |got - ref| / bound}; an exact entry gives 0 or inf; NaN in the reference (a tensor no op wrote) must be NaN in `got`"""
    out = {}
    assert set(got) == set(want), (sorted(set(got) ^ set(want)))
    for key, (ref, bound) in want.items():
        g = np.asarray(got[key], np.float64).reshape(ref.shape)
        nan = np.isnan(ref)
        if nan.any():
            out[key] = 0.0 if np.isnan(g[nan]).all() else float('inf')
            if nan.all():
                continue
        ok = ~nan
        err = np.abs(g[ok] - ref[ok])
        if not np.isfinite(err).all():
            out[key] = float('inf')
        elif bound is None:
            out[key] = max(out.get(key, 0.0), 0.0 if (err == 0).all() else float('inf'))
        else:
            out[key] = max(out.get(key, 0.0), float((err / (bound[ok] + 1e-300)).max()) if err.size else 0.0)
    return out


def worst_element(got, want, key):
    ref, bound = want[key]
    g = np.asarray(got[key], np.float64).reshape(ref.shape)
    r = np.abs(g - ref) / ((bound if bound is not None else 0) + 1e-300)
    r = np.where(np.isnan(r), np.inf, r)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return "%s%s: got %.9g, reference %.9g, bound %.3g" % (key, list(i), g[i], ref[i], (bound[i] if bound is not None else 0.0))
