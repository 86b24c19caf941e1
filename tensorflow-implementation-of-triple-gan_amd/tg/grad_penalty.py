"""The WGAN-GP gradient penalty of the reference's _gradient_penalty (Training/train_base.py:598-620) on the package's discriminators
(DESIGN §9.1): x = real + alpha (fake - real) with alpha ~ U[0,1) per image, gx = d sum(logits) / dx, s = sqrt(reduce_sum(gx^2, axis=1))
(axis 1 of the tensor passed in: H of NHWC, the features of MNIST's [N, F]), gp = mean((s - 1)^2).

A model's discriminator_gradient_penalty(real, fake, y, weight=1.0, in_step=False) hands `penalty` below a description of its
discriminator (Layer rows and a head entry) and one of the two sweep bodies.  real, fake: Act of one shape; y: label Act
[N,NUM_CLASSES].  It returns (weight * gp as a 1-element device tensor, weight * d gp / d theta_D as a flat buffer laid out like the
discriminator's ParamStore.g, valid until the next call); ParamStore.g is not touched.

With its dropout masks and noise drawn the network is piecewise linear in x, and weight norm W = g V/||V|| only reparametrises the
effective filter, so gp's parameter gradient needs no second-order machinery: four first-order sweeps over the layer rows, all on the
implicit-GEMM launches (dense layers as 1x1 ones) —
  1. forward with the stored activations y_k (their signs are lrelu'; for MNIST the activation BEFORE its additive noise: lrelu' is the
     sign of the pre-activation, the noise is a constant), filters prepared by _filter_prep,
  2. input-gradient sweep seeded with 1 per image, keeping each layer's pre-activation gradient dpre_k,
  3. the penalty (tg_grad_penalty_f32 for NHWC, tg_grad_penalty_rows_f32 for [N, F]: slopes, gp, r = weight * d gp / d gx), then a
     tangent forward from r: cond-concat with zero labels, the convolution without its bias, * lrelu'(y_k) * dropout mask
     (tg_actgrad_f32), no noise,
  4. dW_eff_k = wgrad(tangent input of layer k, dpre_k); the head's is the sum over images of its tangent input (_filter_grad maps each
     to the variables' gradients at their store offsets); every bias entry stays exactly 0.
Masks, noise and alpha are drawn in their own RNG scope 'GP' ('alpha', 'drop0', 'drop1', ... / 'noise0', ...); buffers live under the
phase 'wgan_gp', apart from every buffer a recorded launch plan or graph of the trainer names.  in_step=True (the trainer's D-update
with config.LOSS = 'WGAN_GP'): the same sweeps inside the caller's solver run (Context.detached) — no phase of their own, buffers and
draws at call sites of the caller's phase, so that its launch plan or graph records them.  After a call the model's last_gp_state holds
x, alpha, masks or noise, acts, gx, r and out (the penalty kernel's device result: [0] the penalty, for R1 [1] mean_i ||gx_i||^2).

Two penalties share the sweeps; what differs between them is written once each, in a rule object (Wgan, R1) the frame hands the sweep body:
where the input gradient is evaluated (`point`), the penalty kernel (`penalise`), and the names of its RNG scope, phase and buffers.
R1 (config.R1_GAMMA; a model's discriminator_r1_penalty(real, y, gamma, in_step=False)): gamma / 2 * mean_i ||gx_i||^2 at the
real rows themselves with their own labels — no interpolation, no alpha; the norm runs over ALL elements of image i (tg_r1_penalty_f32),
r = gamma / n * gx; RNG scope 'R1', phase 'r1'."""
import collections

from tg import geom, lib, ops
from tg.lib import ACT
from tg.runtime import Act, ctx, pad32

KEEP = 0.8          # every dropout of the discriminators keeps 0.8
LRE = ACT['lrelu']

# One layer of a discriminator: the store names of its filter (w), of its weight-norm gain (g; None: a plain filter) and of its bias (b),
# filters, stride, dropout behind the activation, label copies concatenated in front of it.
Layer = collections.namedtuple('Layer', 'w g b cout stride drop copies')


def plain(name, cout, stride=1, drop=False, copies=1):
    """a tf.layers layer: discriminator/<name>/<name>/kernel, bias."""
    p = 'discriminator/%s/%s/' % (name, name)
    return Layer(p + 'kernel', None, p + 'bias', cout, stride, drop, copies)


def weight_normed(name, cout, stride=1, drop=False, copies=1):
    """a weight-normalised layer: discriminator/<name>/V, g, b."""
    p = 'discriminator/%s/' % name
    return Layer(p + 'V', p + 'g', p + 'b', cout, stride, drop, copies)


def check_supported(who, mfma_dtype, minibatch_dis):
    """the two configurations no sweep body supports, for a model's penalty (the context's MFMA dtype) and for
    Training/Train_goodGAN.check_loss (the config alone, no device)."""
    if mfma_dtype != 'f32':
        raise lib.TgError("%s: MFMA_DTYPE = 'f32' needed (got %r): the penalty differentiates a gradient, and bf16-rounded operands in "
                          "the four sweeps are not pinned to a reference" % (who, mfma_dtype))
    if minibatch_dis:
        raise lib.TgError("%s: MINIBATCH_DIS = True is not supported: minibatch discrimination couples the images of a batch, so the "
                          "discriminator is not piecewise linear in one image and the penalty's gradient needs second-order terms" % who)


class _Rule(object):
    """what one penalty kind decides.  who: the model method, for messages; scope: the RNG scope of its draws; phase: the phase of a
    standalone call, and the prefix of its gradient buffer."""

    def penalise(self, cx, gx):
        """sweep 3's kernel on the input gradient gx (an Act in the layout the penalty reduces over) -> (penalty[0:1] on the device, r = d
        penalty / d gx as an Act of gx's shape: rank-2 [N, F] channel-padded, NHWC with gx's row stride, padding written 0)."""
        rank2 = (gx.h, gx.w) == (1, 1)
        r = cx.new_act(gx.n, gx.h, gx.w, gx.c, pad32(gx.c) if rank2 else gx.ld)
        out = cx.scratch('gp', 4)
        self._kernel(cx, gx, r, rank2, out)
        return out, r


class Wgan(_Rule):
    """WGAN-GP: evaluated at real + alpha (fake - real), alpha ~ U[0,1) per image; weight * mean((s - 1)^2) over the slopes along axis 1."""
    who, scope, phase = 'discriminator_gradient_penalty', 'GP', 'wgan_gp'

    def __init__(self, fake, weight):
        self.fake, self.weight, self.alpha = fake, float(weight), None

    def check(self, real):
        fake = self.fake
        if (real.n, real.h, real.w, real.c) != (fake.n, fake.h, fake.w, fake.c):
            raise lib.TgError("%s: real %s and fake %s differ in shape — bring both to one layout with model.as_image() first"
                              % (self.who, (real.n, real.h, real.w, real.c), (fake.n, fake.h, fake.w, fake.c)))
        return getattr(fake, 'dtype', 'f32') == 'f32'

    def begin(self, cx, n):
        self.alpha = cx.rng.uniform(cx, 'alpha', n, 0.0, 1.0)

    def point(self, cx, real, *shape):
        """the interpolates as a dense Act of `shape` = (n, h, w, c, ld): [N,H,W,C], or [N,F] whatever real's layout."""
        x, fake = cx.new_act(*shape), self.fake
        lib.call('tg_wgan_interp_f32', real.ptr, real.ld, fake.ptr, fake.ld, lib.ptr(self.alpha), x.ptr, real.c, real.n, real.h * real.w, real.c,
                 cx.stream)
        return x

    def _kernel(self, cx, gx, r, rank2, out):
        n, h, w, c = gx.n, gx.h, gx.w, gx.c
        if rank2:                                                    # axis 1 is the feature axis: one slope per image
            partials = cx.scratch('gpp', 2 * n)
            lib.call('tg_grad_penalty_rows_f32', gx.ptr, gx.ld, n, c, self.weight, r.ptr, r.ld, lib.ptr(partials), lib.ptr(out), cx.stream)
        else:                                                        # axis 1 is H
            partials = cx.scratch('gpp', 2 * ((n * w * r.ld + 255) // 256))
            lib.call('tg_grad_penalty_f32', gx.ptr, gx.ld, n, h, w, c, self.weight, r.ptr, r.ld, lib.ptr(partials), lib.ptr(out), cx.stream)

    def state(self):
        return dict(alpha=self.alpha)


class R1(_Rule):
    """R1: evaluated at the real rows; gamma / 2 * mean_i ||gx_i||^2, the norm over all elements of image i.  gamma: a number, or a
    1-element device tensor the kernel reads (the trainer's: a replayed plan or graph follows Train.set_r1_gamma)."""
    who, scope, phase = 'discriminator_r1_penalty', 'R1', 'r1'

    def __init__(self, gamma):
        self.gamma = gamma

    def check(self, real):
        return True

    def begin(self, cx, n):
        if not hasattr(self.gamma, 'data_ptr'):
            value, self.gamma = float(self.gamma), cx.scratch('r1gamma', 4)
            lib.call('tg_fill_f32', lib.ptr(self.gamma), value, 1, cx.stream)

    def point(self, cx, real, *shape):
        """real itself, viewed as `shape`; a channel-padded real is brought to the dense layout the sweeps read first."""
        if real.ld == real.c:
            return Act(real.t, *shape)
        x = cx.new_act(*shape)
        ops.copy2d(x.t, real.c, 0, real.t, real.ld, real.rows, real.c)
        return x

    def _kernel(self, cx, gx, r, rank2, out):
        partials = cx.scratch('gpp', 2 * gx.n)
        lib.call('tg_r1_penalty_f32', gx.ptr, gx.ld, gx.n, gx.h * gx.w, gx.c, lib.ptr(self.gamma), r.ptr, r.ld, lib.ptr(partials), lib.ptr(out),
                 cx.stream)

    def state(self):
        return dict(gamma=self.gamma)


def penalty(model, sweeps, layers, head, rule, real, y, in_step, minibatch_dis=False):
    """the frame of a model's discriminator_gradient_penalty / discriminator_r1_penalty: checks, the gradient buffer, phase and RNG scope,
    zero fill, the rule's own draws (Wgan: alpha), then sweeps(cx, st, layers, head, rule, real, y, grad) -> (penalty, state), and
    model.last_gp_state."""
    who = rule.who
    cx = ctx()
    check_supported(who, cx.mfma_dtype, minibatch_dis)
    f32 = rule.check(real)
    if y.n != real.n or y.ld != y.c or getattr(real, 'dtype', 'f32') != 'f32' or not f32:
        raise lib.TgError("%s: dense fp32 labels [%d] and fp32 images of %d expected" % (who, y.n, real.n))
    st = cx.stores['discriminator']
    grad = cx.scratch('gpgrad', st.n_p) if in_step else cx.ws(rule.phase + ':grad', st.n_p)
    with (cx.detached() if in_step else cx.phase_scope(rule.phase, record=False)), cx.rng_scoped(rule.scope):
        lib.call('tg_fill_f32', lib.ptr(grad), 0.0, st.n_p, cx.stream)
        rule.begin(cx, real.n)
        gp, state = sweeps(cx, st, layers, head, rule, real, y, grad)
    state.update(rule.state(), out=gp)
    model.last_gp_state = state
    return gp[0:1], grad


def _igemm(cx, name, *args):
    lib.call(name, *ops.igemm_scratch(cx, name, args, False))


def _filter_prep(cx, st, row, t, c_in):
    """the effective filter of `row` in the MFMA layouts (OTI [co_p][t][ci_p], HWIO [t][ci_p][co_p]): g V/||V|| for a weight-normalised
    row (as ops.conv2d(wn=...)), the kernel itself for a plain one."""
    c_out = row.cout
    ci_p, co_p = pad32(c_in), pad32(c_out)
    scale = cx.scratch('wns', c_out) if row.g is not None else None
    w_oti, w_hwio = cx.scratch('woti', co_p * t * ci_p), cx.scratch('whwio', t * ci_p * co_p)
    ops.prep_filter(cx, st.value(row.w), st.value(row.g) if row.g is not None else None, scale, w_oti, w_hwio, t, c_in, c_out, ci_p, co_p)
    return w_oti, w_hwio


def _filter_grad(cx, st, grad, row, desc, t_in, dpre, t, c_in):
    """sweep 4 of one layer: dW_eff = wgrad(t_in, dpre) (desc: its geometry; None: the head, dpre = 1 per image, dW_eff = column sums of
    t_in).  A plain row's goes straight to the store offset of its kernel in `grad`; a weight-normalised row's to scratch, then dV, dg
    (ops.filter_grad_tail: tg_wn_bwd_f32) to the store offsets of .../V and .../g."""
    c_out = row.cout
    ow = st.offset(row.w)
    dw, wn = grad[ow:ow + t * c_in * c_out], None
    if row.g is not None:
        og = st.offset(row.g)
        wn = (st.value(row.w), st.value(row.g), dw, grad[og:og + c_out])
        dw = cx.scratch('dweff', t * c_in * c_out + 4)
    if desc is not None:
        ops.filter_grad(desc, t_in.t, dpre.t, t, c_in, c_out, dw, wn=wn, defer=False)
        return
    ops.colstats(0, t_in.t, t_in.ld, None, 0, t_in.rows, c_in, [t_in.rows], s1=dw)
    ops.filter_grad_tail(cx, dw, t, c_in, c_out, wn)


def _label_copies(cx, y, copies):
    """device tensor [N, copies k] = [y, y, ...] (the SVHN discriminator concatenates the label twice in front of its last convolution)."""
    if copies == 1:
        return y.t
    ld = copies * y.c
    out = cx.new_act(y.n, 1, 1, ld, ld, tag='yy')
    for i in range(copies):
        ops.copy2d(out.t, ld, i * y.c, y.t, y.c, y.n, y.c)
    return out.t


def conv_sweeps(cx, st, layers, head, rule, real, y, grad):
    """the sweeps on a convolutional discriminator: input dropout, lrelu 3x3 convolutions (`layers`: label concat in front, dropout
    behind where the row says so), global mean, label concat, dense `head`."""
    n, H, W, c0 = real.n, real.h, real.w, real.c
    ncls, s = y.c, cx.stream
    c_img = st.shape(layers[0].w)[2] - layers[0].copies * ncls
    if c0 != c_img or (H, W) == (1, 1):
        raise lib.TgError("%s: images [N,H,W,%d] expected, got %s" % (rule.who, c_img, (H, W, c0)))
    if layers[-1].drop:
        raise lib.TgError("%s: a dropout behind the last convolution is not supported" % rule.who)
    labels = {k: _label_copies(cx, y, k) for k in {row.copies for row in layers}}
    zlab = cx.scratch('zlab', max(labels) * n * ncls)
    lib.call('tg_fill_f32', lib.ptr(zlab), 0.0, max(labels) * n * ncls, s)
    x = rule.point(cx, real, n, H, W, c0, c0)
    m0 = cx.rng.keep_mask(cx, cx.next_rng_name('drop'), n * H * W * c0, KEEP)
    # ---- sweep 1: forward, keeping every layer's input, activation and filter layouts
    L = []
    src, mask = x, m0
    for row in layers:
        nl = row.copies * ncls
        c_in = src.c + nl
        a = cx.new_act(n, src.h, src.w, c_in, pad32(c_in))
        lib.call('tg_cond_concat_f32', src.ptr, src.ld, src.c, lib.ptr(mask), src.c, 1.0 / KEEP if mask is not None else 1.0,
                 lib.ptr(labels[row.copies]), nl, a.ptr, a.ld, n, src.h * src.w, s)
        w_oti, w_hwio = _filter_prep(cx, st, row, 9, c_in)
        d = geom.conv_fwd(n, a.h, a.w, a.ld, pad32(row.cout), 3, row.stride, 'SAME', act='lrelu', alpha=0.2)
        yk = cx.new_act(n, d.h_out, d.w_out, row.cout, pad32(row.cout))
        _igemm(cx, 'tg_igemm_f32', d, a.ptr, lib.ptr(w_oti), lib.ptr(st.value(row.b)), yk.ptr, s)
        mask = cx.rng.keep_mask(cx, cx.next_rng_name('drop'), yk.rows * row.cout, KEEP) if row.drop else None
        L.append(dict(row=row, a=a, y=yk, w_oti=w_oti, w_hwio=w_hwio, mask=mask, nl=nl))
        src = yk
    last = L[-1]['y']
    cl, hw = last.c, last.h * last.w
    # (a plain [c, 1] kernel is its own OTI layout)
    w_head = st.value(head.w) if head.g is None else _filter_prep(cx, st, head, 1, cl + ncls)[0]
    # ---- sweep 2: d sum(logits) / dx; dpre_k = gradient at layer k's pre-activation
    dp = cx.scratch('dp', n * pad32(cl))
    lib.call('tg_copy2d_f32', lib.ptr(w_head), 0, lib.ptr(dp), pad32(cl), n, cl, s)      # W_eff of the head (its feature rows) per image
    dpre = cx.new_act(n, last.h, last.w, cl, last.ld)
    lib.call('tg_gavgpool_bwd_f32', lib.ptr(dp), pad32(cl), last.ptr, last.ld, dpre.ptr, dpre.ld, n, hw, cl, LRE, 0.2, s)
    for k in range(len(L) - 1, -1, -1):
        Lk = L[k]
        Lk['dpre'] = dpre
        a = Lk['a']
        da = cx.new_act(n, a.h, a.w, a.c, a.ld)
        dds = lib.desc_array(geom.conv_dgrad(n, a.h, a.w, a.ld, dpre.ld, 3, Lk['row'].stride, 'SAME', ld_out=a.ld, n_store=a.ld))
        _igemm(cx, 'tg_igemm_multi_f32', dds, len(dds), dpre.ptr, lib.ptr(Lk['w_hwio']), None, da.ptr, s)
        if k > 0:
            yp, mp = L[k - 1]['y'], L[k - 1]['mask']
            dpre = cx.new_act(n, yp.h, yp.w, yp.c, yp.ld)
            lib.call('tg_actgrad_f32', da.ptr, da.ld, yp.ptr, yp.ld, lib.ptr(mp), yp.c, 1.0 / KEEP if mp is not None else 1.0, dpre.ptr, dpre.ld,
                     yp.rows, yp.c, LRE, 0.2, s)
    gx = cx.new_act(n, H, W, c0, pad32(c0))
    lib.call('tg_actgrad_f32', da.ptr, da.ld, None, 0, lib.ptr(m0), c0, 1.0 / KEEP, gx.ptr, gx.ld, gx.rows, c0, 0, 0.0, s)
    # ---- sweep 3: the penalty (Wgan: slopes over H, axis 1 of NHWC; R1: per image), then the tangent forward from r = d penalty / d gx
    gp, r = rule.penalise(cx, gx)
    src, mask = r, m0
    for Lk in L:
        a, yk, row = Lk['a'], Lk['y'], Lk['row']
        ta = cx.new_act(n, a.h, a.w, a.c, a.ld)
        lib.call('tg_cond_concat_f32', src.ptr, src.ld, src.c, lib.ptr(mask), src.c, 1.0 / KEEP if mask is not None else 1.0, lib.ptr(zlab), Lk['nl'],
                 ta.ptr, ta.ld, n, a.h * a.w, s)
        d = geom.conv_fwd(n, a.h, a.w, a.ld, yk.ld, 3, row.stride, 'SAME')
        tz = cx.new_act(n, yk.h, yk.w, yk.c, yk.ld)
        _igemm(cx, 'tg_igemm_f32', d, ta.ptr, lib.ptr(Lk['w_oti']), None, tz.ptr, s)
        mk = Lk['mask']
        th = cx.new_act(n, yk.h, yk.w, yk.c, yk.ld)
        lib.call('tg_actgrad_f32', tz.ptr, tz.ld, yk.ptr, yk.ld, lib.ptr(mk), yk.c, 1.0 / KEEP if mk is not None else 1.0, th.ptr, th.ld, yk.rows,
                 yk.c, LRE, 0.2, s)
        # ---- sweep 4 (per layer): dW_eff = wgrad(tangent input, dpre_k)
        desc = geom.conv_wgrad(n, a.h, a.w, a.ld, yk.ld, 3, row.stride, 'SAME')
        _filter_grad(cx, st, grad, row, desc, ta, Lk['dpre'], 9, a.c)
        src, mask = th, None
    tp = cx.new_act(n, 1, 1, cl + ncls, pad32(cl + ncls))
    lib.call('tg_gavgpool_concat_f32', src.ptr, src.ld, cl, lib.ptr(zlab), ncls, tp.ptr, tp.ld, n, hw, s)
    _filter_grad(cx, st, grad, head, None, tp, None, 1, cl + ncls)
    return gp, dict(x=x, masks=[m0] + [Lk['mask'] for Lk in L if Lk['mask'] is not None], acts=[Lk['y'] for Lk in L], gx=gx, r=r)


def mnist_sweeps(cx, st, layers, head, rule, real, y, grad):
    """the sweeps on the MNIST discriminator: lrelu dense `layers` with additive noise behind each activation, label concats, dense
    `head`.  real, fake: [N,784] (the generator's and as_image()'s layout: one slope per image) or [N,28,28,1] (slopes over H)."""
    n, ncls, s = real.n, y.c, cx.stream
    F = real.h * real.w * real.c
    if F + ncls != st.shape(layers[0].w)[0]:
        raise lib.TgError("%s: MNIST images of %d values expected, got %s" % (rule.who, st.shape(layers[0].w)[0] - ncls, (real.h, real.w, real.c)))
    P = lib.ptr
    zlab = cx.scratch('zlab', n * ncls)
    lib.call('tg_fill_f32', P(zlab), 0.0, n * ncls, s)
    x = rule.point(cx, real, n, 1, 1, F, F)                            # dense [N, F] whatever the input's layout

    def noisy_concat(h, noise):                                        # concat([h + noise, y], 1)
        a = cx.new_act(n, 1, 1, h.c + ncls, pad32(h.c + ncls))
        lib.call('tg_pad_add_f32', h.ptr, h.ld, h.c, P(noise), h.c, a.ptr, a.ld, n, s)
        ops.copy2d(a.t, a.ld, h.c, y.t, y.ld, n, ncls)
        return a
    # ---- sweep 1: forward, keeping each layer's input and its activation before the noise
    noises = [cx.rng.normal(cx, cx.next_rng_name('noise'), n * F, 0.2)]
    a = noisy_concat(x, noises[0])
    L = []
    for row in layers:
        w_oti, w_hwio = _filter_prep(cx, st, row, 1, a.c)
        co_p = pad32(row.cout)
        d = geom.conv_fwd(n, 1, 1, a.ld, co_p, 1, 1, 'SAME', act='lrelu', alpha=0.2)
        h = cx.new_act(n, 1, 1, row.cout, co_p)
        _igemm(cx, 'tg_igemm_f32', d, a.ptr, P(w_oti), P(st.value(row.b)), h.ptr, s)
        L.append(dict(row=row, a=a, h=h, w_oti=w_oti, w_hwio=w_hwio))
        noises.append(cx.rng.normal(cx, cx.next_rng_name('noise'), n * row.cout, 0.2))
        a = noisy_concat(h, noises[-1])
    w_head, _ = _filter_prep(cx, st, head, 1, a.c)
    # ---- sweep 2: d sum(logits) / dx; the noise passes the gradient through, lrelu' comes from the pre-noise activation
    da = cx.new_act(n, 1, 1, a.c, a.ld)
    lib.call('tg_copy2d_f32', P(w_head), 0, da.ptr, da.ld, n, a.c, s)          # W_eff of the head, one row per image
    for Lk in reversed(L):
        h, ak = Lk['h'], Lk['a']
        dpre = cx.new_act(n, 1, 1, h.c, h.ld)
        lib.call('tg_actgrad_f32', da.ptr, da.ld, h.ptr, h.ld, None, 0, 1.0, dpre.ptr, dpre.ld, n, h.c, LRE, 0.2, s)
        Lk['dpre'] = dpre
        da = cx.new_act(n, 1, 1, ak.c, ak.ld)
        dds = lib.desc_array(geom.conv_dgrad(n, 1, 1, ak.ld, dpre.ld, 1, 1, 'SAME', ld_out=ak.ld, n_store=ak.ld))
        _igemm(cx, 'tg_igemm_multi_f32', dds, len(dds), dpre.ptr, P(Lk['w_hwio']), None, da.ptr, s)
    gx = cx.new_act(n, 1, 1, F, F)
    lib.call('tg_actgrad_f32', da.ptr, da.ld, None, 0, None, 0, 1.0, gx.ptr, F, n, F, 0, 0.0, s)
    # ---- sweep 3: the penalty (Wgan: over axis 1 of the tensor passed in, the features of [N, F], H of NHWC — gx is viewed in real's
    # layout; R1: per image in either), then the tangent forward
    gp, r = rule.penalise(cx, Act(gx.t, n, real.h, real.w, real.c, real.c))
    r_ld = r.h * r.w * r.ld                                            # r as [N, F]: its row stride
    ta = cx.new_act(n, 1, 1, F + ncls, L[0]['a'].ld)
    lib.call('tg_cond_concat_f32', r.ptr, r_ld, F, None, 0, 1.0, P(zlab), ncls, ta.ptr, ta.ld, n, 1, s)
    for Lk in L:
        h = Lk['h']
        d = geom.conv_fwd(n, 1, 1, ta.ld, h.ld, 1, 1, 'SAME')
        tz = cx.new_act(n, 1, 1, h.c, h.ld)
        _igemm(cx, 'tg_igemm_f32', d, ta.ptr, P(Lk['w_oti']), None, tz.ptr, s)
        # ---- sweep 4 (per layer): dW_eff = wgrad(tangent input, dpre) -> dV, dg
        desc = geom.conv_wgrad(n, 1, 1, ta.ld, h.ld, 1, 1, 'SAME')
        _filter_grad(cx, st, grad, Lk['row'], desc, ta, Lk['dpre'], 1, ta.c)
        th = cx.new_act(n, 1, 1, h.c, h.ld)
        lib.call('tg_actgrad_f32', tz.ptr, tz.ld, h.ptr, h.ld, None, 0, 1.0, th.ptr, th.ld, n, h.c, LRE, 0.2, s)
        ta = cx.new_act(n, 1, 1, h.c + ncls, pad32(h.c + ncls))
        lib.call('tg_cond_concat_f32', th.ptr, th.ld, h.c, None, 0, 1.0, P(zlab), ncls, ta.ptr, ta.ld, n, 1, s)
    _filter_grad(cx, st, grad, head, None, ta, None, 1, ta.c)
    return gp, dict(x=x, noise=noises, acts=[Lk['h'] for Lk in L], gx=gx, r=r)
