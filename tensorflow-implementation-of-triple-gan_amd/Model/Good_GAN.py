"""Good_GAN — MI355X-native counterpart of the reference's Model/Good_GAN.py (MNIST and SVHN configs; its unused
cifar10 branches are the svhn ones verbatim and are served by the same code).

Same class and method protocol (`Model(config)`, `.good_generator(z, y)`, `.discriminator(image, y)`,
`.classifier(image, train_ph)`, `.good_sampler(z, y)`, `.forward_pass(...)`); line references are to the reference
file.  Layers run in the gfx950 kernels of csrc/ through Model/model_base.py.

Eager-execution notes: tensors are tg.runtime.Act handles, `train_ph` is a Python bool; variables are
created in the constructor with the initialisers the reference passes — including its quirk that
`tf.random_normal_initializer(0.02)` / `tf.truncated_normal_initializer(0.02)` set the MEAN to 0.02 with stddev 1.0
(Model/modle_base.py:28,159,248); nonlinearities are fused into the producing kernel.
`segments=` (extension): the classifier uses full batch norm, whose statistics are per application, so a batched
call runs the applications one after the other and concatenates the logits.
"""
import numpy as np

from Model import model_base
from tg import ops
from tg.runtime import Act, ParamStore, ctx, pad32

D_MNIST_DENSE = (1000, 500, 250, 250, 250)                    # d_h0_wndense0 .. d_h4_wndense0 (:93-124), then the head d_h5_wndense0
D_SVHN_CONVS = [  # name, filters, stride, dropout after, label copies concatenated in front (:126-165)
    ('d_h0_wnconv0', 32, 1, False, 1), ('d_h0_wnconv1', 32, 2, True, 1), ('d_h1_wnconv0', 64, 1, False, 1),
    ('d_h1_wnconv1', 64, 2, True, 1), ('d_h2_wnconv0', 128, 1, False, 1), ('d_h2_wnconv1', 128, 1, False, 2)]


def _trunc_normal(rng, shape):
    x = rng.standard_normal(shape)
    bad = np.abs(x) > 2
    while bad.any():
        x[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(x) > 2
    return x


class Good_GAN(model_base.NN_Base):
    def __init__(self, config):
        super(Good_GAN, self).__init__(config.BATCH_NORM_DECAY, config.BATCH_NORM_EPSILON)
        self.config = config
        if config.DATA_NAME not in ('mnist', 'svhn', 'cifar10'):
            raise ValueError("The specified dataset is not yet implemented!")
        self.mnist = config.DATA_NAME == 'mnist'
        self._create_variables(getattr(config, 'SEED', 0))

    # ------------------------------------------------------------------ variables
    def param_specs(self):
        """{network: [(name, shape, trainable, init)]} in TF creation order."""
        k, zd = self.config.NUM_CLASSES, self.config.Z_DIM
        g, d, c = [], [], []

        def dense(L, p, cin, cout):
            L += [(p + '/kernel', (cin, cout), True, 'n02'), (p + '/bias', (cout,), True, 0.)]

        def wn(L, p, shape):
            L += [(p + '/V', shape, True, 'n05'), (p + '/g', (shape[-1] if len(shape) != 4 or shape[0] == 3 else shape[2],), True, 1.),
                  (p + '/b', (shape[-1] if len(shape) != 4 or shape[0] == 3 else shape[2],), True, 0.)]

        def bn(L, p, ch):
            L += [(p + '/beta', (ch,), True, 0.), (p + '/gamma', (ch,), True, 1.), (p + '/moving_mean', (ch,), False, 0.),
                  (p + '/moving_variance', (ch,), False, 1.)]

        G, D, C = 'good_generator/', 'discriminator/', 'classifier/'
        if self.mnist:
            dense(g, G + 'gg_h0_lin/gg_h0_lin', zd + k, 500); bn(g, G + 'gg_bn0', 500)
            dense(g, G + 'gg_h1_lin/gg_h1_lin', 500 + k, 500); bn(g, G + 'gg_bn1', 500)
            wn(g, G + 'gg_h2_lin', (500 + k, 784))
            cin = 784
            for i, n in enumerate((1000, 500, 250, 250, 250, 1)):
                wn(d, D + 'd_h%d_wndense0' % i, (cin + k, n))
                cin = n
            cin = 1
            for name, bname, cout in (('c_h0_conv0', 'c_h0_bn0', 32), ('c_h1_conv0', 'c_h1_bn0', 64), ('c_h1_conv1', 'c_h1_bn1', 64),
                                      ('c_h2_conv0', 'c_h2_bn0', 128), ('c_h2_conv1', 'c_h2_bn1', 128)):
                c += [(C + '%s/%s/kernel' % (name, name), (3, 3, cin, cout), True, 'tn02'), (C + '%s/%s/bias' % (name, name), (cout,), True, 0.)]
                bn(c, C + bname, cout)
                cin = cout
        else:
            dense(g, G + 'gg_h0_lin/gg_h0_lin', zd + k, 8192); bn(g, G + 'gg_bn0', 512)
            cin = 512
            for i, cout in enumerate((256, 128)):
                p = G + 'gg_dconv%d/gg_dconv%d' % (i, i)
                g += [(p + '/kernel', (5, 5, cout, cin + k), True, 'n02'), (p + '/bias', (cout,), True, 0.)]
                bn(g, G + 'gg_bn%d' % (i + 1), cout)
                cin = cout
            wn(g, G + 'gg_wndconv0', (5, 5, 3, cin + k))
            cin = 3
            for name, cout, extra in (('d_h0_wnconv0', 32, k), ('d_h0_wnconv1', 32, k), ('d_h1_wnconv0', 64, k), ('d_h1_wnconv1', 64, k),
                                      ('d_h2_wnconv0', 128, k), ('d_h2_wnconv1', 128, 2 * k)):
                wn(d, D + name, (3, 3, cin + extra, cout))
                cin = cout
            if getattr(self.config, 'MINIBATCH_DIS', False):                              # Good_GAN.py:159-162
                d += [(D + 'w', (cin + k, 100 * 5), True, 'xavier'), (D + 'b', (100,), True, 0.)]
                dense(d, D + 'd_h3_lin/d_h3_lin', cin + k + 100, 1)
            else:
                wn(d, D + 'd_h3_wndense', (cin + k, 1))
            cin = 3
            for name, bname, cout in (('c_h0_conv0', 'c_h0_bn0', 128), ('c_h0_conv1', 'c_h0_bn1', 128), ('c_h0_conv2', 'c_h0_bn2', 128),
                                      ('c_h1_conv0', 'c_h1_bn0', 256), ('c_h1_conv1', 'c_h1_bn1', 256), ('c_h1_conv2', 'c_h1_bn2', 256),
                                      ('c_h2_conv0', 'c_h2_bn0', 512)):
                c += [(C + '%s/%s/kernel' % (name, name), (3, 3, cin, cout), True, 'tn02'), (C + '%s/%s/bias' % (name, name), (cout,), True, 0.)]
                bn(c, C + bname, cout)
                cin = cout
            for name, bname, cout in (('c_h2_nin0', 'c_h2_bn1', 256), ('c_h2_nin1', 'c_h2_bn2', 128)):
                wn(c, C + name, (cin, cout))
                bn(c, C + bname, cout)
                cin = cout
        dense(c, C + 'c_h2_lin/c_h2_lin', cin, k)
        bn(c, C + 'c_h3_bn0', k)
        return {'good_generator': g, 'discriminator': d, 'classifier': c}

    def _create_variables(self, seed):
        cx = ctx()
        rng = np.random.default_rng(seed)
        for net, specs in self.param_specs().items():
            if net in cx.stores:
                continue
            st = ParamStore(net, [(n, s, t) for n, s, t, _ in specs], cx.device)
            for name, shape, _, init in specs:
                if init == 'n02':
                    st.set(name, 0.02 + rng.standard_normal(shape))
                elif init == 'tn02':
                    st.set(name, 0.02 + _trunc_normal(rng, shape))
                elif init == 'n05':
                    st.set(name, 0.05 * rng.standard_normal(shape))
                elif init == 'xavier':                                   # tf.contrib.layers.xavier_initializer(): uniform, fan_avg
                    lim = np.sqrt(6.0 / (shape[0] + shape[1]))
                    st.set(name, rng.uniform(-lim, lim, shape))
                else:
                    st.set(name, np.full(shape, init, np.float32))
            cx.stores[net] = st
        cx.stores['classifier'].enable_ema()

    # ------------------------------------------------------------------ helpers
    def as_image(self, a):
        """common per-image layout for batch concatenation: MNIST images travel flattened ([N,784], as the generator emits them)."""
        if self.mnist and (a.h, a.w) != (1, 1):
            return ops.view(a, 1, 1, a.h * a.w * a.c)
        return a

    def zca(self):
        return None

    # ------------------------------------------------------------------ networks
    def good_generator(self, z, y, reuse=False):
        """:15-83."""
        cx = ctx()
        with cx.variable_scope('good_generator'):
            zy = ops.cond_concat(z, y.t, y.c)
            if self.mnist:                                                                     # :19-33
                h0 = self._linear_fc(zy, 500, 'gg_h0_lin', activation=self._softplus)
                h0 = self._batch_norm_contrib(h0, 'gg_bn0', train=True)
                h1 = self._linear_fc(ops.cond_concat(h0, y.t, y.c), 500, 'gg_h1_lin', activation=self._softplus)
                h1 = self._batch_norm_contrib(h1, 'gg_bn1', train=True)
                return self._WN_dense(ops.cond_concat(h1, y.t, y.c), 28 * 28, 'gg_h2_lin', activation=self._sigmoid, narrow=True)
            h0 = self._linear_fc(zy, 4 * 4 * 512, 'gg_h0_lin', activation=self._relu)           # relu commutes with the reshape (:40-42)
            h0 = self._batch_norm_contrib(ops.reshape(h0, z.n, 4, 4, 512), 'gg_bn0', train=True)
            h0 = self._deconv2d(self._conv_cond_concat(h0, y), 256, k_w=5, k_h=5, d_w=2, d_h=2, name='gg_dconv0', activation=self._relu)
            h0 = self._batch_norm_contrib(h0, 'gg_bn1', train=True)
            h1 = self._deconv2d(self._conv_cond_concat(h0, y), 128, k_w=5, k_h=5, d_w=2, d_h=2, name='gg_dconv1', activation=self._relu)
            h1 = self._batch_norm_contrib(h1, 'gg_bn2', train=True)
            return self._WN_deconv2d(self._conv_cond_concat(h1, y), 3, k_w=5, k_h=5, d_w=2, d_h=2, init_scale=0.1, init=False,
                                     name='gg_wndconv0', activation=self._tanh, narrow=True)

    def good_sampler(self, z, y, reuse=True):
        """:356-426 — the generator graph with reuse."""
        return self.good_generator(z, y, reuse=True)

    def _d_out(self, logits, want_prob):
        """(tf.nn.sigmoid(logits), logits) (:124,206); no loss differentiates through the sigmoid."""
        if not want_prob:
            return None, logits
        with ctx().no_record():
            return ops.activation(logits, 'sigmoid'), logits

    def discriminator(self, image, y, reuse=False, want_prob=True):
        """:89-206.  Returns (sigmoid(logits), logits [N,1]); want_prob=False (extension, the trainer's solver runs): (None, logits)."""
        cx = ctx()
        lre = self._leaky_relu
        with cx.variable_scope('discriminator'):
            if self.mnist:                                                                     # :93-124
                h = self._add_noise(self.as_image(image), stddev=0.2)
                for i in range(5):
                    h = self._WN_dense(ops.cond_concat(h, y.t, y.c), (1000, 500, 250, 250, 250)[i], 'd_h%d_wndense0' % i, init=False, activation=lre)
                    h = self._add_noise(h, stddev=0.2)
                return self._d_out(self._WN_dense(ops.cond_concat(h, y.t, y.c), 1, 'd_h5_wndense0', init=False, narrow=True), want_prob)
            image = self._drop_out(image, 0.2, True, fuse_next=True)                           # :126-165
            # (layers whose output goes straight into the next concat write that concatenation themselves: then_concat, ops.conv2d(concat=...))
            h0 = self._WN_conv2d(self._conv_cond_concat(image, y), 32, k_h=3, k_w=3, d_h=1, d_w=1, init=False, name="d_h0_wnconv0", activation=lre,
                                 then_concat=y)
            h0 = self._WN_conv2d(self._conv_cond_concat(h0, y), 32, k_h=3, k_w=3, d_h=2, d_w=2, init=False, name="d_h0_wnconv1", activation=lre)
            h0 = self._drop_out(h0, 0.2, True, fuse_next=True)
            h1 = self._WN_conv2d(self._conv_cond_concat(h0, y), 64, k_h=3, k_w=3, d_h=1, d_w=1, init=False, name="d_h1_wnconv0", activation=lre,
                                 then_concat=y)
            h1 = self._WN_conv2d(self._conv_cond_concat(h1, y), 64, k_h=3, k_w=3, d_h=2, d_w=2, init=False, name="d_h1_wnconv1", activation=lre)
            h1 = self._drop_out(h1, 0.2, True, fuse_next=True)
            y2 = _twice(y)
            h2 = self._WN_conv2d(self._conv_cond_concat(h1, y), 128, k_h=3, k_w=3, d_h=1, d_w=1, init=False, name="d_h2_wnconv0", activation=lre,
                                 then_concat=(y2, 2 * y.c))
            h2 = ops.cond_concat(h2, y2, 2 * y.c)                                               # y is concatenated twice (:151-153)
            h2 = self._WN_conv2d(h2, 128, k_h=3, k_w=3, d_h=1, d_w=1, init=False, name="d_h2_wnconv1", activation=lre)
            h3 = ops.global_avgpool_concat(h2, y.t, y.c)                                        # reduce_mean + concat y
            if self.config.MINIBATCH_DIS:                                                      # :159-162 (off in every config of the reference)
                h3 = self._minibatch_discrimination(h3, 100, concat_input=True)               # f = ...; h3 = tf.concat([h3, f], 1)
                return self._d_out(self._linear_fc(h3, 1, 'd_h3_lin', narrow=True), want_prob)
            return self._d_out(self._WN_dense(h3, 1, 'd_h3_wndense', narrow=True), want_prob)

    # ------------------------------------------------------------------ WGAN-GP
    def discriminator_gradient_penalty(self, real, fake, y, weight=1.0, in_step=False):
        """gp and d gp / d theta_D of the reference's _gradient_penalty (Training/train_base.py:598-620) on this discriminator, with the
        contract of Good_GAN_cifar10.discriminator_gradient_penalty: x = real + alpha (fake - real), alpha ~ U[0,1) per image, gx =
        d sum(logits) / dx, s = sqrt(reduce_sum(gx^2, axis=1)), gp = mean((s - 1)^2).  Returns (weight * gp as a 1-element device tensor,
        weight * d gp / d theta_D as a flat buffer laid out like the discriminator's ParamStore.g, valid until the next call); ParamStore.g
        is not touched.  real, fake: Act of one shape — MNIST [N,784] (the generator's and as_image()'s layout: axis 1 is the feature
        axis, one slope per image) or [N,28,28,1] (axis 1 is H), SVHN [N,32,32,3]; y: label Act [N,NUM_CLASSES].

        With its dropout masks and noise drawn the network is piecewise linear in x, and weight norm W = g V/||V|| only reparametrises
        the effective filter, so the four first-order sweeps of DESIGN §9.1 give d gp / dW_eff exactly (all on the implicit-GEMM
        launches, the dense layers as 1x1 ones):
          1. forward (filters weight-normalised by tg_wn_scale_f32 + tg_filter_prep_f32, as ops.conv2d(wn=...)), keeping each layer's
             activation — for MNIST the one BEFORE its additive noise: lrelu' is the sign of the pre-activation, the noise is a constant;
          2. input-gradient sweep seeded with 1 per image, keeping each layer's pre-activation gradient dpre_k;
          3. the penalty (tg_grad_penalty_rows_f32 for [N, F], tg_grad_penalty_f32 for NHWC), then a tangent forward from r = d gp / d gx:
             zero label channels, no biases, * lrelu', the same dropout masks, no noise;
          4. dW_eff_k = wgrad(tangent input of layer k, dpre_k); the head's is the sum over images of its tangent input.  tg_wn_bwd_f32
             maps each to dV, dg at the store offsets of .../V and .../g; every .../b entry stays exactly 0.
        Masks, noise and alpha are drawn in the RNG scope 'GP' ('alpha', 'drop0..2' / 'noise0..5'); buffers live under the phase
        'wgan_gp'.  Minibatch discrimination (config.MINIBATCH_DIS) couples the images of a batch and is refused, as are the bf16 MFMA
        operands.  in_step=True: inside the caller's solver run, as
        Good_GAN_cifar10.discriminator_gradient_penalty."""
        from tg import lib
        cx = ctx()
        if getattr(self.config, 'MINIBATCH_DIS', False):
            raise lib.TgError("discriminator_gradient_penalty: MINIBATCH_DIS = True is not supported: minibatch discrimination couples the "
                              "images of a batch, so the discriminator is not piecewise linear in one image and the penalty's gradient needs "
                              "second-order terms")
        if cx.mfma_dtype != 'f32':
            raise lib.TgError("discriminator_gradient_penalty: fp32 MFMA path only (MFMA_DTYPE %r): the penalty differentiates a gradient, "
                              "and bf16-rounded operands in the four sweeps are not pinned to a reference" % (cx.mfma_dtype,))
        if (real.n, real.h, real.w, real.c) != (fake.n, fake.h, fake.w, fake.c):
            raise lib.TgError("discriminator_gradient_penalty: real %s and fake %s differ in shape — bring both to one layout with "
                              "model.as_image() first" % ((real.n, real.h, real.w, real.c), (fake.n, fake.h, fake.w, fake.c)))
        if y.n != real.n or y.ld != y.c or getattr(real, 'dtype', 'f32') != 'f32' or getattr(fake, 'dtype', 'f32') != 'f32':
            raise lib.TgError("discriminator_gradient_penalty: dense fp32 labels [%d] and fp32 images of %d expected" % (y.n, real.n))
        st = cx.stores['discriminator']
        grad = cx.scratch('gpgrad', st.n_p) if in_step else cx.ws('wgan_gp:grad', st.n_p)
        with (cx.detached() if in_step else cx.phase_scope('wgan_gp', record=False)), cx.rng_scoped('GP'):
            lib.call('tg_fill_f32', lib.ptr(grad), 0.0, st.n_p, cx.stream)
            alpha = cx.rng.uniform(cx, 'alpha', real.n, 0.0, 1.0)
            sweeps = self._gp_mnist if self.mnist else self._gp_svhn
            gp, state = sweeps(cx, st, real, fake, y, float(weight), alpha, grad)
        state['alpha'] = alpha
        self.last_gp_state = state
        return gp[0:1], grad

    @staticmethod
    def _gp_wn_prep(cx, st, name, t, c_in, c_out):
        """the effective filter g V/||V|| of `name` in the MFMA layouts (as ops.conv2d(wn=...)): (OTI [co_p][t][ci_p], HWIO [t][ci_p][co_p])."""
        from tg import lib
        pre = 'discriminator/%s/' % name
        ci_p, co_p = pad32(c_in), pad32(c_out)
        scale = cx.scratch('wns', c_out)
        lib.call('tg_wn_scale_f32', lib.ptr(st.value(pre + 'V')), lib.ptr(st.value(pre + 'g')), t * c_in, c_out, lib.ptr(scale), cx.stream)
        w_oti, w_hwio = cx.scratch('woti', co_p * t * ci_p), cx.scratch('whwio', t * ci_p * co_p)
        lib.call('tg_filter_prep_f32', lib.ptr(st.value(pre + 'V')), lib.ptr(scale), None, t, c_in, c_out, ci_p, co_p, lib.ptr(w_hwio),
                 lib.ptr(w_oti), t * ci_p, ci_p, cx.stream)
        return w_oti, w_hwio

    @staticmethod
    def _gp_wn_grad(cx, st, grad, name, desc, t_in, dpre, t, c_in, c_out):
        """sweep 4 of one weight-normalised layer: dW_eff = wgrad(t_in, dpre) (desc: its geometry; None: the head, dpre = 1 per image,
        dW_eff = column sums of t_in), then dV, dg (tg_wn_bwd_f32) written at the store offsets of .../V and .../g in `grad`."""
        from tg import lib
        pre = 'discriminator/%s/' % name
        ov, og = st.offset(pre + 'V'), st.offset(pre + 'g')
        v, g = st.value(pre + 'V'), st.value(pre + 'g')
        dv, dg = grad[ov:ov + t * c_in * c_out], grad[og:og + c_out]
        dw = cx.scratch('dweff', t * c_in * c_out + 4)
        if desc is not None:
            ops.filter_grad(desc, t_in.t, dpre.t, t, c_in, c_out, dw, wn=(v, g, dv, dg), defer=False)
            return
        ops.colstats(0, t_in.t, t_in.ld, None, 0, t_in.rows, c_in, [t_in.rows], s1=dw)
        coef = cx.scratch('coef', 2 * c_out)
        lib.call('tg_wn_bwd_f32', lib.ptr(dw), lib.ptr(v), lib.ptr(g), t * c_in, c_out, lib.ptr(dv), lib.ptr(dg), lib.ptr(coef), cx.stream)

    def _gp_mnist(self, cx, st, real, fake, y, weight, alpha, grad):
        """the sweeps on the MNIST discriminator: five lrelu dense layers with additive noise behind each activation, label concats."""
        from tg import geom, lib
        from tg.lib import ACT
        n, ncls, s, lre = real.n, y.c, cx.stream, ACT['lrelu']
        F = real.h * real.w * real.c
        if F + ncls != st.shape('discriminator/d_h0_wndense0/V')[0]:
            raise lib.TgError("discriminator_gradient_penalty: MNIST images of %d values expected, got %s" % (
                st.shape('discriminator/d_h0_wndense0/V')[0] - ncls, (real.h, real.w, real.c)))
        rows2 = (real.h, real.w) == (1, 1)
        P = lib.ptr
        igemm = lambda name, *args: lib.call(name, *ops.igemm_scratch(cx, name, args, False))
        zlab = cx.scratch('zlab', n * ncls)
        lib.call('tg_fill_f32', P(zlab), 0.0, n * ncls, s)
        x = cx.new_act(n, 1, 1, F, F)                                      # dense [N, F] whatever the input's layout
        lib.call('tg_wgan_interp_f32', real.ptr, real.ld, fake.ptr, fake.ld, P(alpha), x.ptr, real.c, n, real.h * real.w, real.c, s)

        def noisy_concat(h, noise):                                        # concat([h + noise, y], 1)
            a = cx.new_act(n, 1, 1, h.c + ncls, pad32(h.c + ncls))
            lib.call('tg_pad_add_f32', h.ptr, h.ld, h.c, P(noise), h.c, a.ptr, a.ld, n, s)
            ops.copy2d(a.t, a.ld, h.c, y.t, y.ld, n, ncls)
            return a
        # ---- sweep 1: forward, keeping each layer's input and its activation before the noise
        noises = [cx.rng.normal(cx, cx.next_rng_name('noise'), n * F, 0.2)]
        a = noisy_concat(x, noises[0])
        L = []
        for i, cout in enumerate(D_MNIST_DENSE):
            name = 'd_h%d_wndense0' % i
            w_oti, w_hwio = self._gp_wn_prep(cx, st, name, 1, a.c, cout)
            co_p = pad32(cout)
            d = geom.conv_fwd(n, 1, 1, a.ld, co_p, 1, 1, 'SAME', act='lrelu', alpha=0.2)
            h = cx.new_act(n, 1, 1, cout, co_p)
            igemm('tg_igemm_f32', d, a.ptr, P(w_oti), P(st.value('discriminator/%s/b' % name)), h.ptr, s)
            L.append(dict(name=name, a=a, h=h, w_oti=w_oti, w_hwio=w_hwio))
            noises.append(cx.rng.normal(cx, cx.next_rng_name('noise'), n * cout, 0.2))
            a = noisy_concat(h, noises[-1])
        head = 'd_h5_wndense0'
        w_head, _ = self._gp_wn_prep(cx, st, head, 1, a.c, 1)
        # ---- sweep 2: d sum(logits) / dx; the noise passes the gradient through, lrelu' comes from the pre-noise activation
        da = cx.new_act(n, 1, 1, a.c, a.ld)
        lib.call('tg_copy2d_f32', P(w_head), 0, da.ptr, da.ld, n, a.c, s)          # W_eff of the head, one row per image
        for Lk in reversed(L):
            h, ak = Lk['h'], Lk['a']
            dpre = cx.new_act(n, 1, 1, h.c, h.ld)
            lib.call('tg_actgrad_f32', da.ptr, da.ld, h.ptr, h.ld, None, 0, 1.0, dpre.ptr, dpre.ld, n, h.c, lre, 0.2, s)
            Lk['dpre'] = dpre
            da = cx.new_act(n, 1, 1, ak.c, ak.ld)
            dds = lib.desc_array(geom.conv_dgrad(n, 1, 1, ak.ld, dpre.ld, 1, 1, 'SAME', ld_out=ak.ld, n_store=ak.ld))
            igemm('tg_igemm_multi_f32', dds, len(dds), dpre.ptr, P(Lk['w_hwio']), None, da.ptr, s)
        gx = cx.new_act(n, 1, 1, F, F)
        lib.call('tg_actgrad_f32', da.ptr, da.ld, None, 0, None, 0, 1.0, gx.ptr, F, n, F, 0, 0.0, s)
        # ---- sweep 3: the penalty (axis 1 of the tensor passed in: the features of [N, F], H of NHWC), then the tangent forward
        gp = cx.scratch('gp', 4)
        if rows2:
            r = cx.new_act(n, 1, 1, F, pad32(F))
            partials = cx.scratch('gpp', 2 * n)
            lib.call('tg_grad_penalty_rows_f32', gx.ptr, F, n, F, weight, r.ptr, r.ld, P(partials), P(gp), s)
            r_ld = r.ld
        else:
            hh, ww, cc = real.h, real.w, real.c
            r = cx.new_act(n, hh, ww, cc, cc)
            partials = cx.scratch('gpp', 2 * ((n * ww * cc + 255) // 256))
            lib.call('tg_grad_penalty_f32', gx.ptr, cc, n, hh, ww, cc, weight, r.ptr, cc, P(partials), P(gp), s)
            r_ld = F
        ta = cx.new_act(n, 1, 1, F + ncls, L[0]['a'].ld)
        lib.call('tg_cond_concat_f32', r.ptr, r_ld, F, None, 0, 1.0, P(zlab), ncls, ta.ptr, ta.ld, n, 1, s)
        for Lk in L:
            h = Lk['h']
            d = geom.conv_fwd(n, 1, 1, ta.ld, h.ld, 1, 1, 'SAME')
            tz = cx.new_act(n, 1, 1, h.c, h.ld)
            igemm('tg_igemm_f32', d, ta.ptr, P(Lk['w_oti']), None, tz.ptr, s)
            # ---- sweep 4 (per layer): dW_eff = wgrad(tangent input, dpre) -> dV, dg
            desc = geom.conv_wgrad(n, 1, 1, ta.ld, h.ld, 1, 1, 'SAME')
            self._gp_wn_grad(cx, st, grad, Lk['name'], desc, ta, Lk['dpre'], 1, ta.c, h.c)
            th = cx.new_act(n, 1, 1, h.c, h.ld)
            lib.call('tg_actgrad_f32', tz.ptr, tz.ld, h.ptr, h.ld, None, 0, 1.0, th.ptr, th.ld, n, h.c, lre, 0.2, s)
            ta = cx.new_act(n, 1, 1, h.c + ncls, pad32(h.c + ncls))
            lib.call('tg_cond_concat_f32', th.ptr, th.ld, h.c, None, 0, 1.0, P(zlab), ncls, ta.ptr, ta.ld, n, 1, s)
        self._gp_wn_grad(cx, st, grad, head, None, ta, None, 1, ta.c, 1)
        return gp, dict(x=x, noise=noises, acts=[Lk['h'] for Lk in L], gx=gx, r=r)

    def _gp_svhn(self, cx, st, real, fake, y, weight, alpha, grad):
        """the sweeps on the SVHN discriminator: input dropout, six lrelu 3x3 convolutions (dropout behind the two stride-2 ones, the
        label concatenated twice in front of the last), global mean, label concat, dense head — all weight-normalised."""
        from tg import geom, lib
        from tg.lib import ACT
        n, H, W, c0 = real.n, real.h, real.w, real.c
        ncls, keep, s, lre = y.c, 0.8, cx.stream, ACT['lrelu']
        c_img = st.shape('discriminator/d_h0_wnconv0/V')[2] - ncls
        if c0 != c_img or (H, W) == (1, 1):
            raise lib.TgError("discriminator_gradient_penalty: SVHN images [N,H,W,%d] expected, got %s" % (c_img, (H, W, c0)))
        P = lambda t: None if t is None else lib.ptr(t)
        igemm = lambda name, *args: lib.call(name, *ops.igemm_scratch(cx, name, args, False))
        labels = {1: (y.t, ncls), 2: (_twice(y), 2 * ncls)}
        zlab = cx.scratch('zlab', 2 * n * ncls)
        lib.call('tg_fill_f32', P(zlab), 0.0, 2 * n * ncls, s)
        x = cx.new_act(n, H, W, c0, c0)
        lib.call('tg_wgan_interp_f32', real.ptr, real.ld, fake.ptr, fake.ld, P(alpha), x.ptr, x.ld, n, H * W, c0, s)
        m0 = cx.rng.keep_mask(cx, cx.next_rng_name('drop'), n * H * W * c0, keep)
        # ---- sweep 1: forward, keeping every layer's input, activation and filter layouts
        L = []
        src, mask = x, m0
        for name, cout, stride, drop, copies in D_SVHN_CONVS:
            lab, nl = labels[copies]
            c_in = src.c + nl
            a = cx.new_act(n, src.h, src.w, c_in, pad32(c_in))
            lib.call('tg_cond_concat_f32', src.ptr, src.ld, src.c, P(mask), src.c, 1.0 / keep if mask is not None else 1.0, P(lab), nl,
                     a.ptr, a.ld, n, src.h * src.w, s)
            w_oti, w_hwio = self._gp_wn_prep(cx, st, name, 9, c_in, cout)
            d = geom.conv_fwd(n, a.h, a.w, a.ld, pad32(cout), 3, stride, 'SAME', act='lrelu', alpha=0.2)
            yk = cx.new_act(n, d.h_out, d.w_out, cout, pad32(cout))
            igemm('tg_igemm_f32', d, a.ptr, P(w_oti), P(st.value('discriminator/%s/b' % name)), yk.ptr, s)
            mask = cx.rng.keep_mask(cx, cx.next_rng_name('drop'), yk.rows * cout, keep) if drop else None
            L.append(dict(name=name, stride=stride, a=a, y=yk, w_oti=w_oti, w_hwio=w_hwio, mask=mask, nl=nl))
            src = yk
        last = L[-1]['y']
        cl, hw = last.c, last.h * last.w
        head = 'd_h3_wndense'
        w_head, _ = self._gp_wn_prep(cx, st, head, 1, cl + ncls, 1)
        # ---- sweep 2: d sum(logits) / dx; dpre_k = gradient at layer k's pre-activation
        dp = cx.scratch('dp', n * pad32(cl))
        lib.call('tg_copy2d_f32', P(w_head), 0, P(dp), pad32(cl), n, cl, s)              # W_eff of the head (its feature rows) per image
        dpre = cx.new_act(n, last.h, last.w, cl, last.ld)
        lib.call('tg_gavgpool_bwd_f32', P(dp), pad32(cl), last.ptr, last.ld, dpre.ptr, dpre.ld, n, hw, cl, lre, 0.2, s)
        for k in range(len(L) - 1, -1, -1):
            Lk = L[k]
            Lk['dpre'] = dpre
            a = Lk['a']
            da = cx.new_act(n, a.h, a.w, a.c, a.ld)
            dds = lib.desc_array(geom.conv_dgrad(n, a.h, a.w, a.ld, dpre.ld, 3, Lk['stride'], 'SAME', ld_out=a.ld, n_store=a.ld))
            igemm('tg_igemm_multi_f32', dds, len(dds), dpre.ptr, P(Lk['w_hwio']), None, da.ptr, s)
            if k > 0:
                yp, mp = L[k - 1]['y'], L[k - 1]['mask']
                dpre = cx.new_act(n, yp.h, yp.w, yp.c, yp.ld)
                lib.call('tg_actgrad_f32', da.ptr, da.ld, yp.ptr, yp.ld, P(mp), yp.c, 1.0 / keep if mp is not None else 1.0, dpre.ptr, dpre.ld,
                         yp.rows, yp.c, lre, 0.2, s)
        gx = cx.new_act(n, H, W, c0, pad32(c0))
        lib.call('tg_actgrad_f32', da.ptr, da.ld, None, 0, P(m0), c0, 1.0 / keep, gx.ptr, gx.ld, gx.rows, c0, 0, 0.0, s)
        # ---- sweep 3: the penalty (slopes over H, axis 1 of NHWC), then the tangent forward from r
        r = cx.new_act(n, H, W, c0, gx.ld)
        partials = cx.scratch('gpp', 2 * ((n * W * r.ld + 255) // 256))
        gp = cx.scratch('gp', 4)
        lib.call('tg_grad_penalty_f32', gx.ptr, gx.ld, n, H, W, c0, weight, r.ptr, r.ld, P(partials), P(gp), s)
        src, mask = r, m0
        for Lk in L:
            a, yk = Lk['a'], Lk['y']
            ta = cx.new_act(n, a.h, a.w, a.c, a.ld)
            lib.call('tg_cond_concat_f32', src.ptr, src.ld, src.c, P(mask), src.c, 1.0 / keep if mask is not None else 1.0, P(zlab), Lk['nl'],
                     ta.ptr, ta.ld, n, a.h * a.w, s)
            d = geom.conv_fwd(n, a.h, a.w, a.ld, yk.ld, 3, Lk['stride'], 'SAME')
            tz = cx.new_act(n, yk.h, yk.w, yk.c, yk.ld)
            igemm('tg_igemm_f32', d, ta.ptr, P(Lk['w_oti']), None, tz.ptr, s)
            mk = Lk['mask']
            th = cx.new_act(n, yk.h, yk.w, yk.c, yk.ld)
            lib.call('tg_actgrad_f32', tz.ptr, tz.ld, yk.ptr, yk.ld, P(mk), yk.c, 1.0 / keep if mk is not None else 1.0, th.ptr, th.ld, yk.rows,
                     yk.c, lre, 0.2, s)
            # ---- sweep 4 (per layer): dW_eff = wgrad(tangent input, dpre) -> dV, dg
            desc = geom.conv_wgrad(n, a.h, a.w, a.ld, yk.ld, 3, Lk['stride'], 'SAME')
            self._gp_wn_grad(cx, st, grad, Lk['name'], desc, ta, Lk['dpre'], 9, a.c, yk.c)
            src, mask = th, None
        tp = cx.new_act(n, 1, 1, cl + ncls, pad32(cl + ncls))
        lib.call('tg_gavgpool_concat_f32', src.ptr, src.ld, cl, P(zlab), ncls, tp.ptr, tp.ld, n, hw, s)
        self._gp_wn_grad(cx, st, grad, head, None, tp, None, 1, cl + ncls, 1)
        return gp, dict(x=x, masks=[m0] + [Lk['mask'] for Lk in L if Lk['mask'] is not None], acts=[Lk['y'] for Lk in L], gx=gx, r=r)

    def classifier(self, image, train_ph, reuse=False, segments=None):
        """:212-350.  Returns (logits [N,10], feature).  `segments` (extension): image counts of the applications batched into
        `image` — the convolutions run once over the whole batch, every batch norm keeps per-application statistics and
        updates its moving statistics application by application (tg_bn_train_f32)."""
        cx = ctx()
        lre = self._leaky_relu

        def cbr(x, cname, bname, cout, k=3, bf16_out=False):
            # conv -> leaky relu -> batch norm: in training the batch-norm statistics are taken in the convolution's epilogue.
            # bf16_out: the next layer is a 3x3 / stride-1 convolution and nothing else reads the batch norm's output (config.ACT_DTYPE)
            x = self._conv2d(x, cout, k_h=k, k_w=k, d_h=1, d_w=1, name=cname, activation=lre,
                             bn_segments=(segments or [x.n]) if train_ph else None)
            return self._batch_norm_contrib(x, name=bname, train=train_ph, segments=segments, bf16_out=bf16_out)

        def pool_drop(x, key):
            mask = cx.rng.keep_mask(cx, key, x.rows // 4 * x.c, 0.5) if train_ph else None
            return ops.maxpool2_dropout(x, mask, 2.0)

        with cx.variable_scope('classifier'):
            if self.mnist:                                                                         # :216-247
                img = ops.view(image, 28, 28, 1) if (image.h, image.w) == (1, 1) else image
                noise = cx.rng.normal(cx, 'noise', img.rows * img.c, 0.3)
                x = ops.im2col3x3_add(img, noise)                    # _add_noise + the 1-channel 3x3 window gathered once
                x = cbr(x, 'c_h0_conv0', 'c_h0_bn0', 32, k=1)
                x = pool_drop(x, 'drop1')
                x = cbr(x, 'c_h1_conv0', 'c_h1_bn0', 64)
                x = cbr(x, 'c_h1_conv1', 'c_h1_bn1', 64)
                x = pool_drop(x, 'drop2')
                x = cbr(x, 'c_h2_conv0', 'c_h2_bn0', 128)
                x = cbr(x, 'c_h2_conv1', 'c_h2_bn1', 128)
            else:                                                                                  # :249-299
                image = self._drop_out(image, 0.2, train_ph, name='drop0')
                x = ops.im2col3x3_add(image, None)
                x = cbr(x, 'c_h0_conv0', 'c_h0_bn0', 128, k=1, bf16_out=True)
                x = cbr(x, 'c_h0_conv1', 'c_h0_bn1', 128, bf16_out=True)
                x = cbr(x, 'c_h0_conv2', 'c_h0_bn2', 128)
                x = pool_drop(x, 'drop1')
                x = cbr(x, 'c_h1_conv0', 'c_h1_bn0', 256, bf16_out=True)
                x = cbr(x, 'c_h1_conv1', 'c_h1_bn1', 256, bf16_out=True)
                x = cbr(x, 'c_h1_conv2', 'c_h1_bn2', 256)
                x = pool_drop(x, 'drop2')
                x = cbr(x, 'c_h2_conv0', 'c_h2_bn0', 512)
                x = self._batch_norm_contrib(self._nin(x, 256, name='c_h2_nin0', activation=lre), name='c_h2_bn1', train=train_ph, segments=segments)
                x = self._batch_norm_contrib(self._nin(x, 128, name='c_h2_nin1', activation=lre), name='c_h2_bn2', train=train_ph, segments=segments)
            fm = ops.global_avgpool(x)                                                             # tf.reduce_mean(axis=[1,2])
            h = self._linear_fc(fm, self.config.NUM_CLASSES, 'c_h2_lin')
            return self._batch_norm_contrib(h, name='c_h3_bn0', train=train_ph, segments=segments), fm

    def forward_pass(self, z_g, y_g, x_l_c, y_l_c, x_l_d, y_l_d, x_u_d, x_u_c, train):
        """:428-472 (evaluation / tests; the trainer runs per-solver sub-graphs)."""
        from tg.batching import concat_acts
        cx = ctx()
        k = self.config.NUM_CLASSES
        G = self.good_generator(z_g, y_g)
        parts = [self.as_image(a) for a in (x_l_c, x_u_c, x_u_d, G)]
        segs = [p.n for p in parts]
        with cx.rng_scoped(cx.phase + '/C'):
            logits, _ = self.classifier(concat_acts(parts), train, segments=segs)
        offs = [int(v) for v in np.cumsum([0] + segs)]
        C_real, C_unl, C_unl_d, C_fake = [logits.view_rows(offs[i], offs[i + 1]) for i in range(4)]
        oh_d = Act(ops.argmax_onehot(C_unl_d, k), C_unl_d.n, 1, 1, k, k)
        oh_u = Act(ops.argmax_onehot(C_unl, k), C_unl.n, 1, 1, k, k)
        ximg = concat_acts([self.as_image(a) for a in (x_l_d, x_u_d, G, x_u_c)])
        yall = concat_acts([y_l_d, oh_d, y_g, oh_u])
        with cx.rng_scoped(cx.phase + '/D'):
            dp, dl = self.discriminator(ximg, yall)
        n_p = x_l_d.n + x_u_d.n
        cut = lambda a: [a.view_rows(0, n_p), a.view_rows(n_p, n_p + G.n), a.view_rows(n_p + G.n, a.n)]
        (p_real, p_fake, p_unl), (l_real, l_fake, l_unl) = cut(dp), cut(dl)
        return [G, [p_real, l_real, p_fake, l_fake, p_unl, l_unl], [C_real, C_unl, C_unl_d, C_fake]]


def _twice(y):
    """device tensor [N, 2k] = [y, y] for the doubled cond-concat of the SVHN discriminator."""
    from tg.batching import concat_acts
    cx = ctx()
    out = cx.new_act(y.n, 1, 1, 2 * y.c, 2 * y.c, tag='yy')
    ops.copy2d(out.t, 2 * y.c, 0, y.t, y.c, y.n, y.c)
    ops.copy2d(out.t, 2 * y.c, y.c, y.t, y.c, y.n, y.c)
    return out.t
