"""Good_GAN_cifar10 — MI355X-native counterpart of the reference's Model/Good_GAN_cifar10.py.

Same class, method names and call protocol (`Model(config)`, `.good_generator(z, y)`,
`.discriminator(image, y)`, `.classifier(inp, is_training)`, `.good_sampler(z, y)`,
`.forward_pass(...)`); every layer runs in the hand-written gfx950 kernels of csrc/ through
Model/nn.py and Model/model_base.py, which also holds what this model shares with Model/Good_GAN.py
(variable creation, forward_pass); the reference's `cifar10_ZCA` lives in Model/zca.py.  This file
holds the layer tables and the networks.  Line references are to the reference file.  Differences forced by eager execution:
  * tensors are tg.runtime.Act handles, `is_training` is a Python bool;
  * variables are created (with the reference's initialisers) when the Model
    is constructed — the reference's throw-away `init=True` builds (:216,227,263) only create variables
    (their g / b assigns are never run); `data_dependent_init` runs them (config.WN_INIT = 'data');
  * `segments=` (extension) batches several applications of C or D into one call: identical maths,
    since D has no batch statistics and C's mean-only BN is computed per segment.
"""
from Model import model_base
from Model import nn
from Model import zca
from tg import grad_penalty, ops
from tg.runtime import ctx


# layer tables (class attributes so that a deeper variant only lists more rows, Model/Good_GAN_stress64.py)
C_CONVS = [  # name, filters, padding, max-pool + dropout after       (:106-149)
    ('conv1_1', 128, 'SAME', False), ('conv1_2', 128, 'SAME', False), ('conv1_3', 128, 'SAME', True),
    ('conv2_1', 256, 'SAME', False), ('conv2_2', 256, 'SAME', False), ('conv2_3', 256, 'SAME', True), ('conv3', 512, 'VALID', False)]
D_CONVS = [  # name, filters, stride, dropout after                 (:66-91)
    ('conv2d_00', 32, 1, False), ('conv2d_01', 32, 2, True), ('conv2d_10', 64, 1, False), ('conv2d_11', 64, 2, True),
    ('conv2d_20', 128, 1, False), ('conv2d_21', 128, 1, False)]
G_DECONVS = [('gg_dconv0', 256), ('gg_dconv1', 128), ('gg_dconv2', 3)]      # (:44-57); the last one is the tanh image layer


class Good_GAN_cifar10(model_base.NN_Base):
    C_CONVS, D_CONVS, G_DECONVS = C_CONVS, D_CONVS, G_DECONVS
    # Data-parallel gradient buckets: per network, the first variable (creation order) of every bucket after the first.
    # A bucket is one contiguous slice of the network's flat gradient buffer; the forward pass marks the matching boundary right before
    # the layer that owns the variable (Context.grad_bucket_boundary), so that the backward pass — run bucket by bucket — has the slice
    # from that variable on final when it comes back to the mark, and its all-reduce runs on the exchange stream beside the rest:
    #   classifier     [conv2_1 ... output_dense] (87 % of 12.5 MB) beside the backward pass of the first block, then [conv1_1 ... conv1_3]
    #   generator      [gg_dconv0 ... gg_dconv2] (17 of 20.5 MB; the 13 MB gg_dconv0 filter gradient is final here) beside bn0 / gg_h0_lin
    #   discriminator  one bucket per resolution stage: [conv2d_20 ... lin], [conv2d_10, conv2d_11], [conv2d_00, conv2d_01]
    GRAD_BUCKETS = {'classifier': ['classifier/conv2_1/V'],
                    'good_generator': ['good_generator/gg_dconv0/gg_dconv0/kernel'],
                    'discriminator': ['discriminator/conv2d_10/conv2d_10/kernel', 'discriminator/conv2d_20/conv2d_20/kernel']}

    def __init__(self, config):
        super(Good_GAN_cifar10, self).__init__(config.BATCH_NORM_DECAY, config.BATCH_NORM_EPSILON)
        self.config = config
        self._create_variables(getattr(config, 'SEED', 0), self.param_specs(config.Z_DIM, config.NUM_CLASSES))
        self._zca = None
        # (sweep body, layer rows, head) of the discriminator for the gradient penalty
        self._gp = (grad_penalty.conv_sweeps, [grad_penalty.plain(*row) for row in self.D_CONVS], grad_penalty.plain('lin', 1))

    # ------------------------------------------------------------------ variables
    @classmethod
    def param_specs(cls, z_dim=100, ncls=10):
        """(network, name, shape, trainable, init) in TF creation order."""
        g, d, c = [], [], []
        C_CONVS, D_CONVS, G_DECONVS = cls.C_CONVS, cls.D_CONVS, cls.G_DECONVS
        p = 'good_generator/'
        g += [(p + 'gg_h0_lin/gg_h0_lin/kernel', (z_dim + ncls, 8192), True, 'he'), (p + 'gg_h0_lin/gg_h0_lin/bias', (8192,), True, 0.)]
        cin = 512
        for i, (name, cout) in enumerate([('bn0', 8192)] + G_DECONVS):
            if i > 0:
                g += [(p + '%s/%s/kernel' % (name, name), (5, 5, cout, cin + ncls), True, 'he'),
                      (p + '%s/%s/bias' % (name, name), (cout,), True, 0.)]
                cin = cout
            if i < len(G_DECONVS):
                bn = p + 'gg_bn%d/' % i
                g += [(bn + 'beta', (cout,), True, 0.), (bn + 'gamma', (cout,), True, 1.),
                      (bn + 'moving_mean', (cout,), False, 0.), (bn + 'moving_variance', (cout,), False, 1.)]
        cin = 3
        for name, cout, _, _ in D_CONVS:
            q = 'discriminator/%s/%s/' % (name, name)
            d += [(q + 'kernel', (3, 3, cin + ncls, cout), True, 'he'), (q + 'bias', (cout,), True, 0.)]
            cin = cout
        d += [('discriminator/lin/lin/kernel', (cin + ncls, 1), True, 'he'), ('discriminator/lin/lin/bias', (1,), True, 0.)]
        cin = 3
        layers = [('classifier/%s/' % n, (3, 3, cin_, co)) for (n, co, _, _), cin_ in
                  zip(C_CONVS, [3] + [co for _, co, _, _ in C_CONVS[:-1]])]
        layers += [('classifier/NiN1/NiN1/', (512, 256)), ('classifier/NiN2/NiN2/', (256, 128)), ('classifier/output_dense/', (128, ncls))]
        for q, shape in layers:
            c += [(q + 'V', shape, True, 'n05'), (q + 'b', (shape[-1],), True, 0.),
                  (q + 'meanOnlyBatchNormalization/pop_mean', (shape[-1],), False, 0.), (q + 'g', (shape[-1],), True, 1.)]
        return {'good_generator': g, 'discriminator': d, 'classifier': c}

    def _bucket_mark(self, net, first_variable):
        """a gradient-bucket boundary in front of the layer that owns `first_variable` (GRAD_BUCKETS)."""
        if first_variable in self.GRAD_BUCKETS.get(net, ()):
            ctx().grad_bucket_boundary(net)

    # ------------------------------------------------------------------ activations
    def leakyReLu(self, x, alpha=0.2, name=None):
        """relu(x) - alpha*relu(-x) (:19-27).  Called on a tensor it is one elementwise launch; passed as `nonlinearity=` /
        `activation=` (what the networks below do) it is fused into the producing kernel's epilogue with the default slope."""
        return self._leakyReLu_impl(x, alpha)
    leakyReLu.tg_act = ('lrelu', 0.2)

    def _leakyReLu_impl(self, x, alpha):
        return ops.activation(x, 'lrelu', alpha)

    def gaussian_noise_layer(self, input_layer, std):
        """input_layer + N(0, std) (:29-31)."""
        return self._add_noise(input_layer, stddev=std)

    # ------------------------------------------------------------------ networks
    def good_generator(self, z, y, init=False, reuse=False):
        """:33-58.  z: Act [N,Z_DIM]; y: Act [N,NUM_CLASSES] one-hot.  Returns Act [N,32,32,3]."""
        cx = ctx()
        with cx.variable_scope('good_generator'):
            zy = ops.cond_concat(z, y.t, y.c)                                        # tf.concat([z, y], 1)
            h0 = self._linear_fc(zy, 4 * 4 * 512, 'gg_h0_lin', activation=self._relu)   # dense + relu (gg_rl0)
            h0 = ops.reshape(self._batch_norm_contrib(_dense_view(h0), 'gg_bn0', train=True), z.n, 4, 4, 512)
            h = h0
            for i, (name, cout) in enumerate(self.G_DECONVS):                        # [8,8], [16,16], [32,32]
                self._bucket_mark('good_generator', 'good_generator/%s/%s/kernel' % (name, name))
                h = self._conv_cond_concat(h, y)
                if i + 1 < len(self.G_DECONVS):
                    h = self._deconv2d(h, cout, k_w=5, k_h=5, d_w=2, d_h=2, name=name, activation=self._relu)
                    h = self._batch_norm_contrib(h, 'gg_bn%d' % (i + 1), train=True)
                else:
                    h = self._deconv2d(h, cout, k_w=5, k_h=5, d_w=2, d_h=2, name=name, activation=self._tanh, narrow=True)
            h2 = h
        return h2

    def good_sampler(self, z, y):
        """:176-202 — the same graph as good_generator with reuse=True (BN stays in training mode)."""
        return self.good_generator(z, y, reuse=True)

    def discriminator(self, image, y, init=False, reuse=False, getter=None, want_prob=True):
        """:60-99.  image: Act [N,32,32,3]; y: Act [N,10].  Returns (tf.nn.sigmoid(h3), h3) = (Act [N,1], logits Act [N,1]).
        Dropout 0.2 is ALWAYS active (training=True literal, :63,73,83).  want_prob=False (extension; the trainer's solver runs, which
        fetch only the losses): the sigmoid launch is skipped and None returned in its place."""
        cx = ctx()
        lre = self.leakyReLu
        with cx.variable_scope('discriminator'):
            image = self._drop_out(image, 0.2, True, fuse_next=True)
            h2 = image
            for i, (name, cout, stride, drop) in enumerate(self.D_CONVS):
                self._bucket_mark('discriminator', 'discriminator/%s/%s/kernel' % (name, name))
                # a layer whose output goes straight into the next _conv_cond_concat (no dropout in between) writes that concatenation itself
                cat = y if (not drop and i + 1 < len(self.D_CONVS)) else None
                h2 = self._conv2d(self._conv_cond_concat(h2, y), cout, k_h=3, k_w=3, d_h=stride, d_w=stride, name=name, activation=lre,
                                  then_concat=cat)
                if drop:
                    h2 = self._drop_out(_dense_view(h2), 0.2, True, fuse_next=True)
            assert h2.pending is None, "a dropout behind the last convolution has no concat to fuse into"
            h3 = ops.global_avgpool_concat(h2, y.t, y.c)                             # avg_pool 8 + squeeze + concat y
            h3 = self._linear_fc(h3, 1, 'lin', narrow=True)
        return self._d_out(h3, want_prob)

    def discriminator_gradient_penalty(self, real, fake, y, weight=1.0, in_step=False):
        """weight * gp and weight * d gp / d theta_D of the WGAN-GP gradient penalty on this discriminator: tg/grad_penalty.py (contract,
        the four sweeps, in_step) over D_CONVS and the dense head.  real, fake: Act [N,H,W,3]; y: label Act [N,NUM_CLASSES]."""
        return grad_penalty.penalty(self, *self._gp, grad_penalty.Wgan(fake, weight), real, y, in_step)

    def discriminator_r1_penalty(self, real, y, gamma, in_step=False):
        """gamma / 2 * mean_i ||d logit_i / d x_i||^2 at the real rows `real` with their own labels y, and its gradient laid out like the
        discriminator's ParamStore.g (R1): the same sweeps, tg/grad_penalty.py.  gamma: a number or a 1-element device
        tensor."""
        return grad_penalty.penalty(self, *self._gp, grad_penalty.R1(gamma), real, y, in_step)

    def classifier(self, inp, is_training, init=False, reuse=False, getter=None, segments=None):
        """:101-174.  inp: Act [N,32,32,3] (ZCA-whitened).  Returns (logits Act [N,10], feature Act [N,128]).
        The Gaussian input noise is always on (also at evaluation, :104); dropout only when training.
        getter: the reference's custom_getter hook (:101-102; it never passes one).  Any truthy value selects the averaged weights: every
        trainable variable reads as its EMA shadow, pop_mean as it is (Context.reading_shadows) — forward only, outside the step."""
        cx = ctx()
        if getter:
            with cx.reading_shadows('classifier'):
                return self.classifier(inp, is_training, init=init, reuse=reuse, getter=None, segments=segments)
        kw = dict(init=init, use_weight_normalization=True, use_batch_normalization=False,
                  use_mean_only_batch_normalization=True, deterministic=not is_training, nonlinearity=self.leakyReLu,
                  segments=segments)
        with cx.variable_scope('classifier'):
            # x = self._add_noise(x, stddev=0.15) followed by conv1_1 (:104-110): with 3 input channels the 3x3 window is
            # gathered once (x + noise -> [N,32,32,27]) and conv1_1 runs as a 1x1 product on it with the same variable V
            # ([3,3,3,128] and [1,1,27,128] are the same bytes)
            # (the data-dependent initialisation pass draws nothing: Context.assigning_init)
            noise = None if cx.assign_init else cx.rng.normal(cx, 'noise', inp.rows * inp.c, 0.15)
            x = ops.im2col3x3_add(inp, noise)
            for i, (name, cout, pad, pool) in enumerate(self.C_CONVS):
                self._bucket_mark('classifier', 'classifier/%s/V' % name)
                then_pool = None
                if pool:                                                             # max_pool_k + dropout_k (:123-124,142-143): in the layer's apply launch
                    mask = None
                    if is_training:
                        mask = cx.rng.keep_mask(cx, 'drop' + name[4], x.rows // 4 * cout, 0.5)
                    then_pool = (mask, 2.0)
                x = nn.conv2d_WN(x, num_filters=cout, name=name, pad=pad, filter_size=[1, 1] if i == 0 else [3, 3], then_pool=then_pool, **kw)
            x = nn.NiN_WN(x, num_units=256, name='NiN1', **kw)
            x = nn.NiN_WN(x, num_units=128, name='NiN2', **kw)
            x = ops.global_maxpool(x)                                                # tf.layers.max_pooling2d(pool 6) named avg_pool_0
            intermediate_layer = x
            kw['nonlinearity'] = None
            logits = nn.dense_WN(x, num_units=self.config.NUM_CLASSES, name='output_dense', **kw)
        return logits, intermediate_layer

    # ------------------------------------------------------------------ data-dependent initialisation
    @property
    def WN_INIT_LAYERS(self):
        """{network: scopes of its weight-normalised layers, in the order the pass initialises them}."""
        return {'good_generator': (), 'discriminator': (),
                'classifier': tuple('classifier/' + row[0] for row in self.C_CONVS) + ('classifier/NiN1/NiN1', 'classifier/NiN2/NiN2',
                                                                                     'classifier/output_dense')}

    def data_dependent_init(self, z_g, y_g, x_l_d, y_l_d, x_u_d, x_u_c):
        """The reference's `init=True` builds (:216,227,263) with their assigns run: one forward pass per network, layer by
        layer, each weight-normalised layer setting g <- init_scale / sqrt(var + eps), b <- -mean * g from its unit-gain pre-activation and
        handing its initialised output on.  Here only the classifier has such layers (on x_u_c, ZCA-whitened where the model whitens:
        :222,227); the generator and the discriminator are skipped.  Input noise and dropout are off: the pass is a function of the variables and the batch, and only
        */g and */b change.  Returns {network: [scopes of the layers initialised]}."""
        cx = ctx()
        with cx.assigning_init() as done:
            with cx.rng_scoped('init/C'):
                self.classifier(x_u_c if self.zca() is None else self.zca().apply(x_u_c), False, init=True)
        return self._by_network(done)

    # ------------------------------------------------------------------ whole graph (evaluation / tests)
    CONSISTENCY = True        # forward_pass returns C_unl_logits_rep and _loss_GAN adds lambda_2 * MSE (:232-235, train_base.py:118)

    def zca(self):
        if self._zca is None:
            self._zca = zca.cifar10_ZCA(self.config)
        return self._zca


def _dense_view(a):
    """an Act whose channel stride equals its channel count (true for every multiple-of-32 layer here)."""
    assert a.ld == a.c, "layer width must be a multiple of 32 here"
    return a

