"""NN_Base — MI355X-native counterpart of the reference's Model/modle_base.py (sic; the reference's
models import it as `model_base`, Model/Good_GAN.py:8 — both spellings are provided here).

Method names and arguments follow Model/modle_base.py:27-48 (_linear_fc), :157-168 (_conv2d),
:190-202 (_drop_out, _add_noise), :229-237 (_batch_norm_contrib), :239-244 (_conv_cond_concat),
:246-259 (_deconv2d).  Tensors are tg.runtime.Act handles; variables are looked up in the active
Context under the names TF would create ('<scope>/<name>/<name>/kernel' for tf.layers.* called
inside `with tf.variable_scope(name)` with `name=name`).

Extensions (keyword-only, default = reference behaviour): `activation` fuses the nonlinearity the
model applies next into the MFMA kernel's epilogue; `narrow` stores only the logical channels.
Initialisers are applied when the Model creates its variables (NN_Base._create_variables over the model's
param_specs), so `kernel_initializer` is accepted and ignored here.

NN_Base also carries what the models of this package share above the layers: variable creation, the whole-graph
forward_pass (steered by the model's CONSISTENCY, as_image and zca()), the discriminator's no-gradient sigmoid output and the
arg-max one-hot labels.

`init=True` of the _WN_* layers is the reference's live tf.assign branch (modle_base.py:68-71,103-106,150-153): g and b are assigned
from the moments of the unit-gain pre-activation (eps 1e-10, init_scale honoured) and the layer's value is computed through them
(NN_Base._wn_init).  The fused layouts (narrow, then_concat) serve init=False; the init runs through the plain one.
"""
import numpy as np

from tg import ops
from tg.runtime import Act, ParamStore, ctx


def _act_of(fn):
    if fn is None:
        return None, 0.2
    a = getattr(fn, 'tg_act', None)
    if a is None:
        raise ValueError("activation must be a tg activation (leakyReLu, tf-like relu/tanh helpers)")
    return a


def _cat_of(then_concat):
    """(label tensor, number of label channels) of a `then_concat=` argument: a label Act, such a tuple, or None."""
    if then_concat is None or isinstance(then_concat, tuple):
        return then_concat
    return (then_concat.t, then_concat.c)


def _trunc_normal(rng, shape):
    """tf.truncated_normal: standard normal draws (float64), those beyond two standard deviations drawn again."""
    x = rng.standard_normal(shape)
    bad = np.abs(x) > 2
    while bad.any():
        x[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(x) > 2
    return x


def _fan_in(shape):
    return shape[-2] * int(np.prod(shape[:-2])) if len(shape) > 2 else shape[0]


def _xavier_uniform(rng, shape):
    """tf.contrib.layers.xavier_initializer(): uniform, fan_avg."""
    lim = np.sqrt(6.0 / (shape[0] + shape[1]))
    return rng.uniform(-lim, lim, shape)


# initialiser name of a param_specs() row -> float64 draw(rng, shape); a row may also carry a float, the constant the variable starts at
INITIALISERS = {
    # tf.random_normal_initializer(0.02) / tf.truncated_normal_initializer(0.02): the MEAN is 0.02, stddev 1.0 (modle_base.py:28,159,248)
    'n02': lambda rng, shape: 0.02 + rng.standard_normal(shape),
    'tn02': lambda rng, shape: 0.02 + _trunc_normal(rng, shape),
    'n05': lambda rng, shape: 0.05 * rng.standard_normal(shape),                                        # nn.py:478
    'xavier': _xavier_uniform,
    # variance_scaling_initializer(): factor 2, FAN_IN, truncated normal, std sqrt(1.3*2/fan_in) (Good_GAN_cifar10.py:8-9)
    'he': lambda rng, shape: _trunc_normal(rng, shape) * np.sqrt(1.3 * 2.0 / _fan_in(shape)),
}


class NN_Base(object):
    CONSISTENCY = False        # True: forward_pass applies C to x_u_c a second time and returns C_unl_logits_rep (Good_GAN_cifar10.py:232-235)
    GRAD_BUCKETS = {}          # {network: first variable of every data-parallel gradient bucket after the first} (Good_GAN_cifar10)

    def __init__(self, batch_norm_decay=0.9, batch_norm_epsilon=1e-5):
        self._batch_norm_decay = batch_norm_decay
        self._batch_norm_epsilon = batch_norm_epsilon

    def _create_variables(self, seed, specs):
        """the three networks' variables — specs: the model's param_specs(), {network: [(name, shape, trainable, init)]} in TF creation
        order — each in a ParamStore of the active Context, initialised from ONE np.random.default_rng(seed) network after network and
        row after row (INITIALISERS, in float64, rounded to float32 once).  A store that exists already is left alone (reuse=True) and
        draws nothing.  The classifier gets its EMA shadows (Train_goodGAN.py:101-103)."""
        cx = ctx()
        rng = np.random.default_rng(seed)
        for net in ('good_generator', 'discriminator', 'classifier'):
            if net in cx.stores:
                continue
            st = ParamStore(net, [(n, s, t) for n, s, t, _ in specs[net]], cx.device)
            for name, shape, _, init in specs[net]:
                st.set(name, INITIALISERS[init](rng, shape) if isinstance(init, str) else np.full(shape, init, np.float32))
            cx.stores[net] = st
        cx.stores['classifier'].enable_ema()

    def as_image(self, a):
        """the per-image layout in which batches of this model's images are concatenated."""
        return a

    def zca(self):
        """the whitening in front of the classifier (Model/zca.py), or None: the classifier sees the images as they are."""
        return None

    def _d_out(self, logits, want_prob=True):
        """the discriminator's return value (tf.nn.sigmoid(logits), logits) (Good_GAN.py:124,206, Good_GAN_cifar10.py:99).  The sigmoid is an
        output only: no loss of the reference differentiates through it (they all take the logits), so it is not recorded — and with
        want_prob=False (the trainer's solver runs, which fetch only the losses) not launched: None in its place."""
        if not want_prob:
            return None, logits
        with ctx().no_record():
            return ops.activation(logits, 'sigmoid'), logits

    @staticmethod
    def _by_network(scopes):
        """data_dependent_init's return value: {network: [those of `scopes` that lie in it]}."""
        return {net: [s for s in scopes if s.startswith(net + '/')] for net in ('good_generator', 'classifier', 'discriminator')}

    def _onehot_act(self, logits):
        """one_hot(argmax(logits)) as a label Act [n, NUM_CLASSES]."""
        k = self.config.NUM_CLASSES
        return Act(ops.argmax_onehot(logits, k), logits.n, 1, 1, k, k)

    def forward_pass(self, z_g, y_g, x_l_c, y_l_c, x_l_d, y_l_d, x_u_d, x_u_c, train):
        """Good_GAN.py:428-472 / Good_GAN_cifar10.py:204-278.  Executes every application eagerly (the trainer runs per-solver sub-graphs
        instead, Training/Train_goodGAN.py).  Returns [G, [D_real, D_real_logits, D_fake, D_fake_logits, D_unl, D_unl_logits],
        [C_real_logits, C_unl_logits, C_unl_d_logits, C_fake_logits]] as Act handles, with CONSISTENCY C_unl_logits_rep behind them.  The
        three discriminator applications run as one batched call (no batch statistics in D: identical arithmetic), the classifier ones as
        one call with per-application statistics and running-statistics updates in the reference's call-site order (real, unl, unl_rep
        with CONSISTENCY, unl_d, fake: Good_GAN_cifar10.py:228-240), each part whitened on its own where the model has a zca()."""
        from tg.batching import concat_acts
        cx = ctx()
        G = self.good_generator(z_g, y_g)
        w = self.zca()
        parts = [self.as_image(a) for a in [x_l_c, x_u_c] + ([x_u_c] if self.CONSISTENCY else []) + [x_u_d, G]]
        segs = [p.n for p in parts]
        if w is not None:
            parts = [w.apply(p) for p in parts]
        with cx.rng_scoped(cx.phase + '/C'):
            logits, _ = self.classifier(concat_acts(parts), train, segments=segs)
        offs = [int(v) for v in np.cumsum([0] + segs)]
        C = [logits.view_rows(offs[i], offs[i + 1]) for i in range(len(segs))]
        C_rep = [C.pop(2)] if self.CONSISTENCY else []
        C_real, C_unl, C_unl_d, C_fake = C
        oh_d = self._onehot_act(C_unl_d)
        oh_u = self._onehot_act(C_unl)
        ximg = concat_acts([self.as_image(a) for a in (x_l_d, x_u_d, G, x_u_c)])
        yall = concat_acts([y_l_d, oh_d, y_g, oh_u])
        with cx.rng_scoped(cx.phase + '/D'):
            dp, dl = self.discriminator(ximg, yall)
        n_p = x_l_d.n + x_u_d.n
        cut = lambda a: [a.view_rows(0, n_p), a.view_rows(n_p, n_p + G.n), a.view_rows(n_p + G.n, a.n)]
        (p_real, p_fake, p_unl), (l_real, l_fake, l_unl) = cut(dp), cut(dl)
        return [G, [p_real, l_real, p_fake, l_fake, p_unl, l_unl], C + C_rep]

    # ---- activations: callable on a tensor (one elementwise launch, modle_base.py:170-188) AND usable as `activation=` /
    # `nonlinearity=` of a layer, which fuses them into the producing kernel's epilogue (what the models of this package do)
    def _relu(self, x):
        return ops.activation(x, 'relu')
    _relu.tg_act = ('relu', 0.0)

    def _tanh(self, x):
        return ops.activation(x, 'tanh')
    _tanh.tg_act = ('tanh', 0.0)

    def _leaky_relu(self, x, alpha=0.2):
        """tf.nn.leaky_relu (modle_base.py:181-182); as `activation=` the slope is the default 0.2."""
        return ops.activation(x, 'lrelu', alpha)
    _leaky_relu.tg_act = ('lrelu', 0.2)

    def _softplus(self, x):
        return ops.activation(x, 'softplus')
    _softplus.tg_act = ('softplus', 0.0)

    def _sigmoid(self, x):
        return ops.activation(x, 'sigmoid')
    _sigmoid.tg_act = ('sigmoid', 0.0)

    # ---- layers -----------------------------------------------------------------------------------
    def _linear_fc(self, input_, output_size, scope=None, bias_start=0.0, use_bias=True, kernel_initializer=None,
                   activation=None, narrow=False):
        """tf.layers.dense + bias (Model/modle_base.py:27-48); runs as a 1-tap MFMA implicit GEMM."""
        cx = ctx()
        act, alpha = _act_of(activation)
        with cx.variable_scope(scope), cx.variable_scope(scope):
            tr = cx.trains()
            return ops.conv2d(input_, cx.var('kernel'), cx.var('bias') if use_bias else None, output_size, 1, 1, 'SAME',
                              act=act, alpha=alpha, kernel_grad=cx.var_grad('kernel') if tr else None,
                              bias_grad=cx.var_grad('bias') if (tr and use_bias) else None,
                              n_store_ld=(output_size, output_size) if narrow else None)

    def _conv2d(self, input_, output_dim, k_h=5, k_w=5, d_h=2, d_w=2, kernel_initializer=None, name="conv2d",
                activation=None, bn_segments=None, then_concat=None):
        """tf.layers.conv2d 'same' + bias (Model/modle_base.py:157-168).  bn_segments (extension): a training-mode _batch_norm_contrib over
        these application segments follows directly — its statistics pass is taken in this layer's launch (ops.conv2d(bn_stats=True)).
        then_concat (extension): the label Act a _conv_cond_concat right behind this layer will append — the launch writes the concatenated
        tensor itself (ops.conv2d(concat=...)) and that _conv_cond_concat becomes a view."""
        assert k_h == k_w and d_h == d_w
        cx = ctx()
        act, alpha = _act_of(activation)
        with cx.variable_scope(name), cx.variable_scope(name):
            tr = cx.trains()
            return ops.conv2d(input_, cx.var('kernel'), cx.var('bias'), output_dim, k_h, d_h, 'SAME', act=act, alpha=alpha,
                              kernel_grad=cx.var_grad('kernel') if tr else None, bias_grad=cx.var_grad('bias') if tr else None,
                              segments=bn_segments if bn_segments else None, bn_stats=bn_segments is not None,
                              concat=_cat_of(then_concat))

    def _deconv2d(self, input_, output_shape, k_h=5, k_w=5, d_h=2, d_w=2, name="deconv2d", use_bias=True,
                  kernel_initializer=None, activation=None, narrow=False):
        """tf.layers.conv2d_transpose 'same' + bias (Model/modle_base.py:246-259); output_shape = channels."""
        assert (k_h, k_w, d_h, d_w) == (5, 5, 2, 2) and use_bias
        cx = ctx()
        act, _ = _act_of(activation)
        with cx.variable_scope(name), cx.variable_scope(name):
            tr = cx.trains()
            return ops.deconv2d(input_, cx.var('kernel'), cx.var('bias'), output_shape, act=act,
                                kernel_grad=cx.var_grad('kernel') if tr else None, bias_grad=cx.var_grad('bias') if tr else None,
                                narrow_out=narrow)

    def _batch_norm_contrib(self, x, name, train=False, segments=None, bf16_out=False):
        """tf.contrib.layers.batch_norm(decay, eps, scale=True, updates_collections=None) (modle_base.py:229-237).
        train=True: batch statistics, moving statistics updated in place; train=False: moving statistics.
        segments (extension): image counts of the applications batched into x — statistics per application.
        bf16_out (extension): the output's only reader is a bf16-operand 3x3 convolution — in training it is stored as bf16 when
        config.ACT_DTYPE = 'bf16' (ops.batch_norm_train(out_bf16=True)); evaluation stays fp32."""
        cx = ctx()
        with cx.variable_scope(name):
            if train and cx.assign_init:
                # the data-dependent initialisation pass: batch statistics, moving statistics left as they are (Context.assigning_init)
                return ops.batch_norm_train(x, cx.var('gamma'), cx.var('beta'), None, None, self._batch_norm_epsilon, self._batch_norm_decay,
                                            segments=segments)
            if not train:
                return ops.batch_norm_eval(x, cx.var('gamma'), cx.var('beta'), cx.var('moving_mean'), cx.var('moving_variance'),
                                           self._batch_norm_epsilon)
            tr = cx.trains()
            return ops.batch_norm_train(x, cx.var('gamma'), cx.var('beta'), cx.var('moving_mean'), cx.var('moving_variance'),
                                        self._batch_norm_epsilon, self._batch_norm_decay,
                                        gamma_grad=cx.var_grad('gamma') if tr else None, beta_grad=cx.var_grad('beta') if tr else None,
                                        segments=segments, out_bf16=bf16_out)

    def _wn_init(self, t, init_scale, act, alpha, narrow):
        """init=True of a _WN_* layer, inside its variable scope: g <- init_scale / sqrt(var(t) + 1e-10), b <- -mean(t) * g assigned from the
        unit-gain pre-activation t, act(g*t + b) returned (ops.wn_data_init) — in the plain channel-padded layout, or, narrow, copied to
        the dense one the layer's caller expects.  A then_concat behind the layer is left to the cond_concat that follows."""
        cx = ctx()
        y = ops.wn_data_init(t, cx.var('g'), cx.var('b'), 1e-10, init_scale, act, alpha)
        if cx.assign_init:
            cx.wn_inited.append(cx.scope_name())
        if narrow and y.ld != y.c:
            out = cx.new_act(y.n, y.h, y.w, y.c, y.c)
            ops.copy2d(out.t, y.c, 0, y.t, y.ld, y.rows, y.c)
            return out
        return y

    def _ones(self, n):
        cx = ctx()
        ones = cx.ws('const:ones', max(n, 1024))
        ops.fill(ones, 1.0)
        return ones

    def _WN_dense(self, input_, output_size, scope, init_scale=1.0, init=False, activation=None, narrow=False):
        """g * (x @ l2_normalize(V,[0])) + b (modle_base.py:50-73); init=True assigns g and b first (:68-71, _wn_init)."""
        cx = ctx()
        act, alpha = _act_of(activation)
        with cx.variable_scope(scope):
            if init:
                with cx.no_record():
                    t = ops.conv2d(input_, cx.var('V'), None, output_size, 1, 1, 'SAME', wn=(self._ones(output_size), None))
                    return self._wn_init(t, init_scale, act, alpha, narrow)
            tr = cx.trains()
            return ops.conv2d(input_, cx.var('V'), cx.var('b'), output_size, 1, 1, 'SAME', act=act, alpha=alpha,
                              wn=(cx.var('g'), cx.var_grad('g') if tr else None), kernel_grad=cx.var_grad('V') if tr else None,
                              bias_grad=cx.var_grad('b') if tr else None, n_store_ld=(output_size, output_size) if narrow else None)

    def _WN_conv2d(self, input_, output_dim, k_h=5, k_w=5, d_h=2, d_w=2, padding='SAME', init_scale=1.0, init=False, name="conv2d",
                   activation=None, then_concat=None):
        """g * conv(x, l2_normalize(V,[0,1,2])) + b (modle_base.py:75-108); init=True assigns g and b first (:103-106, _wn_init).  then_concat
        (extension): as in _conv2d — (label tensor, count) or a label Act the _conv_cond_concat / cond_concat right behind this layer appends."""
        assert k_h == k_w and d_h == d_w
        cx = ctx()
        act, alpha = _act_of(activation)
        with cx.variable_scope(name):
            if init:
                with cx.no_record():
                    t = ops.conv2d(input_, cx.var('V'), None, int(output_dim), k_h, d_h, padding, wn=(self._ones(int(output_dim)), None))
                    return self._wn_init(t, init_scale, act, alpha, False)
            tr = cx.trains()
            return ops.conv2d(input_, cx.var('V'), cx.var('b'), int(output_dim), k_h, d_h, padding, act=act, alpha=alpha,
                              wn=(cx.var('g'), cx.var_grad('g') if tr else None), kernel_grad=cx.var_grad('V') if tr else None,
                              bias_grad=cx.var_grad('b') if tr else None, concat=_cat_of(then_concat))

    def _WN_deconv2d(self, input_, output_dim, k_h=3, k_w=3, d_h=2, d_w=2, padding='SAME', init_scale=1.0, init=False, name="deconv2d",
                     activation=None, narrow=False):
        """g * conv2d_transpose(x, l2_normalize(V,[0,1,3])) + b, V [kh,kw,Cout,Cin] (modle_base.py:130-155); 5x5 s2 'SAME' only
        (the only configuration the reference's models use); init=True assigns g and b first (:150-153, _wn_init)."""
        assert (k_h, k_w, d_h, d_w, padding) == (5, 5, 2, 2, 'SAME')
        cx = ctx()
        act, alpha = _act_of(activation)
        with cx.variable_scope(name):
            if init:
                with cx.no_record():
                    t = ops.deconv2d(input_, cx.var('V'), None, int(output_dim), wn=(self._ones(int(output_dim)), None))
                    return self._wn_init(t, init_scale, act, alpha, narrow)
            tr = cx.trains()
            return ops.deconv2d(input_, cx.var('V'), cx.var('b'), int(output_dim), act=act, kernel_grad=cx.var_grad('V') if tr else None,
                                bias_grad=cx.var_grad('b') if tr else None, narrow_out=narrow,
                                wn=(cx.var('g'), cx.var_grad('g') if tr else None))

    def _minibatch_discrimination(self, input, num_kernels, dim_per_kernel=5, name="minibatch_discrim", concat_input=False):
        """modle_base.py:110-128: variables `w` [features, num_kernels*dim_per_kernel] (Xavier) and `b` [num_kernels] of the enclosing
        variable scope (tf.name_scope does not prefix tf.get_variable).  concat_input (extension): return concat([input, f], 1), the
        only use the reference makes of the result (Good_GAN.py:160-161), from the same launch."""
        cx = ctx()
        tr = cx.trains()
        return ops.minibatch_discrimination(input, cx.var('w'), cx.var('b'), num_kernels, dim_per_kernel,
                                            w_grad=cx.var_grad('w') if tr else None, b_grad=cx.var_grad('b') if tr else None,
                                            concat_input=concat_input)

    def _nin(self, input, num_units, name, activation=None, init=False):
        """network-in-network (1x1 conv): reshape + _WN_dense + reshape (modle_base.py:204-209)."""
        return self._WN_dense(input, num_units, name, init=init, activation=activation)

    def _conv_cond_concat(self, x, y):
        """Concatenate conditioning vector on feature map axis (modle_base.py:239-244); y: Act [N,ncls]."""
        return ops.cond_concat(x, y.t, y.c)

    def _drop_out(self, x, rate=0.5, train=False, name=None, fuse_next=False):
        """tf.layers.dropout (modle_base.py:190-191): x*mask/keep with a floor(keep+U) keep-mask.  fuse_next (extension): the
        result goes straight into _conv_cond_concat, which applies the mask in its own launch (ops.scale_mask(defer=True))."""
        cx = ctx()
        if not train or cx.assign_init:                  # the data-dependent initialisation pass draws nothing (Context.assigning_init)
            return x
        mask = cx.rng.keep_mask(cx, name or cx.next_rng_name('drop'), x.rows * x.c, 1.0 - rate)
        assert x.ld == x.c
        return ops.scale_mask(x, mask, 1.0 / (1.0 - rate), defer=fuse_next)

    def _add_noise(self, inputs, mean=0.0, stddev=0.001, name=None):
        """inputs + N(mean, stddev) (modle_base.py:193-202) on a dense activation; the gradient passes through."""
        assert mean == 0.0
        cx = ctx()
        if cx.assign_init:                               # see _drop_out
            return inputs
        noise = cx.rng.normal(cx, name or cx.next_rng_name('noise'), inputs.rows * inputs.c, stddev)
        return ops.add_noise(inputs, noise)
