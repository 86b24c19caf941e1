"""Train_base — loss / optimiser library, counterpart of the reference's Training/train_base.py.

`_loss_GAN(D, C, Y, Lambda)` (train_base.py:113-154) is the loss the entry point calls by default (config.LOSS = 'WGAN_GP' selects the
WGAN-GP heads further down instead); it is evaluated by three fused
single-launch kernels (tg_d_loss_f32 / tg_g_loss_f32 / tg_c_loss_k_f32) that also write d(loss)/d(logits) into the
logits' gradient buffers.  The helper methods it is written with in the reference — `_entropy`, `_balance_entropy` (:43-57),
`_softmax_cross_entropy_loss_w_logits`, `_sigmoid_cross_entopy_w_logits` (:75-84), `_accuracy_metric` (:107) — keep their names and
argument order as stand-alone single-launch heads.  `_Adam_optimizer` (:91-97) returns the TF-form Adam configuration applied by
tg_adam_f32 over a network's flat buffers; `_SGD_w_Momentum_optimizer` (:86-89) and `_RMSProp_optimizer` (:99-105) return the other two
(tg_momentum_f32, tg_rmsprop_f32; config.OPTIMIZER); `_train_op` applies whichever it is handed, and `_train_op_w_grads`
(:70-73) applies it and hands back the gradients — with `clip`, clipped by their global norm first (tg_grad_norm_clip_f32 and the
tg_*_clip_f32 optimisers; config.CLIP_NORM).

Eager-mode conventions: a loss value is a 1-element DEVICE tensor (float(t) synchronises); every head also leaves d(value)/d(logits)
in `logits.grad` — written when the tensor has no gradient yet, ADDED when it has, so a loss summed from several heads accumulates
its gradient the way TensorFlow's autodiff would; `weight` scales value and gradient.
"""
import ctypes as C_

import torch

from tg import lib
from tg.batching import concat_acts
from tg.runtime import ctx


def _launch_update(name, clip_name, args, factor_dev):
    """launch optimiser kernel `name` on `args`, or its twin `clip_name` with the DEVICE scalar `factor_dev` added."""
    if factor_dev is None:
        lib.call(name, *args, ctx().stream)
    else:
        lib.call(clip_name, *args, lib.ptr(factor_dev), ctx().stream)


def _c_terms_head(members, n_real, n_unl, n_rep, n_fake, y_real, y_fake, d_unl, w6, loss_ptr, terms_ptr):
    """tg_c_loss_terms_k_f32 over the concatenated `members` (rows [real | unl | unl_rep | fake], any of the last two absent) with the
    HOST weights w6; y_fake / d_unl may be None.  Every member's `.grad` becomes its row range of the concatenated gradient.  Returns
    the concatenated logits."""
    cx = ctx()
    ccat = concat_acts(members)
    g = cx.new_act(ccat.n, 1, 1, ccat.c, ccat.ld, tag='dl')
    lib.call('tg_c_loss_terms_k_f32', ccat.ptr, ccat.ld, n_real, n_unl, n_rep, n_fake, ccat.c, y_real.ptr,
             y_fake.ptr if y_fake is not None else None, d_unl.ptr if d_unl is not None else None, d_unl.ld if d_unl is not None else 0,
             (C_.c_float * 6)(*w6), g.ptr, g.ld, loss_ptr, terms_ptr, cx.stream)
    ccat.grad = g
    off = 0
    for m in members:                                                  # the members' gradients are row ranges of the concatenated one
        m.grad = g.view_rows(off, off + m.n)
        off += m.n
    return ccat


class StreamingAccuracy(object):
    """tf.metrics.accuracy (train_base.py:107): device counters {correct, total}; float(metric) = the accuracy so far."""

    def __init__(self, num_classes=10):
        self.k = num_classes
        self.counters = torch.zeros(2, dtype=torch.float32, device=ctx().device)

    def update(self, labels, logits):
        """labels: one-hot Act [n,k]; logits: Act [n,k] — arg-max of both is taken in the kernel."""
        lib.call('tg_accuracy_count_f32', logits.ptr, logits.ld, labels.ptr, logits.n, self.k, lib.ptr(self.counters), ctx().stream)
        return self

    def reset(self):
        lib.call('tg_fill_f32', lib.ptr(self.counters), 0.0, 2, ctx().stream)
        return self

    def result(self):
        correct, total = self.counters.cpu().numpy()
        return float(correct) / max(float(total), 1.0)

    __float__ = result


class AdamOptimizer(object):
    """tf.train.AdamOptimizer(learning_rate, beta1, beta2=0.999, epsilon=1e-8); lr is a DEVICE scalar."""
    kind = 'adam'

    def __init__(self, lr_dev, beta1, beta2=0.999, epsilon=1e-8, name='Adam_optimizer'):
        self.lr_dev, self.beta1, self.beta2, self.epsilon, self.name = lr_dev, beta1, beta2, epsilon, name

    def bind(self, store):
        """`store` is trained by this optimiser from here on: both slots start at zero (a fresh store's already do and are left alone)."""
        store.optimizer = self.kind
        for which, v in store.slot_init.items():
            if v != 0.0:
                store.init_slot(which, 0.0)

    def apply(self, store, grad_scale=1.0, factor_dev=None):
        """factor_dev: DEVICE scalar the scaled gradient is multiplied by (the clip factor of tg_grad_norm_clip_f32); None = unclipped."""
        args = (lib.ptr(store.p), lib.ptr(store.g), lib.ptr(store.m), lib.ptr(store.v), store.n_p,
                lib.ptr(self.lr_dev), self.beta1, self.beta2, self.epsilon, lib.ptr(store.step), grad_scale)
        _launch_update('tg_adam_f32', 'tg_adam_clip_f32', args, factor_dev)


class MomentumOptimizer(object):
    """tf.train.MomentumOptimizer(learning_rate, momentum), use_nesterov=False: accum = accum*momentum + g; p -= lr*accum [UNVERIFIED-TF].
    lr is a DEVICE scalar; store.m is the `momentum` slot (zeros), store.v is not touched; no step count."""
    kind = 'momentum'

    def __init__(self, lr_dev, momentum, name='Momentum'):
        self.lr_dev, self.momentum, self.name = lr_dev, momentum, name

    def bind(self, store):
        store.optimizer = self.kind
        store.init_slot('m', 0.0)

    def apply(self, store, grad_scale=1.0, factor_dev=None):
        args = (lib.ptr(store.p), lib.ptr(store.g), lib.ptr(store.m), store.n_p, lib.ptr(self.lr_dev), self.momentum, grad_scale)
        _launch_update('tg_momentum_f32', 'tg_momentum_clip_f32', args, factor_dev)


class RMSPropOptimizer(object):
    """tf.train.RMSPropOptimizer(learning_rate, decay=0.9, momentum=0.0, epsilon=1e-10, centered=False): ms += (g^2 - ms)(1 - decay);
    mom = mom*momentum + (g*lr)/sqrt(ms + epsilon); p -= mom [UNVERIFIED-TF].  lr is a DEVICE scalar; store.v is the `rms` slot, which
    starts at ONE (bind() sees to it wherever the store's buffers come to exist), store.m the `momentum` slot (zeros, kept even with
    momentum 0 as TensorFlow keeps it); no step count."""
    kind = 'rmsprop'

    def __init__(self, lr_dev, decay=0.9, momentum=0.0, epsilon=1e-10, name='RMSProp_optimizer'):
        self.lr_dev, self.decay, self.momentum, self.epsilon, self.name = lr_dev, decay, momentum, epsilon, name

    def bind(self, store):
        store.optimizer = self.kind
        store.init_slot('m', 0.0)
        store.init_slot('v', 1.0)

    def apply(self, store, grad_scale=1.0, factor_dev=None):
        args = (lib.ptr(store.p), lib.ptr(store.g), lib.ptr(store.v), lib.ptr(store.m), store.n_p, lib.ptr(self.lr_dev),
                self.decay, self.momentum, self.epsilon, grad_scale)
        _launch_update('tg_rmsprop_f32', 'tg_rmsprop_clip_f32', args, factor_dev)


class GradViews(object):
    """the `grads` of _train_op_w_grads: {variable name: that variable's slice of store.g}, sliced when asked for (an iteration that does
    not look at them pays nothing)."""

    def __init__(self, store):
        self.store = store

    def keys(self):
        return self.store.names(True)

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())

    def __contains__(self, nm):
        return nm in self.store.index and self.store.index[nm][0] == 'p'

    def __getitem__(self, nm):
        if nm not in self:
            raise KeyError(nm)
        return self.store.grad(nm)

    def items(self):
        return [(nm, self[nm]) for nm in self.keys()]

    def values(self):
        return [self[nm] for nm in self.keys()]


def clip_workspace_floats(store):
    """floats of tg_grad_norm_clip_f32's workspace for `store`, sized for everything the store has reserved: a store that grows within its
    reserve never regrows the workspace a recorded plan or graph holds."""
    return (lib.call('tg_grad_norm_workspace_bytes', max(store._full['g'].numel(), 1)) + 3) // 4


class Train_base(object):
    def __init__(self):
        pass

    def _input_fn(self):
        raise NotImplementedError('metirc() is implemented in Model sub classes')

    def _build_train_graph(self):
        raise NotImplementedError('loss() is implemented in Model sub classes')

    # ---- helper heads (train_base.py:43-57,75-84,107) -----------------------------------------------
    @staticmethod
    def _grad_of_logits(logits):
        """(gradient Act, accumulate flag) — see the module docstring."""
        cx = ctx()
        if logits.grad is None:
            logits.grad = cx.new_act(logits.n, logits.h, logits.w, logits.c, logits.ld, tag='dl')
            return logits.grad, 0
        return logits.grad, 1

    def _entropy(self, logits, weight=1.0):
        """mean_n(logsumexp(l) - sum_k softmax_k l_k) (train_base.py:43-48)."""
        cx = ctx()
        out = cx.scratch('lossv', 4)
        g, acc = self._grad_of_logits(logits)
        lib.call('tg_entropy_terms_f32', logits.ptr, logits.ld, logits.n, logits.c, float(weight), 0.0, g.ptr, g.ld, acc, lib.ptr(out), cx.stream)
        return out[0:1]

    def _balance_entropy(self, logits, weight=1.0):
        """-sum_k (1/K) log(mean_n softmax_k + 1e-12) (train_base.py:50-57)."""
        cx = ctx()
        out = cx.scratch('lossv', 4)
        g, acc = self._grad_of_logits(logits)
        lib.call('tg_entropy_terms_f32', logits.ptr, logits.ld, logits.n, logits.c, 0.0, float(weight), g.ptr, g.ld, acc, lib.ptr(out), cx.stream)
        return out[0:1]

    def _softmax_cross_entropy_loss_w_logits(self, labels, logits, weight=1.0):
        """reduce_mean(softmax_cross_entropy_with_logits_v2(labels, logits)) (train_base.py:75-79); labels: dense Act [n,k]."""
        cx = ctx()
        assert labels.ld == labels.c == logits.c and labels.n == logits.n
        out = cx.scratch('lossv', 4)
        g, acc = self._grad_of_logits(logits)
        lib.call('tg_softmax_ce_f32', logits.ptr, logits.ld, labels.ptr, logits.n, logits.c, float(weight), g.ptr, g.ld, acc, lib.ptr(out), cx.stream)
        return out[0:1]

    def _sigmoid_cross_entopy_w_logits(self, labels, logits, weight=1.0):
        """reduce_mean(sigmoid_cross_entropy_with_logits(labels, logits)) (train_base.py:81-84).  labels: an Act of the logits' shape, or a
        number standing for tf.ones_like(logits) / tf.zeros_like(logits) (:123-128)."""
        cx = ctx()
        out = cx.scratch('lossv', 4)
        g, acc = self._grad_of_logits(logits)
        const = not hasattr(labels, 'ptr')
        lib.call('tg_bce_logits_f32', logits.ptr, logits.ld, None if const else labels.ptr, 0 if const else labels.ld, float(labels) if const else 0.0,
                 logits.rows, logits.c, float(weight), g.ptr, g.ld, acc, lib.ptr(out), cx.stream)
        return out[0:1]

    def _accuracy_metric(self, labels, predictions, metric=None):
        """tf.metrics.accuracy(labels, predictions) (train_base.py:107) -> (accuracy, update_op): one update with this batch on `metric`
        (a new StreamingAccuracy when None); float(accuracy) reads the running value, update_op(labels, predictions) adds a batch.
        labels: one-hot Act; predictions: logits Act (the arg-max of Train._metric, Train_goodGAN.py:432-433, happens in the kernel)."""
        metric = metric if metric is not None else StreamingAccuracy(predictions.c)
        metric.update(labels, predictions)
        return metric, metric.update

    def _Adam_optimizer(self, lr, beta1, name='Adam_optimizer'):
        return AdamOptimizer(lr, beta1, name=name)

    def _SGD_w_Momentum_optimizer(self, lr, momentum):
        """train_base.py:86-89."""
        return MomentumOptimizer(lr, momentum)

    def _RMSProp_optimizer(self, lr, name='RMSProp_optimizer'):
        """train_base.py:99-105 (decay 0.9)."""
        return RMSPropOptimizer(lr, decay=0.9, name=name)

    def _train_op(self, optimizer, store, grad_scale=1.0):
        """optimizer.minimize(loss, var_list) (train_base.py:64-68): the gradients are already in store.g."""
        ctx().prep_invalidate(store)
        optimizer.apply(store, grad_scale)

    def _clip_state(self, store):
        """(threshold, {norm, factor}) device tensors of `store`'s network: the trainer's (Train._build_train_graph lays all three networks'
        out in one buffer), else a buffer of the context's under the network's name."""
        views = getattr(self, '_clip_views', {}).get(store.name)
        if views is not None:
            return views
        t = ctx().ws('clip:state:' + store.name, 4)
        return t[0:1], t[2:4]

    def _train_op_w_grads(self, optimizer, store, grad_scale=1.0, clip=None):
        """train_base.py:70-73: compute_gradients / apply_gradients -> grads ({variable name: gradient view}; the gradients are already in
        store.g).  clip: where a TF1 user writes tf.clip_by_global_norm(grads, clip) between the two — None applies the gradients as they
        are; a positive number, or a 1-element DEVICE tensor holding it (read at launch, so a replayed plan or graph follows it), clips
        the network's gradients by their global norm [UNVERIFIED-TF]: norm = grad_scale*sqrt(sum g^2), factor = clip*min(1/norm, 1/clip),
        g_used = (g*grad_scale)*factor.  {norm, factor} stay on the device (_clip_state(store)[1]); store.g is not written."""
        cx = ctx()
        cx.prep_invalidate(store)
        if clip is None:
            optimizer.apply(store, grad_scale)
            return GradViews(store)
        thr, out2 = self._clip_state(store)
        if isinstance(clip, torch.Tensor):
            thr = clip
        else:
            if not 0.0 < float(clip) < float('inf'):
                raise lib.TgError("_train_op_w_grads: clip must be a positive finite number or a device scalar, got %r" % (clip,))
            thr.fill_(float(clip))
        need = lib.call('tg_grad_norm_workspace_bytes', store.n_p)
        wsp = cx.ws('clip:ws:' + store.name, max(clip_workspace_floats(store), (need + 3) // 4))
        lib.call('tg_grad_norm_clip_f32', lib.ptr(store.g), store.n_p, grad_scale, lib.ptr(thr), lib.ptr(out2), lib.ptr(wsp), wsp.numel() * 4,
                 cx.stream)
        optimizer.apply(store, grad_scale, out2[1:2])
        return GradViews(store)

    # ---- _loss_GAN split by solver (each writes value + d/dlogits) --------------------------------
    def _d_loss(self, d_logits, n_real, n_fake, n_unl, loss_out):
        """d_loss = BCE(D_real,1) + .5 BCE(D_fake,0) + .5 BCE(D_unl,0) (train_base.py:123-126); rows [real|fake|unl]."""
        cx = ctx()
        g = cx.new_act(d_logits.n, 1, 1, 1, 32, tag='dl')
        lib.call('tg_d_loss_f32', d_logits.ptr, d_logits.ld, n_real, n_fake, n_unl, g.ptr, g.ld, lib.ptr(loss_out), cx.stream)
        d_logits.grad = g

    def _g_loss(self, d_fake_logits, loss_out):
        """g_loss = 1/2 BCE(D_fake,1) (train_base.py:128)."""
        cx = ctx()
        g = cx.new_act(d_fake_logits.n, 1, 1, 1, 32, tag='dl')
        lib.call('tg_g_loss_f32', d_fake_logits.ptr, d_fake_logits.ld, d_fake_logits.n, g.ptr, g.ld, lib.ptr(loss_out), cx.stream)
        d_fake_logits.grad = g

    def _c_loss(self, c_logits, n_real, n_unl, n_rep, n_fake, y_l_c, y_g, d_unl_logits, lambdas_dev, loss_out):
        """c_loss (train_base.py:118,130-152); rows of c_logits [real|unl|unl_rep|fake]."""
        cx = ctx()
        g = cx.new_act(c_logits.n, 1, 1, c_logits.c, c_logits.ld, tag='dl')
        lib.call('tg_c_loss_k_f32', c_logits.ptr, c_logits.ld, n_real, n_unl, n_rep, n_fake, c_logits.c, y_l_c.ptr, y_g.ptr,
                 d_unl_logits.ptr, d_unl_logits.ld, lib.ptr(lambdas_dev), g.ptr, g.ld, lib.ptr(loss_out), cx.stream)
        c_logits.grad = g

    @staticmethod
    def _lambda_dev(Lambda):
        """Lambda = [lambda_1(, lambda_2)] as the device pair the loss heads read: a device tensor as it is, numbers copied to one."""
        if isinstance(Lambda, torch.Tensor):
            return Lambda
        vals = [float(v) for v in Lambda] + [0.0, 0.0]
        lam = ctx().scratch('loss_lambda', 2)
        lam.copy_(torch.tensor(vals[:2], dtype=torch.float32))
        return lam

    def _loss_GAN(self, D, C, Y, Lambda):
        """train_base.py:113-154 on the outputs of Model.forward_pass, the reference's arguments:
        D = [D_real, D_real_logits, D_fake, D_fake_logits, D_unl, D_unl_logits]; C = [C_real_logits, C_unl_logits, C_unl_d_logits,
        C_fake_logits(, C_unl_logits_rep — config.DATA_NAME 'cifar10')]; Y = [y_g, y_l_c]; Lambda = [lambda_1(, lambda_2)] as numbers or
        a device tensor.  Returns (d_loss, g_loss, c_loss), 1-element device tensors."""
        loss_out = ctx().scratch('loss_gan', 4)
        lam = self._lambda_dev(Lambda)
        _, d_real, _, d_fake, _, d_unl = D
        dcat = concat_acts([d_real, d_fake, d_unl])
        self._d_loss(dcat, d_real.n, d_fake.n, d_unl.n, loss_out[0:1])
        self._g_loss(d_fake, loss_out[1:2])
        c_real, c_unl, _c_unl_d, c_fake = C[:4]
        c_rep = C[4] if len(C) > 4 else None
        ccat = concat_acts([c_real, c_unl] + ([c_rep] if c_rep is not None else []) + [c_fake])
        y_g, y_l_c = Y
        self._c_loss(ccat, c_real.n, c_unl.n, c_rep.n if c_rep is not None else 0, c_fake.n, y_l_c, y_g, d_unl, lam, loss_out[2:3])
        self.last_loss_inputs = (dcat, ccat)                   # the concatenated logits that carry d(loss)/d(logits)
        return loss_out[0:1], loss_out[1:2], loss_out[2:3]

    # ---- loss variants of train_base.py:156-574 -----------------------------------------------------------------
    # No trainer of the reference repository calls these (Train_goodGAN.py uses _loss_GAN); they are kept for the sibling trainers'
    # models: the same argument tuples (Acts instead of tensors), the same return nesting (Python floats: ONE device->host copy of the
    # term values at the end), and d(loss)/d(input) left in the inputs' `.grad`:
    #     D logits <- d_loss (concatenated copy in `self.last_d_cat`), D_fake_logits.grad <- gG_loss, C_bG_fake_feat.grad <- bG_loss,
    #     every classifier logit tensor <- c_loss.
    # Lambda: Python floats.  Every variant is a weighted sum of the same terms: tg_d_loss_terms_f32, tg_g_loss_f32,
    # tg_c_loss_terms_k_f32, tg_true_fake_loss_k_f32, tg_sqdiff_rows_loss_f32, tg_feature_match_f32, tg_pull_away_f32.

    def _variant_terms(self, D, c_real, c_unl, c_rep, c_gfake, c_bfake, c_pert, f_bfake, f_unl, y_l_c, y_g, w6, w_bad, w_pert, pt):
        """runs the term kernels; returns the host array [d, d_real, d_fake, d_unl, gG, c_head, T_real, T_unl, T_H, T_bal, T_gfake, T_mse,
        tf_w, T_bad_unl, T_bfake, sq_w, T_sq, fm, pt]."""
        cx = ctx()
        lv = torch.zeros(24, dtype=torch.float32, device=cx.device)
        P = lambda i: lib.ptr(lv[i:])
        if D is not None:
            _, d_real, _, d_fake, _, d_unl = D
            dcat = concat_acts([d_real, d_fake, d_unl])
            g = cx.new_act(dcat.n, 1, 1, 1, 32, tag='dl')
            lib.call('tg_d_loss_terms_f32', dcat.ptr, dcat.ld, d_real.n, d_fake.n, d_unl.n, g.ptr, g.ld, P(0), P(1), cx.stream)
            dcat.grad = g
            self.last_d_cat = dcat
            gg = cx.new_act(d_fake.n, 1, 1, 1, 32, tag='dl')
            lib.call('tg_g_loss_f32', d_fake.ptr, d_fake.ld, d_fake.n, gg.ptr, gg.ld, P(4), cx.stream)
            d_fake.grad = gg
        else:
            d_unl = None
        members = [c_real, c_unl] + ([c_rep] if c_rep is not None else []) + ([c_gfake] if c_gfake is not None else [])
        ccat = _c_terms_head(members, c_real.n, c_unl.n, c_rep.n if c_rep is not None else 0, c_gfake.n if c_gfake is not None else 0, y_l_c,
                             y_g if c_gfake is not None else None, d_unl, w6, P(5), P(6))
        k = ccat.c
        g_unl = c_unl.grad
        gb = cx.new_act(c_bfake.n, 1, 1, c_bfake.c, c_bfake.ld, tag='dl')
        unl_rows = ccat.view_rows(c_real.n, c_real.n + c_unl.n)
        assert c_bfake.c == k, (c_bfake.c, k)
        lib.call('tg_true_fake_loss_k_f32', unl_rows.ptr, ccat.ld, c_unl.n, c_bfake.ptr, c_bfake.ld, c_bfake.n, k, w_bad, w_bad, g_unl.ptr,
                 g_unl.ld, 1, gb.ptr, gb.ld, 0, P(12), cx.stream)
        c_bfake.grad = gb
        if c_pert is not None:
            gp = cx.new_act(c_pert.n, 1, 1, c_pert.c, c_pert.ld, tag='dl')
            lib.call('tg_sqdiff_rows_loss_f32', c_pert.ptr, c_pert.ld, c_bfake.ptr, c_bfake.ld, c_pert.n, c_pert.c, w_pert, gp.ptr, gp.ld, 0,
                     gb.ptr, gb.ld, 1, P(15), cx.stream)
            c_pert.grad = gp
        # bad generator: feature matching (+ pull-away) on dense [n][c] features
        assert f_bfake.ld == f_bfake.c and f_unl.ld == f_unl.c, "features must be dense [n][c]"
        gf = cx.new_act(f_bfake.n, 1, 1, f_bfake.c, f_bfake.c, tag='dl')
        gu = cx.scratch('dfu', f_unl.n * f_unl.c)
        lib.call('tg_feature_match_f32', f_bfake.ptr, f_bfake.n, f_unl.ptr, f_unl.n, f_bfake.c, gf.ptr, lib.ptr(gu), P(17), cx.stream)
        if pt is not None:
            n, c = f_bfake.n, f_bfake.c
            gpt = cx.scratch('dpt', n * c)
            lib.call('tg_pull_away_f32', f_bfake.ptr, n, c, 1 if pt == 'masked' else 0, lib.ptr(cx.scratch('pts', n * c + n * n + n)), lib.ptr(gpt),
                     P(18), cx.stream)
            lib.call('tg_add_f32', gf.ptr, gf.ptr, lib.ptr(gpt), n * c, cx.stream)
        f_bfake.grad = gf
        return [float(v) for v in lv.cpu().numpy()]

    def _loss_BGAN(self, C, Y, Lambda=None):
        """train_base.py:156-184 -> (g_loss, c_loss); C = [C_real, C_unl, C_fake logits, feat_real, feat_unl, feat_fake]."""
        c_real, c_unl, c_fake, _f_real, f_unl, f_fake = C
        v = self._variant_terms(None, c_real, c_unl, None, None, c_fake, None, f_fake, f_unl, Y[0], None, [1.0, 0.0, 0.1, 1e-3, 0.0, 0.0], 1.0, 0.0,
                                'masked')
        return v[17] + v[18], v[5] + v[12]

    def _good_bad(self, D, C, Y, Lambda, perturb):
        if perturb:
            c_real, c_unl, _cud, c_gfake, c_bfake, c_pert, _fr, f_unl, f_bfake, _fp = C
        else:
            (c_real, c_unl, _cud, c_gfake, c_bfake, _fr, f_unl, f_bfake), c_pert = C, None
        y_g, y_l_c = Y
        lam1 = float(Lambda[0])
        v = self._variant_terms(D, c_real, c_unl, None, c_gfake, c_bfake, c_pert, f_bfake, f_unl, y_l_c, y_g,
                                [1.0, 0.01 * 0.5, 0.3, 1e-3, lam1, 0.0], 1.0, 1e-3, 'unmasked')
        return v[0], v[4], v[17] + v[18], v[5] + v[12] + (v[15] if perturb else 0.0)

    def _loss_GoodBadGAN(self, D, C, Y, Lambda):
        """train_base.py:186-240 -> (d_loss, gG_loss, bG_loss, c_loss)."""
        return self._good_bad(D, C, Y, Lambda, False)

    def _loss_GoodRegBadGAN(self, D, C, Y, Lambda):
        """train_base.py:519-574 -> (d_loss, gG_loss, bG_loss, c_loss)."""
        return self._good_bad(D, C, Y, Lambda, True)

    def _good_reg(self, D, C, Y, Lambda, variant):
        y_g, y_l_c = Y
        c_rep = None
        if variant == 'plain':
            c_real, c_unl, _cud, c_gfake, c_bfake, c_pert, _fr, f_unl, f_bfake, _fp = C
        elif variant == 'cifar10':
            c_real, c_unl, _cud, c_gfake, c_bfake, c_pert, _fr, f_unl, f_bfake, _fp, c_rep = C
        elif variant == 'BS':
            c_real, c_unl, _cud, c_gfake, c_bfake, c_pert, _cub, _fr, _fu, f_bfake, _fp, f_unl = C
        else:
            c_real, c_unl, _cud, c_gfake, c_bfake, c_pert, _cub, _fr, _fu, f_bfake, _fp, f_unl, _c_rep = C
        fast = variant == 'BS_cifar10' and getattr(getattr(self, 'config', None), 'FAST_MODE', False)
        w_h = {'plain': 0.3, 'cifar10': 0.3, 'BS': 1e-5, 'BS_cifar10': 1e-7}[variant]
        lam = [float(x) for x in Lambda]
        l1, l2, l3 = lam[:3]
        l4 = lam[3] if len(lam) > 3 else 0.0
        w6 = [1.0, l2 * 0.01 * 0.5, l2 * w_h, l2 * 1e-3, l2 * l1, l4 if variant == 'cifar10' else 0.0]
        v = self._variant_terms(D, c_real, c_unl, c_rep if variant == 'cifar10' else None, None if fast else c_gfake, c_bfake, c_pert, f_bfake,
                                f_unl, y_l_c, y_g, w6, l3, l3 * 1e-3, 'masked' if variant in ('plain', 'cifar10') else None)
        t_real, t_unl, t_h, t_bal, t_gf, t_mse = v[6:12]
        confid, unl, bal = w_h * t_h, 0.01 * 0.5 * t_unl, 1e-3 * t_bal
        c_gG = confid + unl + l1 * t_gf + bal
        pert = 1e-3 * v[16]
        c_bG = v[13] + v[14] + pert
        c_list = [v[5] + v[12] + v[15], t_real, c_gG, confid, unl, bal, t_gf, c_bG, v[13], v[14], pert]
        if variant == 'cifar10':
            c_list.append(l4 * t_mse)
        elif variant == 'BS_cifar10':
            c_list.append(l4)                                        # train_base.py:503: the constant lambda_4
            c_list[0] += l4
        return [v[0], v[1], v[2], v[3]], v[4], v[17] + (v[18] if variant in ('plain', 'cifar10') else 0.0), c_list

    def _loss_GoodRegGAN(self, D, C, Y, Lambda):
        """train_base.py:242-305."""
        return self._good_reg(D, C, Y, Lambda, 'plain')

    def _loss_GoodRegGAN_cifar10(self, D, C, Y, Lambda):
        """train_base.py:307-374."""
        return self._good_reg(D, C, Y, Lambda, 'cifar10')

    def _loss_GoodRegGAN_BS(self, D, C, Y, Lambda):
        """train_base.py:376-442."""
        return self._good_reg(D, C, Y, Lambda, 'BS')

    def _loss_GoodRegGAN_BS_cifar10(self, D, C, Y, Lambda):
        """train_base.py:444-515 (config.FAST_MODE drops the generated-sample cross-entropy)."""
        return self._good_reg(D, C, Y, Lambda, 'BS_cifar10')

    # ---- WGAN-GP (train_base.py:576-620) --------------------------------------------------------------------------------------------
    # The penalty differentiates the discriminator's input gradient; with its dropout masks and noise fixed the network is piecewise linear
    # in the image, so d gp / d theta_D takes four first-order sweeps (tg/grad_penalty.py, which a model's discriminator_gradient_penalty
    # hands its layer table).  It goes to a flat buffer laid out like the discriminator's ParamStore.g, `self.last_gp_grad`, never into store.g
    # (the caller's D backward owns that, and its filter-gradient launches overwrite); `_add_gp_grad()` adds it once that backward ran.

    @staticmethod
    def _gp_sweeps(f):
        """the model method behind the discriminator callable `f` (a bound Model.discriminator, or the model itself)."""
        model = getattr(f, '__self__', f)
        fn = getattr(model, 'discriminator_gradient_penalty', None)
        if fn is None:
            raise lib.TgError("_gradient_penalty: %s has no discriminator_gradient_penalty; WGAN-GP is implemented for Good_GAN (MNIST / "
                              "SVHN), Good_GAN_cifar10 and Good_GAN_stress64 — of their discriminators only the one with minibatch "
                              "discrimination (MINIBATCH_DIS = True) is not piecewise linear in the image, and the model refuses it"
                              % type(model).__name__)
        return fn

    def _gradient_penalty(self, real, fake, label, f, weight=1.0):
        """train_base.py:598-620: gp = mean((sqrt(reduce_sum(gx^2, axis=1)) - 1)^2) with gx = d sum(logits) / dx at x = real + alpha
        (fake - real), alpha ~ U[0,1) per image ('GP/alpha').  real, fake: Act [N,H,W,C], or [N,F] (MNIST: axis 1 is then the feature
        axis, one slope per image), of one shape; label: Act [N,NUM_CLASSES]; f: the
        discriminator (its logits, element [1] of the pair it returns, are differentiated).  Returns weight * gp (1-element device tensor)
        and leaves weight * d gp / d theta_D in self.last_gp_grad.  No gradient reaches the generator or `real` (TF's d_solver)."""
        if not (real.n == fake.n == label.n):
            raise lib.TgError("_gradient_penalty: batch sizes differ (real %d, fake %d, labels %d)" % (real.n, fake.n, label.n))
        gp, self.last_gp_grad = self._gp_sweeps(f)(real, fake, label, weight)
        return gp

    def _r1_penalty(self, real, label, f, gamma):
        """R1 (config.R1_GAMMA; not in the reference): gamma / 2 * mean_i ||d logit_i / d x_i||^2 at the real rows `real`
        with their own labels `label`, the norm over all elements of image i.  f: the discriminator, as in _gradient_penalty; gamma: a
        number or a 1-element device tensor.  Returns the penalty (1-element device tensor) and leaves its parameter gradient in
        self.last_gp_grad, for _add_gp_grad()."""
        if real.n != label.n:
            raise lib.TgError("_r1_penalty: batch sizes differ (real %d, labels %d)" % (real.n, label.n))
        model = getattr(f, '__self__', f)
        fn = getattr(model, 'discriminator_r1_penalty', None)
        if fn is None:
            raise lib.TgError("_r1_penalty: %s has no discriminator_r1_penalty; R1 is implemented for Good_GAN (MNIST / SVHN), "
                              "Good_GAN_cifar10 and Good_GAN_stress64" % type(model).__name__)
        pen, self.last_gp_grad = fn(real, label, gamma)
        return pen

    def _loss_WGAN_GP(self, G, D, C, X, Y, Lambda, discriminator):
        """train_base.py:576-596 -> (d_loss, g_loss, c_loss) as Python floats.  G: the generated images (the penalty's `fake`);
        D: the reference's 9-tuple (D_real, D_real_logits, fm_real, D_fake, D_fake_logits, fm_fake, D_unl, D_unl_logits, fm_unl; the fm
        entries may be None) or this port's 6-tuple; C = (C_real_logits, C_fake_logits, C_unlabel_logits); X: real images; Y: their
        labels (one tensor for both cross-entropies, as the reference); Lambda = (lambda_1, lambda_2).
        Gradients: self.last_d_cat.grad <- d_loss w.r.t. the [real | fake | unl] logits (without the penalty), D_fake_logits.grad <-
        g_loss, the three classifier logit tensors' .grad <- c_loss, and self.last_gp_grad <- 10 d gp / d theta_D (add it to the
        discriminator's store.g after its backward pass: _add_gp_grad)."""
        if len(D) == 9:
            _, d_real, _, _, d_fake, _, _, d_unl, _ = D
        elif len(D) == 6:
            _, d_real, _, d_fake, _, d_unl = D
        else:
            raise lib.TgError("_loss_WGAN_GP: D must be the reference's 9-tuple or the 6-tuple of forward_pass, got %d entries" % len(D))
        c_real, c_fake, c_unl = C
        lam1, lam2 = (float(v) for v in Lambda[:2])
        if not (X.n == G.n == Y.n == c_real.n == c_fake.n):
            raise lib.TgError("_loss_WGAN_GP: batch sizes differ (X %d, G %d, Y %d, C_real %d, C_fake %d)" % (X.n, G.n, Y.n, c_real.n, c_fake.n))
        cx = ctx()
        lv = torch.zeros(16, dtype=torch.float32, device=cx.device)
        P = lambda i: lib.ptr(lv[i:])
        dcat = concat_acts([d_real, d_fake, d_unl])
        g = cx.new_act(dcat.n, 1, 1, 1, 32, tag='dl')
        gf = cx.new_act(d_fake.n, 1, 1, 1, 32, tag='dl')
        lib.call('tg_wgan_loss_f32', dcat.ptr, dcat.ld, d_real.n, d_fake.n, d_unl.n, lam1, lam2, g.ptr, g.ld, gf.ptr, gf.ld, P(0), cx.stream)
        dcat.grad, d_fake.grad = g, gf
        self.last_d_cat = dcat
        # rows [real | unl | fake]; the unl terms weigh 0
        _c_terms_head([c_real, c_unl, c_fake], c_real.n, c_unl.n, 0, c_fake.n, Y, Y, None, (1.0, 0.0, 0.0, 0.0, lam2, 0.0), P(5), P(6))
        gp10 = self._gradient_penalty(X, G, Y, discriminator, weight=10.0)
        lv[12:13].copy_(gp10)
        v = [float(x) for x in lv.cpu().numpy()]
        self.last_wgan_terms = dict(wd1=v[2], wd2=v[3], wd3=v[4], gp=v[12] / 10.0)
        return v[0] + v[12], v[1], v[5]

    # ---- the training step's WGAN-GP (config.LOSS = 'WGAN_GP', Training/Train_goodGAN.py): replayable heads ---------------
    # lambda_1 / lambda_2 are read from a device pair (the trainer's hyper[2:4]) and the weighted penalty from the device scalar the sweeps
    # wrote, so a recorded launch plan or graph follows set_hyper(); nothing is synchronised.
    GP_WEIGHT = 10.0                                   # train_base.py:581: d_loss = -(...) + 10 gp

    def _wgan_d_head(self, d_logits, n_real, n_fake, n_unl, lambdas_dev, gp_w, loss_out):
        """d_loss = -(wd1 + l1 wd2 + l2 wd3) + gp_w (rows [real | fake | unl]); d(loss)/d(logits) in d_logits.grad.  The unweighted terms
        {wd1, wd2, wd3, gp} stay on the device in self.wgan_terms_dev."""
        cx = ctx()
        g = cx.new_act(d_logits.n, 1, 1, 1, 32, tag='dl')
        self.wgan_terms_dev = cx.scratch('wgterms', 4)
        lib.call('tg_wgan_d_head_f32', d_logits.ptr, d_logits.ld, n_real, n_fake, n_unl, lib.ptr(lambdas_dev), lib.ptr(gp_w), self.GP_WEIGHT,
                 g.ptr, g.ld, lib.ptr(loss_out), lib.ptr(self.wgan_terms_dev), cx.stream)
        d_logits.grad = g

    def _wgan_g_head(self, d_fake_logits, loss_out):
        """g_loss = -mean(D_fake_logits) (train_base.py:588)."""
        cx = ctx()
        g = cx.new_act(d_fake_logits.n, 1, 1, 1, 32, tag='dl')
        lib.call('tg_wgan_g_head_f32', d_fake_logits.ptr, d_fake_logits.ld, d_fake_logits.n, g.ptr, g.ld, lib.ptr(loss_out), cx.stream)
        d_fake_logits.grad = g

    def _wgan_c_head(self, c_logits, n_real, n_zero, n_fake, y_l_c, y_g, lambdas_dev, loss_out):
        """c_loss = CE(y_l_c, C_real) + l2 CE(y_g, C_fake) (train_base.py:590-594); rows of c_logits [real | zero (n_zero) | fake], the
        zero rows (unl / rep) get a zero gradient."""
        cx = ctx()
        g = cx.new_act(c_logits.n, 1, 1, c_logits.c, c_logits.ld, tag='dl')
        lib.call('tg_wgan_c_head_f32', c_logits.ptr, c_logits.ld, n_real, n_zero, n_fake, c_logits.c, y_l_c.ptr, y_g.ptr, lib.ptr(lambdas_dev),
                 g.ptr, g.ld, lib.ptr(loss_out), None, cx.stream)
        c_logits.grad = g

    def _loss_WGAN_GP_step(self, G, D, C, X, Y, Lambda, discriminator):
        """the loss of the training step with config.LOSS = 'WGAN_GP' on the outputs of Model.forward_pass (the port decisions of DESIGN §9.1):
        D = [D_real, D_real_logits, D_fake, D_fake_logits, D_unl, D_unl_logits]; C = [C_real_logits, C_unl_logits, C_unl_d_logits,
        C_fake_logits(, C_unl_logits_rep)]; X: the real images of the penalty (X_P), G: its fake ones, both as model.as_image() gives them;
        Y = [y_g, y_l_c] (the penalty's labels are y_g); Lambda: device pair or numbers.  Returns (d_loss, g_loss, c_loss), 1-element device
        tensors — the penalty runs in the caller's phase (discriminator_gradient_penalty(in_step=True)); its parameter gradient is left in
        self.last_gp_grad."""
        loss_out = ctx().scratch('loss_wgan', 4)
        lam = self._lambda_dev(Lambda)
        _, d_real, _, d_fake, _, d_unl = D
        y_g, y_l_c = Y
        gp_w, self.last_gp_grad = self._gp_sweeps(discriminator)(X, G, y_g, self.GP_WEIGHT, in_step=True)
        dcat = concat_acts([d_real, d_fake, d_unl])
        self._wgan_d_head(dcat, d_real.n, d_fake.n, d_unl.n, lam, gp_w, loss_out[0:1])
        self._wgan_g_head(d_fake, loss_out[1:2])
        c_real, c_unl, _c_unl_d, c_fake = C[:4]
        c_rep = C[4] if len(C) > 4 else None
        ccat = concat_acts([c_real, c_unl] + ([c_rep] if c_rep is not None else []) + [c_fake])
        self._wgan_c_head(ccat, c_real.n, c_unl.n + (c_rep.n if c_rep is not None else 0), c_fake.n, y_l_c, y_g, lam, loss_out[2:3])
        self.last_loss_inputs = (dcat, ccat)
        return loss_out[0:1], loss_out[1:2], loss_out[2:3]

    def _add_gp_grad(self, store=None):
        """store.g += self.last_gp_grad (the discriminator's store by default): call after the D backward pass that wrote store.g."""
        store = store if store is not None else ctx().stores['discriminator']
        gp = getattr(self, 'last_gp_grad', None)
        if gp is None or gp.numel() != store.n_p:
            raise lib.TgError("_add_gp_grad: no gradient-penalty gradient laid out like store %r (run _gradient_penalty first)" % store.name)
        lib.call('tg_add_f32', lib.ptr(store.g), lib.ptr(store.g), lib.ptr(gp), store.n_p, ctx().stream)
