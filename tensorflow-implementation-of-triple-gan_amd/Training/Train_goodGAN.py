"""Train — the Triple-GAN training driver, counterpart of the reference's Training/Train_goodGAN.py.

Same entry point: `Train(config, log_dir, save_dir, **kwargs).train(Dataset, Model, sample_y)`
(Train_goodGAN.py:27,43) and the same iteration protocol (:230-278):

    D-update  (sess.run([d_solver, d_loss]))   G fwd, C(x_u_c), C(x_u_d) fwd, D x3 fwd, D bwd, Adam(D)
    G-update  (sess.run([g_solver, g_loss]))   G fwd, D(G) fwd, D data-bwd, G bwd, Adam(G)
    C-update  (sess.run([c_solver, c_loss]))   G fwd, C x4 fwd, D(x_u_c) fwd, C bwd, Adam(C), EMA(C)

Each solver run executes only the sub-graph its fetches need and re-samples dropout / noise, exactly as three
TF session calls on one feed do.  Instead of a TF graph + Session the three runs are captured
once into hipGraphs and replayed (config.USE_HIP_GRAPH); hyper-parameters that change (lr, lambdas, Adam step,
RNG step) live in device memory.  Applications of one network inside a solver run are batched into one call
(D: [D_real|D_fake|D_unl] = 250 images; C: [C_real|C_unl|C_unl_rep|C_fake] = 250 images, mean-only-BN per
application).  Data-parallel replicas (one process per GPU) sum-all-reduce the trained network's flat gradient
buffer over RCCL after each backward (tg/dist.py); the reference has no multi-device path.
"""
import contextlib
import math
import os
import time

import numpy as np
import torch

from config import Config
from Model.zca import resolve_zca, synthetic_zca as _synthetic_zca         # (tools/ reach the synthetic rotation under this name)
from Training.options import (LOSSES, NETS, NUM_CLASSES_RANGE, OPTIMIZERS, Options, check_act_dtype, check_clip_norm, check_eval_ema,  # noqa: F401
                              check_eval_report, check_loss, check_mfma_dtype, check_num_classes, check_optimizer, check_sample_manifold_k,
                              check_sample_metrics, check_wn_init, check_zca, cla_lr, opt, resolve)
from Training.train_base import Train_base, clip_workspace_floats
from tg import dist as tgdist
from tg import executor, lib, ops
from tg.batching import concat_acts
from tg.runtime import Act, Context, PhiloxRNG, ctx, set_context


class _Scores(object):
    """what Train._score_batch adds a scored batch to: the streaming accuracy, a tg.metrics.ClassifierReport (handed in, or None) and —
    features — the tg.metrics.FeatureMoments of the classifier's pooled feature plus, bank, a tg.metrics.FeatureBank of its rows; those
    two are sized by the first feature seen and stay None on a side that saw no batch."""

    def __init__(self, report=None, features=False, bank=False):
        self.report, self.features, self.want_bank = report, features, bank
        self.accuracy = self.moments = self.bank = None


class Train(Train_base):
    def __init__(self, config, log_dir, save_dir, **kwargs):
        super(Train, self).__init__()
        self.config = config
        self.save_dir = save_dir
        self.log_dir = log_dir
        self.comments = kwargs.get('comments', '')
        o = self.options = resolve(config)           # every device-free check, before a device is initialised (Training/options.py)
        self.world, self.rank, self.local_rank = tgdist.init()
        try:
            self.cx = ctx()
        except lib.TgError:
            self.cx = set_context(Context('cuda:%d' % self.local_rank, seed=o.seed + 7919 * self.rank))
        cx = self.cx
        cx.mfma_dtype = o.mfma_dtype                 # 'bf16': the MFMA kernels round their operands to bf16 (options.check_mfma_dtype)
        # 'bf16': the batch norms the model marks store their output as bf16 — same numbers, half the bytes (Context.act_dtype)
        cx.act_dtype = o.act_dtype
        self.loss_kind = o.loss                      # 'GAN' | 'WGAN_GP': the loss heads of the three solver runs
        self.optimizer_kinds = o.optimizers          # (D, G, C), each 'adam' | 'rmsprop' | 'momentum' 
        self.clip_norms = o.clip_norms               # (D, G, C), each a threshold or None: clip_by_global_norm
        self.clip_dev = None                         # with a clip: per network [threshold, 0, norm, factor] on the device
        self._clip_views = {}                        # network -> (threshold, {norm, factor}) views of it (Train_base._clip_state)
        self._gp_w = self._gp_grad = None            # WGAN-GP: the D-update's weighted penalty and its parameter gradient (device)
        cx.bf16_act_layers = set()
        # device-resident hyper-parameters (the reference's lr_ph / cla_lr_ph / lambda placeholders, :30-31,416-420)
        self.hyper = torch.zeros(4, dtype=torch.float32, device=cx.device)       # lr, cla_lr, lambda_1, lambda_2
        self.loss_dev = torch.zeros(3, dtype=torch.float32, device=cx.device)    # d_loss, g_loss, c_loss
        self.model = None
        self.executor = executor.StepExecutor(cx)        # how an iteration is launched, and every graph / launch plan it replays
        self._refusal_warned = False
        self._g_saved = None             # the D-update's generator forward pass, kept for the G-update on the same feed
        self._rest = {}                  # solver run -> (unexecuted head of its backward tape, call-site counter): bucketed backward passes
        self.iteration = 0
        self._label_override = {}        # see label_override()
        self.wn_initialised = None       # {network: layers initialised} once data_dependent_init() has run (config.WN_INIT = 'data')
        self.zca_source = None           # config.ZCA = 'fit' resolved by train() (Model/zca.resolve_zca): 'files' | 'fit' (rank 0) | 'broadcast' (other ranks)
        self._metric_latents = None      # (z, y) host arrays of sample_metrics(), drawn once per trainer from config.SEED
        self.last_reports = {}           # config.EVAL_REPORT: the last epoch tail's report dicts {'val', 'val_ema', 'g'} (_tail_metrics)
        self._hist_runs = {}             # network -> (store layout key, tg.summary.StoreHistograms): see histograms()
        self.summary_train = self.summary_val = None
        if o.summary and log_dir and self.rank == 0:          # :37-41
            from Training.Summary import Summary
            self.summary_train = Summary(log_dir, config, log_type='train', log_comments=kwargs.get('comments', ''))
            self.summary_val = Summary(log_dir, config, log_type='val', log_comments=kwargs.get('comments', ''))

    @property
    def bf16_act_edges(self):
        """how many batch-norm outputs this trainer's step stores as bf16 (config.ACT_DTYPE = 'bf16'; 0 with 'f32' or on a model with no
        eligible edge, e.g. Good_GAN_cifar10) — counted per layer, after the first iteration."""
        return len(self.cx.bf16_act_layers)

    # ------------------------------------------------------------------ graph build
    def _build_train_graph(self, Model):
        """:400-426: the placeholders become persistent device buffers of the static batch sizes."""
        c, cx = self.config, self.cx
        dims = c.IMAGE_DIM

        def ph(key, n, shape):
            t = cx.ws('ph:' + key, n * int(np.prod(shape)))
            return Act(t, n, *(shape if len(shape) == 3 else (1, 1, shape[0])), ld=shape[-1])

        self.z_g_ph = ph('z_g', c.BATCH_SIZE_G, [c.Z_DIM])
        self.y_g_ph = ph('y_g', c.BATCH_SIZE_G, [c.NUM_CLASSES])
        self.x_l_c_ph = ph('x_l_c', c.BATCH_SIZE_L_C, dims)
        self.y_l_c_ph = ph('y_l_c', c.BATCH_SIZE_L_C, [c.NUM_CLASSES])
        self.x_l_d_ph = ph('x_l_d', c.BATCH_SIZE_L_D, dims)
        self.y_l_d_ph = ph('y_l_d', c.BATCH_SIZE_L_D, [c.NUM_CLASSES])
        self.x_u_d_ph = ph('x_u_d', c.BATCH_SIZE_U_D, dims)
        self.x_u_c_ph = ph('x_u_c', c.BATCH_SIZE_U_C, dims)
        self.model = Model(c)
        st = cx.stores
        # three optimisers, Adam unless config.OPTIMIZER says otherwise (:85-87): G and D share lr_ph / config.BETA1, C uses cla_lr_ph / 0.5
        kd, kg, kc = self.optimizer_kinds
        self.d_optimizer = self._make_optimizer(kd, self.hyper[0:1], c.BETA1)
        self.g_optimizer = self._make_optimizer(kg, self.hyper[0:1], c.BETA1)
        self.c_optimizer = self._make_optimizer(kc, self.hyper[1:2], 0.5)
        for opt, net in ((self.d_optimizer, 'discriminator'), (self.g_optimizer, 'good_generator'), (self.c_optimizer, 'classifier')):
            opt.bind(st[net])                    # the store's slots start where this optimiser's do (RMSProp: rms = 1), now and when they grow
        self.set_hyper(c.LEARNING_RATE, cla_lr(c), 0.0, 0.0)
        if any(v is not None for v in self.clip_norms):
            # thresholds and results live on the device, and the norm's workspace exists before anything records: plans and graphs hold both
            self.clip_dev = torch.zeros(4 * len(NETS), dtype=torch.float32, device=cx.device)
            for k, (net, v) in enumerate(zip(NETS, self.clip_norms)):
                if v is not None:
                    self._clip_views[net] = (self.clip_dev[4 * k:4 * k + 1], self.clip_dev[4 * k + 2:4 * k + 4])
                    cx.ws('clip:ws:' + net, clip_workspace_floats(st[net]))
            self.set_clip_norm(*self.clip_norms)
        if tgdist.active():                      # identical initial weights on every replica
            for s in st.values():
                tgdist.broadcast_(s.p)
                tgdist.broadcast_(s.s)
            st['classifier'].ema.copy_(st['classifier'].p)
        PH = [self.z_g_ph, self.y_g_ph, self.x_l_c_ph, self.y_l_c_ph, self.x_l_d_ph, self.y_l_d_ph, self.x_u_d_ph,
              self.x_u_c_ph, True, self.hyper[2:4]]
        return PH, self.model

    def _make_optimizer(self, kind, lr_dev, beta1):
        """one network's optimiser on the device learning rate `lr_dev`: Adam(beta1), RMSProp (decay 0.9, momentum 0, as the reference's
        factory) or momentum SGD (config.MOMENTUM)."""
        if kind == 'adam':
            return self._Adam_optimizer(lr_dev, beta1)
        if kind == 'rmsprop':
            return self._RMSProp_optimizer(lr_dev)
        return self._SGD_w_Momentum_optimizer(lr_dev, self.options.momentum)

    def set_hyper(self, lr=None, cla_lr=None, lambda_1=None, lambda_2=None):
        vals = self.hyper.detach().cpu().numpy()
        for i, v in enumerate((lr, cla_lr, lambda_1, lambda_2)):
            if v is not None:
                vals[i] = v
        self.hyper.copy_(torch.from_numpy(vals))

    def set_clip_norm(self, d=None, g=None, c=None):
        """new thresholds for the networks given (None keeps one), written to the device like set_hyper: a replayed plan or graph follows.
        Only a network clipped at build time (config.CLIP_NORM) can be changed — the others' launches hold no clip."""
        if self.clip_dev is None:
            if (d, g, c) == (None, None, None):
                return
            raise lib.TgError("set_clip_norm: this trainer was built with CLIP_NORM = None; a clip is part of the recorded launches")
        new = []
        for net, v in zip(NETS, (d, g, c)):
            if v is None:
                continue
            if net not in self._clip_views:
                raise lib.TgError("set_clip_norm: network %r was built unclipped (CLIP_NORM = %r)" % (net, self.clip_norms))
            if not 0.0 < float(v) < float('inf'):
                raise lib.TgError("set_clip_norm: the threshold of %r must be a positive finite number, got %r" % (net, v))
            new.append((net, float(v)))
        for net, v in new:                               # only the threshold elements: {norm, factor} beside them are the kernels'
            self._clip_views[net][0].fill_(v)

    def grad_norms(self):
        """{'d': (norm, factor), 'g': ..., 'c': ...} of the last iteration's gradients as floats — ONE device->host copy; None for an
        unclipped network (and (0, 0) for one whose solver has not run yet).  A NaN factor is a non-finite norm."""
        if self.clip_dev is None:
            return dict(d=None, g=None, c=None)
        vals = self.clip_dev.detach().cpu().numpy()
        return {key: ((float(vals[4 * k + 2]), float(vals[4 * k + 3])) if net in self._clip_views else None)
                for k, (key, net) in enumerate(zip('dgc', NETS))}

    def _apply(self, optimizer, net, grad_scale):
        """the optimiser step of `net`: through _train_op_w_grads with the device threshold when the network is clipped, else _train_op."""
        st = self.cx.stores[net]
        views = self._clip_views.get(net)
        if views is None:
            self._train_op(optimizer, st, grad_scale)
        else:
            self._train_op_w_grads(optimizer, st, grad_scale, clip=views[0])

    # ------------------------------------------------------------------ the three solver runs
    def _d_forward_backward(self, split=False):
        """split: stop the backward pass at the discriminator's last gradient-bucket boundary (the rest runs in _backward_rest)."""
        c, cx, m = self.config, self.cx, self.model
        with cx.phase_scope('D', train_nets=('discriminator',)):
            # The G-update that follows runs the generator on the same feed with the same (not yet updated) weights, and the
            # generator is deterministic (no dropout / noise): TF recomputes it in the second sess.run, here the forward
            # pass and its backward closures are kept for _g_forward_backward (bit-identical result, one G forward saved).
            g_replay = []
            # (eager launches with the side stream, Context.wgrad_side: the generator's forward pass — small launches — runs beside the
            # classifier's, which it does not depend on; the two meet where the discriminator's batch is assembled)
            wgan = self.loss_kind == 'WGAN_GP'
            with cx.wgrad_on_side():
                with cx.sub_tape(('good_generator',), replay=g_replay) as g_tape:
                    G = m.good_generator(self.z_g_ph, self.y_g_ph)
                if wgan:
                    # the penalty needs X_P, G, y_g and the discriminator's weights only: it goes beside the classifier's forward pass too,
                    # and the join below completes it before anything reads it
                    xp = concat_acts([m.as_image(self.x_l_d_ph), m.as_image(self.x_u_d_ph)])
                    self._gp_w, self._gp_grad = m.discriminator_gradient_penalty(xp, m.as_image(G), self.y_g_ph, self.GP_WEIGHT, in_step=True)
            self._g_saved = (G, g_tape, g_replay)
            xz = concat_acts([m.as_image(self.x_u_c_ph), m.as_image(self.x_u_d_ph)])
            if m.zca() is not None:
                xz = m.zca().apply(xz)
            with cx.rng_scoped('D/C'):
                c_logits, _ = m.classifier(xz, True, segments=[c.BATCH_SIZE_U_C, c.BATCH_SIZE_U_D])
            cx.join_wgrad_side()
            oh = ops.argmax_onehot(c_logits, c.NUM_CLASSES)                       # [C_unl_hard | C_unl_d_hard]
            self._d_logits = c_logits                    # (parity tests read the logits the labels were taken from)
            if self._label_override.get('D') is not None:      # parity tests against a precomputed fixture: see label_override()
                oh.copy_(self._label_override['D'])
            k = c.NUM_CLASSES
            oh_unl = Act(oh[:c.BATCH_SIZE_U_C * k], c.BATCH_SIZE_U_C, 1, 1, k, k)
            oh_unl_d = Act(oh[c.BATCH_SIZE_U_C * k:], c.BATCH_SIZE_U_D, 1, 1, k, k)
            self._d_labels = (oh_unl, oh_unl_d)          # the labels this run's discriminator sees (parity tests read them back)
            ximg = concat_acts([m.as_image(a) for a in (self.x_l_d_ph, self.x_u_d_ph, G, self.x_u_c_ph)])   # X_P | G | x_u_c (:258-271)
            yall = concat_acts([self.y_l_d_ph, oh_unl_d, self.y_g_ph, oh_unl])
            with cx.rng_scoped('D/D'):
                _, d_logits = m.discriminator(ximg, yall, want_prob=False)
            if wgan:
                self._wgan_d_head(d_logits, c.BATCH_SIZE_L_D + c.BATCH_SIZE_U_D, c.BATCH_SIZE_G, c.BATCH_SIZE_U_C, self.hyper[2:4], self._gp_w,
                                  self.loss_dev[0:1])
            else:
                self._d_loss(d_logits, c.BATCH_SIZE_L_D + c.BATCH_SIZE_U_D, c.BATCH_SIZE_G, c.BATCH_SIZE_U_C, self.loss_dev[0:1])
            self._keep_rest('D', cx.backward(stop_at_boundary='discriminator' if split else False))

    def _g_forward_backward(self, split=False):
        cx, m = self.cx, self.model
        with cx.phase_scope('G', train_nets=('good_generator',)):
            saved = self._g_saved
            if saved is not None:                       # generator forward of the D-update on the same feed and weights
                G, g_tape, g_replay = saved
                self._g_saved = None
                for fn in g_replay:                     # the state a re-executed forward pass would have advanced: batch-norm moving
                    fn()                                # statistics get their second update of the iteration (the C-update makes the third)
            else:
                G, g_tape = m.good_generator(self.z_g_ph, self.y_g_ph), None
            with cx.rng_scoped('G/D'):
                _, d_fake = m.discriminator(G, self.y_g_ph, want_prob=False)
            if self.loss_kind == 'WGAN_GP':
                self._wgan_g_head(d_fake, self.loss_dev[1:2])
            else:
                self._g_loss(d_fake, self.loss_dev[1:2])
            rest = cx.backward(stop_at_boundary='good_generator' if (split and g_tape is None) else False)
            if g_tape is not None:                      # the discriminator's input gradient is complete: now the kept generator tape
                rest = cx.run_tape(g_tape, stop_at_boundary='good_generator' if split else False)
            self._keep_rest('G', rest)

    def _c_forward_backward(self, split=False):
        """split: stop the backward pass at the classifier's last gradient-bucket boundary (the rest runs in _backward_rest)."""
        c, cx, m = self.config, self.cx, self.model
        rep = m.CONSISTENCY                                # Good_GAN_cifar10 only: second stochastic pass on x_u_c
        with cx.phase_scope('C', train_nets=('classifier',)):
            G = m.good_generator(self.z_g_ph, self.y_g_ph)
            parts = [self.x_l_c_ph, self.x_u_c_ph] + ([self.x_u_c_ph] if rep else []) + [G]
            segs = [p.n for p in parts]
            xc = concat_acts([m.as_image(p) for p in parts])
            if m.zca() is not None:
                xc = m.zca().apply(xc)
            with cx.rng_scoped('C/C'):
                c_logits, _ = m.classifier(xc, True, segments=segs)
            c_unl = c_logits.view_rows(segs[0], segs[0] + segs[1])
            if self.loss_kind == 'WGAN_GP':
                # CE(y_l_c, C_real) + lambda_2 CE(y_g, C_fake): the unl / rep rows weigh 0 and nothing reads D(x_u_c), so it is not run
                self._c_logits = c_unl
                self._wgan_c_head(c_logits, segs[0], sum(segs[1:-1]), G.n, self.y_l_c_ph, self.y_g_ph, self.hyper[2:4], self.loss_dev[2:3])
                self._keep_rest('C', cx.backward(stop_at_boundary='classifier' if split else False))
                return
            k = c.NUM_CLASSES
            oh_c = ops.argmax_onehot(c_unl, k)
            self._c_logits = c_unl
            if self._label_override.get('C') is not None:
                oh_c.copy_(self._label_override['C'])
            oh_unl = Act(oh_c, c_unl.n, 1, 1, k, k)
            with cx.rng_scoped('C/D'):
                _, d_unl = m.discriminator(self.x_u_c_ph, oh_unl, want_prob=False)
            self._c_loss(c_logits, segs[0], segs[1], segs[1] if rep else 0, G.n, self.y_l_c_ph, self.y_g_ph, d_unl,
                         self.hyper[2:4], self.loss_dev[2:3])
            self._keep_rest('C', cx.backward(stop_at_boundary='classifier' if split else False))

    def _keep_rest(self, phase, rest):
        """the unexecuted head `rest` of solver run `phase`'s backward tape, with the call-site counter _backward_rest resumes it at."""
        self._rest[phase] = (rest, self.cx.counter)

    def _backward_rest(self, phase, net, split):
        """continue the backward pass of solver run `phase` — down to the trained network's next bucket boundary (split) or to its end."""
        rest, counter = self._rest[phase]
        if rest:
            with self.cx.phase_scope(phase, train_nets=(net,), counter=counter):
                self._keep_rest(phase, self.cx.run_tape(rest, stop_at_boundary=net if split else False))

    def _add_gp_slice(self, sl):
        """WGAN-GP: add the penalty's parameter gradient to the slice `sl` of the discriminator's store.g, once the D backward pass has
        finished that slice and before it is exchanged (with replicas it is averaged like every other gradient)."""
        st = self.cx.stores['discriminator']
        off = (sl.data_ptr() - st.g.data_ptr()) // sl.element_size()
        lib.call('tg_add_f32', lib.ptr(sl), lib.ptr(sl), lib.ptr(self._gp_grad[off:off + sl.numel()]), sl.numel(), self.cx.stream)

    def _c_apply(self):
        st = self.cx.stores['classifier']
        self._apply(self.c_optimizer, 'classifier', 1.0 / self.world)
        # ema.apply(c_vars) under control-dependency on the C step (:101-103)
        lib.call('tg_ema_f32', lib.ptr(st.ema), lib.ptr(st.p), st.n_p, 0.9999, self.cx.stream)
        self.cx.rng.advance(self.cx)

    def _bucket_slices(self, net):
        """the flat gradient buffer of `net` cut at the model's GRAD_BUCKETS, in the order the backward pass completes them (last
        variables first); one slice — the whole buffer — without replicas."""
        st = self.cx.stores[net]
        names = self.model.GRAD_BUCKETS.get(net, ())
        if not tgdist.active() or self.options.no_grad_buckets or not names:
            return [st.g]
        offs = [0] + sorted(st.offset(n) for n in names) + [st.n_p]
        return [st.g[offs[i]:offs[i + 1]] for i in range(len(offs) - 2, -1, -1)]

    def _phase_segments(self, phase, net, first_fn, before=None):
        """[(callable, gradient slice to exchange once it has run)] of one solver run: the forward pass + the backward pass down to the
        last bucket boundary, then one segment per remaining bucket.  `before` (the previous network's optimiser step) opens the first."""
        slices = self._bucket_slices(net)
        split = len(slices) > 1
        head = (lambda: first_fn(split)) if before is None else (lambda: (before(), first_fn(split)))
        segs = [(head, slices[0])]
        for k, sl in enumerate(slices[1:]):
            last = k == len(slices) - 2
            segs.append((lambda last=last: self._backward_rest(phase, net, not last), sl))
        if net == 'discriminator' and self.loss_kind == 'WGAN_GP':
            segs = [(lambda fn=fn, sl=sl: (fn(), self._add_gp_slice(sl)), sl) for fn, sl in segs]
        return segs

    def _segments(self, pre_train=False):
        """[(callable, flat gradient slice to exchange afterwards or None, wait for the pending exchanges first?)] — each callable is
        one hipGraph.  With replicas every backward pass is cut at the model's bucket boundaries: a finished bucket is all-reduced on
        the exchange stream while the next segment (the rest of the backward pass) runs; the optimiser step of a network opens the
        next solver run's first segment and waits for that network's buckets."""
        w = 1.0 / self.world
        if pre_train:                                          # :182-226: pre-training runs c_solver only
            phases = [self._phase_segments('C', 'classifier', self._c_forward_backward)]
        else:
            phases = [self._phase_segments('D', 'discriminator', self._d_forward_backward),
                      self._phase_segments('G', 'good_generator', self._g_forward_backward,
                                           lambda: self._apply(self.d_optimizer, 'discriminator', w)),
                      self._phase_segments('C', 'classifier', self._c_forward_backward,
                                           lambda: self._apply(self.g_optimizer, 'good_generator', w))]
        out = []
        for k, segs in enumerate(phases):
            for j, (fn, grads) in enumerate(segs):
                out.append((fn, grads, j == 0 and k > 0))       # a solver run that opens with the previous network's optimiser step
        return out + [(self._c_apply, None, True)]

    # ------------------------------------------------------------------ one iteration
    def feed(self, batch):
        """host feed_dict (:249-263) -> placeholders.  batch keys: z_g,y_g,x_l_c,y_l_c,x_l_d,y_l_d,x_u_d,x_u_c
        (numpy arrays or device Acts)."""
        dev = []
        for key, ph in (('z_g', self.z_g_ph), ('y_g', self.y_g_ph), ('x_l_c', self.x_l_c_ph), ('y_l_c', self.y_l_c_ph),
                        ('x_l_d', self.x_l_d_ph), ('y_l_d', self.y_l_d_ph), ('x_u_d', self.x_u_d_ph), ('x_u_c', self.x_u_c_ph)):
            if key not in batch:
                continue
            v = batch[key]
            if isinstance(v, Act):
                dev.append((ph.t, 0, v.t, ph.t.numel()))
            else:
                a = np.ascontiguousarray(v, np.float32).reshape(-1)
                assert a.size == ph.t.numel(), (key, a.size, ph.t.numel())
                ph.t.copy_(torch.from_numpy(a), non_blocking=False)
        if dev:
            ops.copy_many(dev)                   # device-resident batch: all placeholders in one launch

    def label_override(self, d_labels=None, c_labels=None):
        """TEST HOOK (eager launches only).  The discriminator's labels for unlabelled images are the arg-max of the classifier's logits
        (Model/Good_GAN.py:447-455, Good_GAN_cifar10.py:243-262): a near-tie can come out differently under another summation order or operand
        rounding, and the discriminator's gradient then differs for a reason that is not the discriminator's.  A test that compares against a
        PRECOMPUTED oracle run hands in the one-hot labels that run used — d_labels: [U_C + U_D, k] host array for the D-update ([C_unl | C_unl_d]),
        c_labels: [U_C, k] for the C-update — after checking on the logits (kept in _d_logits / _c_logits) that every disagreement is a
        near-tie.  None clears."""
        cx = self.cx
        to_dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).to(cx.device)
        self._label_override = {'D': to_dev(d_labels), 'C': to_dev(c_labels)}

    def sample_latent(self):
        """z ~ U(-1,1), y ~ onehot(U{0..9}) (:234-239) drawn on the device."""
        cx = self.cx
        with cx.rng_scoped('latent'):
            if hasattr(cx.rng, 'latents'):
                cx.rng.latents(cx, self.z_g_ph.t, self.y_g_ph.t, self.y_g_ph.n, self.config.NUM_CLASSES)
            else:
                cx.rng.uniform(cx, 'z', self.z_g_ph.t.numel(), -1.0, 1.0, out=self.z_g_ph.t)
                cx.rng.onehot(cx, 'y', self.y_g_ph.n, self.config.NUM_CLASSES, out=self.y_g_ph.t)

    def _require_eager(self, what, it_is):
        """lib.TgError when `what` is called while a hipGraph is captured or a launch plan recorded: its launches belong outside both."""
        if self.cx.capturing or lib._recorder is not None:
            raise lib.TgError("%s: called inside a hipGraph capture / launch-plan recording; it is an %s" % (what, it_is))

    def data_dependent_init(self):
        """config.WN_INIT = 'data' (DESIGN §9.9): the model's data-dependent initialisation pass, run eagerly on the batch the placeholders
        hold (feed() + sample_latent()) — every weight-normalised layer's g and b are assigned from that batch, nothing else changes.  Then
        the classifier's EMA shadows are seeded from the weights again, as at build time.  With replicas every rank runs the pass on its own
        batch (the ranks stay in lock-step) and rank 0's result is broadcast: the single-process initialisation on rank 0's batch.
        Happens before anything is recorded, so it works in every EXEC_MODE; lib.TgError once a training iteration has run, or inside a
        capture / recording.  Returns {network: number of layers initialised} (0 for a network without such layers: it is not run)."""
        cx = self.cx
        if self.model is None:
            raise lib.TgError("data_dependent_init: no model yet (_build_train_graph first)")
        self._require_eager("data_dependent_init", "eager pass before the step")
        if self.iteration > 0:
            raise lib.TgError("data_dependent_init: %d training iteration(s) have run; the initialisation belongs before the first (the optimiser "
                              "slots, the EMA shadows and any recorded launch already follow the present g and b)" % self.iteration)
        with cx.phase_scope('wn_init', record=False):
            done = self.model.data_dependent_init(self.z_g_ph, self.y_g_ph, self.x_l_d_ph, self.y_l_d_ph, self.x_u_d_ph, self.x_u_c_ph)
        if tgdist.active():
            for st in cx.stores.values():
                tgdist.broadcast_(st.p)
                tgdist.broadcast_(st.s)
        st = cx.stores['classifier']
        st.ema.copy_(st.p)
        self.wn_initialised = {net: len(v) for net, v in done.items()}
        return dict(self.wn_initialised)

    def train_iteration(self, pre_train=False, use_graph=None):
        """D-update, G-update, C-update on the current placeholder contents (:266-276), launched the way tg.executor.resolve_launch reads
        out of config.EXEC_MODE / USE_HIP_GRAPH.  No host sync."""
        ex, key = self.executor, 'pre' if pre_train else 'full'
        if use_graph is None:
            use_graph = opt(self.config, 'USE_HIP_GRAPH')
        how, refused = executor.resolve_launch(opt(self.config, 'EXEC_MODE'), use_graph, isinstance(self.cx.rng, PhiloxRNG),
                                               tgdist.graphs_allowed(), ex.replay[key].auto.next)
        if refused and not self._refusal_warned:          # torch's RCCL process group: its watchdog cannot coexist with a capture
            self._refusal_warned = True
            if self.rank == 0:
                print("tg: backend %r cannot run beside hipGraph capture (tg/dist.py) - launching eagerly; "
                      "use TG_DIST_BACKEND=rccl-direct for graphs" % tgdist.backend_name(), flush=True)
        if how in ('graph', 'plan') and any(v is not None for v in self._label_override.values()):
            raise lib.TgError("label_override() is a test hook of eager launches: a replayed graph / launch plan would not see it")
        segs = self._segments(pre_train)
        if how == 'graph':
            ex.capture(segs, key)                         # from the second iteration of this key on, whatever has no graph yet
        ex.run(segs, key, how)
        self.iteration += 1

    # ---- thin views of self.executor (tg/executor.py), under the names bench.py, tools/ and the tests use
    AUTO_TIMED, AUTO_SETTLE, AUTO_BLOCKS, AUTO_ITERS = executor.AUTO_TIMED, executor.AUTO_SETTLE, executor.AUTO_BLOCKS, executor.AUTO_ITERS

    def exec_mode_chosen(self, key='full'):
        """(mode, {candidate: seconds per iteration}) of EXEC_MODE = 'auto' once decided, else (None, partial timings)."""
        return self.executor.replay[key].auto.chosen()

    @property
    def _auto(self):
        """{key: {'t': {candidate: [seconds per iteration of each timed block]}}} of the keys whose measurement has begun (bench.py's
        `exec_mode_blocks_ms` reads it under this name)."""
        return {key: {'t': st.auto.times} for key, st in self.executor.replay.items() if st.auto.n}

    def measure_exposed(self, on=True):
        """start (or stop) bracketing every wait for a network's gradient buckets in train_iteration."""
        self.executor.measure_exposed(on)

    def exposed_ms(self):
        """total time the launch stream spent stalled in those waits since measure_exposed(True).  Synchronises the device."""
        return self.executor.exposed_ms()

    def losses(self):
        """(d_loss, g_loss, c_loss) of the last iteration — a device->host sync; call sparingly."""
        return tuple(float(v) for v in self.loss_dev.detach().cpu().numpy())

    def training_statistics(self):
        """The reference's end-of-epoch "Get the training statistics" run (:280-285): ONE forward-only sess.run of
        [merged_summary_train, d_loss, g_loss, c_loss] on the epoch's LAST feed with train_ph = True.  One session call evaluates the
        whole graph of Model.forward_pass once: a single set of fresh dropout / noise draws shared by the three losses (the training
        iterations re-draw per solver run), every classifier application of forward_pass — C_real, C_unl, (C_unl_rep,) C_unl_d, C_fake —
        updating pop_mean / the batch-norm moving statistics once more in call-site order, the generator's batch norm too; no
        gradient, no optimiser step.  THESE losses are what the reference logs and writes to the train summary (:287-293), not the
        last iteration's.  Returns (d_loss, g_loss, c_loss) as floats (a device->host sync)."""
        cx = self.cx
        with cx.phase_scope('stats', record=False):
            PH = [self.z_g_ph, self.y_g_ph, self.x_l_c_ph, self.y_l_c_ph, self.x_l_d_ph, self.y_l_d_ph, self.x_u_d_ph, self.x_u_c_ph]
            G, D, C = self.model.forward_pass(*PH, True)                                                       # :422
            d, g, c = self._goodGAN_loss(G, D, C, None, [self.y_g_ph, self.y_l_c_ph], self.hyper[2:4], self.model.discriminator)
            out = (float(d), float(g), float(c))
        cx.rng.advance(cx)                       # the next iteration draws fresh numbers again
        return out

    # ------------------------------------------------------------------ evaluation
    def _metric(self, real_lab_logits, real_lab, metric=None):
        """:428-447: streaming accuracy of argmax(real_lab_logits) against argmax(real_lab).  Returns the reference's tuple
        (accuracy, update_op, reset_op, prediction, probs): accuracy — float(accuracy) reads the running value (this batch already
        counted); update_op(labels, logits) adds a batch; reset_op() clears the counters; prediction — one-hot arg-max of the logits
        (device tensor [n,k]); probs — None (the reference's `probs` output is never fetched)."""
        accuracy, update_op = self._accuracy_metric(real_lab, real_lab_logits, metric)
        return accuracy, update_op, accuracy.reset, ops.argmax_onehot(real_lab_logits, real_lab_logits.c), None

    def _goodGAN_loss(self, G, D, C, X, Y, Lambda, discriminator=None):
        """:449-454, dispatched on config.LOSS.  'WGAN_GP': X = None (the reference's training call) stands for the discriminator's real
        images X_P = [x_l_d | x_u_d], the penalty's `real`."""
        if self.loss_kind == 'WGAN_GP':
            m = self.model
            if X is None:
                X = concat_acts([m.as_image(self.x_l_d_ph), m.as_image(self.x_u_d_ph)])
            return self._loss_WGAN_GP_step(m.as_image(G), D, C, X, Y, Lambda, discriminator or m.discriminator)
        return self._loss_GAN(D, C, Y, Lambda)

    def _classifier_weights(self, ema):
        """the weights a forward-only classifier pass reads: the variables, or (ema) their EMA shadows — Context.reading_shadows."""
        return self.cx.reading_shadows('classifier') if ema else contextlib.nullcontext()

    def evaluate(self, batches, ema=False, report=None):
        """streaming accuracy of argmax C_real_logits vs argmax y over test batches with train=False (:295-351, :428-447).
        batches: iterable of (x [n,h,w,c], y onehot [n,k]) host arrays.  Returns accuracy.
        report: a tg.metrics.ClassifierReport that every batch is also added to, from the same logits (one more
        tg_eval_report_f32 call per batch); None: the pass issues what it always did.
        ema: evaluate the averaged classifier — every trainable variable read from its EMA shadow (ParamStore.ema: decay 0.9999 per
        C-update, no bias correction), pop_mean / batch-norm moving statistics from the store as they are: what the reference's getter
        (nn.py:98-110) would have returned had it been passed, since ema.apply covered c_vars only.  The pass leaves no
        trace: it writes no store, draws from the Philox state without advancing it, and runs outside every prepared-filter cache."""
        cx, scores = self.cx, _Scores(report)
        for x, y in batches:
            with cx.phase_scope('val', record=False), self._classifier_weights(ema):
                self._score_batch(cx.from_numpy(x, key='val:x'), cx.from_numpy(y, key='val:y'), scores)
        return float(scores.accuracy) if scores.accuracy is not None else 0.0

    def _score_batch(self, x, y, scores, take=None):
        """Score one device batch with the classifier, inside the caller's phase (and its _classifier_weights): whiten the images x where
        the model whitens, classifier(x, False), then add the batch — its first `take` rows; None: all of it — to `scores` (_Scores):
        the streaming accuracy of the arg-max against the labels y (what _metric, :428-447, counts; its one-hot prediction output is
        not needed here), the report, the feature moments and the feature bank, in that order.
        The input noise is drawn under evaluate's Philox stream id whatever the caller's phase: ids are handed out in order of first
        use, and a pass that registered one of its own would shift those of a solver run that first runs later (the full step after
        pre-training)."""
        from tg import metrics as tgm
        cx, m = self.cx, self.model
        if m.zca() is not None:
            x = m.zca().apply(m.as_image(x))
        with cx.rng_scoped('val/C'):
            logits, fm = m.classifier(x, False)
        if take is not None:
            y, logits, fm = y.view_rows(0, take), logits.view_rows(0, take), fm.view_rows(0, take)
        scores.accuracy = self._accuracy_metric(y, logits, scores.accuracy)[0]
        if scores.report is not None:
            scores.report.add(y, logits, cx.stream)
        if scores.features:
            if scores.moments is None:
                scores.moments = tgm.FeatureMoments(fm.c, cx.device)
            scores.moments.add(fm, cx.stream)
            if scores.want_bank:
                if scores.bank is None:
                    scores.bank = tgm.FeatureBank(fm.c, cx.device)
                scores.bank.add(fm, cx.stream)

    @contextlib.contextmanager
    def _running_state_kept(self):
        """every store's `s` (pop_mean, batch-norm moving statistics) as it is on entry, put back on the way out: around a pass whose
        sampler — batch norms in training mode (reference :176-202) — moves them."""
        kept = {net: st.s.clone() for net, st in self.cx.stores.items()}
        try:
            yield
        finally:
            for net, s_before in kept.items():
                self.cx.stores[net].s.copy_(s_before)

    def _new_report(self):
        """an empty tg.metrics.ClassifierReport for this trainer's classifier."""
        from tg import metrics as tgm
        return tgm.ClassifierReport(self.options.num_classes, self.cx.device)

    def evaluate_report(self, batches, ema=False):
        """evaluate's pass with the per-class report on top -> the dict of tg.metrics.report_from_counts: confusion matrix,
        per-class recall / precision / F1, balanced accuracy, macro F1, top-5 accuracy, NLL, Brier score, ECE and the reliability table.
        One pass: its `accuracy` (trace / sum of the confusion matrix) is what evaluate returns on the same batches, bit for bit — the
        kernel takes both arg-maxes by tg_accuracy_count_f32's scan.  Leaves the trainer's state as evaluate leaves it."""
        report = self._new_report()
        self.evaluate(batches, ema=ema, report=report)
        return report.result()

    def _sample_latents(self, n_batches):
        """(z [n_batches * B, Z_DIM], y one-hot of class i % NUM_CLASSES) of sample_metrics: drawn once per trainer from a RandomState
        of its own seeded by config.SEED (NumPy's global state and the device Philox state are not touched), the same every epoch.  A
        longer request extends the draw; its head stays what it was."""
        c = self.config
        rows = n_batches * c.BATCH_SIZE_G
        if self._metric_latents is None or self._metric_latents[0].shape[0] < rows:
            rs = np.random.RandomState((int(self.options.seed) * 1000003 + 0x5A17) % (1 << 32))
            z = rs.uniform(low=-1.0, high=1.0, size=(rows, c.Z_DIM)).astype(np.float32)
            y = np.eye(c.NUM_CLASSES, dtype=np.float32)[np.arange(rows) % c.NUM_CLASSES]
            self._metric_latents = (z, y)
        z, y = self._metric_latents
        return z[:rows], y[:rows]

    def sample_metrics(self, batches, n_samples, ema=False):
        """Score the generator with the run's own classifier -> dict(val_accuracy, g_class_accuracy, frechet_distance,
        n_real, n_fake).
        Real side: ONE pass over `batches` exactly as evaluate makes it (raw weights, or the shadows with `ema`), which yields
        val_accuracy and the moments of the pooled feature `fm` (the classifier's second return value).
        Generated side: ceil(n_samples / BATCH_SIZE_G) batches of BATCH_SIZE_G fixed latents (_sample_latents; the generator's batch
        norms use batch statistics, so the batch size is part of the definition) through good_sampler, as_image, the model's ZCA and
        classifier(x, False); the first n_samples are scored.  g_class_accuracy: the share whose arg-max is the class asked for
        (tg_accuracy_count_f32).  frechet_distance: tg.metrics.frechet_distance between the two Gaussians fitted to the features
        (tg_feature_moments_f32 in fp64 on the device, the c x c algebra on the host); NaN with fewer than two rows on either side.
        The sampler's batch norms move their running statistics: every store's `s` is put back afterwards, and nothing else is
        written — weights, shadows, optimiser slots, step counters and the Philox state are what they were.  The pass runs under
        phases of its own ('metrics', 'metrics_g': unrecorded, buffer keys of their own), so no buffer a launch plan or graph names
        is touched.  Synchronises the device.
        sample_manifold_metrics is this pass with the k-nearest-neighbour metrics on top, sample_metrics_report with the per-class
        reports of both sides."""
        return self._sample_metrics_pass(batches, n_samples, ema, None)[0]

    def sample_metrics_report(self, batches, n_samples, ema=False, manifold_k=None):
        """sample_metrics (manifold_k None) or sample_manifold_metrics with the per-class report of each side on top ->
        their keys, then `val_report` and `g_report`, two tg.metrics.report_from_counts dicts: the real side's as evaluate_report gives
        it; the generated side's with the class asked for as target, over the n_samples rows that were scored — its per-class recall
        says which classes the generator fails to render.  The same pass with one more tg_eval_report_f32 call per batch; what
        sample_metrics says about the trainer's state holds unchanged.  A method of its own, as sample_manifold_metrics is: the
        parameter lists of those two are pinned by tests."""
        from tg import metrics as tgm
        if manifold_k is not None:
            manifold_k = tgm.check_k(manifold_k, 'sample_metrics_report: manifold_k')
        return self._sample_metrics_pass(batches, n_samples, ema, manifold_k, (self._new_report(), self._new_report()))[0]

    def sample_manifold_metrics(self, batches, n_samples, manifold_k, ema=False, return_banks=False):
        """sample_metrics plus the k-nearest-neighbour manifold metrics -> its five keys, then `precision`, `recall`,
        `density` and `coverage`.  manifold_k: the k of the radii, 1..16 (tg.metrics.check_k).
        The same two passes also keep their feature rows — every real one, the first n_samples generated ones — in a
        tg.metrics.FeatureBank each, and tg.metrics.manifold_metrics (tg_knn_self_f32 and tg_manifold_query_f32, twice each) turns the
        banks into the four numbers.  They are NaN, and the kernels are not called, when a side's moment sums are not finite (a
        diverged run) or a side has fewer than k + 1 rows.  The banks are buffers of their own and the kernels write nothing else:
        what sample_metrics says about the trainer's state holds unchanged.
        return_banks: return (result, (real bank, fake bank)) — the rows that were scored — instead of the result alone."""
        from tg import metrics as tgm
        manifold_k = tgm.check_k(manifold_k, 'sample_manifold_metrics: manifold_k')
        out, banks = self._sample_metrics_pass(batches, n_samples, ema, manifold_k)
        return (out, banks) if return_banks else out

    def _sample_metrics_pass(self, batches, n_samples, ema, manifold_k, reports=None):
        """the pass behind sample_metrics (manifold_k None), sample_manifold_metrics and sample_metrics_report -> (result, (real bank,
        fake bank) or None).  reports: None, or (real side, generated side) tg.metrics.ClassifierReport accumulators, either of which
        may be None: each is added the rows its side's accuracy counts, and the result carries `val_report` / `g_report` for those
        given."""
        from tg import metrics as tgm
        cx, m, c = self.cx, self.model, self.config
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError("sample_metrics: n_samples must be a positive integer, got %r" % (n_samples,))
        self._require_eager("sample_metrics", "eager pass beside the step")
        B = int(c.BATCH_SIZE_G)
        n_batches = -(-n_samples // B)
        z, y = self._sample_latents(n_batches)
        rep_real, rep_fake = reports if reports is not None else (None, None)
        real, fake = _Scores(rep_real, True, manifold_k is not None), _Scores(rep_fake, True, manifold_k is not None)
        with self._running_state_kept():
            for xb, yb in batches:
                with cx.phase_scope('metrics', record=False), self._classifier_weights(ema):
                    self._score_batch(cx.from_numpy(xb, key='metrics:x'), cx.from_numpy(yb, key='metrics:y'), real)
            for k in range(n_batches):
                with cx.phase_scope('metrics_g', record=False), self._classifier_weights(ema):
                    za = cx.from_numpy(z[k * B:(k + 1) * B], key='metrics:z')
                    yg = cx.from_numpy(y[k * B:(k + 1) * B], key='metrics:y_g')
                    self._score_batch(m.as_image(m.good_sampler(za, yg)), yg, fake, take=min(B, n_samples - k * B))
            seen = real.moments is not None                         # (a real side without batches: no moments, no bank)
            (n_real, sum_r, gram_r), (n_fake, sum_f, gram_f) = real.moments.sums() if seen else (0, None, None), fake.moments.sums()
            mu_r, cov_r = tgm.mean_cov(n_real, sum_r, gram_r) if seen else (None, None)
            mu_f, cov_f = tgm.mean_cov(n_fake, sum_f, gram_f)
            fd = tgm.frechet_distance(mu_r, cov_r, mu_f, cov_f) if n_real >= 2 and n_fake >= 2 else float('nan')
            out = dict(val_accuracy=float(real.accuracy) if real.accuracy is not None else 0.0, g_class_accuracy=float(fake.accuracy),
                       frechet_distance=fd, n_real=int(n_real), n_fake=int(n_fake))
            if manifold_k is not None:
                finite = seen and all(bool(np.isfinite(a).all()) for a in (sum_r, gram_r, sum_f, gram_f))
                out.update(tgm.manifold_metrics(real.bank, fake.bank, manifold_k, cx.stream) if finite
                           else dict.fromkeys(tgm.MANIFOLD_KEYS, float('nan')))
            if rep_real is not None:
                out['val_report'] = rep_real.result()
            if rep_fake is not None:
                out['g_report'] = rep_fake.result()
        return out, (None if manifold_k is None else (real.bank, fake.bank))

    def sync_running_state(self):
        """Replicas keep their own running statistics (pop_mean, batch-norm moving mean / variance) and EMA shadows while
        training; they are averaged over the replicas before evaluation and before a checkpoint is written."""
        if tgdist.active():
            for st in self.cx.stores.values():
                tgdist.allreduce_mean_(st.s)
                if st.ema is not None:
                    tgdist.allreduce_mean_(st.ema)

    def sample(self, sample_z, sample_y):
        """model.good_sampler on fixed latents (:68,353-364) -> host array [N,H,W,C] in [-1,1]."""
        cx = self.cx
        with cx.phase_scope('sample', record=False):
            out = self.model.good_sampler(cx.from_numpy(sample_z, key='smp:z'), cx.from_numpy(sample_y, key='smp:y'))
            return out.numpy().reshape([-1] + list(self.config.IMAGE_DIM))

    HISTOGRAM_BUFFERS = {'value': 'p', 'grad': 'g', 'ema': 'ema'}

    def histograms(self, which='value', nets=NETS):
        """tf.summary.histogram of every trainable variable of the networks `nets`: {TF variable name (as Saver spells it): {min, max, num,
        sum, sum_squares, limits, counts, nan, inf}} — TensorFlow's 1 551 bucket limits (shared array) and the count of every bucket,
        uncompressed; nan / inf count the non-finite elements, which are in no bucket and no statistic.
        which: 'value' (store.p), 'grad' (store.g: the gradient as the last iteration's optimiser READ it — summed over the replicas when
        there are several, before the 1/world scale and before any clip factor; a network whose solver did not run keeps its last one) or
        'ema' (the classifier's shadows; networks without one are skipped).
        One tg_tf_histogram_f32 call and ONE device->host copy per network.  Launched eagerly on the launch stream, outside the replayed
        step, and it only reads the stores: usable at any time, also while a launch plan or a hipGraph is held."""
        from tg import summary as tgsum
        if which not in self.HISTOGRAM_BUFFERS:
            raise ValueError("histograms: which must be one of %s, got %r" % (', '.join(repr(k) for k in self.HISTOGRAM_BUFFERS), which))
        self._require_eager("histograms", "eager launch beside the step")
        out = {}
        for net in nets:
            st = self.cx.stores[net]
            buf = getattr(st, self.HISTOGRAM_BUFFERS[which])
            if buf is None:
                continue
            names = st.names(True)
            key = (len(st.specs), st.n_p)
            run = self._hist_runs.get(net)
            if run is None or run[0] != key:
                run = self._hist_runs[net] = (key, tgsum.StoreHistograms([st.index[nm][1:3] for nm in names], self.cx.device))
            counts, stats = run[1].run(buf, self.cx.stream)
            out.update(tgsum.as_dicts(names, counts, stats))
        return out

    def _register_summaries(self, want_hist, want_img):
        """the reference's image / histogram keys (Summary.py:37-40) on the train summary, beside the scalars it already holds: the
        samples as 'generated', every trainable variable of D, G and C under its name and its gradient under 'gradients/<name>'."""
        c, sm = self.config, self.summary_train
        kinds = dict(scalar=dict.fromkeys(sm._tags)) if sm._tags else {}
        if want_img:
            kinds['image'] = {'generated': None}
        if want_hist:
            tags = [nm for net in NETS for nm in self.cx.stores[net].names(True)]
            kinds['histogram'] = dict.fromkeys(tags + ['gradients/' + nm for nm in tags])
        sm.add_summary(kinds)
        if want_img:                                     # (add_summary registers images with the reference's default max_outputs of 2)
            sm._image_outputs = sm._image_summary(kinds['image'], min(self.options.summary_image_max_outputs, int(c.SAMPLE_SIZE)))

    def _norm_tags(self):
        """the train summary's extra scalars: '<d|g|c>_grad_norm' for every clipped network (none without a clip)."""
        return tuple(k + '_grad_norm' for k, net in zip('dgc', NETS) if net in self._clip_views)

    def _tail_rows(self):
        """the epoch tail's extra records and val-summary scalars, in order, as (tag, result, key): the value of `tag` is `key` of the
        result dict named `result` that _tail_metrics gathers — 'sm', the sample-metrics pass (with config.EVAL_EMA alone: evaluate's
        pass over the shadows), or one of the report dicts 'val', 'val_ema', 'g' of self.last_reports.
        'val_accuracy_ema' with config.EVAL_EMA, 'g_class_accuracy' and 'frechet_distance' with config.SAMPLE_METRICS, then 'precision',
        'recall', 'density' and 'coverage' with config.SAMPLE_MANIFOLD_K (none with all off).  config.EVAL_REPORT appends, behind all of
        those, REPORT_TAGS with a 'val_' prefix ('val_top5_accuracy' only with more than five classes), with EVAL_EMA the same again
        with an '_ema' suffix, and with SAMPLE_METRICS 'g_worst_class_accuracy' (the generated side's target is the class asked for:
        recall = class accuracy)."""
        from tg import metrics as tgm
        o = self.options
        rows = [('val_accuracy_ema', 'sm', 'val_accuracy')] if o.eval_ema else []
        if o.sample_metrics:
            rows += [(k, 'sm', k) for k in ('g_class_accuracy', 'frechet_distance') + (tgm.MANIFOLD_KEYS if o.sample_manifold_k else ())]
        if o.eval_report:
            keys = self._report_keys()
            rows += [('val_' + k, 'val', k) for k in keys] + ([('val_' + k + '_ema', 'val_ema', k) for k in keys] if o.eval_ema else [])
            rows += [('g_worst_class_accuracy', 'g', 'worst_class_recall')] if o.sample_metrics else []
        return rows

    def _tail_metric_tags(self):
        """the tags of _tail_rows(), in order: what _tail_metrics returns a value for."""
        return tuple(tag for tag, _, _ in self._tail_rows())

    REPORT_TAGS = ('balanced_accuracy', 'macro_f1', 'nll', 'ece', 'top5_accuracy')

    def _report_keys(self):
        """the keys of an evaluation report that the epoch tail records: REPORT_TAGS, top-5 accuracy only where it is defined."""
        return tuple(k for k in self.REPORT_TAGS if k != 'top5_accuracy' or self.options.num_classes > 5)

    def _tail_metrics(self, NNIO, init_op_val, main_report=None):
        """{tag: value} of _tail_metric_tags() for this epoch tail, after sync_running_state: every replica computes the same numbers
        from the same averaged state, the same validation split and the same latents — no collective.  With both settings on, the
        averaged accuracy comes out of the metrics pass itself (its real side is evaluate's pass with the shadows): the split is run
        once for both.
        main_report (config.EVAL_REPORT): the ClassifierReport the epoch's evaluate pass filled.  The pass that reads the shadows
        and the generated side of the metrics pass fill one more each — no forward pass is added — and self.last_reports keeps the
        report dicts {'val', 'val_ema', 'g'} of those that ran."""
        o = self.options
        res = {'val': main_report.result()} if o.eval_report else {}
        if o.sample_metrics:
            init_op_val()
            # the pass of sample_metrics / sample_manifold_metrics; its real side reads the shadows only with EVAL_EMA, and only then
            # does its report differ from the main one
            pair = (self._new_report() if o.eval_ema else None, self._new_report()) if o.eval_report else None
            sm = res['sm'] = self._sample_metrics_pass(NNIO.val_batches(), o.sample_metrics, o.eval_ema, o.sample_manifold_k, pair)[0]
            if o.eval_report:
                res.update([('g', sm['g_report'])] + ([('val_ema', sm['val_report'])] if o.eval_ema else []))
        elif o.eval_ema:
            init_op_val()
            ema_report = self._new_report() if o.eval_report else None
            res['sm'] = dict(val_accuracy=self.evaluate(NNIO.val_batches(), ema=True, report=ema_report))
            if o.eval_report:
                res['val_ema'] = ema_report.result()
        if o.eval_report:
            self.last_reports = {k: res[k] for k in ('val', 'val_ema', 'g') if k in res}
        return {tag: res[name][key] for tag, name, key in self._tail_rows()}

    # ------------------------------------------------------------------ the reference's entry point
    def train(self, Dataset, Model, sample_y):
        """:43-381.  Dataset(data_dir, config, num_label, subset, use_augmentation).inputpipline_train_val(val)
        -> (init_op_train, init_op_val, NNIO); NNIO.next() yields the feed of one iteration, NNIO.val_batches()
        the test split."""
        c = self.config
        dataset_train = Dataset(c.DATA_DIR, c, c.NUM_LABEL, 'train', True)
        dataset_val = Dataset(c.DATA_DIR, c, c.NUM_LABEL, 'test', False)
        if isinstance(opt(c, 'ZCA'), str):                                             # 'fit': the constants, before the model first whitens
            check_zca(c, dataset_train)
            c.ZCA, self.zca_source = resolve_zca(c, dataset_train, self.rank, self.cx.device)
        init_op_train, init_op_val, NNIO = dataset_train.inputpipline_train_val(dataset_val)
        self._build_train_graph(Model)
        sample_z = np.random.uniform(low=-1.0, high=1.0, size=(c.SAMPLE_SIZE, c.Z_DIM)).astype(np.float32)   # :130
        lr, c_lr = c.LEARNING_RATE, cla_lr(c)
        start_epoch = 0
        saver = None
        wn_pending = self.options.wn_init == 'data'                                    # a restored run never re-initialises (below)
        if self.save_dir:
            from Training.Saver import Saver
            saver = Saver(self.save_dir)
            if c.RESTORE:                                                              # :140-147
                start_epoch = saver.restore(self, dir_names=c.RUN, epoch=c.RESTORE_EPOCH)
                wn_pending = False
                if start_epoch >= 300:
                    lr = lr * 0.995 ** (start_epoch - 300)
                    c_lr = c_lr * 0.99 ** (start_epoch - 300)
            elif self.rank == 0:
                saver.set_save_path(comments=self.comments)                            # :150
        if self.summary_train is not None and self.options.summary_scalar:             # :105-118
            self.summary_train.add_summary({'scalar': dict.fromkeys(('g_loss', 'd_loss', 'c_loss', 'train_accuracy') + self._norm_tags())})
            self.summary_val.add_summary({'scalar': dict.fromkeys(('val_accuracy',) + self._tail_metric_tags())})
        grid = bool(c.SAMPLE_DIR) and sample_y is not None                             # the sample grid: only for labels handed in
        if sample_y is None and self.summary_train is not None and self.options.summary_image:
            sample_y = np.eye(c.NUM_CLASSES, dtype=np.float32)[np.arange(c.SAMPLE_SIZE) % c.NUM_CLASSES]      # the entry points' cyclic ones
        history = []
        iters = int(c.TRAIN_SIZE / c.BATCH_SIZE)
        for epoch in range(1, c.EPOCHS + 1):
            lambda_1 = c.FAKE_G_LAMBDA if (start_epoch + epoch) > 200 else 0.          # :165
            lambda_2 = (0.5 if epoch > 67 else 0.) if self.model.CONSISTENCY else 0.                       # :171
            if start_epoch + epoch >= 300:                                             # :175-177
                lr, c_lr = lr * 0.995, c_lr * 0.99
            self.set_hyper(lr, c_lr, lambda_1, lambda_2)
            init_op_train()
            pre = bool(c.PRE_TRAIN and (start_epoch + epoch <= 30))                    # :182
            t0 = time.time()
            for i in range(iters):
                self.feed(NNIO.next())
                self.sample_latent()
                if wn_pending:                                                         # WN_INIT = 'data': on the first batch, which is
                    self.data_dependent_init()                                         # then iteration 1 as well
                    wn_pending = False
                self.train_iteration(pre_train=pre)
            torch.cuda.synchronize()
            dt = time.time() - t0
            d_loss, g_loss, c_loss = self.training_statistics() if iters > 0 else self.losses()        # :280-285
            init_op_val()
            self.sync_running_state()
            main_report = self._new_report() if self.options.eval_report else None    # EVAL_REPORT: filled by the same pass
            acc = self.evaluate(NNIO.val_batches()) if main_report is None else self.evaluate(NNIO.val_batches(), report=main_report)
            rec = dict(epoch=epoch + start_epoch, d_loss=d_loss, g_loss=g_loss, c_loss=c_loss, val_accuracy=acc,
                       images_per_sec=iters * c.BATCH_SIZE * self.world / dt)
            extra = self._tail_metrics(NNIO, init_op_val, main_report)                 # EVAL_EMA / SAMPLE_METRICS / EVAL_REPORT: {} with all off
            rec.update(extra)
            history.append(rec)
            samples = None
            if self.summary_train is not None:                                         # :293,346
                samples = self._write_epoch_summaries(rec, sample_z, sample_y, grid, first=epoch == 1)
            if saver is not None and self.rank == 0 and epoch % c.SAVE_PER_EPOCH == 0:  # :366-369
                saver.save(self, 'model_' + str(epoch + start_epoch).zfill(4) + '.ckpt')
            if self.rank == 0:
                print("epoch {epoch}: g_loss {g_loss:.3f} d_loss {d_loss:.3f} c_loss {c_loss:.3f} val_acc {val_accuracy:.4f} "
                      "{images_per_sec:.0f} img/s".format(**rec) + "".join(" %s %.4f" % (k, rec[k]) for k in extra), flush=True)
                if grid:
                    self._save_sample_grid(samples if samples is not None else self.sample(sample_z, sample_y), rec['epoch'])
        if saver is not None and self.rank == 0 and c.EPOCHS > 0:                      # :378-379 (after all epochs)
            saver.save(self, 'model_' + str(c.EPOCHS + start_epoch).zfill(4) + '.ckpt')
        return history

    def _write_epoch_summaries(self, rec, sample_z, sample_y, grid, first):
        """The summaries of one epoch tail (:293,346): the losses and the validation accuracy of `rec`, the last iteration's gradient norms
        of the clipped networks and, with config.SUMMARY_HISTOGRAM / SUMMARY_IMAGE, the histograms and the epoch's samples — which are
        returned (None without images) for the sample grid to reuse when one follows (`grid`).  first: this train() call's first tail."""
        o = self.options
        norms = self.grad_norms() if self._norm_tags() else {}
        hists = imgs = samples = None
        if first and (o.summary_histogram or o.summary_image):                         # at the first tail: by now every variable exists
            self._register_summaries(o.summary_histogram, o.summary_image)
        if o.summary_histogram:                                                        # values, and store.g as the last optimiser step read it
            hists = self.histograms('value')
            hists.update(('gradients/' + nm, h) for nm, h in self.histograms('grad').items())
        if o.summary_image:
            # The sampler's batch norms run in training mode (reference :176-202) and move their running statistics.  A run
            # without the flag samples only for the sample grid: when there is none, the statistics are put back, so the
            # summary leaves every store as it found it.
            with contextlib.nullcontext() if grid else self._running_state_kept():
                samples = self.sample(sample_z, sample_y)
            imgs = {'generated': samples}
        self.summary_train.write(dict(dict(g_loss=rec['g_loss'], d_loss=rec['d_loss'], c_loss=rec['c_loss']),
                                      **{k + '_grad_norm': v[0] for k, v in norms.items() if v is not None}), rec['epoch'],
                                 histograms=hists, images=imgs)
        self.summary_val.write(dict(dict(val_accuracy=rec['val_accuracy']), **{k: rec[k] for k in self._tail_metric_tags()}), rec['epoch'])
        if o.eval_report:                                                              # the matrices behind the scalars, int64 [K, K]
            for name, key in (('confusion', 'val'), ('g_confusion', 'g')):
                if key in self.last_reports:
                    np.save(os.path.join(self.summary_val.log_dir, '%s_%04d.npy' % (name, rec['epoch'])), self.last_reports[key]['confusion'])
        return samples

    def _save_sample_grid(self, samples, epoch):
        """:359-363: the epoch's samples as one image, SAMPLE_DIR/train_<epoch>.png."""
        from utils import save_images, image_manifold_size
        os.makedirs(self.config.SAMPLE_DIR, exist_ok=True)
        save_images(samples, image_manifold_size(samples.shape[0]), os.path.join(self.config.SAMPLE_DIR, 'train_{:02d}.png'.format(epoch)))


def rampup(epoch):
    """:456-462 (unused by the reference's loop; kept for API parity)."""
    if epoch < 300:
        p = 1.0 - max(0.0, float(epoch)) / float(300)
        return math.exp(-p * p * 5.0)
    return 1.0


def rampdown(epoch):
    """:464-469."""
    if epoch >= (300 - 50):
        ep = (epoch - (300 - 50)) * 0.5
        return math.exp(-(ep * ep) / 50)
    return 1.0


# ---------------------------------------------------------------------------------------------------------------------
# Experiment entry points (Training/Train_goodGAN.py:472-725).  Same TempConfig attribute values as the reference; the
# datasets / sample_y files of the reference are not part of its repository, so the synthetic Dataset (same protocol) and a
# cyclic sample_y are used unless a Dataset class is passed in.  SVHN / CIFAR-10 batch composition: the reference's own
# pipelines disagree with its placeholders; the consistent protocol is L_C / L_D / U_D+U_C per iteration.
# ---------------------------------------------------------------------------------------------------------------------

def _root_dir():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _customize_config(tmp_config, FLAGS):
    """:707-720: override config attributes from an argparse-like object."""
    for k in dir(FLAGS):
        v = getattr(FLAGS, k)
        if not k.startswith('_') and not callable(v) and v is not None and hasattr(tmp_config, k.upper()):
            setattr(tmp_config, k.upper(), v)


class ExperimentConfig(Config):
    """what the five experiments share; a subclass holds what differs.  The directories are relative to the package root (`_run` roots
    them at _root_dir() when the experiment is started), SAMPLE_DIR to Training/."""
    NAME = "Good_GAN"
    BATCH_SIZE_G = 100
    BATCH_SIZE_bG = 10
    BATCH_SIZE_L_C = 50
    BATCH_SIZE_U_C = 50
    BATCH_SIZE_L_D = 20                      # [x_l_d | x_u_d] is the discriminator's real batch, as large as the generated one
    BATCH_SIZE_U_D = 80
    BATCH_SIZE = BATCH_SIZE_G
    IMAGE_HEIGHT, IMAGE_WIDTH, CHANNEL = 32, 32, 3
    REPEAT = -1
    Z_DIM = 100
    NUM_CLASSES = 10
    MINIBATCH_DIS = False
    RESTORE = False                          # the reference resumes a run directory that is not in its repository (:588-592)
    LEARNING_RATE = 3e-4
    CLA_LEARNINIG_RATE = 3e-3
    FAKE_G_LAMBDA = 0.3
    EPOCHS = 1000
    SAVE_PER_EPOCH = 1
    VAL_STEP = None


class SvhnConfig(ExperimentConfig):
    DATA_NAME, DATA_DIR, NUM_LABEL = "svhn", "DataSet/svhn", 500
    BATCH_SIZE_bG = 20
    FAKE_G_LAMBDA = 0.03
    CLA_LEARNINIG_RATE = 3e-4
    TRAIN_SIZE = 73257 - NUM_LABEL
    SAMPLE_DIR, WEIGHT_DIR, LOG_DIR = "good_GAN_svhn_500", "Training/Weight_svhn", "Training/Log_svhn"


class Cifar10Config(ExperimentConfig):
    DATA_NAME, DATA_DIR, NUM_LABEL = "cifar10", "DataSet/cifar_10", 4000
    TRAIN_SIZE = 60000 - NUM_LABEL
    SAMPLE_DIR, WEIGHT_DIR, LOG_DIR = "cifar10_good_GAN_4000", "Training/Weight_cifar10", "Training/Log_cifar10"


class Cifar100Config(ExperimentConfig):
    DATA_NAME, DATA_DIR, NUM_LABEL = "cifar100", "DataSet/cifar_100", 10000
    NUM_CLASSES = 100
    TRAIN_SIZE = 50000 - NUM_LABEL
    SAMPLE_DIR, WEIGHT_DIR, LOG_DIR = "cifar100_good_GAN_10000", "Training/Weight_cifar100", "Training/Log_cifar100"


class MnistConfig(ExperimentConfig):
    DATA_NAME, DATA_DIR, NUM_LABEL = "mnist", "DataSet/mnist", 100
    BATCH_SIZE_bG = BATCH_SIZE_L_C = BATCH_SIZE_U_C = 100
    IMAGE_HEIGHT, IMAGE_WIDTH, CHANNEL = 28, 28, 1
    FAKE_G_LAMBDA = 0.1
    LEARNING_RATE = 1e-3
    CLA_LEARNINIG_RATE = 3e-4
    TRAIN_SIZE = 60000 - NUM_LABEL
    SAMPLE_DIR, WEIGHT_DIR, LOG_DIR = "mnist_good_GAN_100", "Training/Weight_mnist", "Training/Log_mnist"


class Stress64Config(ExperimentConfig):
    DATA_NAME, DATA_DIR, NUM_LABEL = "stress64", "DataSet/stress64", 4000
    BATCH_SIZE_G = 256
    BATCH_SIZE_L_C = BATCH_SIZE_U_C = 128
    BATCH_SIZE_L_D, BATCH_SIZE_U_D = 51, 205
    BATCH_SIZE = BATCH_SIZE_G
    IMAGE_HEIGHT, IMAGE_WIDTH, CHANNEL = 64, 64, 3
    TRAIN_SIZE = 60000 - NUM_LABEL
    SAMPLE_DIR, WEIGHT_DIR, LOG_DIR = "stress64_good_GAN", "Training/Weight_stress64", "Training/Log_stress64"


def _run(TempConfig, Model, Dataset, FLAGS, comments, epochs=None):
    from Input_Pipeline.syntheticDataset import syntheticDataset
    tmp_config = TempConfig()
    for k in ('DATA_DIR', 'WEIGHT_DIR', 'LOG_DIR'):
        setattr(tmp_config, k, os.path.join(_root_dir(), getattr(tmp_config, k)))
    _synthetic_zca(tmp_config)                                         # a default like the class body's: FLAGS below override it
    if FLAGS:
        _customize_config(tmp_config, FLAGS)
        # --wn-init data, --eval-ema, --sample-metrics N, --sample-manifold-k K, --eval-report: Config does not declare these settings, so
        # the hasattr rule of _customize_config would drop them (Training/options.check_wn_init ... check_eval_report).  Flag objects
        # without the attribute are common: getattr with a default
        for name in Options.EXTRAS:
            if getattr(FLAGS, name, None) is not None:
                setattr(tmp_config, name.upper(), getattr(FLAGS, name))
    if epochs is not None:
        tmp_config.EPOCHS = epochs
    tmp_config.SAMPLE_DIR = os.path.join(_root_dir(), "Training", tmp_config.SAMPLE_DIR)
    if tmp_config.NUM_LABEL < 1000:
        tmp_config.PRE_TRAIN = True                                    # :537-538,614-615
    check_zca(tmp_config, Dataset or syntheticDataset)                 # --zca fit: before any device work
    tmp_config.display()
    training = Train(tmp_config, tmp_config.LOG_DIR, tmp_config.WEIGHT_DIR, comments=comments + tmp_config.config_str())
    sample_y = np.eye(tmp_config.NUM_CLASSES, dtype=np.float32)[np.arange(tmp_config.SAMPLE_SIZE) % tmp_config.NUM_CLASSES]
    return training.train(Dataset or syntheticDataset, Model, sample_y)


def _main_training_svhn(FLAGS=None, Dataset=None, epochs=None):
    """:472-549."""
    from Model.Good_GAN import Good_GAN as Model
    return _run(SvhnConfig, Model, Dataset, FLAGS, "This training is for svhn dataset.", epochs)


def _main_training_cifar10(FLAGS=None, Dataset=None, epochs=None):
    """:551-626.  config.ZCA must carry (mean, mat) when DATA_DIR holds no cifar10_zca_*.npy, or be 'fit' (--zca fit, with a TFRecord
    Dataset): fitted from the training split and written there; without either, _synthetic_zca."""
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10 as Model
    return _run(Cifar10Config, Model, Dataset, FLAGS, "This training is for cifar10 dataset.", epochs)


def _main_training_cifar100(FLAGS=None, Dataset=None, epochs=None):
    """CIFAR-100 (not an entry point of the reference): the networks and algorithm of _main_training_cifar10 with NUM_CLASSES = 100, so the
    classifier heads run the general-K kernels (csrc/loss.hip).  ZCA as for CIFAR-10, with cifar100_zca_*.npy."""
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10 as Model
    return _run(Cifar100Config, Model, Dataset, FLAGS, "This training is for cifar100 dataset.", epochs)


def _main_training_mnist(FLAGS=None, Dataset=None, epochs=None):
    """:628-705."""
    from Model.Good_GAN import Good_GAN as Model
    return _run(MnistConfig, Model, Dataset, FLAGS, "This training is for mnist dataset.", epochs)


def _main_training_stress64(FLAGS=None, Dataset=None, epochs=None):
    """Build-defined 64x64x3 / batch-256 stress configuration (not in the reference)."""
    from Model.Good_GAN_stress64 import Good_GAN_stress64 as Model
    return _run(Stress64Config, Model, Dataset, FLAGS, "64x64 stress configuration.", epochs)


if __name__ == "__main__":
    # :722-725 — the reference launches the MNIST experiment
    _main_training_mnist()
