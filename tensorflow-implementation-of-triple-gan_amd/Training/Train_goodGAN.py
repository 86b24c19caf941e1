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
import math
import os
import time

import numpy as np
import torch

from config import Config
from Model.zca import resolve_zca, synthetic_zca as _synthetic_zca         # (tools/ reach the synthetic rotation under this name)
from Training.epoch_tail import EpochTail
from Training.evaluation import Evaluation
from Training.options import (LOSSES, NETS, NUM_CLASSES_RANGE, OPTIMIZERS, Options, check_act_dtype, check_clip_norm, check_eval_ema,  # noqa: F401
                              check_eval_report, check_loss, check_mfma_dtype, check_num_classes, check_optimizer, check_r1_gamma,
                              check_sample_manifold_k, check_sample_metrics, check_sample_nearest, check_wn_init, check_zca, cla_lr, opt,
                              resolve)
from Training.schedule import epoch_schedule
from Training.train_base import Train_base, clip_workspace_floats
from tg import dist as tgdist
from tg import executor, lib, ops
from tg.batching import concat_acts
from tg.runtime import Act, Context, PhiloxRNG, ctx, set_context

# The placeholders of the training graph (:400-413), in the order of Model.forward_pass's arguments: (feed key, the config attribute
# that holds its batch size, what it holds).  What it holds decides a row's dimensions: see _build_train_graph.
PLACEHOLDERS = (('z_g', 'BATCH_SIZE_G', 'latent'), ('y_g', 'BATCH_SIZE_G', 'labels'),
                ('x_l_c', 'BATCH_SIZE_L_C', 'image'), ('y_l_c', 'BATCH_SIZE_L_C', 'labels'),
                ('x_l_d', 'BATCH_SIZE_L_D', 'image'), ('y_l_d', 'BATCH_SIZE_L_D', 'labels'),
                ('x_u_d', 'BATCH_SIZE_U_D', 'image'), ('x_u_c', 'BATCH_SIZE_U_C', 'image'))


class Train(Evaluation, EpochTail, Train_base):
    """The trainer: the device state of a run, the three solver runs and the reference's epoch loop.  Its forward-only scoring passes
    are Training/evaluation.py, what follows an epoch's iterations Training/epoch_tail.py, the epoch schedule Training/schedule.py."""

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
        self._gp_w = self._gp_grad = None            # WGAN-GP / R1: the D-update's weighted penalty and its parameter gradient (device)
        # config.R1_GAMMA: [gamma] on the device, read by the penalty kernel — None with the option off, and nothing else
        # of R1 exists then; _r1_out: the in-step penalty's {R1, mean_i ||g_i||^2}, at its call site of phase D
        self.r1_dev = self._r1_out = None
        cx.bf16_act_layers = set()
        # device-resident hyper-parameters (the reference's lr_ph / cla_lr_ph / lambda placeholders, :30-31,416-420)
        self.hyper = torch.zeros(4, dtype=torch.float32, device=cx.device)       # lr, cla_lr, lambda_1, lambda_2
        self.loss_dev = torch.zeros(3, dtype=torch.float32, device=cx.device)    # d_loss, g_loss, c_loss
        if o.r1_gamma is not None:
            self.r1_dev = torch.full((1,), o.r1_gamma, dtype=torch.float32, device=cx.device)
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
        self._nearest = {}               # {'pixel': nearest_training()'s resident training bytes, labels and kept controls}
        self._dataset_train = None       # the training Dataset of train(): what the epoch tail's nearest_training() searches
        self.last_reports = {}           # config.EVAL_REPORT: the last epoch tail's report dicts {'val', 'val_ema', 'g'} (_tail_metrics)
        self.last_kid_per_class = None   # config.SAMPLE_KID = 'per_class': the last tail's kernel_distance_per_class, float64 [NUM_CLASSES]
        self.last_nearest = None         # config.SAMPLE_NEAREST: (result, (query bank, training bank)) of the last tail's nearest_training
        self.nearest_decoded = 0         # training records nearest_training has decoded so far (Evaluation._training_pixels: once)
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
        shapes = dict(latent=[c.Z_DIM], labels=[c.NUM_CLASSES], image=c.IMAGE_DIM)

        def ph(key, n, shape):
            t = cx.ws('ph:' + key, n * int(np.prod(shape)))
            return Act(t, n, *(shape if len(shape) == 3 else (1, 1, shape[0])), ld=shape[-1])

        # the eight Acts in PLACEHOLDERS' order; each is self.<key>_ph as well.  feed and training_statistics read the list, the step
        # reads the attributes: the two name the same Acts and neither is rebound after the build
        self.placeholders = []
        for key, size, holds in PLACEHOLDERS:
            self.placeholders.append(ph(key, getattr(c, size), shapes[holds]))
            setattr(self, key + '_ph', self.placeholders[-1])
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
        PH = self.placeholders + [True, self.hyper[2:4]]
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

    def set_r1_gamma(self, gamma):
        """a new R1 weight, written to the device like set_hyper: a replayed plan or graph follows.  Only for a trainer built with
        config.R1_GAMMA — without it the recorded launches hold no penalty."""
        if self.r1_dev is None:
            raise lib.TgError("set_r1_gamma: this trainer was built with R1_GAMMA = None; the penalty is part of the recorded launches")
        if isinstance(gamma, bool) or not 0.0 < float(gamma) < float('inf'):
            raise lib.TgError("set_r1_gamma: gamma must be a positive finite number, got %r" % (gamma,))
        self.r1_dev.fill_(float(gamma))

    def r1_terms(self):
        """{'penalty': gamma / 2 * mean_i ||g_i||^2, 'grad_sq_mean': mean_i ||g_i||^2} of the last D-update as floats — ONE device->host
        copy; zeros before the first D-update.  lib.TgError for a trainer built with R1_GAMMA = None."""
        if self.r1_dev is None:
            raise lib.TgError("r1_terms: this trainer was built with R1_GAMMA = None")
        if self._r1_out is None:
            return dict(penalty=0.0, grad_sq_mean=0.0)
        v = self._r1_out[:2].detach().cpu().numpy()
        return dict(penalty=float(v[0]), grad_sq_mean=float(v[1]))

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
            if self.r1_dev is not None:
                # R1 at the rows the head counts as real, X_P with [y_l_d | oh_unl_d]: the labels are this run's classifier's (after the
                # override), so the penalty cannot go beside the classifier's forward pass as WGAN-GP's does.  With the side stream it
                # goes beside the discriminator's forward pass (it reads the batch and the weights, and writes buffers of its own call
                # sites only) and is joined before the head adds it; without one (eager, graph) it is on the chain
                n_real = c.BATCH_SIZE_L_D + c.BATCH_SIZE_U_D
                with cx.wgrad_on_side():
                    self._gp_w, self._gp_grad = m.discriminator_r1_penalty(ximg.view_rows(0, n_real), yall.view_rows(0, n_real), self.r1_dev,
                                                                           in_step=True)
                self._r1_out = m.last_gp_state['out']
            with cx.rng_scoped('D/D'):
                _, d_logits = m.discriminator(ximg, yall, want_prob=False)
            if self.r1_dev is not None:
                cx.join_wgrad_side()
            if wgan:
                self._wgan_d_head(d_logits, c.BATCH_SIZE_L_D + c.BATCH_SIZE_U_D, c.BATCH_SIZE_G, c.BATCH_SIZE_U_C, self.hyper[2:4], self._gp_w,
                                  self.loss_dev[0:1])
            else:
                self._d_loss(d_logits, c.BATCH_SIZE_L_D + c.BATCH_SIZE_U_D, c.BATCH_SIZE_G, c.BATCH_SIZE_U_C, self.loss_dev[0:1])
                if self.r1_dev is not None:              # d_loss += R1, on the device
                    lib.call('tg_add_f32', lib.ptr(self.loss_dev[0:1]), lib.ptr(self.loss_dev[0:1]), lib.ptr(self._gp_w), 1, cx.stream)
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
        """WGAN-GP / R1: add the penalty's parameter gradient to the slice `sl` of the discriminator's store.g, once the D backward pass has
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
        if net == 'discriminator' and (self.loss_kind == 'WGAN_GP' or self.r1_dev is not None):       # the D-update has a penalty
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
        for (key, _, _), ph in zip(PLACEHOLDERS, self.placeholders):
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
            G, D, C = self.model.forward_pass(*self.placeholders, True)                                        # :422
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

    def sync_running_state(self):
        """Replicas keep their own running statistics (pop_mean, batch-norm moving mean / variance) and EMA shadows while
        training; they are averaged over the replicas before evaluation and before a checkpoint is written."""
        if tgdist.active():
            for st in self.cx.stores.values():
                tgdist.allreduce_mean_(st.s)
                if st.ema is not None:
                    tgdist.allreduce_mean_(st.ema)

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
        check_sample_nearest(c, dataset_train)                                         # SAMPLE_NEAREST: a TFRecord training split
        self._dataset_train = dataset_train
        init_op_train, init_op_val, NNIO = dataset_train.inputpipline_train_val(dataset_val)
        self._build_train_graph(Model)
        sample_z = np.random.uniform(low=-1.0, high=1.0, size=(c.SAMPLE_SIZE, c.Z_DIM)).astype(np.float32)   # :130
        saver, start_epoch = self._open_run()
        wn_pending = self.options.wn_init == 'data'
        if saver is not None and c.RESTORE:                                            # a restored run never re-initialises
            wn_pending = False
        if self.summary_train is not None and self.options.summary_scalar:             # :105-118
            self.summary_train.add_summary({'scalar': dict.fromkeys(('g_loss', 'd_loss', 'c_loss', 'train_accuracy') + self._norm_tags())})
            self.summary_val.add_summary({'scalar': dict.fromkeys(('val_accuracy',) + self._tail_metric_tags())})
        grid = bool(c.SAMPLE_DIR) and sample_y is not None                             # the sample grid: only for labels handed in
        if sample_y is None and self.summary_train is not None and self.options.summary_image:
            sample_y = np.eye(c.NUM_CLASSES, dtype=np.float32)[np.arange(c.SAMPLE_SIZE) % c.NUM_CLASSES]      # the entry points' cyclic ones
        history = []
        iters = int(c.TRAIN_SIZE / c.BATCH_SIZE)
        for epoch, now in zip(range(1, c.EPOCHS + 1), epoch_schedule(c, self.model.CONSISTENCY, start_epoch)):
            self.set_hyper(now.lr, now.cla_lr, now.lambda_1, now.lambda_2)
            init_op_train()
            t0 = time.time()
            for i in range(iters):
                self.feed(NNIO.next())
                self.sample_latent()
                if wn_pending:                                                         # WN_INIT = 'data': on the first batch, which is
                    self.data_dependent_init()                                         # then iteration 1 as well
                    wn_pending = False
                self.train_iteration(pre_train=now.pre_train)
            torch.cuda.synchronize()
            dt = time.time() - t0
            history.append(self._epoch_tail(NNIO, init_op_val, epoch, start_epoch, iters, dt, sample_z, sample_y, grid, saver))
        if saver is not None and self.rank == 0 and c.EPOCHS > 0:                      # :378-379 (after all epochs)
            saver.save(self, 'model_' + str(c.EPOCHS + start_epoch).zfill(4) + '.ckpt')
        return history

    def _open_run(self):
        """the run directory of this train() call (:139-150) -> (saver, start_epoch): with config.RESTORE the state of the run
        config.RUN / config.RESTORE_EPOCH is read back and start_epoch is the number of epochs behind it; else rank 0 names a new run
        directory and start_epoch is 0.  (None, 0) without a save_dir."""
        c = self.config
        if not self.save_dir:
            return None, 0
        from Training.Saver import Saver
        saver, start_epoch = Saver(self.save_dir), 0
        if c.RESTORE:                                                                  # :140-147
            start_epoch = saver.restore(self, dir_names=c.RUN, epoch=c.RESTORE_EPOCH)
        elif self.rank == 0:
            saver.set_save_path(comments=self.comments)                                # :150
        return saver, start_epoch


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
        # --wn-init data, --r1-gamma X, --eval-ema, --sample-metrics N, --sample-manifold-k K, --eval-report, --sample-kid [per_class],
        # --sample-nearest K: Config does not declare these settings, so the hasattr rule of _customize_config would drop them
        # (Training/options.check_wn_init, check_r1_gamma ... check_sample_nearest).  Flag objects without the attribute are common: getattr with a default
        for name in Options.EXTRAS:
            if getattr(FLAGS, name, None) is not None:
                setattr(tmp_config, name.upper(), getattr(FLAGS, name))
    if epochs is not None:
        tmp_config.EPOCHS = epochs
    tmp_config.SAMPLE_DIR = os.path.join(_root_dir(), "Training", tmp_config.SAMPLE_DIR)
    if tmp_config.NUM_LABEL < 1000:
        tmp_config.PRE_TRAIN = True                                    # :537-538,614-615
    check_zca(tmp_config, Dataset or syntheticDataset)                 # --zca fit: before any device work
    check_sample_nearest(tmp_config, Dataset or syntheticDataset)      # --sample-nearest K: it needs a training split to search
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
