"""EpochTail — what Train.train() does after an epoch's iterations (reference Training/Train_goodGAN.py:280-369): the statistics pass, the
validation passes and their extra metric rows, the summaries with histograms and images, the periodic checkpoint, the log line and the
sample grid.  Train (Training/Train_goodGAN.py) inherits it.

_epoch_tail is the whole tail in the reference's order; the other methods are its parts, usable on their own (histograms by tools and
tests at any time).  The tail calls the trainer's training_statistics, sync_running_state, grad_norms and the scoring passes of
Training/evaluation.py, and reads config, options, cx.stores, _clip_views, rank, world and the two Summary writers.  It OWNS four
attributes, set by Train.__init__: `last_reports` (the report dicts of the last tail), `last_kid_per_class` (config.SAMPLE_KID =
'per_class': the last tail's per-class kernel distances), `last_nearest` (config.SAMPLE_NEAREST: the last tail's nearest_training
result and its two banks) and `_hist_runs` (the histogram launches per network).  Apart from what
training_statistics moves — as the reference's run does — it leaves the training state alone."""
import contextlib
import os

import numpy as np

from Training.options import NETS
from tg import metrics as tgm
from tg import summary as tgsum


NEAREST_GRID_ROWS = 16


def write_nearest_grid(path, nn_idx, fake, train, image_dim, rows=NEAREST_GRID_ROWS):
    """Train.nearest_training's pixel result as one PNG (the epoch tail's SAMPLE_DIR/nearest_<epoch>.png, tools/nearest_training.py):
    one row for each of the first min(rows, N) samples — the sample, as the bytes that were compared, then its k nearest training
    images, nearest first (a black cell where the training split has fewer than k images).  nn_idx: int32 [N, k]; fake, train: the
    tg.metrics.PixelBank pair the distances were taken between."""
    import torch
    from utils import merge, write_png
    h, w, ch = (int(v) for v in image_dim)
    rows = min(int(rows), fake.n)
    idx = np.asarray(nn_idx)[:rows]
    cells = np.zeros((rows, 1 + idx.shape[1], h, w, ch), np.uint8)
    cells[:, 0] = fake.rows(0, rows).cpu().numpy().reshape(rows, h, w, ch)
    pick = torch.from_numpy(np.maximum(idx, 0).reshape(-1).astype(np.int64)).to(train.device)
    near = train.rows()[pick].cpu().numpy().reshape(rows, idx.shape[1], h, w, ch)
    cells[:, 1:] = np.where((idx >= 0)[:, :, None, None, None], near, 0)
    write_png(path, merge(cells.reshape((-1, h, w, ch)) / 255.0, (rows, 1 + idx.shape[1])))


class EpochTail(object):
    def _epoch_tail(self, NNIO, init_op_val, epoch, start_epoch, iters, dt, sample_z, sample_y, grid, saver):
        """the tail of epoch `epoch` of this train() call (`start_epoch` epochs lie before it), whose `iters` iterations took `dt`
        seconds -> the epoch's record.  NNIO / init_op_val: the input pipeline and its switch to the validation split; sample_z,
        sample_y: the fixed latents of the image summary and of the sample grid (`grid`: write one); saver: a Saver or None."""
        c = self.config
        d_loss, g_loss, c_loss = self.training_statistics() if iters > 0 else self.losses()        # :280-285
        init_op_val()
        self.sync_running_state()
        main_report = self._new_report() if self.options.eval_report else None    # EVAL_REPORT: filled by the same pass
        acc = self.evaluate(NNIO.val_batches()) if main_report is None else self.evaluate(NNIO.val_batches(), report=main_report)
        rec = dict(epoch=epoch + start_epoch, d_loss=d_loss, g_loss=g_loss, c_loss=c_loss, val_accuracy=acc,
                   images_per_sec=iters * c.BATCH_SIZE * self.world / dt)
        if self.options.r1_gamma:                                                  # R1_GAMMA: the last D-update's penalty
            rec['d_r1'] = self.r1_terms()['penalty']
        extra = self._tail_metrics(NNIO, init_op_val, main_report)                 # EVAL_EMA / SAMPLE_METRICS / EVAL_REPORT: {} with all off
        rec.update(extra)
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
            if self.options.sample_nearest and c.SAMPLE_DIR:
                self._save_nearest_grid(rec['epoch'])
        return rec

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
        """the train summary's extra scalars: '<d|g|c>_grad_norm' for every clipped network (none without a clip), then 'd_r1' with
        config.R1_GAMMA."""
        return tuple(k + '_grad_norm' for k, net in zip('dgc', NETS) if net in self._clip_views) + (('d_r1',) if self.options.r1_gamma else ())

    def _tail_rows(self):
        """the epoch tail's extra records and val-summary scalars, in order, as (tag, result, key): the value of `tag` is `key` of the
        result dict named `result` that _tail_metrics gathers — 'sm', the sample-metrics pass (with config.EVAL_EMA alone: evaluate's
        pass over the shadows), or one of the report dicts 'val', 'val_ema', 'g' of self.last_reports.
        'val_accuracy_ema' with config.EVAL_EMA, 'g_class_accuracy' and 'frechet_distance' with config.SAMPLE_METRICS, then 'precision',
        'recall', 'density' and 'coverage' with config.SAMPLE_MANIFOLD_K (none with all off).  config.EVAL_REPORT appends, behind all of
        those, REPORT_TAGS with a 'val_' prefix ('val_top5_accuracy' only with more than five classes), with EVAL_EMA the same again
        with an '_ema' suffix, and with SAMPLE_METRICS 'g_worst_class_accuracy' (the generated side's target is the class asked for:
        recall = class accuracy).  config.SAMPLE_KID appends 'kernel_distance' and, as 'per_class', 'kernel_distance_worst'
        (Train.sample_kernel_distance).  config.SAMPLE_NEAREST appends, last of all, 'g_nn_rmse', 'g_nn_rmse_min',
        'g_nn_class_agreement' and 'val_nn_rmse' (Train.nearest_training)."""
        o = self.options
        rows = [('val_accuracy_ema', 'sm', 'val_accuracy')] if o.eval_ema else []
        if o.sample_metrics:
            rows += [(k, 'sm', k) for k in ('g_class_accuracy', 'frechet_distance') + (tgm.MANIFOLD_KEYS if o.sample_manifold_k else ())]
        if o.eval_report:
            keys = self._report_keys()
            rows += [('val_' + k, 'val', k) for k in keys] + ([('val_' + k + '_ema', 'val_ema', k) for k in keys] if o.eval_ema else [])
            rows += [('g_worst_class_accuracy', 'g', 'worst_class_recall')] if o.sample_metrics else []
        if o.sample_kid:                                # config.SAMPLE_KID: behind the report rows, out of the same 'sm' pass
            rows += [(k, 'sm', k) for k in ('kernel_distance',) + (('kernel_distance_worst',) if o.sample_kid == 'per_class' else ())]
        if o.sample_nearest:                            # config.SAMPLE_NEAREST: behind every other row (result 'nn': nearest_training)
            rows += [(k, 'nn', k) for k in self.NEAREST_KEYS]
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
            # (the keyword is passed only with config.SAMPLE_KID: with it off the call is what it was)
            kid = dict(kernel_distance=o.sample_kid) if o.sample_kid else {}
            sm = res['sm'] = self._sample_metrics_pass(NNIO.val_batches(), o.sample_metrics, o.eval_ema, o.sample_manifold_k, pair, **kid)[0]
            if o.sample_kid == 'per_class':
                self.last_kid_per_class = sm['kernel_distance_per_class']
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
        if o.sample_nearest:
            # the nearest training images of the samples that pass scored (same latents, same batch-norm rule), against the training
            # split train() opened; last_nearest keeps the result and the two banks for the grid
            init_op_val()
            self.last_nearest = self.nearest_training(self._dataset_train, NNIO.val_batches(), o.sample_metrics, o.sample_nearest,
                                                      return_banks=True)
            res['nn'] = self.last_nearest[0]
        return {tag: res[name][key] for tag, name, key in self._tail_rows()}

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
                                      **dict({k + '_grad_norm': v[0] for k, v in norms.items() if v is not None},
                                             **({'d_r1': rec['d_r1']} if 'd_r1' in rec else {}))), rec['epoch'],
                                 histograms=hists, images=imgs)
        self.summary_val.write(dict(dict(val_accuracy=rec['val_accuracy']), **{k: rec[k] for k in self._tail_metric_tags()}), rec['epoch'])
        if o.eval_report:                                                              # the matrices behind the scalars, int64 [K, K]
            for name, key in (('confusion', 'val'), ('g_confusion', 'g')):
                if key in self.last_reports:
                    np.save(os.path.join(self.summary_val.log_dir, '%s_%04d.npy' % (name, rec['epoch'])), self.last_reports[key]['confusion'])
        if o.sample_kid == 'per_class':                                                # the per-class distances behind the worst one, float64 [K]
            np.save(os.path.join(self.summary_val.log_dir, 'kid_per_class_%04d.npy' % rec['epoch']), self.last_kid_per_class)
        return samples

    def _save_nearest_grid(self, epoch):
        """config.SAMPLE_NEAREST: SAMPLE_DIR/nearest_<epoch>.png from the last tail's nearest_training (write_nearest_grid)."""
        out, (fake, train) = self.last_nearest
        os.makedirs(self.config.SAMPLE_DIR, exist_ok=True)
        write_nearest_grid(os.path.join(self.config.SAMPLE_DIR, 'nearest_{:04d}.png'.format(epoch)), out['nn_idx'], fake, train,
                           self.config.IMAGE_DIM)

    def _save_sample_grid(self, samples, epoch):
        """:359-363: the epoch's samples as one image, SAMPLE_DIR/train_<epoch>.png."""
        from utils import save_images, image_manifold_size
        os.makedirs(self.config.SAMPLE_DIR, exist_ok=True)
        save_images(samples, image_manifold_size(samples.shape[0]), os.path.join(self.config.SAMPLE_DIR, 'train_{:02d}.png'.format(epoch)))
