"""Evaluation — the trainer's forward-only scoring passes: evaluate, the per-class report, the generated-sample, manifold and kernel-distance
metrics, and the sampler.  Train (Training/Train_goodGAN.py) inherits it; the methods are used as `Train.<method>`.

The contract, once for all of them.  These passes READ from the trainer

    cx                 the device context: stores, phases, Philox scopes, buffers keyed per pass
    model              classifier, good_sampler, as_image, zca
    config, options    batch sizes and dimensions; seed, class count
    _accuracy_metric   the streaming accuracy of Train_base
    _require_eager     refuses a pass inside a hipGraph capture / launch-plan recording

and OWN `_metric_latents` (the fixed latents of sample_metrics) and `_nearest` / `nearest_decoded` (nearest_training's resident
training bytes and cached control, and the records decoded for them), all set by Train.__init__.  They write no store:
no weight, shadow, optimiser slot or step counter, and the Philox state is not advanced.  The one exception is every store's `s`
(pop_mean, batch-norm moving statistics), which a sampler pass moves and _running_state_kept puts back."""
import contextlib

import numpy as np

from tg import metrics as tgm


class _Scores(object):
    """what Train._score_batch adds a scored batch to: the streaming accuracy, a tg.metrics.ClassifierReport (handed in, or None) and —
    features — the tg.metrics.FeatureMoments of the classifier's pooled feature plus, bank, a tg.metrics.FeatureBank of its rows; those
    two are sized by the first feature seen and stay None on a side that saw no batch."""

    def __init__(self, report=None, features=False, bank=False):
        self.report, self.features, self.want_bank = report, features, bank
        self.accuracy = self.moments = self.bank = None


class Evaluation(object):
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

    def sample_kernel_distance(self, batches, n_samples, ema=False, per_class=False, return_banks=False):
        """sample_metrics plus the unbiased kernel distance of the generated samples -> its five keys, then
        `kernel_distance`: the cubic-kernel MMD^2 (the "Kernel Inception Distance" of Binkowski et al. 2018) between the pooled
        features of the real and the generated rows, unbiased at any sample count (and so possibly negative).  per_class adds
        `kernel_distance_per_class` (float64 [NUM_CLASSES]: the same estimator between the rows of each class — the real side's by
        its label, the generated side's by the class asked for — NaN where a class has fewer than two rows on either side),
        `kernel_distance_worst` (its largest non-NaN entry) and `kernel_distance_worst_class` (the lowest index attaining it, -1
        if there is none): which class's samples are distributed least like that class.
        The same two passes keep their feature rows in a tg.metrics.FeatureBank each, as sample_manifold_metrics does, and
        tg.metrics.kernel_distance (tg_poly3_sums_f32: three launches, with per_class three more over the class segments) turns
        them into the numbers; the labels are the host arg-max of the one-hot rows the pass already holds.  They are NaN, and the
        kernel is not called, when a side's moment sums are not finite (a diverged run).  The banks are buffers of their own and
        the kernel writes nothing else: what sample_metrics says about the trainer's state holds unchanged.  A method of its own:
        the parameter lists and result keys of sample_metrics, sample_manifold_metrics and sample_metrics_report are pinned by tests.
        The extractor is the run's own classifier, which moves: compare generators under one classifier, not epochs.
        return_banks: return (result, (real bank, fake bank)) — the rows that were scored — instead of the result alone."""
        out, banks = self._sample_metrics_pass(batches, n_samples, ema, None, kernel_distance='per_class' if per_class else True)
        return (out, banks) if return_banks else out

    def sample_metrics_report(self, batches, n_samples, ema=False, manifold_k=None):
        """sample_metrics (manifold_k None) or sample_manifold_metrics with the per-class report of each side on top ->
        their keys, then `val_report` and `g_report`, two tg.metrics.report_from_counts dicts: the real side's as evaluate_report gives
        it; the generated side's with the class asked for as target, over the n_samples rows that were scored — its per-class recall
        says which classes the generator fails to render.  The same pass with one more tg_eval_report_f32 call per batch; what
        sample_metrics says about the trainer's state holds unchanged.  A method of its own, as sample_manifold_metrics is: the
        parameter lists of those two are pinned by tests."""
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
        manifold_k = tgm.check_k(manifold_k, 'sample_manifold_metrics: manifold_k')
        out, banks = self._sample_metrics_pass(batches, n_samples, ema, manifold_k)
        return (out, banks) if return_banks else out

    def _sample_metrics_pass(self, batches, n_samples, ema, manifold_k, reports=None, *, kernel_distance=None):
        """the pass behind sample_metrics (manifold_k None), sample_manifold_metrics, sample_metrics_report and
        sample_kernel_distance -> (result, (real bank, fake bank) or None).  reports: None, or (real side, generated side)
        tg.metrics.ClassifierReport accumulators, either of which may be None: each is added the rows its side's accuracy counts, and
        the result carries `val_report` / `g_report` for those given.  kernel_distance: None / False (off), True or 'per_class' — the
        result also carries tg.metrics.kernel_distance of the two banks, with 'per_class' over the classes of the rows' labels."""
        cx, m, c = self.cx, self.model, self.config
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError("sample_metrics: n_samples must be a positive integer, got %r" % (n_samples,))
        self._require_eager("sample_metrics", "eager pass beside the step")
        B = int(c.BATCH_SIZE_G)
        n_batches = -(-n_samples // B)
        z, y = self._sample_latents(n_batches)
        rep_real, rep_fake = reports if reports is not None else (None, None)
        want_bank = manifold_k is not None or bool(kernel_distance)       # the manifold metrics or the kernel distance ask for the rows
        real, fake = _Scores(rep_real, True, want_bank), _Scores(rep_fake, True, want_bank)
        lab_real, lab_fake = [], []                                       # per_class: the host arg-max of the one-hot rows, batch by batch
        with self._running_state_kept():
            for xb, yb in batches:
                with cx.phase_scope('metrics', record=False), self._classifier_weights(ema):
                    self._score_batch(cx.from_numpy(xb, key='metrics:x'), cx.from_numpy(yb, key='metrics:y'), real)
                if kernel_distance == 'per_class':
                    lab_real.append(np.argmax(np.asarray(yb), axis=1))
            for k in range(n_batches):
                with cx.phase_scope('metrics_g', record=False), self._classifier_weights(ema):
                    za = cx.from_numpy(z[k * B:(k + 1) * B], key='metrics:z')
                    yg = cx.from_numpy(y[k * B:(k + 1) * B], key='metrics:y_g')
                    self._score_batch(m.as_image(m.good_sampler(za, yg)), yg, fake, take=min(B, n_samples - k * B))
                if kernel_distance == 'per_class':
                    lab_fake.append(np.argmax(y[k * B:k * B + min(B, n_samples - k * B)], axis=1))
            seen = real.moments is not None                         # (a real side without batches: no moments, no bank)
            (n_real, sum_r, gram_r), (n_fake, sum_f, gram_f) = real.moments.sums() if seen else (0, None, None), fake.moments.sums()
            mu_r, cov_r = tgm.mean_cov(n_real, sum_r, gram_r) if seen else (None, None)
            mu_f, cov_f = tgm.mean_cov(n_fake, sum_f, gram_f)
            fd = tgm.frechet_distance(mu_r, cov_r, mu_f, cov_f) if n_real >= 2 and n_fake >= 2 else float('nan')
            out = dict(val_accuracy=float(real.accuracy) if real.accuracy is not None else 0.0, g_class_accuracy=float(fake.accuracy),
                       frechet_distance=fd, n_real=int(n_real), n_fake=int(n_fake))
            finite = want_bank and seen and all(bool(np.isfinite(a).all()) for a in (sum_r, gram_r, sum_f, gram_f))
            if manifold_k is not None:
                out.update(tgm.manifold_metrics(real.bank, fake.bank, manifold_k, cx.stream) if finite
                           else dict.fromkeys(tgm.MANIFOLD_KEYS, float('nan')))
            if kernel_distance:
                out.update(self._kernel_distance(real.bank, fake.bank, lab_real, lab_fake, kernel_distance == 'per_class', finite))
            if rep_real is not None:
                out['val_report'] = rep_real.result()
            if rep_fake is not None:
                out['g_report'] = rep_fake.result()
        return out, ((real.bank, fake.bank) if want_bank else None)

    def _kernel_distance(self, real_bank, fake_bank, lab_real, lab_fake, per_class, finite):
        """tg.metrics.kernel_distance of the two banks of a sample-metrics pass (lab_*: the per-batch host labels, used with
        per_class); every number NaN, and no launch, unless `finite` (both sides seen, their moment sums finite)."""
        K = int(self.options.num_classes)
        if not finite:
            out = dict(kernel_distance=float('nan'))
            if per_class:
                out.update(kernel_distance_per_class=np.full(K, np.nan), kernel_distance_worst=float('nan'), kernel_distance_worst_class=-1)
            return out
        if not per_class:
            return tgm.kernel_distance(real_bank, fake_bank, stream=self.cx.stream)
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
        return tgm.kernel_distance(real_bank, fake_bank, cat(lab_real), cat(lab_fake), K, stream=self.cx.stream)

    NEAREST_KEYS = ('g_nn_rmse', 'g_nn_rmse_min', 'g_nn_class_agreement', 'val_nn_rmse')

    def _training_pixels(self, dataset_train):
        """(tg.metrics.PixelBank of the training split's bytes, its labels int32 [n]) in the order of
        Input_Pipeline.tfrecordDataset.training_chunks — the training index.  Decoded once per trainer and kept on the device (n x d
        bytes: 150 MB for CIFAR); `nearest_decoded` counts the records decoded so far."""
        from Input_Pipeline.tfrecordDataset import training_chunks
        kept = self._nearest.get('pixel')
        if kept is not None and kept['dataset'] is dataset_train:
            return kept['bank'], kept['labels']
        bank = tgm.PixelBank(int(np.prod(self.config.IMAGE_DIM)), self.cx.device)
        labels = bank.add_records(training_chunks(dataset_train))
        self.nearest_decoded += bank.n
        if bank.n == 0:
            raise tgm.lib.TgError("nearest_training: the training split is empty")
        self._nearest['pixel'] = dict(dataset=dataset_train, bank=bank, labels=labels, val={})
        return bank, labels

    def _pixel_scaling(self, dataset_train):
        """(scale, shift) of the input pipeline's tail x = u / 255 * scale + shift for this dataset."""
        return (1.0, 0.0) if dataset_train.UNIT_RANGE else (2.0, -1.0)

    def _generated(self, n_samples, each):
        """run the first n_samples samples of _sample_latents through the sampler, batch by batch as sample_metrics does, and hand
        each(images Act, labels Act, rows to take) every batch inside the 'metrics_g' phase."""
        cx, m, B = self.cx, self.model, int(self.config.BATCH_SIZE_G)
        n_batches = -(-n_samples // B)
        z, y = self._sample_latents(n_batches)
        for k in range(n_batches):
            with cx.phase_scope('metrics_g', record=False):
                za = cx.from_numpy(z[k * B:(k + 1) * B], key='metrics:z')
                yg = cx.from_numpy(y[k * B:(k + 1) * B], key='metrics:y_g')
                each(m.as_image(m.good_sampler(za, yg)), yg, min(B, n_samples - k * B))

    def nearest_training(self, dataset_train, val_batches, n_samples, k, space='pixel', return_banks=False):
        """The nearest training images of generated samples: are the samples copies of training images?
        The generated side is the first n_samples samples of _sample_latents — those sample_metrics scores, taken under the same
        batch-norm rule.  dataset_train: the training tfrecordDataset; its records in the order of training_chunks define the training
        index.  -> dict:
          space 'pixel'    the samples, quantised back to the input pipeline's bytes (tg_f32_quantize_u8), against the training split's
                           bytes with tg_nearest_u8_i32: exact integer squared distances, ties to the lower index.
            nn_idx, nn_d2, nn_label   int32 [n_samples, k]: training index, squared distance and label of the k nearest, nearest first
            g_nn_rmse                 mean_i sqrt(d2_i,1 / d) / 255: the root-mean-square pixel difference to the nearest, full range = 1
            g_nn_rmse_min             the smallest of them: the most suspicious sample
            g_nn_class_agreement      the share of samples whose nearest training image carries the class asked for
            val_nn_rmse               the control: g_nn_rmse's statistic for the first n_samples images of val_batches (quantised back
                                      to bytes) — how near a real held-out image lies.  Computed once per trainer and n_samples:
                                      the validation split is taken as fixed, so a later call with the same n_samples returns the
                                      kept control and does not read the val_batches it is handed.
            val_nn_d2                 int32 [<= n_samples]: the control's squared distances, image by image
          Every scalar is reduced in float64 on the host from the exact integers.  No threshold: g_nn_rmse is read against val_nn_rmse.
          space 'feature'  the training split through the classifier in evaluation mode (_score_batch) into a FeatureBank, the samples'
                           pooled features queried with tg_manifold_query_f32: nn_idx int32 and nn_d2 float32 [n_samples, 1]; k must
                           be 1 (ValueError otherwise).
        The training bytes are decoded once per trainer and stay on the device.  Running statistics are put back afterwards and
        nothing else is written: what sample_metrics says about the trainer's state holds unchanged.  Synchronises the device.
        return_banks: return (result, (query bank, training bank)) — the rows that were compared."""
        k = tgm.check_k(k, 'nearest_training: k')
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError("nearest_training: n_samples must be a positive integer, got %r" % (n_samples,))
        if space not in ('pixel', 'feature'):
            raise ValueError("nearest_training: space must be 'pixel' or 'feature', got %r" % (space,))
        if space == 'feature' and k != 1:
            raise ValueError("nearest_training: space 'feature' returns the single nearest row (tg_manifold_query_f32): k must be 1, got %d" % k)
        self._require_eager("nearest_training", "eager pass beside the step")
        cx, c = self.cx, self.config
        with self._running_state_kept():
            if space == 'feature':
                out, banks = self._nearest_features(dataset_train, n_samples)
                return (out, banks) if return_banks else out
            train, labels = self._training_pixels(dataset_train)
            scale, shift = self._pixel_scaling(dataset_train)
            d = train.d
            fake = tgm.PixelBank(d, cx.device)
            self._generated(n_samples, lambda img, yg, take: fake.add_act(img.view_rows(0, take), scale, shift, cx.stream))
            d2, idx = (t.cpu().numpy() for t in tgm.nearest_pixels(fake, train, k, cx.stream))
            rmse = tgm.nearest_rmse(d2, d)
            asked = np.arange(n_samples) % int(c.NUM_CLASSES)
            nn_label = np.where(idx >= 0, labels[np.maximum(idx, 0)], -1).astype(np.int32)
            kept = self._nearest['pixel']['val']
            if n_samples not in kept:
                real, left = tgm.PixelBank(d, cx.device), n_samples
                for xb, _ in val_batches:
                    if left <= 0:                                  # (the rest is drained: the pipeline's prefetch thread ends with it)
                        continue
                    xa = self.model.as_image(cx.from_numpy(np.asarray(xb, np.float32)[:left]))
                    real.add_act(xa, scale, shift, cx.stream)
                    left -= xa.n
                v_d2 = tgm.nearest_pixels(real, train, 1, cx.stream)[0].cpu().numpy()[:, 0] if real.n else np.zeros(0, np.int32)
                kept[n_samples] = (float(tgm.nearest_rmse(v_d2, d).mean()) if real.n else float('nan'), v_d2)
            out = dict(nn_idx=idx, nn_d2=d2, nn_label=nn_label, g_nn_rmse=float(rmse.mean()), g_nn_rmse_min=float(rmse.min()),
                       g_nn_class_agreement=float(np.mean(nn_label[:, 0] == asked)), val_nn_rmse=kept[n_samples][0],
                       val_nn_d2=kept[n_samples][1])
        return (out, (fake, train)) if return_banks else out

    def _nearest_features(self, dataset_train, n_samples):
        """nearest_training's space 'feature' -> ({nn_idx, nn_d2}, (generated FeatureBank, training FeatureBank))."""
        from Input_Pipeline.tfrecordDataset import training_chunks
        cx, c = self.cx, self.config
        train, fake = _Scores(None, True, True), _Scores(None, True, True)
        B = int(c.BATCH_SIZE)
        for rec, idx in training_chunks(dataset_train, B):
            img, lab = np.empty((len(idx),) + tuple(rec.shape), np.uint8), np.empty(len(idx), np.int32)
            rec.gather(idx, img.reshape(-1), lab, n_threads=1)
            xb, yb = dataset_train._to_host(img, lab)
            with cx.phase_scope('metrics', record=False), self._classifier_weights(False):
                self._score_batch(cx.from_numpy(xb, key='metrics:x'), cx.from_numpy(yb, key='metrics:y'), train)
        if train.bank is None:
            raise tgm.lib.TgError("nearest_training: the training split is empty")
        self._generated(n_samples, lambda img, yg, take: self._score_batch(img, yg, fake, take=take))
        _, nn_d2, nn_idx = tgm.manifold_query(fake.bank.rows(), train.bank.rows(), None, cx.stream)
        return dict(nn_idx=nn_idx.cpu().numpy().reshape(-1, 1), nn_d2=nn_d2.cpu().numpy().reshape(-1, 1)), (fake.bank, train.bank)

    def sample(self, sample_z, sample_y):
        """model.good_sampler on fixed latents (:68,353-364) -> host array [N,H,W,C] in [-1,1]."""
        cx = self.cx
        with cx.phase_scope('sample', record=False):
            out = self.model.good_sampler(cx.from_numpy(sample_z, key='smp:z'), cx.from_numpy(sample_y, key='smp:y'))
            return out.numpy().reshape([-1] + list(self.config.IMAGE_DIM))
