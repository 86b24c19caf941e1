"""Evaluation — the trainer's forward-only scoring passes: evaluate, the per-class report, the generated-sample and manifold metrics, and
the sampler.  Train (Training/Train_goodGAN.py) inherits it; the methods are used as `Train.<method>`.

The contract, once for all of them.  These passes READ from the trainer

    cx                 the device context: stores, phases, Philox scopes, buffers keyed per pass
    model              classifier, good_sampler, as_image, zca
    config, options    batch sizes and dimensions; seed, class count
    _accuracy_metric   the streaming accuracy of Train_base
    _require_eager     refuses a pass inside a hipGraph capture / launch-plan recording

and OWN one attribute, `_metric_latents` (the fixed latents of sample_metrics, set to None by Train.__init__).  They write no store:
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

    def _sample_metrics_pass(self, batches, n_samples, ema, manifold_k, reports=None):
        """the pass behind sample_metrics (manifold_k None), sample_manifold_metrics and sample_metrics_report -> (result, (real bank,
        fake bank) or None).  reports: None, or (real side, generated side) tg.metrics.ClassifierReport accumulators, either of which
        may be None: each is added the rows its side's accuracy counts, and the result carries `val_report` / `g_report` for those
        given."""
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

    def sample(self, sample_z, sample_y):
        """model.good_sampler on fixed latents (:68,353-364) -> host array [N,H,W,C] in [-1,1]."""
        cx = self.cx
        with cx.phase_scope('sample', record=False):
            out = self.model.good_sampler(cx.from_numpy(sample_z, key='smp:z'), cx.from_numpy(sample_y, key='smp:y'))
            return out.numpy().reshape([-1] + list(self.config.IMAGE_DIM))
