"""What the trainer reads out of a config object, resolved once and without a device.

config.Config is the only place a default is written: `opt(config, name)` falls back to it, so a duck-typed config that lacks an
attribute means what a Config subclass without it means.  The `check_*` functions validate one setting each and return its normalised
value; `resolve(config)` runs them all and returns the record Train.__init__ fills itself from, before any device is initialised.
This module imports no torch and opens no device."""
import collections

import numpy as np

from config import Config
from tg import lib


def opt(config, name):
    """config.<name>, or the default config.Config declares for it."""
    return getattr(config, name, getattr(Config, name))


def cla_lr(config):
    """the classifier's learning rate: CLA_LEARNINIG_RATE (the reference's spelling; the experiment configs set it, Config does not declare
    it), else LEARNING_RATE."""
    return getattr(config, 'CLA_LEARNINIG_RATE', config.LEARNING_RATE)


def check_mfma_dtype(config):
    """config.MFMA_DTYPE ('f32' default | 'bf16' = BASELINE.json configs[3] "bf16 MFMA conv path": conv / deconv / dense operands rounded
    to bf16 inside the MFMA kernels, fp32 accumulation, fp32 tensors, statistics, master weights and optimiser state)."""
    mfma = opt(config, 'MFMA_DTYPE')
    if mfma not in ('f32', 'bf16'):
        raise ValueError("MFMA_DTYPE must be 'f32' or 'bf16', got %r" % (mfma,))
    return mfma


def check_act_dtype(config):
    """config.ACT_DTYPE ('f32' default | 'bf16') checked against config.MFMA_DTYPE: bf16-stored activations are only the same numbers when
    every reader rounds its operands to bf16 anyway — with fp32 MFMA operands they would silently stop being the reference's arithmetic."""
    act, mfma = opt(config, 'ACT_DTYPE'), opt(config, 'MFMA_DTYPE')
    if act not in ('f32', 'bf16'):
        raise ValueError("ACT_DTYPE must be 'f32' or 'bf16', got %r" % (act,))
    if act == 'bf16' and mfma != 'bf16':
        raise ValueError("ACT_DTYPE = 'bf16' needs MFMA_DTYPE = 'bf16' (got %r): fp32 products of bf16-stored values would not be the "
                         "fp32 arithmetic of the reference" % (mfma,))
    return act


LOSSES = ('GAN', 'WGAN_GP')


def check_loss(config):
    """config.LOSS ('GAN' default | 'WGAN_GP': the reference's _loss_WGAN_GP, train_base.py:576-620, in the three-player step).
    Needs no device.  ValueError for an unknown value; lib.TgError for what the WGAN-GP step cannot run: bf16 MFMA operands (and with them
    ACT_DTYPE = 'bf16'), minibatch discrimination, and a penalty batch whose real and fake halves differ in size."""
    loss = opt(config, 'LOSS')
    if loss not in LOSSES:
        raise ValueError("LOSS must be one of %s, got %r" % (', '.join(repr(v) for v in LOSSES), loss))
    if loss != 'WGAN_GP':
        return loss
    from tg import grad_penalty                       # (tg.runtime behind it imports torch: only on this branch)
    grad_penalty.check_supported("LOSS = 'WGAN_GP'", opt(config, 'MFMA_DTYPE'), opt(config, 'MINIBATCH_DIS'))
    l_d, u_d, b_g = (getattr(config, k, None) for k in ('BATCH_SIZE_L_D', 'BATCH_SIZE_U_D', 'BATCH_SIZE_G'))
    if l_d is None or u_d is None or b_g is None or l_d + u_d != b_g:
        raise lib.TgError("LOSS = 'WGAN_GP' needs BATCH_SIZE_L_D + BATCH_SIZE_U_D == BATCH_SIZE_G (got %r + %r, %r): the penalty "
                          "interpolates the discriminator's real images X_P with the generated ones image for image" % (l_d, u_d, b_g))
    return loss


def check_r1_gamma(config):
    """config.R1_GAMMA: None (default; also when the attribute is absent — config.Config does not declare it) or a positive finite
    number gamma: the D-update adds the R1 gradient penalty gamma / 2 * mean_i ||d D_logit(x_i, y_i) / d x_i||^2 on the discriminator's
    real rows to d_loss.  -> None or float.  Needs no device and no relation between the batch sizes.  ValueError for
    zero, a negative number, NaN, infinity, a bool or anything that is not a number, and when set together with LOSS = 'WGAN_GP' (two
    penalties, one slot for their gradient); lib.TgError for what the penalty's sweeps cannot run: bf16 MFMA operands and minibatch
    discrimination."""
    v = getattr(config, 'R1_GAMMA', None)
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not (0.0 < float(v) < float('inf')):
        raise ValueError("R1_GAMMA must be None or a positive finite number, got %r" % (v,))
    if opt(config, 'LOSS') == 'WGAN_GP':
        raise ValueError("R1_GAMMA = %r cannot be combined with LOSS = 'WGAN_GP': that loss brings its own gradient penalty, and the "
                         "D-update holds one penalty gradient" % (v,))
    from tg import grad_penalty                       # (tg.runtime behind it imports torch: only on this branch)
    grad_penalty.check_supported("R1_GAMMA (the R1 gradient penalty)", opt(config, 'MFMA_DTYPE'), opt(config, 'MINIBATCH_DIS'))
    return float(v)


OPTIMIZERS = ('adam', 'rmsprop', 'momentum')


def check_optimizer(config):
    """config.OPTIMIZER ('adam' default | 'rmsprop' | 'momentum', or a 3-tuple of them for the (D, G, C) networks) -> the
    normalised triple (d, g, c).  Needs no device.  ValueError for an unknown name, a tuple that does not have three entries, or any
    other type."""
    kind = opt(config, 'OPTIMIZER')
    names = ', '.join(repr(v) for v in OPTIMIZERS)
    if isinstance(kind, str):
        triple = (kind,) * 3
    elif isinstance(kind, (tuple, list)):
        if len(kind) != 3:
            raise ValueError("OPTIMIZER as a tuple names the optimisers of (D, G, C): three of %s, got %d entries: %r" % (names, len(kind), kind))
        triple = tuple(kind)
    else:
        raise ValueError("OPTIMIZER must be one of %s or a 3-tuple (D, G, C) of them, got %r" % (names, kind))
    for v in triple:
        if not isinstance(v, str) or v not in OPTIMIZERS:
            raise ValueError("OPTIMIZER must be one of %s or a 3-tuple (D, G, C) of them, got %r" % (names, kind))
    return triple


def check_clip_norm(config):
    """config.CLIP_NORM (None default | a positive float | a 3-tuple for the (D, G, C) networks of positive floats or None)
    -> the normalised triple (d, g, c) of floats / None.  Needs no device.  ValueError for zero, a negative number, NaN or infinity, a
    tuple that does not have three entries, and anything that is not a number."""
    clip = opt(config, 'CLIP_NORM')

    def one(v):
        if v is None:
            return None
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (0.0 < float(v) < float('inf')):
            raise ValueError("CLIP_NORM must be None, a positive finite number or a 3-tuple (D, G, C) of them, got %r" % (clip,))
        return float(v)

    if isinstance(clip, (tuple, list)):
        if len(clip) != 3:
            raise ValueError("CLIP_NORM as a tuple holds the thresholds of (D, G, C): three positive numbers or None, got %d entries: %r"
                             % (len(clip), clip))
        return tuple(one(v) for v in clip)
    return (one(clip),) * 3


NETS = ('discriminator', 'good_generator', 'classifier')      # the order of every (D, G, C) triple


NUM_CLASSES_RANGE = (2, 1024)


def check_num_classes(config):
    """config.NUM_CLASSES: an int in 2..1024, the range of the classifier's loss heads (csrc/loss.hip; 10 runs the ten-class kernels, any
    other count the general ones).  Needs no device; ValueError outside it."""
    k = opt(config, 'NUM_CLASSES')
    lo, hi = NUM_CLASSES_RANGE
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not lo <= k <= hi:
        raise ValueError("NUM_CLASSES must be an integer in %d..%d (the classifier's loss heads), got %r" % (lo, hi, k))
    return int(k)


def check_zca(config, Dataset=None):
    """config.ZCA: None (the reference's DATA_DIR/<data>_zca_*.npy files), (mean, mat) arrays, or 'fit' (fitted from the
    training split by Train.train and written to those files).  Needs no device.  ValueError for any other string; lib.TgError when
    'fit' meets a model without ZCA whitening (DATA_NAME not cifar10 / cifar100: MNIST, SVHN, stress64) or a Dataset (class or instance)
    that is not a uint8 TFRecord source in [-1, 1] scaling, e.g. the default syntheticDataset."""
    zc = opt(config, 'ZCA')
    if not isinstance(zc, str):
        return zc
    if zc != 'fit':
        raise ValueError("ZCA must be None, (mean, mat) arrays or 'fit', got %r" % (zc,))
    from Model.zca import ZCA_DATA
    if opt(config, 'DATA_NAME') not in ZCA_DATA:
        raise lib.TgError("ZCA = 'fit' applies to the ZCA-whitened classifiers of %s; DATA_NAME %r has no ZCA whitening"
                          % (' / '.join(ZCA_DATA), opt(config, 'DATA_NAME')))
    if Dataset is not None:
        from Input_Pipeline.tfrecordDataset import tfrecordDataset
        cls = Dataset if isinstance(Dataset, type) else type(Dataset)
        if not issubclass(cls, tfrecordDataset) or cls.UNIT_RANGE:
            raise lib.TgError("ZCA = 'fit' needs a training split of uint8 TFRecords (a tfrecordDataset such as cifar10Dataset); %s has "
                              "none" % cls.__name__)
    return zc


WN_INITS = (None, 'data')


def check_wn_init(config):
    """config.WN_INIT: None (default; also when the attribute is absent — config.Config does not declare it) or 'data': the
    data-dependent initialisation of the weight-normalised layers on the first training batch.  Needs no device;
    ValueError for any other value."""
    v = getattr(config, 'WN_INIT', None)
    if v is not None and not (isinstance(v, str) and v == 'data'):
        raise ValueError("WN_INIT must be None or 'data', got %r" % (v,))
    return v


def check_eval_ema(config):
    """config.EVAL_EMA: off (default; also when the attribute is absent — config.Config does not declare it) or on: the epoch tail also
    evaluates the classifier's averaged weights and records `val_accuracy_ema` (Train.evaluate(ema=True)).  -> bool.
    Needs no device; ValueError for anything but None, a bool or 0 / 1."""
    v = getattr(config, 'EVAL_EMA', None)
    if v is None:
        return False
    if isinstance(v, (bool, np.bool_)) or (isinstance(v, (int, np.integer)) and v in (0, 1)):
        return bool(v)
    raise ValueError("EVAL_EMA must be None, True or False, got %r" % (v,))


def check_eval_report(config):
    """config.EVAL_REPORT: off (default; also when the attribute is absent — config.Config does not declare it) or on: the epoch tail's
    evaluation passes also accumulate the classifier's per-class report (tg.metrics.ClassifierReport) and record
    `val_balanced_accuracy`, `val_macro_f1`, `val_nll`, `val_ece` and, with more than five classes, `val_top5_accuracy` — with EVAL_EMA
    the same for the averaged weights, with SAMPLE_METRICS `g_worst_class_accuracy`.  -> bool.  Needs no device; ValueError for
    anything but None, a bool or 0 / 1."""
    v = getattr(config, 'EVAL_REPORT', None)
    if v is None:
        return False
    if isinstance(v, (bool, np.bool_)) or (isinstance(v, (int, np.integer)) and v in (0, 1)):
        return bool(v)
    raise ValueError("EVAL_REPORT must be None, True or False, got %r" % (v,))


def check_sample_metrics(config):
    """config.SAMPLE_METRICS: None (default; also when the attribute is absent — config.Config does not declare it) or a positive int N:
    the epoch tail scores N generated samples with the run's own classifier and records `g_class_accuracy` and `frechet_distance`
    (Train.sample_metrics).  -> None or int.  Needs no device; ValueError for zero, a negative number, a bool, a float
    or any other type."""
    v = getattr(config, 'SAMPLE_METRICS', None)
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError("SAMPLE_METRICS must be None or a positive integer (how many samples to score), got %r" % (v,))
    return int(v)


def check_sample_manifold_k(config):
    """config.SAMPLE_MANIFOLD_K: None (default; also when the attribute is absent — config.Config does not declare it) or an int k in
    1..16: the epoch tail's sample metrics also record the k-nearest-neighbour `precision`, `recall`, `density` and `coverage` of the
    generated samples (Train.sample_manifold_metrics; k = 3 in Kynkäänniemi et al. 2019).  -> None or int.  Needs no
    device; ValueError for what tg.metrics.check_k refuses (a value outside 1..16, a bool, a float, any other type) and when set
    without SAMPLE_METRICS (the numbers come out of that pass)."""
    from tg.metrics import check_k                                    # (device-free: the module touches torch only inside its classes)
    v = getattr(config, 'SAMPLE_MANIFOLD_K', None)
    if v is None:
        return None
    v = check_k(v, 'SAMPLE_MANIFOLD_K')
    if check_sample_metrics(config) is None:
        raise ValueError("SAMPLE_MANIFOLD_K = %r needs SAMPLE_METRICS = N: the sample-metrics pass computes the manifold metrics" % (v,))
    return v


def check_sample_kid(config):
    """config.SAMPLE_KID: None / False (default; also when the attribute is absent — config.Config does not declare it), True, or
    'per_class': the epoch tail's sample metrics also record `kernel_distance`, the unbiased cubic-kernel MMD^2 between the real and the
    generated features, and with 'per_class' also `kernel_distance_worst`, the largest of the per-class distances, which are written
    beside the validation events as kid_per_class_<epoch>.npy (Train.sample_kernel_distance).  -> None, True or
    'per_class'.  Needs no device; ValueError for any other value (a number, another string) and when set without SAMPLE_METRICS (the
    numbers come out of that pass)."""
    v = getattr(config, 'SAMPLE_KID', None)
    if v is None or (isinstance(v, (bool, np.bool_)) and not v):
        return None
    if isinstance(v, (bool, np.bool_)):
        v = True
    elif not (isinstance(v, str) and v == 'per_class'):
        raise ValueError("SAMPLE_KID must be None, False, True or 'per_class', got %r" % (v,))
    if check_sample_metrics(config) is None:
        raise ValueError("SAMPLE_KID = %r needs SAMPLE_METRICS = N: the sample-metrics pass computes the kernel distance" % (v,))
    return v


def check_sample_nearest(config, Dataset=None):
    """config.SAMPLE_NEAREST: None (default; also when the attribute is absent — config.Config does not declare it) or an int k in
    1..16: the epoch tail also finds the k nearest training images, in pixel space, of the generated samples the sample-metrics pass
    scores, records `g_nn_rmse`, `g_nn_rmse_min`, `g_nn_class_agreement` and `val_nn_rmse` and writes SAMPLE_DIR/nearest_<epoch>.png
    (Train.nearest_training).  -> None or int.  Needs no device; ValueError for what tg.metrics.check_k refuses (a value
    outside 1..16, a bool, a float, any other type) and when set without SAMPLE_METRICS (which gives it its sample count); lib.TgError
    when a Dataset (class or instance) is given that is not a TFRecord source, e.g. the default syntheticDataset: there is no training
    split to search."""
    from tg.metrics import check_k
    v = getattr(config, 'SAMPLE_NEAREST', None)
    if v is None:
        return None
    v = check_k(v, 'SAMPLE_NEAREST')
    if check_sample_metrics(config) is None:
        raise ValueError("SAMPLE_NEAREST = %r needs SAMPLE_METRICS = N: the nearest training images are those of the N samples that "
                         "pass scores" % (v,))
    if Dataset is not None:
        from Input_Pipeline.tfrecordDataset import tfrecordDataset
        cls = Dataset if isinstance(Dataset, type) else type(Dataset)
        if not issubclass(cls, tfrecordDataset):
            raise lib.TgError("SAMPLE_NEAREST needs a training split of uint8 TFRecords (a tfrecordDataset such as cifar10Dataset); %s has "
                              "none" % cls.__name__)
    return v


_Fields = collections.namedtuple('Options', 'mfma_dtype act_dtype num_classes loss optimizers clip_norms momentum seed no_grad_buckets '
                                            'summary summary_scalar summary_histogram summary_image summary_image_max_outputs')


class Options(_Fields):
    """the record resolve() returns.  Its tuple fields are the settings config.Config declares a default for (and NO_GRAD_BUCKETS);
    `wn_init`, `r1_gamma`, `eval_ema`, `sample_metrics`, `sample_manifold_k`, `eval_report`, `sample_kid` and `sample_nearest` (check_wn_init, check_r1_gamma,
    check_eval_ema, check_sample_metrics, check_sample_manifold_k, check_eval_report, check_sample_kid, check_sample_nearest: settings
    Config deliberately does not declare) are carried as attributes beside them, so the field list — what _asdict() and unpacking give
    — stays what it was.  Two records are equal when the fields and these attributes are."""
    EXTRAS = ('wn_init', 'r1_gamma', 'eval_ema', 'sample_metrics', 'sample_manifold_k', 'eval_report', 'sample_kid', 'sample_nearest')
    _EXTRA_DEFAULTS = (None, None, False, None, None, False, None, None)

    def __new__(cls, wn_init=None, eval_ema=False, sample_metrics=None, sample_manifold_k=None, eval_report=False, sample_nearest=None,
                sample_kid=None, r1_gamma=None, **fields):
        self = super(Options, cls).__new__(cls, **fields)
        self.wn_init, self.eval_ema, self.sample_metrics, self.sample_manifold_k = wn_init, eval_ema, sample_metrics, sample_manifold_k
        self.eval_report, self.sample_kid, self.sample_nearest, self.r1_gamma = eval_report, sample_kid, sample_nearest, r1_gamma
        return self

    def _extras(self):
        return tuple(getattr(self, k) for k in self.EXTRAS)

    def __eq__(self, other):
        return (tuple.__eq__(self, other)
                and tuple(getattr(other, k, d) for k, d in zip(self.EXTRAS, self._EXTRA_DEFAULTS)) == self._extras())

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((tuple(self),) + self._extras())


def resolve(config):
    """every device-free check of `config`, once -> the Options record of what Train reads with a default (EXEC_MODE / USE_HIP_GRAPH
    excepted: those stay live, read per iteration).  The string form of ZCA is checked here; against a Dataset, where one is known."""
    check_zca(config)
    return Options(wn_init=check_wn_init(config), r1_gamma=check_r1_gamma(config), eval_ema=check_eval_ema(config), sample_metrics=check_sample_metrics(config),
                   sample_manifold_k=check_sample_manifold_k(config), eval_report=check_eval_report(config),
                   sample_kid=check_sample_kid(config), sample_nearest=check_sample_nearest(config),
                   mfma_dtype=check_mfma_dtype(config), act_dtype=check_act_dtype(config), num_classes=check_num_classes(config),
                   loss=check_loss(config), optimizers=check_optimizer(config), clip_norms=check_clip_norm(config),
                   momentum=float(opt(config, 'MOMENTUM')), seed=opt(config, 'SEED'),
                   no_grad_buckets=bool(getattr(config, 'NO_GRAD_BUCKETS', False)),      # a debugging switch Config does not declare
                   summary=bool(opt(config, 'SUMMARY')), summary_scalar=bool(opt(config, 'SUMMARY_SCALAR')),
                   summary_histogram=bool(opt(config, 'SUMMARY_HISTOGRAM')), summary_image=bool(opt(config, 'SUMMARY_IMAGE')),
                   summary_image_max_outputs=int(opt(config, 'SUMMARY_IMAGE_MAX_OUTPUTS')))
