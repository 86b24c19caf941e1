"""Base configuration class — same attribute names as the reference's config.py:9-93
(including its spellings, e.g. CLA_LEARNINIG_RATE is set by the experiment configs).  The defaults written here are the only ones: the
trainer reads a config through Training/options.py, which falls back to this class for an attribute a config object lacks."""


class Config(object):
    NAME = None
    ## Input pipeline
    DATA_NAME = None
    DATA_DIR = None
    NUM_LABEL = None
    BATCH_SIZE = None
    BATCH_SIZE_L_D = None
    SAMPLE_SIZE = 64

    IMAGE_HEIGHT = None
    IMAGE_WIDTH = None
    CHANNEL = None
    REPEAT = None

    ## Model architecture
    Z_DIM = None
    NUM_CLASSES = None
    MINIBATCH_DIS = False

    ## Training settings
    RESTORE = False
    RUN = None
    RESTORE_EPOCH = None
    BATCH_NORM_DECAY = 0.9
    BATCH_NORM_EPSILON = 1e-5
    LEARNING_RATE = 3e-4
    BETA1 = 0.5

    PRE_TRAIN = False
    EPOCHS = None
    TRAIN_SIZE = None
    VAL_STEP = None
    SAVE_PER_EPOCH = 1
    SUMMARY = True
    SUMMARY_GRAPH = True
    SUMMARY_SCALAR = True
    SUMMARY_IMAGE = False              # True (--summary-image): the epoch's first generator samples as 'generated/image/<i>' 
    SUMMARY_HISTOGRAM = False          # True (--summary-histogram): every trainable variable and its gradient as a TensorBoard histogram
                                       # per epoch, binned on the device (Train.histograms)

    SAMPLE_DIR = None
    LOG_DIR = None
    WEIGHT_DIR = None
    DEBUG = False

    ## additions of the MI355X build (not in the reference)
    SEED = 0                 # initial weights + Philox stream
    USE_HIP_GRAPH = None     # True: replay the solver runs as captured hipGraphs; False: launch eagerly; None: EXEC_MODE decides
    EXEC_MODE = 'auto'       # 'auto': times 'plan' and 'graph' over the first iterations and keeps the faster (tg.executor.AutoMode);
                             # 'overlap': eager launches, filter gradients and independent forward passes on a second HIP stream beside the
                             # input-gradient chain (measured fastest on MI355X / ROCm 7.2: 14.6 ms against 15.0 ms per CIFAR-10 step);
                             # 'plan': that two-stream launch sequence recorded once per solver run and re-issued natively (tg_plan_replay,
                             # include/tg_plan.h) - no interpreter on the launch path;
                             # 'graph': hipGraph replay (single chain); 'eager': eager launches on one stream
    ZCA = None               # (mean, mat) arrays when DATA_DIR holds no cifar10_zca_*.npy; 'fit' (--zca fit): fitted from the training
                             # TFRecords by Train.train and written to those files, or loaded from them when present
    AUGMENT = False          # True (--augment): random shift and flip of every training batch, fused into the input pipeline
    LOSS = 'GAN'             # the loss of the three solver runs: 'GAN' (_loss_GAN, the reference's training loss) or 'WGAN_GP' (its
                             # _loss_WGAN_GP with the gradient penalty, wired into the step as DESIGN §9.1 decides; fp32 MFMA operands, no
                             # minibatch discrimination, BATCH_SIZE_L_D + BATCH_SIZE_U_D == BATCH_SIZE_G — Training/Train_goodGAN.check_loss)
    OPTIMIZER = 'adam'       # the optimiser of the three networks: 'adam' (the reference's training choice), 'rmsprop' (its _RMSProp_optimizer:
                             # decay 0.9, momentum 0, epsilon 1e-10) or 'momentum' (its _SGD_w_Momentum_optimizer with MOMENTUM), or a 3-tuple
                             # (D, G, C) of them (--optimizer NAME sets all three; Training/Train_goodGAN.check_optimizer)
    MOMENTUM = 0.9           # the momentum of OPTIMIZER 'momentum' only (RMSProp keeps the reference's momentum 0)
    CLIP_NORM = None         # clip each network's gradients by their global norm before the optimiser step (tf.clip_by_global_norm where
                             # the reference's _train_op_w_grads hands out the gradients): None (off — the step is exactly the unclipped one),
                             # a positive float for all three networks (--clip-norm X), or a 3-tuple (D, G, C) of positive floats / None
                             # (Training/Train_goodGAN.check_clip_norm)
    SUMMARY_IMAGE_MAX_OUTPUTS = 2      # how many samples SUMMARY_IMAGE writes per epoch (tf.summary.image's max_outputs; the reference's
                                       # _image_summary default, Training/Summary.py:59), at most SAMPLE_SIZE
    MFMA_DTYPE = 'f32'       # 'bf16': conv/deconv/dense operands rounded to bf16 inside the MFMA kernels (fp32 accumulate)
    ACT_DTYPE = 'f32'        # 'bf16' (needs MFMA_DTYPE = 'bf16', else ValueError): the training-mode batch norms whose only reader is a
                             # bf16-operand 3x3 convolution store their output as bf16 (the SVHN classifier's c_h0_bn0/bn1, c_h1_bn0/bn1) —
                             # the bits that convolution would round it to, so the step is bit-identical with half the bytes on those
                             # edges; Train.bf16_act_edges counts them (0 on a model without such an edge: the switch changes nothing)

    # WN_INIT — NOT declared here (the entry configurations' attribute sets are pinned): an instance or subclass may set
    # WN_INIT = 'data' (--wn-init data) for the data-dependent initialisation of every weight-normalised layer on the first
    # training batch, g <- init_scale / sqrt(var + eps), b <- -mean * g (Salimans & Kingma 2016; Train.data_dependent_init,
    # DESIGN §9.9); absent or None: g = 1, b = 0 as created.  Read by Training/options.check_wn_init.

    # EVAL_EMA, SAMPLE_METRICS, SAMPLE_MANIFOLD_K, EVAL_REPORT, SAMPLE_KID, SAMPLE_NEAREST — NOT declared here either, for the same reason; an
    # instance or subclass may set
    #   EVAL_EMA = True (--eval-ema): the epoch tail also evaluates the classifier's averaged weights (the EMA shadows, decay 0.9999
    #     without bias correction: they lag the weights by roughly 1e4 iterations) and records `val_accuracy_ema`;
    #   SAMPLE_METRICS = N (--sample-metrics N), a positive int: the epoch tail scores N generated samples with the run's own
    #     classifier — `g_class_accuracy`, the share classified as the class they were asked for, and `frechet_distance` between the
    #     classifier features of the validation split and of the samples (with the averaged weights when EVAL_EMA is on).  The
    #     extractor moves with training: compare generators under one classifier, not epochs (Train.sample_metrics).
    #   SAMPLE_MANIFOLD_K = k (--sample-manifold-k k), an int in 1..16, with SAMPLE_METRICS: the same pass also records the
    #     k-nearest-neighbour `precision`, `recall`, `density` and `coverage` of the samples against the validation split (k = 3 in
    #     Kynkäänniemi et al. 2019; tg_knn_self_f32 / tg_manifold_query_f32).  The radii depend on k and on both counts.
    #   EVAL_REPORT = True (--eval-report): the evaluation passes of the epoch tail also accumulate the classifier's per-class report
    #     (tg_eval_report_f32: confusion matrix, rank histogram, calibration bins, NLL; no forward pass is added) and record
    #     `val_balanced_accuracy`, `val_macro_f1`, `val_nll`, `val_ece`, with NUM_CLASSES > 5 `val_top5_accuracy`; with EVAL_EMA the
    #     same with an `_ema` suffix; with SAMPLE_METRICS `g_worst_class_accuracy`, the lowest per-class share of generated samples
    #     classified as asked.  With summaries on, rank 0 writes confusion_<epoch>.npy (and g_confusion_<epoch>.npy) beside the
    #     validation events (Train.evaluate_report).
    #   SAMPLE_KID = True or 'per_class' (--sample-kid [per_class]), with SAMPLE_METRICS = N: the same pass also records
    #     `kernel_distance`, the unbiased cubic-kernel MMD^2 ("Kernel Inception Distance", Binkowski et al. 2018) between the
    #     classifier features of the validation split and of the samples (tg_poly3_sums_f32: fp64 sums on the fp64 MFMA, the Gram
    #     matrices never written); 'per_class' also `kernel_distance_worst`, the largest of the per-class distances (real rows by
    #     label, samples by the class asked for), and with summaries on rank 0 writes kid_per_class_<epoch>.npy beside the
    #     validation events.  Unbiased at any N, so runs scored at different N compare; the extractor still moves with training
    #     (Train.sample_kernel_distance).
    #   SAMPLE_NEAREST = k (--sample-nearest k), an int in 1..16, with SAMPLE_METRICS = N and a TFRecord Dataset: the epoch tail also
    #     finds the k nearest training images, in pixel space, of those N samples (tg_nearest_u8_i32: exact integer distances against
    #     the whole training split, resident on the device as uint8) and records `g_nn_rmse`, `g_nn_rmse_min`,
    #     `g_nn_class_agreement` and the held-out control `val_nn_rmse`; rank 0 writes SAMPLE_DIR/nearest_<epoch>.png
    #     (Train.nearest_training).
    # Absent, None or False: the epoch tail is what it was.  Read by Training/options.check_eval_ema / check_sample_metrics /
    # check_sample_manifold_k / check_eval_report / check_sample_kid / check_sample_nearest.

    # R1_GAMMA — NOT declared here either, for the same reason; absent or None is the default, the step exactly as it is.  An instance
    # or subclass may set R1_GAMMA = gamma (--r1-gamma X), a positive finite number: with LOSS = 'GAN' the D-update adds the R1
    # gradient penalty gamma / 2 * mean_i ||d D_logit(x_i, y_i) / d x_i||^2 on the discriminator's real rows [x_l_d | x_u_d] to d_loss
    # (Mescheder et al. 2018; fp32 MFMA operands, no minibatch discrimination, not with LOSS = 'WGAN_GP'; Train.set_r1_gamma changes it
    # during a run).  Read by Training/options.check_r1_gamma.

    def __init__(self):
        """Set values of computed attributes (config.py:70-73)."""
        self.MIN_QUEUE_EXAMPLES = self.BATCH_SIZE * 3
        self.IMAGE_DIM = [self.IMAGE_HEIGHT, self.IMAGE_WIDTH, self.CHANNEL]

    def display(self):
        print("\nConfigurations:")
        for a in dir(self):
            if not a.startswith("__") and not callable(getattr(self, a)):
                v = getattr(self, a)
                print("{:30} {}".format(a, '<arrays>' if isinstance(v, tuple) and not all(isinstance(e, str) for e in v) else v))
        print("\n")

    def config_str(self):
        s = "\nConfigurations:\n"
        for a in dir(self):
            if not a.startswith("__") and not callable(getattr(self, a)):
                v = getattr(self, a)
                s += "{:30} {}".format(a, '<arrays>' if isinstance(v, tuple) and not all(isinstance(e, str) for e in v) else v)
                s += "\n"
        return s
