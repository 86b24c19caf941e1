"""Float64 NumPy restatement of the data-dependent weight-norm initialisation (Salimans & Kingma 2016; the reference's
Model/nn.py:492-500, Model/modle_base.py:68-71,103-106,150-153 with their assigns run):

  * the per-layer rule (`rule`): from the unit-gain pre-activation t = conv(x, V/||V||), m = mean t, v = mean (t - m)^2 over all axes
    but the last, g = init_scale / sqrt(v + eps), b = -m g, and the layer's value g t + b;
  * the whole initialisation pass of both models (`init_pass_cifar10`, `init_pass_goodgan`): generator on (z_g, y_g), classifier on
    x_u_c, discriminator on X_P = [x_l_d; x_u_d] with Y_P = [y_l_d; labels], every layer consuming the initialised output of the one
    before it; dropout and noise are the identity, batch norms use batch statistics;
  * two models of how a kernel may compute the rule from fp32 data (`kernel_model`, `one_pass_fp32_model`) and the bound that tells them
    apart (K_G, K_B, K_PRE, K_ACT): the tolerance of tests/test_gpu_wn_init.py and its negative control, established on the CPU.

Network layer lists, parameter names and the TF ops come from oracle/ (test infrastructure); nothing here is imported by the package."""
import numpy as np

from oracle import nets_cifar10 as NC
from oracle import nets_goodgan as NG
from oracle import tf_ops as T

U = 2.0 ** -24

# ---- the tolerance of tg_wn_init_f32 against float64 (pointwise class of tests/kernel_check.py: |got - ref64| <= K u magnitude) ----
# The kernel accumulates both moments in fp64, so m and v carry relative errors of order rows * 2^-53: nothing at the scale of u.  What is
# left are the final roundings, counted to first order; SLACK covers the second-order terms (u^2) and those fp64 sums.
#   g32 = fl32(g64):                              one rounding                        |g32 - g64| <= 1 u |g64|
#   b32 = fl32(-m g32):                           g's rounding carried + its own      |b32 - b64| <= 2 u |m||g64|
#   pre = fl32(fl32(g32 t) + b32):                g (1), product (1), sum (1) on |g t|;  b (2), sum (1) on |b|
#                                                                                     |pre - pre64| <= 3 u (|g64||t| + |b64|)
#   y = act(pre): every activation here is 1-Lipschitz, so the error of pre passes through at most unchanged, plus the evaluation of
#   the activation itself, K_ACT u |act| (the constants tests/test_gpu_elementwise.py::test_act holds tg_act_f32 to; lrelu: one product).
SLACK = 1.0 + 2.0 ** -20
K_G = 1 * SLACK
K_B = 2 * SLACK
K_PRE = 3 * SLACK
K_ACT = {'none': 0, 'relu': 0, 'lrelu': 1, 'tanh': 4, 'sigmoid': 6, 'softplus': 6}


def rule(t, eps, init_scale=1.0):
    """t [rows, c] (any float type; evaluated in float64) -> (m, v, g, b), each [c]."""
    t = np.asarray(t, np.float64)
    m = t.mean(axis=0)
    v = np.square(t - m).mean(axis=0)
    g = np.float64(init_scale) / np.sqrt(v + np.float64(eps))
    return m, v, g, -m * g


def y_bound(t, g, b, ref_y, act):
    """the magnitude `mag` with |y - ref_y| <= 1 u mag for the kernel's y (see the derivation above)."""
    pre_mag = np.abs(g) * np.abs(np.asarray(t, np.float64)) + np.abs(b)
    return K_PRE * pre_mag + K_ACT[act] * np.abs(ref_y)


def kernel_model(t32, eps, init_scale=1.0):
    """two passes accumulated in fp64, then rounded as tg_wn_init_f32 rounds: g32 = fl32(s / sqrt(v + eps)), b32 = fl32(-m g32)."""
    t = np.asarray(t32, np.float32).astype(np.float64)
    m = t.sum(axis=0) / t.shape[0]
    v = np.square(t - m).sum(axis=0) / t.shape[0]
    g = (np.float64(np.float32(init_scale)) / np.sqrt(v + np.float64(np.float32(eps)))).astype(np.float32)
    return g, (-m * g.astype(np.float64)).astype(np.float32)


def one_pass_fp32_model(t32, eps, init_scale=1.0):
    """what a single pass with fp32 accumulators would give: v = E[x^2] - m^2 from running fp32 sums (clipped at 0)."""
    t = np.asarray(t32, np.float32)
    s1 = np.zeros(t.shape[1], np.float32)
    s2 = np.zeros(t.shape[1], np.float32)
    for row in t:
        s1 = (s1 + row).astype(np.float32)
        s2 = (s2 + (row * row).astype(np.float32)).astype(np.float32)
    n = np.float32(t.shape[0])
    m = (s1 / n).astype(np.float32)
    v = np.maximum((s2 / n).astype(np.float32) - (m * m).astype(np.float32), np.float32(0))
    g = (np.float32(init_scale) / np.sqrt((v + np.float32(eps)).astype(np.float32))).astype(np.float32)
    return g, (-m * g).astype(np.float32)


def ill_conditioned(rows, c, seed=20160225):
    """fp32 channels of mean 1e3 and standard deviation 1e-2 (an fp32 ulp at 1e3 is 6e-5): the variance is 1e-10 of the second moment,
    far below what an fp32 E[x^2] - m^2 can resolve, while the centred second pass in fp64 sees it exactly.  Fixed inputs."""
    rng = np.random.default_rng(seed)
    return (1e3 + 1e-2 * rng.standard_normal((rows, c))).astype(np.float32)


def within(g, b, t32, eps, init_scale=1.0):
    """(g, b) of a model lie inside the kernel's bound around the float64 rule evaluated on the same fp32 data and fp32 (eps, scale)."""
    m, v, g64, b64 = rule(np.asarray(t32, np.float32), np.float64(np.float32(eps)), np.float64(np.float32(init_scale)))
    ok_g = np.abs(np.asarray(g, np.float64) - g64) <= K_G * U * np.abs(g64)
    ok_b = np.abs(np.asarray(b, np.float64) - b64) <= K_B * U * np.abs(m) * np.abs(g64)
    return bool(ok_g.all() and ok_b.all())


# ---------------------------------------------------------------------------------------------------------------- layers

def _f64(P):
    return {k: np.asarray(v, np.float64) for k, v in P.items()}


def wn_layer(x, V, kind, eps, init_scale=1.0, stride=1, padding='SAME'):
    """One layer's init in float64.  kind: 'dense' (x [..., cin], V [cin, cout]; a 1x1 product over every leading axis),
    'conv' (V [k,k,cin,cout]), 'deconv' (V [5,5,cout,cin], stride 2 SAME).  Returns (t, g, b, g t + b) with t shaped like the output."""
    x, V = np.asarray(x, np.float64), np.asarray(V, np.float64)
    if kind == 'dense':
        t = (x.reshape(-1, x.shape[-1]) @ T.l2_normalize(V, [0])).reshape(x.shape[:-1] + (V.shape[-1],))
    elif kind == 'conv':
        t = T.conv2d(x, T.l2_normalize(V, (0, 1, 2)), (stride, stride), padding)
    else:
        t = T.conv2d_transpose(x, T.l2_normalize(V, (0, 1, 3)))
    m, v, g, b = rule(t.reshape(-1, t.shape[-1]), eps, init_scale)
    return t, g, b, g * t + b


class Record(object):
    """what one layer's init saw and assigned (the self-checks and the GPU comparisons read it)."""

    def __init__(self, name, t, g, b, eps, init_scale):
        self.name, self.t, self.g, self.b, self.eps, self.init_scale = name, t.reshape(-1, t.shape[-1]), g, b, eps, init_scale


# ---------------------------------------------------------------------------------------------------------------- CIFAR-10

def init_pass_cifar10(P, x_u_c, zca):
    """Good_GAN_cifar10: only the classifier has weight-normalised layers (7 conv2d_WN eps 1e-8, NiN1 / NiN2 / output_dense eps 1e-10),
    on ZCA-whitened x_u_c without input noise or dropout.  Returns ({name: new value} for every g and b, [Record])."""
    P = _f64(P)
    new, recs = {}, []
    x = NC.zca_apply(np.asarray(x_u_c, np.float64), *(np.asarray(a, np.float64) for a in zca)).reshape(-1, 32, 32, 3)

    def assign(p, t, g, b, eps):
        new[p + 'g'], new[p + 'b'] = g, b
        recs.append(Record(p.rstrip('/'), t, g, b, eps, 1.0))

    for name, cout, pad in NC.C_CONVS:
        p = 'classifier/%s/' % name
        t, g, b, y = wn_layer(x, P[p + 'V'], 'conv', 1e-8, 1.0, 1, pad)
        assign(p, t, g, b, 1e-8)
        x = T.lrelu(y)
        if name in NC.C_POOL_AFTER:
            x, _ = T.maxpool2(x)
    for name in ('NiN1', 'NiN2'):
        p = 'classifier/%s/%s/' % (name, name)
        t, g, b, y = wn_layer(x, P[p + 'V'], 'dense', 1e-10)
        assign(p, t, g, b, 1e-10)
        x = T.lrelu(y)
    feat, _ = T.global_maxpool(x)
    p = 'classifier/output_dense/'
    t, g, b, y = wn_layer(feat, P[p + 'V'], 'dense', 1e-10)
    assign(p, t, g, b, 1e-10)
    return new, recs


# ---------------------------------------------------------------------------------------------------------------- MNIST / SVHN

INIT_SCALE = {'good_generator/gg_wndconv0': 0.1}          # Good_GAN.py:56; every other layer 1.0


def _seq_init(P, layers, x, y, new, recs, init=True):
    """oracle/nets_goodgan.seq_fwd in the initialisation pass: noise and dropout are the identity, batch norms normalise with batch
    statistics (and move nothing), every weight-normalised layer assigns g and b (eps 1e-10, modle_base.py) and hands on g t + b."""
    for l in layers:
        k = l[0]
        if k == 'concat_y':
            x = np.concatenate([x, y], axis=1)
        elif k == 'cond_concat':
            x = T.conv_cond_concat(x, y)
        elif k == 'reshape':
            x = x.reshape((x.shape[0],) + tuple(l[1]))
        elif k == 'dense':
            x = x @ P[l[1] + '/kernel'] + P[l[1] + '/bias']
        elif k == 'conv':
            x = T.conv2d(x, P[l[1] + '/kernel'], (l[3], l[3]), 'SAME') + P[l[1] + '/bias']
        elif k == 'deconv':
            x = T.conv2d_transpose(x, P[l[1] + '/kernel']) + P[l[1] + '/bias']
        elif k in ('wn_dense', 'nin', 'wn_conv', 'wn_deconv'):
            kind = {'wn_dense': 'dense', 'nin': 'dense', 'wn_conv': 'conv', 'wn_deconv': 'deconv'}[k]
            s = INIT_SCALE.get(l[1], 1.0)
            t, g, b, x = wn_layer(x, P[l[1] + '/V'], kind, 1e-10, s, l[3] if k == 'wn_conv' else 1)
            new[l[1] + '/g'], new[l[1] + '/b'] = g, b
            recs.append(Record(l[1], t, g, b, 1e-10, s))
        elif k == 'act':
            x = NG._ACT[l[1]][0](x)
        elif k == 'bn':
            x, _ = T.batch_norm_train(x, P[l[1] + '/gamma'], P[l[1] + '/beta'], NG.BN_EPS)
        elif k == 'maxpool':
            x, _ = T.maxpool2(x)
        elif k == 'gmean':
            x = x.mean(axis=(1, 2))
        elif k in ('noise', 'dropout', 'feature'):
            pass
        else:
            raise ValueError(k)
    return x


def eval_labels_goodgan(P, data, x_u_d, noise=None):
    """one_hot(argmax C(x_u_d)) of the ordinary evaluation-mode classifier (moving statistics; MNIST: input noise `noise` or none)."""
    rnd = {'noise': np.zeros((x_u_d.shape[0],) + NG.image_shape(data)) if noise is None else noise}
    logits, _, _ = NG.seq_fwd(_f64(P), NG.classifier_layers(data), np.asarray(x_u_d, np.float64), None, rnd, False)
    return T.argmax_onehot(logits, NG.NCLS)


def init_pass_goodgan(P, data, batch, labels=None):
    """Good_GAN (MNIST: gg_h2_lin, then d_h0..5_wndense0; SVHN: gg_wndconv0 with init_scale 0.1, c_h2_nin0 / c_h2_nin1, then the six
    d_h*_wnconv* and d_h3_wndense), all eps 1e-10.  batch: z_g, y_g, x_l_d, y_l_d, x_u_d, x_u_c; labels: the one-hot labels of x_u_d the
    discriminator sees (default: eval_labels_goodgan on the classifier AFTER its own init, without noise).
    Returns ({name: new value}, [Record], labels)."""
    P = _f64(P)
    b = {k: np.asarray(v, np.float64) for k, v in batch.items()}
    new, recs = {}, []
    _seq_init(P, NG.generator_layers(data), b['z_g'], b['y_g'], new, recs)
    _seq_init(P, NG.classifier_layers(data), b['x_u_c'].reshape((-1,) + NG.image_shape(data)), None, new, recs)
    P.update(new)
    if labels is None:
        labels = eval_labels_goodgan(P, data, b['x_u_d'].reshape((-1,) + NG.image_shape(data)))
    xp = np.concatenate([b['x_l_d'], b['x_u_d']], axis=0).reshape((-1,) + NG.image_shape(data))
    yp = np.concatenate([b['y_l_d'], np.asarray(labels, np.float64)], axis=0)
    _seq_init(P, NG.discriminator_layers(data), xp, yp, new, recs)
    return new, recs, labels
