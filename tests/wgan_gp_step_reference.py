"""Float64 restatement of ONE training iteration with config.LOSS = 'WGAN_GP' (Training/Train_goodGAN.py; the port decisions of
DESIGN §9.1): the three solver runs of oracle/step_cifar10.py (CIFAR-10) and oracle/step_goodgan.py (MNIST / SVHN) with the loss of the
reference's _loss_WGAN_GP (Training/train_base.py:576-620) settled as follows:

  D-update  D sees [X_P | G | x_u_c] as with the GAN loss; d_loss = -(wd1 + l1 wd2 + l2 wd3) + 10 gp, the penalty on
            x = X_P + alpha (G - X_P) with the labels y_g and its own draws (RNG scope 'GP');
  G-update  g_loss = -mean D(G, y_g);
  C-update  c_loss = CE(y_l_c, C_real) + l2 CE(y_g, C_fake); the classifier forward (and its pop_mean / moving statistics) as with the
            GAN loss, the unl / rep rows weigh 0, no discriminator application.

Adam and the classifier's EMA as in the oracle.  The penalty's parameter gradient comes from tests/wgan_gp_reference.py /
wgan_gp_goodgan_reference.py (pinned to torch's double backward there); tests/test_wgan_gp_step_reference.py pins the three gradients of
this module by central differences, the GPU tests pin the HIP step against it.

rnd of one iteration: the oracle's {'D': ..., 'G': ..., 'C': ...} plus rnd['D']['GP'] = {'alpha': [B_G], the penalty's masks / noise}."""
import numpy as np

from oracle import nets_cifar10 as NC
from oracle import nets_goodgan as NG
from oracle import step_cifar10 as SC
from oracle import step_goodgan as SG
from oracle import tf_ops as T

import wgan_gp_goodgan_reference as RG
import wgan_gp_reference as RC

GP_WEIGHT = 10.0


def head_d(d_real, d_fake, d_unl, lam1, lam2):
    """(d_loss without the penalty, wd1, wd2, wd3) and d d_loss / d logits per part."""
    (d, _g, wd1, wd2, wd3), g, _gf = RC.wgan_loss_head(d_real, d_fake, d_unl, lam1, lam2)
    nr, nf = np.size(d_real), np.size(d_fake)
    return (d, wd1, wd2, wd3), (g[:nr].reshape(-1, 1), g[nr:nr + nf].reshape(-1, 1), g[nr + nf:].reshape(-1, 1))


def ce_mean(z, y):
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    m = z.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
    p = np.exp(z - lse)
    return float(np.mean(np.sum(y * lse - y * z, axis=1))), (p * y.sum(axis=1, keepdims=True) - y) / z.shape[0]


def penalty(data, P, X_P, Gimg, y_g, gp_rnd):
    """10 gp and 10 d gp / d theta_D at x = X_P + alpha (G - X_P); data 'cifar10' | 'mnist' | 'svhn'."""
    draws = {k: v for k, v in gp_rnd.items() if k != 'alpha'}
    if data == 'cifar10':
        x = RC.interpolate(X_P, Gimg, gp_rnd['alpha'])
        out = RC.gradient_penalty(P, x, y_g, draws)
    else:
        shp = (X_P.shape[0], -1) if data == 'mnist' else X_P.shape          # MNIST: [N, 784], the layout as_image() gives the penalty
        x = RG.interpolate(X_P.reshape(shp), Gimg.reshape(shp), gp_rnd['alpha'])
        out = RG.gradient_penalty(data, P, x, y_g, draws)
    return GP_WEIGHT * out['gp'], {k: GP_WEIGHT * v for k, v in out['grads'].items()}


# ---------------------------------------------------------------------------------------------------------------- CIFAR-10
def d_phase_cifar10(st, b, rnd, hyper, zca, gp_out=None, labels=None):
    """returns d_loss; st['last_grads']['D'] = the gradient Adam applied (penalty included).  gp_out (dict): receives the parts.  labels
    (tests only): {'unl', 'unl_d'} one-hot labels to use instead of the arg-max of the classifier's logits (oracle/step_goodgan.d_phase)."""
    P = st['P']
    Gimg, _ = NC.generator_fwd(P, b['z_g'], b['y_g'], moving=P)
    pops = {}
    c_unl, _, _ = NC.classifier_fwd(P, NC.zca_apply(b['x_u_c'], *zca), True, rnd['C_unl'], pops)
    c_unl_d, _, _ = NC.classifier_fwd(P, NC.zca_apply(b['x_u_d'], *zca), True, rnd['C_unl_d'], pops)
    SC._commit_pop(P, pops)
    X_P = np.concatenate([b['x_l_d'], b['x_u_d']], axis=0)
    oh_unl = T.argmax_onehot(c_unl) if labels is None else np.asarray(labels['unl'], c_unl.dtype)
    oh_unl_d = T.argmax_onehot(c_unl_d) if labels is None else np.asarray(labels['unl_d'], c_unl_d.dtype)
    Y_P = np.concatenate([b['y_l_d'], oh_unl_d], axis=0)
    parts = (('D_real', X_P, Y_P), ('D_fake', Gimg, b['y_g']), ('D_unl', b['x_u_c'], oh_unl))
    fwd = [NC.discriminator_fwd(P, img, y, rnd[key]) for key, img, y in parts]
    (d, wd1, wd2, wd3), dls = head_d(fwd[0][0], fwd[1][0], fwd[2][0], hyper['lambda_1'], hyper['lambda_2'])
    grads = {}
    for (key, _img, _y), (_logits, cache), dl in zip(parts, fwd, dls):
        g, _ = NC.discriminator_bwd(P, cache, dl, rnd[key])
        for k, v in g.items():
            grads[k] = grads.get(k, 0) + v
    gp10, gg = penalty('cifar10', P, X_P, Gimg, b['y_g'], rnd['GP'])
    if gp_out is not None:
        gp_out.update(gp10=gp10, gp_grads=gg, wd=(wd1, wd2, wd3), head_grads={k: v.copy() for k, v in grads.items()})
    for k, v in gg.items():
        grads[k] = grads[k] + v
    SC._adam(st, 'D', grads, hyper['lr'], hyper['beta1'])
    return float(d + gp10)


def g_phase_cifar10(st, b, rnd, hyper):
    P = st['P']
    Gimg, gc = NC.generator_fwd(P, b['z_g'], b['y_g'], moving=P)
    logits, c = NC.discriminator_fwd(P, Gimg, b['y_g'], rnd['D_fake'])
    _, dimg = NC.discriminator_bwd(P, c, np.full_like(logits, -1.0 / logits.shape[0]), rnd['D_fake'], want_weight_grads=False,
                                   want_input_grad=True)
    SC._adam(st, 'G', NC.generator_bwd(P, gc, dimg), hyper['lr'], hyper['beta1'])
    return float(-np.mean(logits))


def c_phase_cifar10(st, b, rnd, hyper, zca):
    P = st['P']
    Gimg, _ = NC.generator_fwd(P, b['z_g'], b['y_g'], moving=P)
    pops = {}
    x_u_c_z = NC.zca_apply(b['x_u_c'], *zca)
    c_real, _, cc_real = NC.classifier_fwd(P, NC.zca_apply(b['x_l_c'], *zca), True, rnd['C_real'], pops)
    NC.classifier_fwd(P, x_u_c_z, True, rnd['C_unl'], pops)                  # pop_mean chain as the GAN step; zero gradient
    NC.classifier_fwd(P, x_u_c_z, True, rnd['C_unl_rep'], pops)
    c_fake, _, cc_fake = NC.classifier_fwd(P, NC.zca_apply(Gimg, *zca), True, rnd['C_fake'], pops)
    SC._commit_pop(P, pops)
    lam2 = hyper['lambda_2']
    l_real, g_real = ce_mean(c_real, b['y_l_c'])
    l_fake, g_fake = ce_mean(c_fake, b['y_g'])
    grads = {}
    for cache, dl, key in ((cc_real, g_real, 'C_real'), (cc_fake, lam2 * g_fake, 'C_fake')):
        for k, v in NC.classifier_bwd(P, cache, dl, rnd[key]).items():
            grads[k] = grads.get(k, 0) + v
    SC._adam(st, 'C', grads, hyper['cla_lr'], 0.5)
    for k in st['ema']:
        st['ema'][k] = T.ema_update(st['ema'][k], P[k])
    return float(l_real + lam2 * l_fake)


# ---------------------------------------------------------------------------------------------------------------- MNIST / SVHN
def d_phase_goodgan(st, data, b, rnd, hyper, gp_out=None, labels=None):
    P = st['P']
    CL, DL = NG.classifier_layers(data), NG.discriminator_layers(data)
    bnu = {}
    Gimg, _, _ = SG._gen(P, data, b, bnu)
    c_unl, _, _ = NG.seq_fwd(P, CL, b['x_u_c'], None, rnd['C_unl'], True, bnu)
    c_unl_d, _, _ = NG.seq_fwd(P, CL, b['x_u_d'], None, rnd['C_unl_d'], True, bnu)
    NG.commit_bn(P, bnu)
    oh_unl = T.argmax_onehot(c_unl) if labels is None else np.asarray(labels['unl'], c_unl.dtype)
    oh_unl_d = T.argmax_onehot(c_unl_d) if labels is None else np.asarray(labels['unl_d'], c_unl_d.dtype)
    st['last_logits'] = {'unl': c_unl, 'unl_d': c_unl_d}
    X_P = np.concatenate([b['x_l_d'], b['x_u_d']], axis=0)
    Y_P = np.concatenate([b['y_l_d'], oh_unl_d], axis=0)
    gimg = Gimg.reshape((-1,) + X_P.shape[1:])
    parts = (('D_real', X_P, Y_P), ('D_fake', gimg, b['y_g']), ('D_unl', b['x_u_c'], oh_unl))
    fwd = [NG.seq_fwd(P, DL, img, y, rnd[key], True) for key, img, y in parts]
    (d, wd1, wd2, wd3), dls = head_d(fwd[0][0], fwd[1][0], fwd[2][0], hyper['lambda_1'], hyper['lambda_2'])
    grads = {}
    for (key, _img, y), (_logits, caches, _), dl in zip(parts, fwd, dls):
        g, _ = NG.seq_bwd(P, DL, caches, dl, y, rnd[key])
        for k, v in g.items():
            grads[k] = grads.get(k, 0) + v
    gp10, gg = penalty(data, P, X_P, gimg, b['y_g'], rnd['GP'])
    if gp_out is not None:
        gp_out.update(gp10=gp10, gp_grads=gg, wd=(wd1, wd2, wd3), head_grads={k: v.copy() for k, v in grads.items()})
    for k, v in gg.items():
        grads[k] = grads.get(k, 0) + v
    SC._adam(st, 'D', grads, hyper['lr'], hyper['beta1'])
    return float(d + gp10)


def g_phase_goodgan(st, data, b, rnd, hyper):
    P = st['P']
    GL, DL = NG.generator_layers(data), NG.discriminator_layers(data)
    bnu = {}
    Gimg, gc, _ = NG.seq_fwd(P, GL, b['z_g'], b['y_g'], {}, True, bnu)
    NG.commit_bn(P, bnu)
    img = Gimg.reshape((-1,) + NG.image_shape(data))
    logits, dc, _ = NG.seq_fwd(P, DL, img, b['y_g'], rnd['D_fake'], True)
    _, dimg = NG.seq_bwd(P, DL, dc, np.full_like(logits, -1.0 / logits.shape[0]), b['y_g'], rnd['D_fake'], want_params=False)
    grads, _ = NG.seq_bwd(P, GL, gc, dimg.reshape(Gimg.shape), b['y_g'], {})
    SC._adam(st, 'G', grads, hyper['lr'], hyper['beta1'])
    return float(-np.mean(logits))


def c_phase_goodgan(st, data, b, rnd, hyper):
    P = st['P']
    CL = NG.classifier_layers(data)
    bnu = {}
    Gimg, _, _ = SG._gen(P, data, b, bnu)
    gimg = Gimg.reshape((-1,) + NG.image_shape(data))
    c_real, cc_real, _ = NG.seq_fwd(P, CL, b['x_l_c'], None, rnd['C_real'], True, bnu)
    NG.seq_fwd(P, CL, b['x_u_c'], None, rnd['C_unl'], True, bnu)                 # moving statistics as the GAN step; zero gradient
    c_fake, cc_fake, _ = NG.seq_fwd(P, CL, gimg, None, rnd['C_fake'], True, bnu)
    NG.commit_bn(P, bnu)
    lam2 = hyper['lambda_2']
    l_real, g_real = ce_mean(c_real, b['y_l_c'])
    l_fake, g_fake = ce_mean(c_fake, b['y_g'])
    grads = {}
    for caches, dl, key in ((cc_real, g_real, 'C_real'), (cc_fake, lam2 * g_fake, 'C_fake')):
        g, _ = NG.seq_bwd(P, CL, caches, dl, None, rnd[key])
        for k, v in g.items():
            grads[k] = grads.get(k, 0) + v
    SC._adam(st, 'C', grads, hyper['cla_lr'], 0.5)
    for k in st['ema']:
        st['ema'][k] = T.ema_update(st['ema'][k], P[k])
    return float(l_real + lam2 * l_fake)


def train_step(data, st, b, rnd, hyper, zca=None):
    """one iteration D -> G -> C; data 'cifar10' | 'mnist' | 'svhn'.  Returns (d_loss, g_loss, c_loss)."""
    if data == 'cifar10':
        return (d_phase_cifar10(st, b, rnd['D'], hyper, zca), g_phase_cifar10(st, b, rnd['G'], hyper),
                c_phase_cifar10(st, b, rnd['C'], hyper, zca))
    return (d_phase_goodgan(st, data, b, rnd['D'], hyper), g_phase_goodgan(st, data, b, rnd['G'], hyper),
            c_phase_goodgan(st, data, b, rnd['C'], hyper))


def gp_draws(data, n, seed, dtype=np.float32):
    """rnd['D']['GP'] of one iteration: alpha ~ U[0,1) per image and the penalty's masks / noise."""
    rng = np.random.default_rng(seed)
    out = {'alpha': rng.random(n).astype(dtype)}
    if data == 'cifar10':
        out.update({'drop0': (rng.random((n, 32, 32, 3)) < 0.8).astype(dtype), 'drop1': (rng.random((n, 16, 16, 32)) < 0.8).astype(dtype),
                    'drop2': (rng.random((n, 8, 8, 64)) < 0.8).astype(dtype)})
    else:
        out.update({k: v.astype(dtype) for k, v in RG.draws(data, n, rng).items()})
    return out
