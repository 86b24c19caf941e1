"""Float64 restatement of the R1 gradient penalty (config.R1_GAMMA; Mescheder, Geiger, Nowozin 2018 — not in the reference)
on the three discriminators, and of the D-update that carries it.

For real rows x_i with their own labels y_i and g_i = d D_logit(x_i, y_i) / d x_i (image elements only):

    R1 = gamma / 2 * mean_i ||g_i||^2      (the norm over ALL elements of image i),      r_i = d R1 / d g_i = gamma / n * g_i

and the parameter gradient is DESIGN §9.1's identity with this r.  Sweeps 1 and 2 (forward, input gradient gx, pre-activation gradients
dpre) are those of tests/wgan_gp_reference.py / wgan_gp_goodgan_reference.py, taken from there; the tangent forward from r and the filter
gradients are restated here, on the oracle's helpers.  test_r1_reference.py pins this against torch's double backward; the GPU tests pin
the HIP path against it."""
import copy

import numpy as np

from oracle import nets_cifar10 as NC
from oracle import nets_goodgan as NG
from oracle import step_cifar10 as SC
from oracle import tf_ops as T

import wgan_gp_goodgan_reference as RG
import wgan_gp_reference as RC
import wgan_gp_step_reference as RS


def r1_value(gx, gamma):
    """(R1, mean_i ||g_i||^2, r) of an input gradient gx [N, ...] in float64."""
    gx = np.asarray(gx, np.float64)
    n = gx.shape[0]
    m = float(np.mean(np.sum(gx.reshape(n, -1) ** 2, axis=1)))
    return 0.5 * gamma * m, m, gamma / n * gx


def penalty_kernel32(gx, gamma, n=None):
    """the float32 restatement of tg_r1_penalty_f32's r: ONE fp32 multiply per element by scale = (float)((double)gamma / (double)n)."""
    gx = np.asarray(gx, np.float32)
    n = gx.shape[0] if n is None else n
    scale = np.float32(np.float64(np.float32(gamma)) / np.float64(n))
    return gx * scale


def _f64(d):
    return {k: np.asarray(v, np.float64) for k, v in d.items()}


def r1_cifar10(P, x, y, rnd, gamma, acts=None):
    """R1 and d R1 / d theta_D of the CIFAR-10 discriminator at the real images x [N,32,32,3] with labels y and keep masks rnd ('drop0..2').
    acts: optional {layer name: activation} whose signs replace the restatement's own as lrelu'.  -> dict(penalty, grad_sq_mean, grads, gx, r)."""
    x, y, P, rnd = np.asarray(x, np.float64), np.asarray(y, np.float64), _f64(P), _f64(rnd)
    with np.errstate(all='ignore'):                                  # (WGAN's own r divides by the slope: not used here)
        base = RC.gradient_penalty(P, x, y, rnd, acts=acts)          # sweeps 1, 2: gx and dpre do not depend on the penalty kind
    gx, dpre = base['gx'], base['dpre']
    pen, m, r = r1_value(gx, gamma)
    _, c = NC.discriminator_fwd(P, x, y, rnd)
    if acts is not None:
        for name, a in acts.items():
            c[name + '/y'] = np.asarray(a, np.float64)
    zy = np.zeros_like(y)
    t = T.dropout(r, rnd['drop0'], 0.2)
    grads = {}
    for name, cout, s, drop in NC.D_CONVS:
        p = 'discriminator/%s/%s/' % (name, name)
        t = T.conv_cond_concat(t, zy)
        grads[p + 'kernel'] = T.conv2d_bwd_filter(t, dpre[name], P[p + 'kernel'].shape, (s, s), 'SAME')
        grads[p + 'bias'] = np.zeros(cout)
        t = T.lrelu_bwd_from_out(c[name + '/y'], T.conv2d(t, P[p + 'kernel'], (s, s), 'SAME'))
        if drop:
            t = T.dropout(t, rnd[drop], 0.2)
    th = np.concatenate([T.global_avgpool(t), zy], axis=1)
    grads['discriminator/lin/lin/kernel'] = th.sum(axis=0)[:, None]
    grads['discriminator/lin/lin/bias'] = np.zeros(1)
    return dict(penalty=pen, grad_sq_mean=m, grads=grads, gx=gx, r=r)


def _signs_goodgan(data, P, W, x, y, rnd, acts):
    """the lrelu activations (before their additive noise) of the `data` discriminator's forward pass, in layer order."""
    n, h, sgn = x.shape[0], x, []
    for l in NG.discriminator_layers(data):
        k = l[0]
        if k == 'reshape':
            h = h.reshape((n,) + tuple(l[1]))
        elif k == 'noise':
            h = h + rnd[l[1]].reshape(h.shape)
        elif k == 'concat_y':
            h = np.concatenate([h, y], axis=1)
        elif k == 'cond_concat':
            h = T.conv_cond_concat(h, y)
        elif k == 'dropout':
            h = T.dropout(h, rnd[l[1]], l[2])
        elif k == 'wn_conv':
            h = T.conv2d(h, W[l[1]], (l[3], l[3]), 'SAME') + P[l[1] + '/b']
        elif k == 'wn_dense':
            h = h @ W[l[1]] + P[l[1] + '/b']
        elif k == 'act':
            h = T.lrelu(h, 0.2)
            sgn.append(h if acts is None else np.asarray(acts[len(sgn)], np.float64).reshape(h.shape))
        elif k == 'gmean':
            h = h.mean(axis=(1, 2))
        else:
            raise ValueError(k)
    return sgn


def r1_goodgan(data, P, x, y, rnd, gamma, acts=None):
    """R1 and d R1 / d theta_D of the `data` ('mnist' / 'svhn') discriminator at the real images x — MNIST [N,784] or [N,28,28,1] (the
    same penalty: the norm is per image), SVHN [N,32,32,3] — with labels y and the draws rnd ('drop0..2' / 'noise0..5').  acts: optional
    list of the lrelu activations in layer order.  -> dict(penalty, grad_sq_mean, grads, gx, r)."""
    x, y, P, rnd = np.asarray(x, np.float64), np.asarray(y, np.float64), _f64(P), _f64(rnd)
    layers = NG.discriminator_layers(data)
    with np.errstate(all='ignore'):
        base = RG.gradient_penalty(data, P, x, y, rnd, acts=acts)    # sweeps 1, 2
    gx, dpre = base['gx'], base['dpre']
    pen, m, r = r1_value(gx, gamma)
    W = {l[1]: RG.weff(P, l[1]) for l in layers if l[0] in ('wn_conv', 'wn_dense')}
    sgn = _signs_goodgan(data, P, W, x, y, rnd, acts)
    n = x.shape[0]
    t, tin, ia = r, {}, 0
    for l in layers:
        k = l[0]
        if k == 'reshape':
            t = t.reshape((n,) + tuple(l[1]))
        elif k == 'concat_y':
            t = np.concatenate([t, np.zeros_like(y)], axis=1)
        elif k == 'cond_concat':
            t = T.conv_cond_concat(t, np.zeros_like(y))
        elif k == 'dropout':
            t = T.dropout(t, rnd[l[1]], l[2])
        elif k == 'wn_conv':
            tin[l[1]] = t
            t = T.conv2d(t, W[l[1]], (l[3], l[3]), 'SAME')
        elif k == 'wn_dense':
            tin[l[1]] = t
            t = t @ W[l[1]]
        elif k == 'act':
            t = T.lrelu_bwd_from_out(sgn[ia], t, 0.2)
            ia += 1
        elif k == 'gmean':
            t = t.mean(axis=(1, 2))
    grads = {}
    for l in layers:
        if l[0] not in ('wn_conv', 'wn_dense'):
            continue
        name = l[1]
        V, g = P[name + '/V'], P[name + '/g']
        dw = T.conv2d_bwd_filter(tin[name], dpre[name], V.shape, (l[3], l[3]), 'SAME') if l[0] == 'wn_conv' else tin[name].T @ dpre[name]
        grads[name + '/V'], grads[name + '/g'] = T.wn_weight_bwd(V, g, dw, -1)
        grads[name + '/b'] = np.zeros(g.shape)
    return dict(penalty=pen, grad_sq_mean=m, grads=grads, gx=gx, r=r)


def r1(data, P, x, y, rnd, gamma, acts=None):
    """data 'cifar10' | 'mnist' | 'svhn'."""
    return r1_cifar10(P, x, y, rnd, gamma, acts) if data == 'cifar10' else r1_goodgan(data, P, x, y, rnd, gamma, acts)


# ---------------------------------------------------------------------------------------------------------------- the D-update
def d_phase(data, st, b, rnd, hyper, gamma, zca=None, out=None, labels=None):
    """the D-update with the GAN loss and R1 (Training/Train_goodGAN.py with config.R1_GAMMA): d_loss = the oracle's GAN d_loss + R1 at
    X_P = [x_l_d | x_u_d] with the labels [y_l_d | oh_unl_d] and the draws rnd['R1']; Adam on the summed gradient.  rnd: the oracle's
    rnd['D'] plus 'R1'.  The GAN part IS the oracle's d_phase (oracle/step_cifar10.py, step_goodgan.py), run on a copy of the state: its
    gradient and everything but the discriminator's Adam step are taken from there, the step is redone with the penalty's gradient
    added.  labels: as the oracle's.  out (dict): receives the parts.  Returns d_loss."""
    new = copy.deepcopy(st)
    if data == 'cifar10':
        d = SC.d_phase(new, b, rnd, hyper, zca, labels=labels)
    else:
        d = RS.SG.d_phase(new, data, b, rnd, hyper, labels=labels)
    head = new['last_grads']['D']
    for k in head:                                                    # undo the oracle's Adam step on D
        new['P'][k], new['m'][k], new['v'][k] = st['P'][k], st['m'][k], st['v'][k]
    new['t']['D'] = st['t']['D']
    oh_unl_d = T.argmax_onehot(new['last_logits']['unl_d']) if labels is None else np.asarray(labels['unl_d'])
    X_P = np.concatenate([b['x_l_d'], b['x_u_d']], axis=0)
    Y_P = np.concatenate([b['y_l_d'], oh_unl_d], axis=0)
    xr = X_P.reshape(X_P.shape[0], -1) if data == 'mnist' else X_P     # MNIST: [N, 784], the layout as_image() gives the penalty
    pen = r1(data, {k: v for k, v in st['P'].items() if k.startswith('discriminator/')}, xr, Y_P, rnd['R1'], gamma)
    if out is not None:
        out.update(gan_d_loss=d, penalty=pen['penalty'], grad_sq_mean=pen['grad_sq_mean'], r1_grads=pen['grads'],
                   head_grads={k: np.array(v, copy=True) for k, v in head.items()}, Y_P=Y_P)
    SC._adam(new, 'D', {k: head[k] + pen['grads'][k].reshape(np.shape(head[k])) for k in head}, hyper['lr'], hyper['beta1'])
    st.clear()
    st.update(new)
    return float(d + pen['penalty'])


def r1_draws(data, n, seed, dtype=np.float32):
    """rnd['D']['R1'] of one iteration: the penalty's masks / noise (no alpha)."""
    return {k: v for k, v in RS.gp_draws(data, n, seed, dtype).items() if k != 'alpha'}
