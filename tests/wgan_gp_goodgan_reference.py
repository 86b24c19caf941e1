"""Float64 restatement of the WGAN-GP penalty of Train_base (reference Training/train_base.py:598-620) on the MNIST and SVHN
discriminators of oracle.nets_goodgan.discriminator_layers(data), with the parameter gradient written as the four first-order sweeps of
DESIGN §9.1 plus the weight-norm chain:

  forward (the lrelu activations, whose signs are lrelu'), input-gradient sweep seeded with 1 per image (pre-activation gradients dpre_k,
  gx = d sum(logits) / dx), slopes s = sqrt(sum over axis 1 of gx^2), gp = mean((s - 1)^2), r = d gp / d gx, a tangent forward from r
  (zero label channels, no biases, * lrelu', the same dropout masks, no noise), dW_eff_k = wgrad(tangent input of layer k, dpre_k), and
  dV, dg from dW_eff through W = g V/||V||; every bias gradient is 0.

Axis 1 is that of the tensor passed in: the feature axis of a rank-2 MNIST batch [N, 784] (one slope per image), H of an NHWC batch.
test_wgan_gp_goodgan_reference.py pins this against torch's double backward; the GPU tests pin the HIP path against this."""
import numpy as np

from oracle import nets_goodgan as N
from oracle import tf_ops as T

NCLS = N.NCLS
N_MNIST_WIDTHS = (1000, 500, 250, 250, 250)            # d_h0_wndense0 .. d_h4_wndense0


def interpolate(real, fake, alpha):
    """x = real + alpha (fake - real), one alpha per image (train_base.py:601-606)."""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    return real + np.asarray(alpha, np.float64).reshape((-1,) + (1,) * (real.ndim - 1)) * (fake - real)


def weff(P, name):
    """the effective filter g V/||V|| (norm over every axis but the last) of a weight-normalised layer."""
    return T.wn_weight(P[name + '/V'], P[name + '/g'], -1)


def gradient_penalty(data, P, x, y, rnd, acts=None, lrelu_from='pre_noise', wn_chain=True):
    """gp and d gp / d theta_D of the `data` ('mnist' / 'svhn') discriminator at the (already interpolated) images x — MNIST [N,784] or
    [N,28,28,1], SVHN [N,32,32,3] — with labels y [N,10] and the draws rnd ('drop0..2' keep masks / 'noise0..5' scaled noise).
    acts: optional list of the lrelu activations in layer order (the HIP forward's, taken before the noise) whose signs replace the
    restatement's own as lrelu'.  Negative controls: lrelu_from='post_noise' takes lrelu' from the activation after its additive noise;
    wn_chain=False writes dW_eff straight into dV.  Returns dict(gp, grads, gx, r, slopes, dpre, dweff)."""
    layers = N.discriminator_layers(data)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    rnd = {k: np.asarray(v, np.float64) for k, v in rnd.items()}
    n = x.shape[0]
    W = {l[1]: weff(P, l[1]) for l in layers if l[0] in ('wn_conv', 'wn_dense')}
    # ---- sweep 1: forward; sgn[i] is the tensor whose sign gives lrelu' of the i-th activation
    h, sgn, shapes = x, [], {}
    for i, l in enumerate(layers):
        k = l[0]
        shapes[i] = h.shape
        if k == 'reshape':
            h = h.reshape((n,) + tuple(l[1]))
        elif k == 'noise':
            h = h + rnd[l[1]].reshape(h.shape)
            if lrelu_from == 'post_noise' and layers[i - 1][0] == 'act':
                sgn[-1] = sgn[-1] + rnd[l[1]].reshape(h.shape)
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
            assert l[1] == 'lrelu'
            h = T.lrelu(h, 0.2)
            sgn.append(h if acts is None else np.asarray(acts[len(sgn)], np.float64).reshape(h.shape))
        elif k == 'gmean':
            h = h.mean(axis=(1, 2))
        else:
            raise ValueError(k)
    # ---- sweep 2: d sum(logits) / dx, seeded with 1 per image; dpre[name] = gradient at the layer's pre-activation
    d, dpre, ia = np.ones((n, 1)), {}, len(sgn)
    for i in range(len(layers) - 1, -1, -1):
        l = layers[i]
        k = l[0]
        if k == 'reshape':
            d = d.reshape(shapes[i])
        elif k in ('concat_y', 'cond_concat'):
            d = d[..., :-NCLS]
        elif k == 'dropout':
            d = T.dropout_bwd(d, rnd[l[1]], l[2])
        elif k == 'wn_conv':
            dpre[l[1]] = d
            d = T.conv2d_bwd_input(shapes[i], W[l[1]], d, (l[3], l[3]), 'SAME')
        elif k == 'wn_dense':
            dpre[l[1]] = d
            d = d @ W[l[1]].T
        elif k == 'act':
            ia -= 1
            d = T.lrelu_bwd_from_out(sgn[ia], d, 0.2)
        elif k == 'gmean':
            hh, ww = shapes[i][1:3]
            d = np.broadcast_to(d[:, None, None, :] / (hh * ww), shapes[i]).copy()
    gx = d
    # ---- the penalty: reduce_sum over axis 1 of the tensor passed in
    sl = np.sqrt(np.sum(gx ** 2, axis=1, keepdims=True))
    gp = float(np.mean((sl - 1.0) ** 2))
    r = 2.0 * (sl - 1.0) / sl * gx / sl.size
    # ---- sweeps 3 and 4: tangent forward from r, dW_eff against dpre, then the weight-norm chain
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
    grads, dweff = {}, {}
    for l in layers:
        if l[0] not in ('wn_conv', 'wn_dense'):
            continue
        name = l[1]
        V, g = P[name + '/V'], P[name + '/g']
        if l[0] == 'wn_conv':
            dw = T.conv2d_bwd_filter(tin[name], dpre[name], V.shape, (l[3], l[3]), 'SAME')
        else:
            dw = tin[name].T @ dpre[name]
        dweff[name] = dw
        dv, dg = T.wn_weight_bwd(V, g, dw, -1)
        grads[name + '/V'] = dv if wn_chain else dw
        grads[name + '/g'] = dg
        grads[name + '/b'] = np.zeros(g.shape)
    return dict(gp=gp, grads=grads, gx=gx, r=r, slopes=sl, dpre=dpre, dweff=dweff)


def draws(data, n, rng, dtype=np.float64):
    """the penalty's random draws in the RNG scope 'GP': keep masks (SVHN, keep 0.8) or noise (MNIST, std 0.2)."""
    if data == 'mnist':
        widths = (784,) + N_MNIST_WIDTHS
        return {'noise%d' % i: (0.2 * rng.standard_normal((n, wd))).astype(dtype) for i, wd in enumerate(widths)}
    return {'drop0': np.floor(0.8 + rng.random((n, 32, 32, 3))).astype(dtype), 'drop1': np.floor(0.8 + rng.random((n, 16, 16, 32))).astype(dtype),
            'drop2': np.floor(0.8 + rng.random((n, 8, 8, 64))).astype(dtype)}

