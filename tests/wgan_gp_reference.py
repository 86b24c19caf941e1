"""Float64 restatement of the WGAN-GP loss of Train_base (reference Training/train_base.py:576-620) on the CIFAR-10 discriminator of
oracle.nets_cifar10, with the parameter gradient of the penalty written as the four first-order sweeps of DESIGN §9.1:

  forward (activations y_k), input-gradient sweep seeded with 1 per image (pre-activation gradients dpre_k, gx = d sum(logits) / dx),
  slopes s = sqrt(sum over H of gx^2), gp = mean((s - 1)^2), r = d gp / d gx, a tangent forward from r through the same masks
  (zero labels, no biases), and d gp / dW_k = conv2d_bwd_filter(tangent input of layer k, dpre_k); d gp / d w_lin = sum over images of
  the pooled tangent; every bias gradient is 0.

test_wgan_gp_reference.py pins this against torch's double backward; the GPU tests pin the HIP path against this."""
import numpy as np

from oracle import nets_cifar10 as N
from oracle import tf_ops as T

NCLS = N.NUM_CLASSES


def interpolate(real, fake, alpha):
    """x = real + alpha (fake - real), one alpha per image (train_base.py:601-606)."""
    return real + np.asarray(alpha).reshape(-1, 1, 1, 1) * (fake - real)


def gradient_penalty(P, x, y, rnd, acts=None, slope_axes=(1,), mask_tangent=True):
    """gp and d gp / d theta_D at the (already interpolated) images x [N,32,32,3] with labels y [N,10] and keep masks rnd
    ('drop0', 'drop1', 'drop2').  acts: optional {layer name: activation} whose signs replace the restatement's own as lrelu'
    (the HIP forward's stored activations — controls for kinks).  slope_axes / mask_tangent: the negative controls (a per-image
    norm is (1, 2, 3); a tangent without the image's dropout mask).  Returns dict(gp, grads, gx, r, slopes, dpre)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    rnd = {k: np.asarray(v, np.float64) for k, v in rnd.items()}
    n = x.shape[0]
    _, c = N.discriminator_fwd(P, x, y, rnd)
    if acts is not None:
        for name, a in acts.items():
            c[name + '/y'] = np.asarray(a, np.float64)
    # input-gradient sweep, seeded with 1 per image
    w_lin = P['discriminator/lin/lin/kernel']
    d = (np.ones((n, 1)) @ w_lin.T)[:, :c['pool/shape'][-1]]
    d = T.global_avgpool_bwd(d, c['pool/shape'])
    dpre = {}
    for name, cout, s, drop in reversed(N.D_CONVS):
        p = 'discriminator/%s/%s/' % (name, name)
        if drop:
            d = T.dropout_bwd(d, rnd[drop], 0.2)
        d = T.lrelu_bwd_from_out(c[name + '/y'], d)
        dpre[name] = d
        xin = c[name + '/x']
        d = T.conv2d_bwd_input(xin.shape, P[p + 'kernel'], d, (s, s), 'SAME')[..., :xin.shape[-1] - NCLS]
    gx = T.dropout_bwd(d, rnd['drop0'], 0.2)
    # the penalty: reduce_sum over axis 1 of NHWC (H) — not the per-image norm
    ss = np.sum(gx ** 2, axis=slope_axes, keepdims=True)
    sl = np.sqrt(ss)
    gp = float(np.mean((sl - 1.0) ** 2))
    r = 2.0 * (sl - 1.0) / sl * gx / sl.size
    # tangent forward from r, filter gradients against dpre
    zy = np.zeros_like(y)
    t = T.dropout(r, rnd['drop0'], 0.2) if mask_tangent else r
    grads = {}
    for name, cout, s, drop in N.D_CONVS:
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
    return dict(gp=gp, grads=grads, gx=gx, r=r, slopes=sl, dpre=dpre)


def wgan_loss_head(d_real, d_fake, d_unl, lam1, lam2):
    """train_base.py:583-589 without the penalty: (d_loss, g_loss, wd1, wd2, wd3), d d_loss / d[real | fake | unl] rows,
    d g_loss / d fake rows."""
    d_real, d_fake, d_unl = (np.asarray(a, np.float64).reshape(-1) for a in (d_real, d_fake, d_unl))
    mr, mf, mu = d_real.mean(), d_fake.mean(), d_unl.mean()
    wd1, wd2, wd3 = 0.5 * (mr - mf), 0.5 * (mr - mu), 0.5 * (mu - mf)
    d_loss = -(wd1 + lam1 * wd2 + lam2 * wd3)
    g = np.concatenate([np.full(d_real.size, (-0.5 - 0.5 * lam1) / d_real.size), np.full(d_fake.size, (0.5 + 0.5 * lam2) / d_fake.size),
                        np.full(d_unl.size, (0.5 * lam1 - 0.5 * lam2) / d_unl.size)])
    return (d_loss, -mf, wd1, wd2, wd3), g, np.full(d_fake.size, -1.0 / d_fake.size)


def c_loss(c_real, c_fake, y, lam2):
    """c_loss = CE(Y, C_real) + lambda_2 CE(Y, C_fake) (train_base.py:591-599) and its logit gradients."""
    def ce(z):
        z = np.asarray(z, np.float64)
        m = z.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
        p = np.exp(z - lse)
        return float(np.mean(np.sum(y * (lse - z), axis=1))), (p - y) / z.shape[0]
    y = np.asarray(y, np.float64)
    vr, gr = ce(c_real)
    vf, gf = ce(c_fake)
    return vr + lam2 * vf, gr, lam2 * gf
