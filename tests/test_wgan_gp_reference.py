"""CPU checks of the WGAN-GP loss (Train_base._loss_WGAN_GP / _gradient_penalty, reference Training/train_base.py:576-620):
the float64 four-sweep restatement of tests/wgan_gp_reference.py against torch's double backward on the CIFAR-10 discriminator's real
shapes, and the package surface of the feature (entry points declared, exported and given plan thunks; the Train_base methods with the
reference's signatures)."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np

import wgan_gp_reference as R
from oracle import nets_cifar10 as N
from oracle import step_cifar10 as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('tg_wgan_interp_f32', 'tg_grad_penalty_f32', 'tg_wgan_loss_f32')


def _case(n, seed):
    rng = np.random.default_rng(seed)
    P = {k: np.asarray(v, np.float64) for k, v in S.init_params(0).items() if k.startswith('discriminator/')}
    x = rng.uniform(-1, 1, (n, 32, 32, 3))
    y = np.eye(10)[rng.integers(0, 10, n)]
    rnd = {'drop0': np.floor(0.8 + rng.random((n, 32, 32, 3))), 'drop1': np.floor(0.8 + rng.random((n, 16, 16, 32))),
           'drop2': np.floor(0.8 + rng.random((n, 8, 8, 64)))}
    return P, x, y, rnd


def _torch_double_backward(P, x, y, rnd):
    """gp and d gp / d theta of the discriminator (Good_GAN_cifar10.py:60-99) through torch.autograd.grad(create_graph=True)."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    params = {k: t(v).requires_grad_(True) for k, v in P.items()}
    xt = t(x).requires_grad_(True)
    yt = t(y)
    n = x.shape[0]
    h = xt * t(rnd['drop0']) / 0.8
    for name, cout, s, drop in N.D_CONVS:
        p = 'discriminator/%s/%s/' % (name, name)
        h = torch.cat([h, yt.reshape(n, 1, 1, 10).expand(n, h.shape[1], h.shape[2], 10)], dim=3)
        hin = h.permute(0, 3, 1, 2)
        size = hin.shape[2]
        out = (size + s - 1) // s
        pad = max((out - 1) * s + 3 - size, 0)                       # TF 'SAME': the extra pixel goes after
        hin = F.pad(hin, (pad // 2, pad - pad // 2, pad // 2, pad - pad // 2))
        z = F.conv2d(hin, params[p + 'kernel'].permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1) + params[p + 'bias']
        h = F.leaky_relu(z, 0.2)
        if drop:
            h = h * t(rnd[drop]) / 0.8
    feat = torch.cat([h.mean(dim=(1, 2)), yt], dim=1)
    logits = feat @ params['discriminator/lin/lin/kernel'] + params['discriminator/lin/lin/bias']
    gx, = torch.autograd.grad(logits.sum(), xt, create_graph=True)
    slopes = torch.sqrt((gx ** 2).sum(dim=1))
    gp = ((slopes - 1.0) ** 2).mean()
    names = list(params)
    grads = torch.autograd.grad(gp, [params[k] for k in names], allow_unused=True)
    return float(gp.detach()), {k: (np.zeros(P[k].shape) if g is None else g.detach().numpy()) for k, g in zip(names, grads)}, gx.detach().numpy()


def test_restatement_matches_torch_double_backward():
    P, x, y, rnd = _case(3, 1)
    ref = R.gradient_penalty(P, x, y, rnd)
    gp, grads, gx = _torch_double_backward(P, x, y, rnd)
    assert abs(ref['gp'] - gp) <= 1e-10 * abs(gp)
    assert np.abs(ref['gx'] - gx).max() <= 1e-10 * np.abs(gx).max()
    assert set(ref['grads']) == set(grads)
    for k, g in grads.items():
        got = ref['grads'][k]
        assert got.shape == g.shape, k
        if k.endswith('/bias'):
            assert not got.any() and np.abs(g).max() <= 1e-12, k       # torch reports the biases unused: exactly zero
        else:
            assert np.abs(got - g).max() <= 1e-8 * np.abs(g).max(), (k, np.abs(got - g).max(), np.abs(g).max())


def test_slopes_reduce_over_h_not_the_image():
    """the reference's axis 1 of an NHWC tensor is H: slopes has shape [N, W, C] (kept as [N, 1, W, C] here), and the per-image norm
    gives a different penalty."""
    P, x, y, rnd = _case(2, 2)
    ref = R.gradient_penalty(P, x, y, rnd)
    assert ref['slopes'].shape == (2, 1, 32, 3)
    per_image = R.gradient_penalty(P, x, y, rnd, slope_axes=(1, 2, 3))
    assert abs(per_image['gp'] - ref['gp']) > 1e-3 * abs(ref['gp'])


def test_loss_head_restatement():
    rng = np.random.default_rng(3)
    dr, df, du = rng.standard_normal(4), rng.standard_normal(5), rng.standard_normal(3)
    (d, g, wd1, wd2, wd3), gd, gg = R.wgan_loss_head(dr, df, du, 0.3, 0.5)
    eps = 1e-6
    z = np.concatenate([dr, df, du])
    for i in range(z.size):
        zp, zm = z.copy(), z.copy()
        zp[i] += eps
        zm[i] -= eps
        fd = (R.wgan_loss_head(zp[:4], zp[4:9], zp[9:], 0.3, 0.5)[0][0] - R.wgan_loss_head(zm[:4], zm[4:9], zm[9:], 0.3, 0.5)[0][0]) / (2 * eps)
        assert abs(fd - gd[i]) <= 1e-8
    assert abs(g + df.mean()) <= 1e-15 and np.allclose(gg, -1.0 / 5)
    assert abs(d + (wd1 + 0.3 * wd2 + 0.5 * wd3)) <= 1e-15


def test_entry_points_declared_exported_and_thunked():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_plan_thunks as gen
    header = open(os.path.join(ROOT, "include", "tg_kernels.h")).read()
    launches = dict(gen.launches())
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in launches, name
        assert all(t.endswith('*') or t in ('int', 'float') for t, _ in launches[name]), launches[name]
    assert all(name in gen.render() for name in ENTRY_POINTS)
    from tg import lib
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    for name in ENTRY_POINTS:
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    assert set(ENTRY_POINTS) <= set(lib.parse_header())


def test_train_base_has_the_reference_signatures():
    from Training.train_base import Train_base
    sig = list(inspect.signature(Train_base._loss_WGAN_GP).parameters)
    assert sig == ['self', 'G', 'D', 'C', 'X', 'Y', 'Lambda', 'discriminator']
    sig = list(inspect.signature(Train_base._gradient_penalty).parameters)
    assert sig[:5] == ['self', 'real', 'fake', 'label', 'f']
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10
    from Model.Good_GAN_stress64 import Good_GAN_stress64
    assert Good_GAN_stress64.discriminator_gradient_penalty is Good_GAN_cifar10.discriminator_gradient_penalty
