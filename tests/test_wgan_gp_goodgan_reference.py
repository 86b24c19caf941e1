"""CPU checks of the WGAN-GP penalty on the MNIST and SVHN discriminators (Good_GAN.discriminator_gradient_penalty, reference
Training/train_base.py:598-620 on Model/Good_GAN.py:89-206): the float64 four-sweep restatement of tests/wgan_gp_goodgan_reference.py
(with the weight-norm chain) against torch's double backward on the real shapes, both MNIST layouts, two negative controls, and the
package surface of the feature (the row-wise penalty entry point declared, exported and thunked; the refusals of the model)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import wgan_gp_goodgan_reference as R
from oracle import nets_goodgan as N
from test_oracle_goodgan import scrambled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('tg_grad_penalty_rows_f32',)


def _case(data, n, seed, layout='rows'):
    rng = np.random.default_rng(seed)
    P = {k: v for k, v in scrambled(data, seed).items() if k.startswith('discriminator/')}
    if data == 'mnist':
        x = rng.random((n, 784)) if layout == 'rows' else rng.random((n, 28, 28, 1))
    else:
        x = rng.uniform(-1, 1, (n, 32, 32, 3))
    y = np.eye(10)[rng.integers(0, 10, n)]
    return P, x, y, R.draws(data, n, rng)


def _torch_double_backward(data, P, x, y, rnd):
    """gp and d gp / d theta of the discriminator through torch.autograd.grad(create_graph=True), weight norm as W = g V/||V||."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    params = {k: t(v).requires_grad_(True) for k, v in P.items()}
    xt = t(x).requires_grad_(True)
    yt = t(y)
    n = x.shape[0]

    def weff(name):
        V, g = params[name + '/V'], params[name + '/g']
        dims = tuple(range(V.dim() - 1))
        return g * V / torch.sqrt((V ** 2).sum(dim=dims, keepdim=True))

    h = xt
    for l in N.discriminator_layers(data):
        k = l[0]
        if k == 'reshape':
            h = h.reshape((n,) + tuple(l[1]))
        elif k == 'noise':
            h = h + t(rnd[l[1]]).reshape(h.shape)
        elif k == 'concat_y':
            h = torch.cat([h, yt], dim=1)
        elif k == 'cond_concat':
            h = torch.cat([h, yt.reshape(n, 1, 1, 10).expand(n, h.shape[1], h.shape[2], 10)], dim=3)
        elif k == 'dropout':
            h = h * t(rnd[l[1]]) / (1.0 - l[2])
        elif k == 'wn_conv':
            s = l[3]
            hin = h.permute(0, 3, 1, 2)
            size = hin.shape[2]
            out = (size + s - 1) // s
            pad = max((out - 1) * s + 3 - size, 0)                   # TF 'SAME': the extra pixel goes after
            hin = F.pad(hin, (pad // 2, pad - pad // 2, pad // 2, pad - pad // 2))
            h = F.conv2d(hin, weff(l[1]).permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1) + params[l[1] + '/b']
        elif k == 'wn_dense':
            h = h @ weff(l[1]) + params[l[1] + '/b']
        elif k == 'act':
            h = F.leaky_relu(h, 0.2)
        elif k == 'gmean':
            h = h.mean(dim=(1, 2))
    gx, = torch.autograd.grad(h.sum(), xt, create_graph=True)
    slopes = torch.sqrt((gx ** 2).sum(dim=1))
    gp = ((slopes - 1.0) ** 2).mean()
    names = list(params)
    grads = torch.autograd.grad(gp, [params[k] for k in names], allow_unused=True)
    return float(gp.detach()), {k: (np.zeros(P[k].shape) if g is None else g.detach().numpy()) for k, g in zip(names, grads)}, gx.detach().numpy()


def _rel_l2(a, b):
    return np.linalg.norm(np.asarray(a) - b) / (np.linalg.norm(b) + 1e-300)


@pytest.mark.parametrize("data,layout,n", [('mnist', 'rows', 4), ('mnist', 'nhwc', 3), ('svhn', 'nhwc', 3)])
def test_restatement_matches_torch_double_backward(data, layout, n):
    P, x, y, rnd = _case(data, n, 11 + n, layout)
    ref = R.gradient_penalty(data, P, x, y, rnd)
    gp, grads, gx = _torch_double_backward(data, P, x, y, rnd)
    assert abs(ref['gp'] - gp) <= 1e-10 * abs(gp), (ref['gp'], gp)
    assert np.abs(ref['gx'] - gx).max() <= 1e-10 * np.abs(gx).max()
    assert set(ref['grads']) == set(grads)
    for k, g in grads.items():
        got = ref['grads'][k]
        assert got.shape == g.shape, k
        if k.endswith('/b'):
            assert not got.any() and np.abs(g).max() <= 1e-12, k       # torch reports the biases unused: exactly zero
        else:
            assert _rel_l2(got, g) <= 1e-8 and np.abs(got - g).max() <= 1e-8 * np.abs(g).max(), (k, _rel_l2(got, g))


def test_axis_rule_of_the_two_mnist_layouts():
    """rank-2 [N, 784]: axis 1 is the feature axis, one slope per image; [N,28,28,1]: axis 1 is H, one slope per (image, column).  The
    same images give different penalties."""
    P, x, y, rnd = _case('mnist', 3, 5)
    rows = R.gradient_penalty('mnist', P, x, y, rnd)
    img = R.gradient_penalty('mnist', P, x.reshape(3, 28, 28, 1), y, rnd)
    assert rows['slopes'].shape == (3, 1) and img['slopes'].shape == (3, 1, 28, 1)
    assert np.allclose(rows['gx'].reshape(3, 28, 28, 1), img['gx'], rtol=0, atol=1e-15)        # the same input gradient
    assert np.allclose(rows['slopes'][:, 0], np.sqrt((img['gx'] ** 2).sum(axis=(1, 2, 3))))
    assert abs(rows['gp'] - img['gp']) > 1e-3 * abs(img['gp'])


@pytest.mark.parametrize("data,layout", [('mnist', 'rows'), ('svhn', 'nhwc')])
def test_negative_control_without_the_weight_norm_chain(data, layout):
    """dW_eff written straight into dV misses the double backward by far more than 10x the GPU bound (1e-4 relative L2)."""
    P, x, y, rnd = _case(data, 3, 17, layout)
    _, grads, _ = _torch_double_backward(data, P, x, y, rnd)
    wrong = R.gradient_penalty(data, P, x, y, rnd, wn_chain=False)
    errs = [_rel_l2(wrong['grads'][k], g) for k, g in grads.items() if k.endswith('/V')]
    assert min(errs) >= 10 * 1e-4, errs


def test_negative_control_lrelu_slope_after_the_noise():
    """MNIST: lrelu' taken from the activation after its additive noise (instead of the pre-activation's sign) misses by more than 10x."""
    P, x, y, rnd = _case('mnist', 4, 19)
    _, grads, _ = _torch_double_backward('mnist', P, x, y, rnd)
    wrong = R.gradient_penalty('mnist', P, x, y, rnd, lrelu_from='post_noise')
    errs = {k: _rel_l2(wrong['grads'][k], g) for k, g in grads.items() if not k.endswith('/b')}
    assert max(errs.values()) >= 10 * 1e-4, errs
    assert abs(wrong['gp'] - R.gradient_penalty('mnist', P, x, y, rnd)['gp']) > 1e-4


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


def test_good_gan_has_the_penalty_and_train_base_names_what_remains():
    from Model.Good_GAN import Good_GAN
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10
    from Training.train_base import Train_base
    from tg import lib
    assert callable(getattr(Good_GAN, 'discriminator_gradient_penalty', None))
    assert Good_GAN.discriminator_gradient_penalty is not Good_GAN_cifar10.discriminator_gradient_penalty

    class NoPenalty(object):
        def discriminator(self):
            pass
    with pytest.raises(lib.TgError) as e:
        Train_base._gp_sweeps(NoPenalty().discriminator)
    msg = str(e.value)
    assert 'MINIBATCH_DIS' in msg and 'Good_GAN' in msg and 'MNIST / SVHN' in msg
