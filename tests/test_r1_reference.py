"""CPU checks of the R1 gradient penalty (config.R1_GAMMA): the float64 restatement of tests/r1_reference.py against torch's
autograd.grad(create_graph=True) on the real layer shapes of the three discriminators at n = 3 (the bounds of
tests/test_wgan_gp_reference.py: 1e-8 relative, biases exactly 0), an image whose input gradient is all zero, the per-image norm against
WGAN-GP's column norm, the float32 restatement of the kernel's r, and the package surface (entry point declared, exported, thunked; the
model and Train_base methods)."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import r1_reference as R
import wgan_gp_reference as RC
from oracle import nets_cifar10 as NC
from oracle import nets_goodgan as NG
from test_wgan_gp_goodgan_reference import _case as _case_goodgan
from test_wgan_gp_reference import _case as _case_cifar10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('tg_r1_penalty_f32',)
GAMMA = 10.0


def _case(data, n, seed):
    if data == 'cifar10':
        return _case_cifar10(n, seed)
    return _case_goodgan(data, n, seed, 'rows')


def _conv_same(F, h, w_hwio, s):
    hin = h.permute(0, 3, 1, 2)
    size = hin.shape[2]
    out = (size + s - 1) // s
    pad = max((out - 1) * s + 3 - size, 0)                           # TF 'SAME': the extra pixel goes after
    hin = F.pad(hin, (pad // 2, pad - pad // 2, pad // 2, pad - pad // 2))
    return F.conv2d(hin, w_hwio.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)


def _torch_r1(data, P, x, y, rnd, gamma):
    """R1 = gamma / 2 * mean_i ||d logit_i / d x_i||^2 and d R1 / d theta through torch's double backward, float64."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    params = {k: t(v).requires_grad_(True) for k, v in P.items()}
    xt, yt, n = t(x).requires_grad_(True), t(y), x.shape[0]
    cat = lambda h: torch.cat([h, yt.reshape(n, 1, 1, 10).expand(n, h.shape[1], h.shape[2], 10)], dim=3)
    if data == 'cifar10':
        h = xt * t(rnd['drop0']) / 0.8
        for name, cout, s, drop in NC.D_CONVS:
            p = 'discriminator/%s/%s/' % (name, name)
            h = F.leaky_relu(_conv_same(F, cat(h), params[p + 'kernel'], s) + params[p + 'bias'], 0.2)
            if drop:
                h = h * t(rnd[drop]) / 0.8
        h = torch.cat([h.mean(dim=(1, 2)), yt], dim=1) @ params['discriminator/lin/lin/kernel'] + params['discriminator/lin/lin/bias']
    else:
        def weff(name):
            V, g = params[name + '/V'], params[name + '/g']
            return g * V / torch.sqrt((V ** 2).sum(dim=tuple(range(V.dim() - 1)), keepdim=True))
        h = xt
        for l in NG.discriminator_layers(data):
            k = l[0]
            if k == 'reshape':
                h = h.reshape((n,) + tuple(l[1]))
            elif k == 'noise':
                h = h + t(rnd[l[1]]).reshape(h.shape)
            elif k == 'concat_y':
                h = torch.cat([h, yt], dim=1)
            elif k == 'cond_concat':
                h = cat(h)
            elif k == 'dropout':
                h = h * t(rnd[l[1]]) / (1.0 - l[2])
            elif k == 'wn_conv':
                h = _conv_same(F, h, weff(l[1]), l[3]) + params[l[1] + '/b']
            elif k == 'wn_dense':
                h = h @ weff(l[1]) + params[l[1] + '/b']
            elif k == 'act':
                h = F.leaky_relu(h, 0.2)
            elif k == 'gmean':
                h = h.mean(dim=(1, 2))
    gx, = torch.autograd.grad(h.sum(), xt, create_graph=True)
    pen = 0.5 * gamma * (gx.reshape(n, -1) ** 2).sum(dim=1).mean()
    names = list(params)
    grads = torch.autograd.grad(pen, [params[k] for k in names], allow_unused=True)
    return float(pen.detach()), {k: (np.zeros(P[k].shape) if g is None else g.detach().numpy()) for k, g in zip(names, grads)}, gx.detach().numpy()


def _is_bias(k):
    return k.endswith('/bias') or k.endswith('/b')


def _compare(ref, pen, grads, gx):
    assert abs(ref['penalty'] - pen) <= 1e-10 * abs(pen), (ref['penalty'], pen)
    assert np.abs(ref['gx'] - gx).max() <= 1e-10 * np.abs(gx).max()
    assert set(ref['grads']) == set(grads)
    for k, g in grads.items():
        got = ref['grads'][k]
        assert got.shape == g.shape, k
        if _is_bias(k):
            assert not got.any() and np.abs(g).max() <= 1e-12, k       # torch reports the biases unused: exactly zero
        else:
            assert np.isfinite(got).all() and np.abs(got - g).max() <= 1e-8 * np.abs(g).max(), (k, np.abs(got - g).max(), np.abs(g).max())


@pytest.mark.parametrize("data", ['cifar10', 'mnist', 'svhn'])
def test_restatement_matches_torch_double_backward(data):
    P, x, y, rnd = _case(data, 3, 31)
    _compare(R.r1(data, P, x, y, rnd, GAMMA), *_torch_r1(data, P, x, y, rnd, GAMMA))


def test_mnist_layouts_give_the_same_penalty():
    """the norm is per image: [N,784] and [N,28,28,1] are one penalty (WGAN-GP's axis rule tells them apart, R1 does not)."""
    P, x, y, rnd = _case('mnist', 3, 5)
    a, b = R.r1('mnist', P, x, y, rnd, GAMMA), R.r1('mnist', P, x.reshape(3, 28, 28, 1), y, rnd, GAMMA)
    assert a['penalty'] == pytest.approx(b['penalty'], rel=1e-13)
    for k in a['grads']:
        assert np.allclose(a['grads'][k], b['grads'][k], rtol=1e-12, atol=0)


@pytest.mark.parametrize("data", ['cifar10', 'svhn'])
def test_an_image_with_an_all_zero_gradient_gives_a_finite_result(data):
    """image 1 loses every input element to its dropout mask: g_1 = 0, r_1 = 0, and penalty and gradients stay finite and right."""
    P, x, y, rnd = _case(data, 3, 7)
    rnd = dict(rnd)
    rnd['drop0'] = np.array(rnd['drop0'], copy=True)
    rnd['drop0'][1] = 0.0
    ref = R.r1(data, P, x, y, rnd, GAMMA)
    assert not ref['gx'][1].any() and not ref['r'][1].any() and ref['gx'][0].any()
    assert np.isfinite(ref['penalty']) and all(np.isfinite(v).all() for v in ref['grads'].values())
    _compare(ref, *_torch_r1(data, P, x, y, rnd, GAMMA))


def test_the_norm_is_per_image_not_wgans_column_norm():
    P, x, y, rnd = _case('cifar10', 2, 2)
    ref = R.r1('cifar10', P, x, y, rnd, GAMMA)
    gx = ref['gx']
    assert ref['grad_sq_mean'] == pytest.approx(np.mean(np.sum(gx ** 2, axis=(1, 2, 3))), rel=1e-14)
    assert ref['penalty'] == pytest.approx(0.5 * GAMMA * ref['grad_sq_mean'], rel=1e-15)
    assert np.array_equal(ref['r'], GAMMA / 2 * gx)
    wgan = RC.gradient_penalty(P, x, y, rnd)
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    k = 'discriminator/lin/lin/kernel'
    assert rel(GAMMA * wgan['grads'][k], ref['grads'][k]) > 1e-2       # another regulariser, not a rescaling


def test_float32_restatement_of_r_is_one_multiply():
    rng = np.random.default_rng(0)
    g = rng.standard_normal((7, 5, 3)).astype(np.float32)
    for gamma, n in ((10.0, 7), (0.3, 7), (1e-3, 100)):
        r = R.penalty_kernel32(g, gamma, n)
        scale = np.float32(np.float64(np.float32(gamma)) / n)
        assert r.dtype == np.float32 and np.array_equal(r, g * scale)
        assert np.abs(r.astype(np.float64) - np.float64(np.float32(gamma)) / n * g).max() <= 2.0 ** -22 * np.abs(r).max()


def test_d_phase_adds_the_penalty_to_the_oracles_gan_step():
    """R1_reference.d_phase: everything but the discriminator's Adam step is the oracle's D-update; the step sees head + penalty."""
    from oracle import step_goodgan as SG
    import wgan_gp_step_reference as RS
    sizes = dict(B_G=4, L_C=2, U_C=3, L_D=2, U_D=2)
    from test_oracle_goodgan import scrambled
    P = scrambled('mnist', 3)
    b, rnd = SG.synth_batch('mnist', 5, sizes), SG.synth_rnd('mnist', 6, sizes)
    rnd['D']['R1'] = R.r1_draws('mnist', 4, 9)
    hyper = dict(lr=1e-3, cla_lr=1e-3, beta1=0.5, lambda_1=0.0, lambda_2=0.0)
    plain, with_r1, out = SG.new_state(dict(P)), SG.new_state(dict(P)), {}
    d0 = SG.d_phase(plain, 'mnist', b, rnd['D'], hyper)
    d1 = R.d_phase('mnist', with_r1, b, rnd['D'], hyper, GAMMA, out=out)
    assert d1 == pytest.approx(d0 + out['penalty'], rel=1e-12) and out['penalty'] > 0 and out['gan_d_loss'] == d0
    assert with_r1['t'] == plain['t']
    for k, v in plain['P'].items():
        if k.startswith('discriminator/'):
            continue
        assert np.array_equal(v, with_r1['P'][k]), k
    g0, g1 = plain['last_grads']['D'], with_r1['last_grads']['D']
    for k in g0:
        assert np.allclose(g1[k] - g0[k], out['r1_grads'][k].reshape(g0[k].shape), rtol=1e-5, atol=1e-12), k
    assert any(not np.array_equal(plain['P'][k], with_r1['P'][k]) for k in g0 if k.endswith('/V'))
    assert RS.GP_WEIGHT == 10.0                                           # (the WGAN restatement this module imports is untouched)


def test_entry_point_declared_exported_and_thunked():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_plan_thunks as gen
    header = open(os.path.join(ROOT, "include", "tg_kernels.h")).read()
    launches = dict(gen.launches())
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in launches, name
        assert all(t.endswith('*') or t in ('int', 'float') for t, _ in launches[name]), launches[name]
        kinds = [t for t, n in launches[name] if n == 'gamma_dev']
        assert kinds == ['const float*'], "gamma reaches the kernel through device memory: a replayed plan follows set_r1_gamma()"
    assert all(name in gen.render() for name in ENTRY_POINTS)
    from tg import lib
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    for name in ENTRY_POINTS:
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    assert set(ENTRY_POINTS) <= set(lib.parse_header())


def test_models_and_train_base_have_the_methods():
    from Model.Good_GAN import Good_GAN
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10
    from Model.Good_GAN_stress64 import Good_GAN_stress64
    from Training.Train_goodGAN import Train
    from Training.train_base import Train_base
    from tg import grad_penalty, lib
    for M in (Good_GAN, Good_GAN_cifar10):
        assert list(inspect.signature(M.discriminator_r1_penalty).parameters) == ['self', 'real', 'y', 'gamma', 'in_step']
    assert Good_GAN_stress64.discriminator_r1_penalty is Good_GAN_cifar10.discriminator_r1_penalty
    assert list(inspect.signature(Train_base._r1_penalty).parameters) == ['self', 'real', 'label', 'f', 'gamma']
    assert callable(Train.set_r1_gamma) and callable(Train.r1_terms)
    # one sweep body per discriminator family serves both penalties: the kinds differ in their rule objects only
    assert [p for p in inspect.signature(grad_penalty.conv_sweeps).parameters] == [p for p in inspect.signature(grad_penalty.mnist_sweeps).parameters]
    assert grad_penalty.R1.scope == 'R1' and grad_penalty.Wgan.scope == 'GP'
    for bad in (dict(mfma_dtype='bf16', minibatch_dis=False), dict(mfma_dtype='f32', minibatch_dis=True)):
        with pytest.raises(lib.TgError, match='discriminator_r1_penalty'):
            grad_penalty.check_supported(grad_penalty.R1.who, **bad)
