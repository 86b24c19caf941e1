"""GPU parity of the R1 gradient penalty through the models (Good_GAN.discriminator_r1_penalty, Good_GAN_cifar10.discriminator_r1_penalty;
config.R1_GAMMA) on CIFAR-10, MNIST and SVHN at n = 6 and CIFAR-10 also at n = 100, as tests/test_gpu_wgan_gp.py does:
the penalty and its parameter gradient against the float64 restatement of tests/r1_reference.py, evaluated with the HIP forward's own
draws and activation signs (last_gp_state).  Bounds: those of tests/test_gpu_wgan_gp.py for these very sweeps — the penalty 1e-5
relative, every gradient 1e-4 relative L2 and 1e-3 of the largest entry, biases exactly 0.  Two negative controls miss them by more than
10x: WGAN-GP's (s - 1)^2 column penalty at the same point, and the penalty with other labels than the real rows' own."""
import numpy as np
import pytest

import r1_reference as R
import wgan_gp_goodgan_reference as RG
import wgan_gp_reference as RC
from oracle import step_cifar10 as SC
from test_gpu_wgan_gp import _ctx, _gp_case as _case_cifar10, _grad_errors
from test_gpu_wgan_gp_goodgan import _flat_to_dict, _gp_case as _case_goodgan, _hip_state, _trainer

pytestmark = pytest.mark.gpu
GAMMA = 10.0


def _setup(data, n, seed):
    """(trainer, real, y, the other labels y_g, draws) with the draws injected under the penalty's own RNG scope 'R1'."""
    from tg.runtime import InjectedRNG
    if data == 'cifar10':
        tr, cx = _ctx()
        cx.stores['discriminator'].load_dict(SC.init_params(0))
        real, _fake, y, _alpha, rnd = _case_cifar10(n, seed)
    else:
        tr = _trainer(data)
        real, _fake, y, _alpha, rnd = _case_goodgan(data, n, seed, 'rows' if data == 'mnist' else 'nhwc')
    y_g = np.roll(y, 1, axis=1)                                       # every row another class
    tr.cx.rng = InjectedRNG({'R1/' + k: v for k, v in rnd.items()}, tr.cx.device)
    return tr, real, y, y_g, rnd


def _hip_draws_and_acts(tr, data):
    if data == 'cifar10':
        s = tr.model.last_gp_state
        return ({'drop%d' % i: v.cpu().numpy() for i, v in enumerate(s['masks'])},
                {name: a.numpy() for (name, _, _, _), a in zip(tr.model.D_CONVS, s['acts'])})
    return _hip_state(tr, data)


def _run(data, n, seed, gamma=GAMMA):
    import torch
    tr, real, y, y_g, rnd = _setup(data, n, seed)
    cx, st = tr.cx, tr.cx.stores['discriminator']
    st.g.copy_(torch.arange(st.n_p, dtype=torch.float32, device=cx.device) * 1e-3)
    g_before = st.g.clone()
    with cx.phase_scope('T', record=False):
        pen = tr._r1_penalty(cx.from_numpy(real), cx.from_numpy(y), tr.model.discriminator, gamma)
    got_pen = float(pen.cpu().numpy()[0])
    assert torch.equal(st.g, g_before), "the penalty must not touch the discriminator's ParamStore.g"
    got = _flat_to_dict(st, tr.last_gp_grad.cpu().numpy())
    state = tr.model.last_gp_state
    rnd_hip, acts = _hip_draws_and_acts(tr, data)
    for k, v in rnd.items():
        assert np.array_equal(rnd_hip[k].reshape(-1), v.reshape(-1)), k   # the draws of scope 'R1' are the ones the sweeps used
    assert 'alpha' not in state and np.array_equal(state['x'].numpy().reshape(real.shape), real), "the sweeps start from real itself"
    out = state['out'].cpu().numpy()
    assert out[0] == np.float32(got_pen)
    P64 = {k: np.asarray(v, np.float64) for k, v in st.to_dict().items()}
    return got_pen, got, dict(P=P64, x=real, y=y, y_g=y_g, rnd=rnd, acts=acts, out=out, r=state['r'].numpy(), gx=state['gx'].numpy())


@pytest.mark.parametrize("data,n", [('cifar10', 6), ('cifar10', 100), ('mnist', 6), ('svhn', 6)])
def test_r1_penalty_matches_float64(data, n):
    got_pen, got, c = _run(data, n, 20 + n)
    ref = R.r1(data, c['P'], c['x'], c['y'], c['rnd'], GAMMA, acts=c['acts'])
    assert abs(got_pen - ref['penalty']) <= 1e-5 * abs(ref['penalty']), (got_pen, ref['penalty'])
    assert abs(c['out'][1] - ref['grad_sq_mean']) <= 1e-5 * ref['grad_sq_mean']
    assert np.array_equal(c['r'], R.penalty_kernel32(c['gx'], GAMMA, n)), "r = (float)(gamma / n) * gx, one fp32 multiply"
    assert set(got) == set(ref['grads'])
    is_bias = lambda k: k.endswith('/bias') or k.endswith('/b')
    for k, (l2, mx) in _grad_errors(got, ref['grads']).items():
        if is_bias(k):
            assert not np.asarray(got[k]).any(), k                    # exactly zero
        else:
            assert l2 <= 1e-4 and mx <= 1e-3, (k, l2, mx)
    # negative controls, each missing the same bounds by more than 10x: WGAN-GP's column penalty (times gamma) at the same point and draws,
    # and R1 with y_g-like labels instead of the real rows' own
    if data == 'cifar10':
        wgan = RC.gradient_penalty(c['P'], c['x'], c['y'], c['rnd'], acts=c['acts'])
    else:
        wgan = RG.gradient_penalty(data, c['P'], c['x'], c['y'], c['rnd'], acts=c['acts'])
    other = R.r1(data, c['P'], c['x'], c['y_g'], c['rnd'], GAMMA)
    for what, value, grads in (('wgan', GAMMA * wgan['gp'], {k: GAMMA * v for k, v in wgan['grads'].items()}),
                               ('labels', other['penalty'], other['grads'])):
        errs = _grad_errors(got, {k: v for k, v in grads.items() if not is_bias(k)})
        assert max(l2 for l2, _ in errs.values()) > 10 * 1e-4, (what, errs)
        assert abs(got_pen - value) > 10 * 1e-5 * abs(value), (what, got_pen, value)


def test_gamma_as_a_device_tensor_and_the_mnist_image_layout():
    """gamma may be a 1-element device tensor (the trainer's); MNIST [N,28,28,1] gives the penalty of [N,784] (the norm is per image)."""
    import torch
    tr, real, y, _, rnd = _setup('mnist', 6, 26)
    cx = tr.cx
    with cx.phase_scope('T', record=False):
        a = float(tr._r1_penalty(cx.from_numpy(real), cx.from_numpy(y), tr.model.discriminator, 2.5).cpu()[0])
        ga = tr.last_gp_grad.clone()
        gdev = torch.full((1,), 2.5, dtype=torch.float32, device=cx.device)
        b = float(tr._r1_penalty(cx.from_numpy(real), cx.from_numpy(y), tr.model.discriminator, gdev).cpu()[0])
        gb = tr.last_gp_grad.clone()
        c = float(tr._r1_penalty(cx.from_numpy(real.reshape(6, 28, 28, 1)), cx.from_numpy(y), tr.model.discriminator, gdev).cpu()[0])
        gc = tr.last_gp_grad.clone()
    assert a == b and torch.equal(ga, gb)
    assert abs(c - a) <= 1e-6 * a and float((gc - ga).norm()) <= 1e-5 * float(ga.norm())


def test_a_channel_padded_real_batch_is_brought_to_the_dense_layout():
    """real with a row stride beyond its channels (ld = 32 for 3 channels): the sweeps read a dense copy, and the result is that of the
    dense batch, to the bit (the same launches on the same numbers)."""
    import torch
    tr, real, y, _, rnd = _setup('cifar10', 6, 27)
    cx = tr.cx
    out = []
    for kw in (dict(), dict(ld=32)):
        with cx.phase_scope('T', record=False):
            pen = tr._r1_penalty(cx.from_numpy(real, **kw), cx.from_numpy(y), tr.model.discriminator, GAMMA)
        x = tr.model.last_gp_state['x']
        assert (x.ld, x.c) == (3, 3) and np.array_equal(x.numpy(), real)
        out.append((float(pen.cpu()[0]), tr.last_gp_grad.clone()))
    assert out[0][0] == out[1][0] and out[0][0] > 0 and torch.equal(out[0][1], out[1][1])


def test_refusals_name_r1():
    from tg import lib
    real, _fake, y, _alpha, _rnd = _case_goodgan('svhn', 4, 1, 'nhwc')
    for over, what in ((dict(MINIBATCH_DIS=True), 'MINIBATCH_DIS'), (dict(MFMA_DTYPE='bf16'), 'MFMA_DTYPE')):
        tr = _trainer('svhn', **over)
        cx = tr.cx
        with pytest.raises(lib.TgError, match='r1_penalty.*' + what):
            tr._r1_penalty(cx.from_numpy(real), cx.from_numpy(y), tr.model.discriminator, 1.0)
    tr = _trainer('svhn')
    cx = tr.cx
    with pytest.raises(lib.TgError, match='batch sizes differ'):
        tr._r1_penalty(cx.from_numpy(real), cx.from_numpy(y[:3]), tr.model.discriminator, 1.0)
