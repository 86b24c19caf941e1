"""GPU parity of the WGAN-GP penalty on the MNIST and SVHN discriminators (Good_GAN.discriminator_gradient_penalty, reference
Training/train_base.py:598-620): the row-wise penalty kernel tg_grad_penalty_rows_f32 at edge shapes against float64 (bound
1e-6 * sum|terms| per element, as tests/test_gpu_wgan_gp.py), the penalty's value and V / g gradients against the float64 four-sweep
restatement of tests/wgan_gp_goodgan_reference.py with the HIP forward's activation signs and draws, two negative controls, the whole
loss through a Good_GAN trainer, a trainer that runs the penalty between two launch-plan iterations, and the refusals."""
import numpy as np
import pytest

import gpu_common as G
import wgan_gp_goodgan_reference as R
import wgan_gp_reference as RC
from oracle import nets_goodgan as N
from oracle import step_goodgan as S
from test_oracle_goodgan import scrambled

pytestmark = pytest.mark.gpu
GARBAGE = 7.0e3                       # pre-filled into every output buffer: padding that is not written shows up
SMALL = dict(B_G=6, L_C=4, U_C=4, L_D=2, U_D=4)


def _trainer(data, P=None, **over):
    from Model.Good_GAN import Good_GAN
    over.setdefault('MFMA_DTYPE', 'f32')
    P = P if P is not None else {k: v.astype(np.float32) for k, v in scrambled(data, 3).items()}
    return G.fresh_trainer(G.make_config_goodgan(data, SMALL, **over), P, Good_GAN)


def _dev(cx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).to(cx.device)


def _garbage(cx, numel):
    import torch
    return torch.full((numel,), GARBAGE, dtype=torch.float32, device=cx.device)


def _within(got, ref, terms, what):
    bad = np.abs(np.asarray(got, np.float64) - ref) > 1e-6 * terms + 1e-30
    assert not bad.any(), (what, int(bad.sum()), np.abs(got - ref).max())


# n = 1; F = 1; F = 784 with ld 800 (the MNIST rows); F not a multiple of 64; n = 100; rows longer than the registers hold (scalar: 1024
# floats, float4: 4096) — the scalar path where F, ld_g or ld_r is not a multiple of 4
@pytest.mark.parametrize("n,f,ld_g,ld_r", [(1, 784, 800, 800), (5, 1, 1, 32), (100, 784, 784, 800), (6, 37, 40, 37), (3, 100, 100, 128),
                                           (3, 1500, 1501, 1504), (2, 4400, 4400, 4416)])
def test_grad_penalty_rows_kernel(n, f, ld_g, ld_r):
    from tg import lib
    tr = _trainer('mnist')
    cx = tr.cx
    rng = np.random.default_rng(n + f)
    weight = 10.0
    g = np.zeros((n, ld_g), np.float32)
    g[:, :f] = rng.standard_normal((n, f)) * rng.uniform(0.2, 3.0, (n, 1)) / np.sqrt(f)
    if n >= 3:
        g[1, :f] = 0.0                                                # one zero row: s = 0
    dg = _dev(cx, g)
    outs = []
    for _ in range(2):
        r, gp, partials = _garbage(cx, n * ld_r), _garbage(cx, 4), _garbage(cx, 2 * n)
        lib.call('tg_grad_penalty_rows_f32', lib.ptr(dg), ld_g, n, f, weight, lib.ptr(r), ld_r, lib.ptr(partials), lib.ptr(gp), cx.stream)
        outs.append((r.cpu().numpy().reshape(n, ld_r), gp.cpu().numpy()[:1]))
    (got_r, got_gp), (r2, gp2) = outs
    assert np.array_equal(got_r.view(np.uint32), r2.view(np.uint32)) and np.array_equal(got_gp.view(np.uint32), gp2.view(np.uint32)), \
        "run-to-run bit identity"
    g64 = g[:, :f].astype(np.float64)
    s = np.sqrt((g64 ** 2).sum(axis=1, keepdims=True))
    ref_gp = weight * np.mean((s - 1.0) ** 2)
    assert abs(float(got_gp[0]) - ref_gp) <= 1e-6 * ref_gp, (got_gp, ref_gp)
    with np.errstate(divide='ignore', invalid='ignore'):
        ref_r = weight * 2.0 * (s - 1.0) / s * g64 / n
        terms = weight * 2.0 * (s + 1.0) / s * np.abs(g64) / n
    ok = np.isfinite(ref_r)
    if n >= 3:
        assert not np.isfinite(got_r[1, :f]).any(), "s = 0 gives a non-finite gradient, as TF's sqrt gradient (not masked)"
    _within(got_r[:, :f][ok], ref_r[ok], terms[ok], 'r')
    assert not got_r[:, f:].any(), "padding columns of r must be written zero"


# ---------------------------------------------------------------- the penalty through the model

def _images(data, n, rng, layout):
    if data == 'mnist':
        real = S.synth_batch('mnist', int(rng.integers(1 << 30)), dict(SMALL, L_D=n))['x_l_d'][:n].astype(np.float32)
        fake = (1.0 / (1.0 + np.exp(-rng.standard_normal((n, 28, 28, 1))))).astype(np.float32)
        if layout == 'rows':
            real, fake = real.reshape(n, 784), fake.reshape(n, 784)
        return real, fake
    real = S.synth_batch('svhn', int(rng.integers(1 << 30)), dict(SMALL, L_D=n))['x_l_d'][:n].astype(np.float32)
    return real, np.tanh(rng.standard_normal((n, 32, 32, 3))).astype(np.float32)


def _gp_case(data, n, seed, layout):
    rng = np.random.default_rng(seed)
    real, fake = _images(data, n, rng, layout)
    y = np.eye(10, dtype=np.float32)[rng.integers(0, 10, n)]
    alpha = rng.random(n).astype(np.float32)
    alpha[0], alpha[1] = 0.0, 1.0
    return real, fake, y, alpha, R.draws(data, n, rng, np.float32)


def _inject(cx, alpha, rnd, extra=None):
    from tg.runtime import InjectedRNG
    arrays = {'GP/alpha': alpha}
    arrays.update({'GP/' + k: v for k, v in rnd.items()})
    arrays.update(extra or {})
    cx.rng = InjectedRNG(arrays, cx.device)


def _grad_errors(got, ref):
    """{variable: (relative L2, max abs error / max |ref|)}."""
    out = {}
    for k, r in ref.items():
        g = np.asarray(got[k], np.float64).reshape(r.shape)
        out[k] = (np.linalg.norm(g - r) / (np.linalg.norm(r) + 1e-300), np.abs(g - r).max() / (np.abs(r).max() + 1e-300))
    return out


def _flat_to_dict(st, flat):
    out = {}
    for k in st.names(True):
        kind, off, num, shape = st.index[k]
        out[k] = flat[off:off + num].reshape(shape)
    return out


def _hip_state(tr, data):
    """the draws and activations the HIP sweeps used, read back from last_gp_state."""
    s = tr.model.last_gp_state
    if data == 'mnist':
        rnd = {'noise%d' % i: v.cpu().numpy() for i, v in enumerate(s['noise'])}
    else:
        rnd = {'drop%d' % i: v.cpu().numpy() for i, v in enumerate(s['masks'])}
    return rnd, [a.numpy() for a in s['acts']]


def _run_gp(data, n, seed, layout, weight=1.0):
    import torch
    tr = _trainer(data)
    cx, st = tr.cx, tr.cx.stores['discriminator']
    real, fake, y, alpha, rnd = _gp_case(data, n, seed, layout)
    _inject(cx, alpha, rnd)
    st.g.copy_(torch.arange(st.n_p, dtype=torch.float32, device=cx.device) * 1e-3)
    g_before = st.g.clone()
    with cx.phase_scope('T', record=False):
        gp = tr._gradient_penalty(cx.from_numpy(real), cx.from_numpy(fake), cx.from_numpy(y), tr.model.discriminator, weight=weight)
    got_gp = float(gp.cpu().numpy()[0])
    assert torch.equal(st.g, g_before), "the penalty must not touch the discriminator's ParamStore.g"
    got = _flat_to_dict(st, tr.last_gp_grad.cpu().numpy())
    rnd_hip, acts = _hip_state(tr, data)
    for k, v in rnd.items():
        assert np.array_equal(rnd_hip[k].reshape(-1), v.reshape(-1)), k
    x = R.interpolate(real, fake, alpha)
    assert np.abs(tr.model.last_gp_state['x'].numpy().reshape(x.shape) - x).max() <= 1e-6 * (np.abs(real).max() + np.abs(fake).max())
    P64 = {k: np.asarray(v, np.float64) for k, v in st.to_dict().items()}
    return got_gp, got, dict(P=P64, x=x, y=y, rnd=rnd, acts=acts)


@pytest.mark.parametrize("data,layout,n", [('mnist', 'rows', 6), ('mnist', 'rows', 100), ('mnist', 'nhwc', 6), ('svhn', 'nhwc', 6),
                                           ('svhn', 'nhwc', 100)])
def test_gradient_penalty_matches_float64(data, layout, n):
    got_gp, got, c = _run_gp(data, n, 20 + n, layout)
    P = c['P']
    ref = R.gradient_penalty(data, P, c['x'], c['y'], c['rnd'], acts=c['acts'])
    assert abs(got_gp - ref['gp']) <= 1e-5 * abs(ref['gp']), (got_gp, ref['gp'])
    assert set(got) == set(ref['grads'])
    for k, (l2, mx) in _grad_errors(got, ref['grads']).items():
        if k.endswith('/b'):
            assert not np.asarray(got[k]).any(), k                    # exactly zero
        else:
            assert l2 <= 1e-4 and mx <= 1e-3, (k, l2, mx)
    # negative controls: dW_eff written straight into dV (no weight-norm chain), and — MNIST — lrelu' taken after the additive noise; each
    # misses the same bounds by at least 10x
    controls = [dict(wn_chain=False)] + ([dict(lrelu_from='post_noise')] if data == 'mnist' else [])
    for kw in controls:
        wrong = R.gradient_penalty(data, P, c['x'], c['y'], c['rnd'], acts=c['acts'], **kw)
        errs = _grad_errors(got, {k: v for k, v in wrong['grads'].items() if not k.endswith('/b')})
        assert max(l2 for l2, _ in errs.values()) >= 10 * 1e-4, (kw, errs)


@pytest.mark.parametrize("data", ['mnist', 'svhn'])
def test_loss_wgan_gp_through_a_good_gan_trainer(data):
    import torch
    tr = _trainer(data)
    cx, st = tr.cx, tr.cx.stores['discriminator']
    n, nu, l1, l2 = 6, 4, 0.3, 0.5
    layout = 'rows' if data == 'mnist' else 'nhwc'
    real, fake, y, alpha, rnd = _gp_case(data, n, 31, layout)
    rng = np.random.default_rng(32)
    unl, _ = _images(data, nu, rng, layout)
    y_unl = np.eye(10, dtype=np.float32)[rng.integers(0, 10, nu)]
    c_real, c_fake, c_unl = (rng.standard_normal((m, 10)).astype(np.float32) for m in (n, n, nu))
    ximg = np.concatenate([real, fake, unl])
    yall = np.concatenate([y, y, y_unl])
    drnd = R.draws(data, 2 * n + nu, rng, np.float32)
    _inject(cx, alpha, rnd, {'T/D/' + k: v for k, v in drnd.items()})
    with cx.phase_scope('T', train_nets=('discriminator',)):
        ia = cx.from_numpy(ximg)
        with cx.rng_scoped('T/D'):
            _, lg = tr.model.discriminator(ia, cx.from_numpy(yall))
        D = [None, lg.view_rows(0, n), None, lg.view_rows(n, 2 * n), None, lg.view_rows(2 * n, 2 * n + nu)]
        C = [cx.from_numpy(a) for a in (c_real, c_fake, c_unl)]
        d_loss, g_loss, c_loss = tr._loss_WGAN_GP(cx.from_numpy(fake), D, C, cx.from_numpy(real), cx.from_numpy(y), (l1, l2),
                                                  tr.model.discriminator)
        lg.grad = tr.last_d_cat.grad
        cx.backward()
    g_wd = st.g.clone()
    tr._add_gp_grad()
    assert torch.equal(st.g, g_wd + tr.last_gp_grad), "_add_gp_grad adds the penalty's gradient to the D backward's"
    logits = lg.numpy().astype(np.float64).reshape(-1)
    head, g_ref, gg_ref = RC.wgan_loss_head(logits[:n], logits[n:2 * n], logits[2 * n:], l1, l2)
    P64 = {k: np.asarray(v, np.float64) for k, v in st.to_dict().items()}
    rnd_hip, acts = _hip_state(tr, data)
    gp_ref = R.gradient_penalty(data, P64, R.interpolate(real, fake, alpha), y, rnd, acts=acts)
    c_ref, gcr, gcf = RC.c_loss(c_real, c_fake, y, l2)
    assert abs(d_loss - (head[0] + 10.0 * gp_ref['gp'])) <= 1e-5 * (abs(head[0]) + 10.0 * gp_ref['gp'])
    assert abs(g_loss - head[1]) <= 1e-6 * np.abs(logits[n:2 * n]).mean() + 1e-7
    assert abs(c_loss - c_ref) <= 1e-5 * c_ref
    np.testing.assert_allclose(tr.last_d_cat.grad.numpy().reshape(-1), g_ref, rtol=1e-6, atol=0)
    np.testing.assert_allclose(D[3].grad.numpy().reshape(-1), gg_ref, rtol=1e-6, atol=0)
    # the penalty's part at the tight bound; the D backward's part (the wd terms) at the bound of tests/test_gpu_goodgan.py
    got_gp = _flat_to_dict(st, tr.last_gp_grad.cpu().numpy())
    for k, (e2, mx) in _grad_errors(got_gp, {k: 10.0 * v for k, v in gp_ref['grads'].items() if not k.endswith('/b')}).items():
        assert e2 <= 1e-4 and mx <= 1e-3, (k, e2, mx)
    layers = N.discriminator_layers(data)
    d64 = {k: v.astype(np.float64) for k, v in drnd.items()}
    _, dc, _ = N.seq_fwd(P64, layers, ximg.astype(np.float64), yall.astype(np.float64), d64, True)
    wd_grads, _ = N.seq_bwd(P64, layers, dc, g_ref[:, None], yall.astype(np.float64), d64)
    got_wd = _flat_to_dict(st, g_wd.cpu().numpy())
    gmax = max(np.abs(v).max() for v in wd_grads.values())
    for k, ref in wd_grads.items():
        d = got_wd[k] - ref
        sc = max(np.abs(ref).max(), 1e-4 * gmax)
        assert np.abs(d).max() <= 5e-2 * sc and np.linalg.norm(d) <= 1e-2 * max(np.linalg.norm(ref), sc), k


@pytest.mark.parametrize("data", ['mnist', 'svhn'])
def test_penalty_between_plan_iterations_leaves_training_bit_identical(data):
    """EXEC_MODE 'plan' with the Philox RNG: two iterations, and a twin that runs the penalty between them — the workspace and the RNG
    streams of the recorded launch plans must not notice."""
    import torch
    P = {k: v.astype(np.float32) for k, v in scrambled(data, 5).items()}
    batches = [S.synth_batch(data, 40 + i, SMALL) for i in range(2)]

    def run(with_gp):
        tr = _trainer(data, P, EXEC_MODE='plan')
        tr.feed(batches[0])
        tr.train_iteration()
        l0 = tr.losses()
        if with_gp:
            cx, m = tr.cx, tr.model
            with cx.phase_scope('X', record=False):
                b = batches[1]
                nd = b['x_l_d'].shape[0]
                tr._gradient_penalty(m.as_image(cx.from_numpy(b['x_l_d'])), m.as_image(cx.from_numpy(b['x_u_d'][:nd])),
                                     cx.from_numpy(b['y_l_d']), m.discriminator)
            torch.cuda.synchronize()
        tr.feed(batches[1])
        tr.train_iteration()
        return [l0, tr.losses()], {k: st.p.cpu().numpy().copy() for k, st in tr.cx.stores.items()}

    la, pa = run(False)
    lb, pb = run(True)
    assert la == lb, (la, lb)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


def test_refusals():
    from tg import lib
    rng = np.random.default_rng(3)
    # minibatch discrimination couples the images of a batch
    tr = _trainer('svhn', MINIBATCH_DIS=True)
    cx = tr.cx
    real, fake, y, alpha, rnd = _gp_case('svhn', 4, 1, 'nhwc')
    _inject(cx, alpha, rnd)
    with pytest.raises(lib.TgError, match='MINIBATCH_DIS'):
        tr._gradient_penalty(cx.from_numpy(real), cx.from_numpy(fake), cx.from_numpy(y), tr.model.discriminator)
    # the bf16 MFMA operands
    tr = _trainer('svhn', MFMA_DTYPE='bf16')
    cx = tr.cx
    _inject(cx, alpha, rnd)
    with pytest.raises(lib.TgError, match='MFMA_DTYPE'):
        tr._gradient_penalty(cx.from_numpy(real), cx.from_numpy(fake), cx.from_numpy(y), tr.model.discriminator)
    # real and fake in different layouts
    tr = _trainer('mnist')
    cx = tr.cx
    real = rng.random((4, 28, 28, 1)).astype(np.float32)
    fake = rng.random((4, 784)).astype(np.float32)
    with pytest.raises(lib.TgError, match='as_image'):
        tr._gradient_penalty(cx.from_numpy(real), cx.from_numpy(fake), cx.from_numpy(y), tr.model.discriminator)
