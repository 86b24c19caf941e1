"""GPU parity of the WGAN-GP loss (Train_base._loss_WGAN_GP / _gradient_penalty, reference Training/train_base.py:576-620): the three
kernels of csrc/wgan_gp.hip at edge shapes against float64 (bound 1e-6 * sum|terms| per element, as tests/test_gpu_igemm.py), the
penalty's value and parameter gradient (Good_GAN_cifar10.discriminator_gradient_penalty) against the float64 four-sweep restatement of
tests/wgan_gp_reference.py with the HIP forward's activation signs, a negative control, the whole loss, and a trainer that runs the
penalty between two launch-plan iterations without noticing it."""
import numpy as np
import pytest

import gpu_common as G
import wgan_gp_reference as R
from oracle import nets_cifar10 as N
from oracle import step_cifar10 as S

pytestmark = pytest.mark.gpu
GARBAGE = 7.0e3                       # pre-filled into every output buffer: padding that is not written shows up


def _ctx():
    tr = G.fresh_trainer(G.make_config(dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)))
    return tr, tr.cx


def _dev(cx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).to(cx.device)


def _garbage(cx, numel):
    import torch
    return torch.full((numel,), GARBAGE, dtype=torch.float32, device=cx.device)


def _within(got, ref, terms, what):
    bad = np.abs(np.asarray(got, np.float64) - ref) > 1e-6 * terms + 1e-30
    assert not bad.any(), (what, int(bad.sum()), np.abs(got - ref).max())


@pytest.mark.parametrize("n,hw,ld_out", [(7, 32 * 32, 32), (3, 5 * 7, 4)])
def test_interp_kernel(n, hw, ld_out):
    from tg import lib
    tr, cx = _ctx()
    rng = np.random.default_rng(n)
    c = 3
    real = rng.uniform(-1, 1, (n * hw, c)).astype(np.float32)
    fake = rng.uniform(-1, 1, (n * hw, 5)).astype(np.float32)        # ld_f = 5 > c
    alpha = rng.random(n).astype(np.float32)
    alpha[0], alpha[-1] = 0.0, 1.0
    out = _garbage(cx, n * hw * ld_out)
    dr, dfk, da = _dev(cx, real), _dev(cx, fake), _dev(cx, alpha)       # held: a freed temporary's memory is re-used by the next one
    lib.call('tg_wgan_interp_f32', lib.ptr(dr), c, lib.ptr(dfk), 5, lib.ptr(da), lib.ptr(out), ld_out, n, hw, c, cx.stream)
    got = out.cpu().numpy().reshape(n * hw, ld_out)
    a = np.repeat(alpha.astype(np.float64), hw)[:, None]
    r64, f64 = real.astype(np.float64), fake[:, :c].astype(np.float64)
    ref = r64 + a * (f64 - r64)
    _within(got[:, :c], ref, np.abs(r64) + np.abs(a * (f64 - r64)), 'interp')
    assert not got[:, c:].any(), "padding columns must be written zero"
    assert np.array_equal(got[:hw, :c], real[:hw])          # alpha 0 is exact; alpha 1 is real + (fake - real), within the bound above


@pytest.mark.parametrize("n,h,w,ld_g,ld_r", [(3, 5, 7, 32, 8), (100, 32, 32, 32, 32), (5, 32, 32, 3, 3)])
def test_grad_penalty_kernel(n, h, w, ld_g, ld_r):
    """slopes over H, gp and r with the weight folded in; n*w*ld_r not a multiple of the block in the first and last case."""
    from tg import lib
    tr, cx = _ctx()
    rng = np.random.default_rng(n + h)
    c, weight = 3, 10.0
    g = np.zeros((n, h, w, ld_g), np.float32)
    g[..., :c] = rng.standard_normal((n, h, w, c)) * rng.uniform(0.01, 0.5, (n, 1, w, c))
    g[0, :, 0, 0] = 0.0                                               # one zero column: s = 0
    r = _garbage(cx, n * h * w * ld_r)
    gp = _garbage(cx, 4)
    partials = _garbage(cx, 2 * ((n * w * ld_r + 255) // 256))
    dg = _dev(cx, g)
    lib.call('tg_grad_penalty_f32', lib.ptr(dg), ld_g, n, h, w, c, weight, lib.ptr(r), ld_r, lib.ptr(partials), lib.ptr(gp), cx.stream)
    got_r = r.cpu().numpy().reshape(n, h, w, ld_r)
    got_gp = float(gp.cpu().numpy()[0])
    g64 = g[..., :c].astype(np.float64)
    s = np.sqrt((g64 ** 2).sum(axis=1, keepdims=True))
    cnt = n * w * c
    ref_gp = weight * np.mean((s - 1.0) ** 2)
    assert abs(got_gp - ref_gp) <= 1e-6 * ref_gp, (got_gp, ref_gp)
    with np.errstate(divide='ignore', invalid='ignore'):
        ref_r = weight * 2.0 * (s - 1.0) / s * g64 / cnt
        terms = weight * 2.0 * (s + 1.0) / s * np.abs(g64) / cnt
    ok = np.isfinite(ref_r)
    assert not np.isfinite(got_r[0, :, 0, 0]).any(), "s = 0 gives a non-finite gradient, as TF's sqrt gradient (not masked)"
    _within(got_r[..., :c][ok], ref_r[ok], terms[ok], 'r')
    assert not got_r[..., c:].any(), "padding columns of r must be written zero"


def test_wgan_loss_kernel():
    from tg import lib
    tr, cx = _ctx()
    rng = np.random.default_rng(4)
    nr, nf, nu, l1, l2 = 3, 5, 2, 0.3, 0.5
    z = rng.standard_normal(nr + nf + nu).astype(np.float32)
    dl, df, loss = _garbage(cx, (nr + nf + nu) * 32), _garbage(cx, nf * 8), _garbage(cx, 8)
    dz = _dev(cx, z)
    lib.call('tg_wgan_loss_f32', lib.ptr(dz), 1, nr, nf, nu, l1, l2, lib.ptr(dl), 32, lib.ptr(df), 8, lib.ptr(loss), cx.stream)
    vals, g, gg = R.wgan_loss_head(z[:nr], z[nr:nr + nf], z[nr + nf:], l1, l2)
    got = loss.cpu().numpy()[:5]
    za = np.abs(z.astype(np.float64))
    scale = (1 + l1 + l2) * (za[:nr].mean() + za[nr:nr + nf].mean() + za[nr + nf:].mean())
    _within(got, np.array(vals), np.full(5, scale), 'wgan loss values')
    gd = dl.cpu().numpy().reshape(-1, 32)
    _within(gd[:, 0], g, np.abs(g), 'd_loss logit gradient')
    assert not gd[:, 1:].any()
    gf = df.cpu().numpy().reshape(nf, 8)
    _within(gf[:, 0], gg, np.abs(gg), 'g_loss logit gradient')
    assert not gf[:, 1:].any()


# ---------------------------------------------------------------- the penalty through the model

def _gp_case(n, seed):
    rng = np.random.default_rng(seed)
    real = S.synth_batch(seed, dict(S.SIZES, L_D=n))['x_l_d'][:n].astype(np.float32)
    fake = np.tanh(rng.standard_normal((n, 32, 32, 3))).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.integers(0, 10, n)]
    alpha = rng.random(n).astype(np.float32)
    alpha[0], alpha[1] = 0.0, 1.0
    rnd = {'drop0': np.floor(0.8 + rng.random((n, 32, 32, 3))), 'drop1': np.floor(0.8 + rng.random((n, 16, 16, 32))),
           'drop2': np.floor(0.8 + rng.random((n, 8, 8, 64)))}
    return real, fake, y, alpha, {k: v.astype(np.float32) for k, v in rnd.items()}


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


def _run_gp(n, seed, weight=1.0):
    import torch
    tr, cx = _ctx()
    P = S.init_params(0)
    st = cx.stores['discriminator']
    st.load_dict(P)
    real, fake, y, alpha, rnd = _gp_case(n, seed)
    _inject(cx, alpha, rnd)
    st.g.copy_(torch.arange(st.n_p, dtype=torch.float32, device=cx.device) * 1e-3)
    g_before = st.g.clone()
    with cx.phase_scope('T', record=False):
        gp = tr._gradient_penalty(cx.from_numpy(real), cx.from_numpy(fake), cx.from_numpy(y), tr.model.discriminator, weight=weight)
    got_gp = float(gp.cpu().numpy()[0])
    flat = tr.last_gp_grad.cpu().numpy()
    assert torch.equal(st.g, g_before), "the penalty must not touch the discriminator's ParamStore.g"
    got = {}
    for k in st.names(True):
        kind, off, num, shape = st.index[k]
        got[k] = flat[off:off + num].reshape(shape)
    acts = {name: a.numpy() for (name, _, _, _), a in zip(tr.model.D_CONVS, tr.model.last_gp_state['acts'])}
    x = R.interpolate(real.astype(np.float64), fake.astype(np.float64), alpha.astype(np.float64))
    P64 = {k: np.asarray(v, np.float64) for k, v in P.items() if k.startswith('discriminator/')}
    return got_gp, got, dict(P=P64, x=x, y=y, rnd=rnd, acts=acts)


@pytest.mark.parametrize("n", [6, 100])
def test_gradient_penalty_matches_float64(n):
    got_gp, got, c = _run_gp(n, 20 + n)
    ref = R.gradient_penalty(c['P'], c['x'], c['y'], c['rnd'], acts=c['acts'])
    assert abs(got_gp - ref['gp']) <= 1e-5 * abs(ref['gp']), (got_gp, ref['gp'])
    for k, (l2, mx) in _grad_errors(got, ref['grads']).items():
        if k.endswith('/bias'):
            assert not np.asarray(got[k]).any(), k                    # exactly zero
        else:
            assert l2 <= 1e-4 and mx <= 1e-3, (k, l2, mx)
    # negative controls: a per-image norm instead of the reference's axis H, and a tangent without the image's dropout mask, each miss the
    # same bounds by at least 10x
    for kw in (dict(slope_axes=(1, 2, 3)), dict(mask_tangent=False)):
        wrong = R.gradient_penalty(c['P'], c['x'], c['y'], c['rnd'], acts=c['acts'], **kw)
        errs = _grad_errors(got, {k: v for k, v in wrong['grads'].items() if not k.endswith('/bias')})
        assert max(l2 for l2, _ in errs.values()) >= 10 * 1e-4, (kw, errs)


def test_loss_wgan_gp_values_gradients_and_full_d_gradient():
    import torch
    tr, cx = _ctx()
    P = S.init_params(0)
    st = cx.stores['discriminator']
    st.load_dict(P)
    n, nu, l1, l2 = 6, 4, 0.3, 0.5
    real, fake, y, alpha, rnd = _gp_case(n, 31)
    rng = np.random.default_rng(32)
    unl = np.tanh(rng.standard_normal((nu, 32, 32, 3))).astype(np.float32)
    y_unl = np.eye(10, dtype=np.float32)[rng.integers(0, 10, nu)]
    c_real, c_fake, c_unl = (rng.standard_normal((m, 10)).astype(np.float32) for m in (n, n, nu))
    ximg = np.concatenate([real, fake, unl])
    yall = np.concatenate([y, y, y_unl])
    drnd = {'drop0': np.floor(0.8 + rng.random((2 * n + nu, 32, 32, 3))), 'drop1': np.floor(0.8 + rng.random((2 * n + nu, 16, 16, 32))),
            'drop2': np.floor(0.8 + rng.random((2 * n + nu, 8, 8, 64)))}
    drnd = {k: v.astype(np.float32) for k, v in drnd.items()}
    _inject(cx, alpha, rnd, {'T/D/' + k: v for k, v in drnd.items()})
    with cx.phase_scope('T', train_nets=('discriminator',)):
        ia = cx.from_numpy(ximg)
        with cx.rng_scoped('T/D'):
            _, lg = tr.model.discriminator(ia, cx.from_numpy(yall))
        D = [None, lg.view_rows(0, n), None, lg.view_rows(n, 2 * n), None, lg.view_rows(2 * n, 2 * n + nu)]
        D9 = [D[0], D[1], None, D[2], D[3], None, D[4], D[5], None]
        C = [cx.from_numpy(a) for a in (c_real, c_fake, c_unl)]
        d_loss, g_loss, c_loss = tr._loss_WGAN_GP(cx.from_numpy(fake), D9, C, cx.from_numpy(real), cx.from_numpy(y), (l1, l2),
                                                  tr.model.discriminator)
        lg.grad = tr.last_d_cat.grad
        cx.backward()
    tr._add_gp_grad()
    logits = lg.numpy().astype(np.float64).reshape(-1)
    head, g_ref, gg_ref = R.wgan_loss_head(logits[:n], logits[n:2 * n], logits[2 * n:], l1, l2)
    x = R.interpolate(real.astype(np.float64), fake.astype(np.float64), alpha.astype(np.float64))
    acts = {name: a.numpy() for (name, _, _, _), a in zip(tr.model.D_CONVS, tr.model.last_gp_state['acts'])}
    P64 = {k: np.asarray(v, np.float64) for k, v in P.items() if k.startswith('discriminator/')}
    gp_ref = R.gradient_penalty(P64, x, y, rnd, acts=acts)
    c_ref, gcr, gcf = R.c_loss(c_real, c_fake, y, l2)
    assert abs(d_loss - (head[0] + 10.0 * gp_ref['gp'])) <= 1e-5 * (abs(head[0]) + 10.0 * gp_ref['gp'])
    assert abs(g_loss - head[1]) <= 1e-6 * np.abs(logits[n:2 * n]).mean() + 1e-7
    assert abs(c_loss - c_ref) <= 1e-5 * c_ref
    np.testing.assert_allclose(tr.last_d_cat.grad.numpy().reshape(-1), g_ref, rtol=1e-6, atol=0)
    np.testing.assert_allclose(D[3].grad.numpy().reshape(-1), gg_ref, rtol=1e-6, atol=0)
    np.testing.assert_allclose(C[0].grad.numpy(), gcr, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(C[1].grad.numpy(), gcf, rtol=1e-4, atol=1e-7)
    assert not C[2].grad.numpy().any()
    # the whole discriminator gradient: the wd part through the D backward, plus 10 d gp / d theta_D
    _, cache = N.discriminator_fwd(P64, ximg.astype(np.float64), yall.astype(np.float64), {k: v.astype(np.float64) for k, v in drnd.items()})
    wd_grads, _ = N.discriminator_bwd(P64, cache, g_ref[:, None], {k: v.astype(np.float64) for k, v in drnd.items()})
    floor = 1e-6 * np.abs(g_ref).sum()          # the logit gradients cancel in d/d b_lin (0 in exact arithmetic): fp32 leaves ~1e-8 there
    for k in wd_grads:
        ref = wd_grads[k] + 10.0 * gp_ref['grads'][k]
        got = st.get(k, 'grad').astype(np.float64)
        assert np.abs(got - ref).max() <= 1e-3 * np.abs(ref).max() + floor, (k, np.abs(got - ref).max(), np.abs(ref).max())


def test_penalty_between_plan_iterations_leaves_training_bit_identical():
    """EXEC_MODE 'plan' with the Philox RNG: two iterations, and a twin that runs the penalty between them — the workspace and the RNG
    streams of the recorded launch plans must not notice."""
    import torch
    sizes = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
    P = S.init_params(0)
    full = dict(S.SIZES, **sizes)
    batches = [S.synth_batch(40 + i, full) for i in range(2)]

    def run(with_gp):
        tr = G.fresh_trainer(G.make_config(sizes, EXEC_MODE='plan'), P)
        tr.feed(batches[0])
        tr.train_iteration()
        l0 = tr.losses()
        if with_gp:
            cx = tr.cx
            with cx.phase_scope('X', record=False):
                b = batches[1]
                tr._gradient_penalty(cx.from_numpy(b['x_l_d']), cx.from_numpy(b['x_u_d'][:b['x_l_d'].shape[0]]), cx.from_numpy(b['y_l_d']),
                                     tr.model.discriminator)
            torch.cuda.synchronize()
        tr.feed(batches[1])
        tr.train_iteration()
        return [l0, tr.losses()], {k: st.p.cpu().numpy().copy() for k, st in tr.cx.stores.items()}

    la, pa = run(False)
    lb, pb = run(True)
    assert la == lb, (la, lb)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
