"""GPU tests of the training step with config.LOSS = 'WGAN_GP' (Training/Train_goodGAN.py): the three replayable loss heads
at edge shapes, one phase-synchronised iteration against the float64 restatement (tests/wgan_gp_step_reference.py) on CIFAR-10, MNIST
and SVHN, bit-identical execution modes that follow set_hyper(), isolation from the standalone penalty, and two data-parallel ranks."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nets_goodgan as NG
from oracle import step_cifar10 as S
from oracle import step_goodgan as SG
import gpu_common as G
import wgan_gp_goodgan_reference as RG
import wgan_gp_reference as RC
import wgan_gp_step_reference as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
HYPER = dict(lr=3e-4, cla_lr=3e-3, beta1=0.5, lambda_1=0.3, lambda_2=0.5)
# networks: tests/test_gpu_step.py; the penalty part: tests/test_gpu_wgan_gp*.py
GRAD_L2_TOL, GRAD_MAX_TOL, LOSS_TOL = 1e-2, 5e-2, 2e-4
GP_TOL, GP_L2_TOL, GP_MAX_TOL = 1e-5, 1e-4, 1e-3
NETS = {'D': 'discriminator', 'G': 'good_generator', 'C': 'classifier'}


def _lib():
    from tg import lib
    lib.load()
    return lib


def _ctx():
    from tg import runtime
    try:
        return runtime.ctx()
    except Exception:
        return runtime.set_context(runtime.Context('cuda:0'))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()


def _ptr(t):
    from tg import lib
    return lib.ptr(t)


# ------------------------------------------------------------------------------------------------------------- the heads
@pytest.mark.parametrize("n_real, n_fake, n_unl, ld, ld_d", [(1, 1, 1, 1, 1), (3, 5, 7, 3, 32), (20, 100, 80, 1, 32), (257, 300, 1, 2, 33)])
def test_d_head_matches_float64_and_is_bit_identical(n_real, n_fake, n_unl, ld, ld_d):
    lib, cx = _lib(), _ctx()
    rng = np.random.default_rng(n_real + n_fake)
    n = n_real + n_fake + n_unl
    z = rng.standard_normal((n, ld)).astype(np.float32)
    lam = np.array([0.3, 0.7], np.float32)
    gp_w = np.float32(3.25)
    outs = []
    for _ in range(2):
        dz = torch.full((n * ld_d,), 7.0, device='cuda')
        loss, terms = torch.full((2,), 7.0, device='cuda'), torch.full((5,), 7.0, device='cuda')
        zt, lt, gt = _dev(z), _dev(lam), _dev([gp_w])                       # (held: the call reads them after the Python expression ends)
        lib.call('tg_wgan_d_head_f32', _ptr(zt), ld, n_real, n_fake, n_unl, _ptr(lt), _ptr(gt), 10.0, _ptr(dz), ld_d, _ptr(loss), _ptr(terms),
                 cx.stream)
        torch.cuda.synchronize()
        outs.append((dz.cpu().numpy().reshape(n, ld_d), loss.cpu().numpy(), terms.cpu().numpy()))
    for a, b in zip(outs[0], outs[1]):
        assert a.tobytes() == b.tobytes()
    dz, loss, terms = outs[0]
    c = z[:, 0].astype(np.float64)
    (d, _g, wd1, wd2, wd3), g_ref, _ = RC.wgan_loss_head(c[:n_real], c[n_real:n_real + n_fake], c[n_real + n_fake:], 0.3, 0.7)
    assert abs(loss[0] - (d + 3.25)) <= 1e-5 * (abs(d) + 3.25)
    assert loss[1] == 7.0 and terms[4] == 7.0                                    # nothing written past the outputs
    np.testing.assert_allclose(terms[:3], [wd1, wd2, wd3], rtol=1e-5, atol=1e-6 * np.abs(c).max())
    assert abs(terms[3] - 0.325) <= 1e-7
    np.testing.assert_allclose(dz[:, 0], g_ref, rtol=1e-6, atol=0)
    assert not dz[:, 1:].any()


@pytest.mark.parametrize("n, ld, ld_d", [(1, 1, 1), (7, 3, 32), (300, 1, 33)])
def test_g_head_matches_float64_and_is_bit_identical(n, ld, ld_d):
    lib, cx = _lib(), _ctx()
    z = np.random.default_rng(n).standard_normal((n, ld)).astype(np.float32)
    outs = []
    for _ in range(2):
        dz, loss = torch.full((n * ld_d,), 7.0, device='cuda'), torch.full((2,), 7.0, device='cuda')
        zt = _dev(z)
        lib.call('tg_wgan_g_head_f32', _ptr(zt), ld, n, _ptr(dz), ld_d, _ptr(loss), cx.stream)
        torch.cuda.synchronize()
        outs.append((dz.cpu().numpy().reshape(n, ld_d), loss.cpu().numpy()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))
    dz, loss = outs[0]
    ref = -z[:, 0].astype(np.float64).mean()
    assert abs(loss[0] - ref) <= 1e-6 * np.abs(z[:, 0]).mean() + 1e-7 and loss[1] == 7.0
    np.testing.assert_allclose(dz[:, 0], -1.0 / n, rtol=1e-7)
    assert not dz[:, 1:].any()


@pytest.mark.parametrize("n_real, n_zero, n_fake, k, ld, ld_d", [(1, 0, 0, 10, 10, 10), (1, 1, 1, 3, 3, 32), (3, 5, 7, 10, 12, 32),
                                                                  (300, 4, 257, 10, 10, 16)])
def test_c_head_matches_float64_and_is_bit_identical(n_real, n_zero, n_fake, k, ld, ld_d):
    lib, cx = _lib(), _ctx()
    rng = np.random.default_rng(n_real + 3 * n_fake)
    n = n_real + n_zero + n_fake
    z = (3 * rng.standard_normal((n, ld))).astype(np.float32)
    yr = np.eye(k, dtype=np.float32)[rng.integers(0, k, n_real)]
    yf = np.eye(k, dtype=np.float32)[rng.integers(0, k, max(n_fake, 1))]
    lam = np.array([0.3, 0.6], np.float32)
    outs = []
    for _ in range(2):
        dl = torch.full((n * ld_d,), 7.0, device='cuda')
        loss, terms = torch.full((2,), 7.0, device='cuda'), torch.full((3,), 7.0, device='cuda')
        zt, yrt, yft, lt = _dev(z), _dev(yr), _dev(yf), _dev(lam)
        lib.call('tg_wgan_c_head_f32', _ptr(zt), ld, n_real, n_zero, n_fake, k, _ptr(yrt), _ptr(yft), _ptr(lt), _ptr(dl), ld_d, _ptr(loss),
                 _ptr(terms), cx.stream)
        torch.cuda.synchronize()
        outs.append((dl.cpu().numpy().reshape(n, ld_d), loss.cpu().numpy(), terms.cpu().numpy()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))
    dl, loss, terms = outs[0]
    vr, gr = W.ce_mean(z[:n_real, :k], yr)
    vf, gf = W.ce_mean(z[n - n_fake:, :k], yf[:n_fake]) if n_fake else (0.0, np.zeros((0, k)))
    assert abs(loss[0] - (vr + 0.6 * vf)) <= 1e-5 * (vr + 0.6 * vf) and loss[1] == 7.0 and terms[2] == 7.0
    np.testing.assert_allclose(terms[:2], [vr, vf], rtol=1e-5)
    np.testing.assert_allclose(dl[:n_real, :k], gr, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(dl[n - n_fake:, :k], 0.6 * gf, rtol=1e-4, atol=1e-7)
    assert not dl[n_real:n - n_fake].any() and not dl[:, k:].any()


# ------------------------------------------------------------------------------------------------------------- one synchronised iteration
def _f64(d):
    return {k: (_f64(v) if isinstance(v, dict) else np.asarray(v, np.float64)) for k, v in d.items()}


def _errs(got, ref):
    d = got - ref
    return np.linalg.norm(d) / (np.linalg.norm(ref) + 1e-30), np.abs(d).max() / (np.abs(ref).max() + 1e-30)


def _check_net(store, ref):
    """worst ratio error / bound over the variables of one network; <= 1 passes.  The bounds of tests/test_gpu_step.py, with the floor of
    tests/test_gpu_goodgan.py (1e-4 of the network's largest gradient).  A variable whose float64 gradient is analytically 0 (a batch
    norm's beta whose output the next batch norm centres; ~1e-16 in the restatement) carries fp32 rounding noise only: it is held to 1e-5
    of the network's largest gradient."""
    worst = 0.0
    gmax = max(np.abs(v).max() for v in ref.values())
    for k, gref in ref.items():
        d = store.get(k, 'grad') - gref
        if np.abs(gref).max() <= 1e-12 * gmax:
            r = np.abs(d).max() / (1e-5 * gmax)
        else:
            sc = max(np.abs(gref).max(), 1e-4 * gmax)
            r = max(np.abs(d).max() / (GRAD_MAX_TOL * sc), np.linalg.norm(d) / (GRAD_L2_TOL * max(np.linalg.norm(gref), sc)))
        if r > worst:
            worst, _check_net.worst = r, (k, np.abs(d).max(), np.abs(gref).max(), np.linalg.norm(d), np.linalg.norm(gref))
    return worst


def _sync(tr, st, key):
    store = tr.cx.stores[NETS[key]]
    for k in store.names():
        store.set(k, st['P'][k])
    for k in store.names(True):
        kind, off, n, shape = store.index[k]
        store.m[off:off + n].copy_(torch.from_numpy(st['m'][k].astype(np.float32).reshape(-1)))
        store.v[off:off + n].copy_(torch.from_numpy(st['v'][k].astype(np.float32).reshape(-1)))
    if key != 'C':
        cs = tr.cx.stores['classifier']
        for k in cs.names(False):
            cs.set(k, st['P'][k])


@pytest.mark.parametrize("data", ['cifar10', 'mnist', 'svhn'])
def test_synchronised_iteration_matches_the_restatement(data):
    from tg.runtime import InjectedRNG
    if data == 'cifar10':
        P = S.init_params(0)
        st = S.new_state(_f64(P))
        tr = G.fresh_trainer(G.make_config(SMALL, LOSS='WGAN_GP'), P)
        full = dict(S.SIZES, **SMALL)
        batch, rnd = S.synth_batch(100, full), S.synth_rnd(200, full)
        arrays = G.injected_arrays(rnd)
        zca = tuple(np.asarray(a, np.float64) for a in G.zca())
    else:
        from Model.Good_GAN import Good_GAN
        P = NG.init_params(data, 0)
        st = SG.new_state(_f64(P))
        tr = G.fresh_trainer(G.make_config_goodgan(data, SMALL, LOSS='WGAN_GP'), P, Good_GAN)
        batch, rnd = SG.synth_batch(data, 100, SMALL), SG.synth_rnd(data, 200, SMALL)
        arrays = G.injected_arrays_goodgan(rnd)
        zca = None
    gp_rnd = W.gp_draws(data, SMALL['B_G'], 300)
    arrays.update({'GP/' + k: v for k, v in gp_rnd.items()})
    rnd['D']['GP'] = gp_rnd
    b64, r64 = _f64(batch), _f64(rnd)
    tr.set_hyper(HYPER['lr'], HYPER['cla_lr'], HYPER['lambda_1'], HYPER['lambda_2'])
    cx, stores = tr.cx, tr.cx.stores
    cx.rng = InjectedRNG(arrays, cx.device)
    tr.feed(batch)
    # ---- D-update: the HIP run first, so that the restatement's discriminator sees the labels the HIP classifier gave (near-ties)
    tr._d_forward_backward()
    oh_unl, oh_unl_d = (a.numpy() for a in tr._d_labels)
    out = {}
    if data == 'cifar10':
        d_ref = W.d_phase_cifar10(st, b64, r64['D'], HYPER, zca, gp_out=out, labels=dict(unl=oh_unl, unl_d=oh_unl_d))
    else:
        d_ref = W.d_phase_goodgan(st, data, b64, r64['D'], HYPER, gp_out=out, labels=dict(unl=oh_unl, unl_d=oh_unl_d))
    sd = stores['discriminator']
    assert _check_net(sd, out['head_grads']) <= 1.0, _check_net.worst                           # the D backward of the head, before the penalty is added
    # the penalty part, against the restatement at the HIP path's own interpolated images and kinks (tests/test_gpu_wgan_gp*.py)
    gs = tr.model.last_gp_state
    y_g = np.asarray(batch['y_g'], np.float64)
    P64 = {k: np.asarray(sd.get(k), np.float64) for k in sd.names()}
    if data == 'cifar10':
        acts = {name: a.numpy() for (name, _, _, _), a in zip(tr.model.D_CONVS, gs['acts'])}
        pref = RC.gradient_penalty(P64, gs['x'].numpy(), y_g, {k: v for k, v in gp_rnd.items() if k != 'alpha'}, acts=acts)
    else:
        x = gs['x'].numpy()
        pref = RG.gradient_penalty(data, P64, x, y_g, {k: v for k, v in gp_rnd.items() if k != 'alpha'}, acts=[a.numpy() for a in gs['acts']])
    assert abs(float(tr._gp_w.cpu()[0]) - 10 * pref['gp']) <= GP_TOL * 10 * pref['gp']
    gflat = tr._gp_grad.cpu().numpy()
    for k, v in pref['grads'].items():
        kind, off, n, shape = sd.index[k]
        got = gflat[off:off + n].reshape(shape)
        if not np.any(v):
            assert not got.any(), k
            continue
        l2, mx = _errs(got, 10 * v)
        assert l2 <= GP_L2_TOL and mx <= GP_MAX_TOL, (k, l2, mx)
    tr._add_gp_slice(sd.g)                                                     # what the D segment adds before its exchange
    total = st['last_grads']['D']
    assert _check_net(sd, total) <= 1.0, _check_net.worst
    # negative control: the D gradient without the penalty term misses the bounds by more than 10x
    assert _check_net(sd, out['head_grads']) > 10.0
    d_got = tr.losses()[0]
    assert abs(d_got - d_ref) <= LOSS_TOL * max(1.0, abs(d_ref)), (d_got, d_ref)
    wd = tr.wgan_terms_dev.cpu().numpy()
    np.testing.assert_allclose(wd[:3], out['wd'], rtol=1e-3, atol=1e-4)
    tr._train_op(tr.d_optimizer, sd)
    _sync(tr, st, 'D')
    # ---- G-update
    g_ref = W.g_phase_cifar10(st, b64, r64['G'], HYPER) if data == 'cifar10' else W.g_phase_goodgan(st, data, b64, r64['G'], HYPER)
    tr._g_forward_backward()
    assert _check_net(stores['good_generator'], st['last_grads']['G']) <= 1.0, _check_net.worst
    assert abs(tr.losses()[1] - g_ref) <= LOSS_TOL * max(1.0, abs(g_ref))
    tr._train_op(tr.g_optimizer, stores['good_generator'])
    _sync(tr, st, 'G')
    # ---- C-update
    c_ref = W.c_phase_cifar10(st, b64, r64['C'], HYPER, zca) if data == 'cifar10' else W.c_phase_goodgan(st, data, b64, r64['C'], HYPER)
    tr._c_forward_backward()
    assert _check_net(stores['classifier'], st['last_grads']['C']) <= 1.0, _check_net.worst
    assert abs(tr.losses()[2] - c_ref) <= LOSS_TOL * max(1.0, abs(c_ref))


# ------------------------------------------------------------------------------------------------------------- execution modes
def _run_modes(mode, iters, sizes, hyper2, stats=False):
    tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=None, EXEC_MODE=mode, SEED=3, LOSS='WGAN_GP'))
    tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
    full = dict(S.SIZES, **sizes)
    tr.feed(S.synth_batch(7, full))
    losses = []
    for it in range(iters):
        if it == iters - 1:
            tr.set_hyper(**hyper2)
        tr.sample_latent()
        tr.train_iteration()
        losses.append(tr.losses())
    torch.cuda.synchronize()
    out = dict(losses=losses, p={k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}, terms=tr.wgan_terms_dev.cpu().numpy())
    if stats:
        out['stats'] = tr.training_statistics()
    return out


def test_eager_plan_graph_are_bit_identical_and_follow_set_hyper():
    """three PhiloxRNG iterations at the reference sizes, then new lambdas and a fourth: a lambda baked into a launch argument of a recorded
    plan or graph would leave the replayed modes on the old values."""
    runs = {m: _run_modes(m, 4, {}, dict(lambda_1=0.9, lambda_2=0.25)) for m in ('eager', 'overlap', 'plan', 'graph')}
    ref = runs['eager']
    for m, r in runs.items():
        assert r['losses'] == ref['losses'], (m, r['losses'], ref['losses'])
        for k in ref['p']:
            assert r['p'][k].tobytes() == ref['p'][k].tobytes(), (m, k)
        assert r['terms'].tobytes() == ref['terms'].tobytes(), m
    # the fourth iteration's d_loss is the head with the NEW lambdas: -(wd1 + .9 wd2 + .25 wd3) + 10 gp
    wd1, wd2, wd3, gp = (float(v) for v in ref['terms'])
    assert abs(ref['losses'][3][0] - (-(wd1 + 0.9 * wd2 + 0.25 * wd3) + 10 * gp)) <= 1e-5 * (1 + abs(ref['losses'][3][0]))
    assert gp > 0 and all(np.isfinite(v) for l in ref['losses'] for v in l)
    # and the lambdas matter: with the old ones the fourth iteration differs
    old = _run_modes('plan', 4, {}, dict(lambda_1=0.3, lambda_2=0.5))
    assert old['losses'][3][0] != ref['losses'][3][0]


def test_training_statistics_report_the_wgan_gp_losses():
    r = _run_modes('plan', 3, SMALL, dict(lambda_1=0.3, lambda_2=0.5), stats=True)
    d, g, c = r['stats']
    assert all(np.isfinite(v) for v in (d, g, c)) and c > 0


def test_plan_iterations_are_isolated_from_a_standalone_penalty():
    """a standalone _gradient_penalty (phase 'wgan_gp', its own buffers) at another n between two plan iterations changes nothing."""
    sizes = SMALL

    def run(interleave):
        tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=None, EXEC_MODE='plan', SEED=4, LOSS='WGAN_GP'))
        tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
        full = dict(S.SIZES, **sizes)
        tr.feed(S.synth_batch(9, full))
        for it in range(5):
            tr.sample_latent()
            tr.train_iteration()
            if interleave and it == 2:
                m, cx = tr.model, tr.cx
                b = S.synth_batch(11, dict(S.SIZES, B_G=40, L_D=20, U_D=20))
                gp = tr._gradient_penalty(cx.from_numpy(b['x_l_d']), cx.from_numpy(b['x_u_d']), cx.from_numpy(b['y_l_d']), m.discriminator, 10.0)
                assert float(gp[0].item()) > 0
        torch.cuda.synchronize()
        return tr.losses(), {k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}
    a, b = run(False), run(True)
    assert a[0] == b[0]
    for k in a[1]:
        assert a[1][k].tobytes() == b[1][k].tobytes(), k


# ------------------------------------------------------------------------------------------------------------- data parallel
WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, os.path.join({root!r}, "tensorflow-implementation-of-triple-gan_amd"))
import torch
import gpu_common as G
from oracle import step_cifar10 as S
sizes = {sizes!r}
tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=None, EXEC_MODE='plan', SEED=5, LOSS='WGAN_GP'))
rank = tr.rank
tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
full = dict(S.SIZES, **sizes)
p0 = {{k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}}
sums = []
for it in range({iters}):
    tr.feed(S.synth_batch(1000 * rank + it, full))
    tr.sample_latent()
    tr.train_iteration()
    sums.append([float(st.p.double().sum().item()) for st in tr.cx.stores.values()])
torch.cuda.synchronize()
torch.save(dict(world=tr.world, rank=rank, sums=sums, losses=tr.losses(), p0=p0, p={{k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}}),
           {out!r} % rank)
torch.distributed.destroy_process_group()
'''


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _one_process_average(sizes, p0, iters):
    """one process, no replicas: per solver run each shard's gradient (its own batch and Philox seed, as rank r draws them) is computed, the
    two are summed as the all-reduce does and the optimiser steps with grad_scale 1/2."""
    tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=False, EXEC_MODE='eager', SEED=5, LOSS='WGAN_GP'))
    tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
    cx, st = tr.cx, tr.cx.stores
    for k, s in st.items():
        s.p.copy_(torch.from_numpy(p0[k]))
    st['classifier'].ema.copy_(st['classifier'].p)
    full = dict(S.SIZES, **sizes)
    phs = [tr.z_g_ph, tr.y_g_ph, tr.x_l_c_ph, tr.y_l_c_ph, tr.x_l_d_ph, tr.y_l_d_ph, tr.x_u_d_ph, tr.x_u_c_ph]
    rng = [torch.tensor([5 + 7919 * r, 0], dtype=torch.int64, device=cx.device) for r in range(2)]
    for it in range(iters):
        feeds = []
        for r in range(2):
            cx.rng.state.copy_(rng[r])
            tr.feed(S.synth_batch(1000 * r + it, full))
            tr.sample_latent()
            feeds.append([p.t.clone() for p in phs])

        def solver(fn, net, opt):
            g = []
            for r in range(2):
                cx.rng.state.copy_(rng[r])
                for p, v in zip(phs, feeds[r]):
                    p.t.copy_(v)
                tr._g_saved = None
                fn()
                if net == 'discriminator':
                    tr._add_gp_slice(st[net].g)
                g.append(st[net].g.clone())
            st[net].g.copy_(g[0] + g[1])
            tr._train_op(opt, st[net], 0.5)
        solver(tr._d_forward_backward, 'discriminator', tr.d_optimizer)
        solver(tr._g_forward_backward, 'good_generator', tr.g_optimizer)
        solver(tr._c_forward_backward, 'classifier', tr.c_optimizer)
        for r in range(2):
            cx.rng.state.copy_(rng[r])
            cx.rng.advance(cx)
            rng[r].copy_(cx.rng.state)
    torch.cuda.synchronize()
    return {k: s.p.cpu().numpy() for k, s in st.items()}


def test_two_ranks_on_one_gpu_average_the_penalty_gradient(tmp_path):
    sizes, iters = SMALL, 2
    port = _free_port()
    out = str(tmp_path / "r%d.pt")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, sizes=sizes, out=out, iters=iters))
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   TG_DIST_BACKEND="gloo", TG_DEVICE_INDEX="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-3000:]
    r = [torch.load(out % i, weights_only=False) for i in range(2)]
    assert r[0]['world'] == r[1]['world'] == 2
    assert r[0]['sums'] == r[1]['sums']
    for k in r[0]['p']:
        np.testing.assert_array_equal(r[0]['p'][k], r[1]['p'][k])
    assert r[0]['losses'] != r[1]['losses']
    ref = _one_process_average(sizes, r[0]['p0'], iters)
    for k in ref:
        assert np.abs(ref[k] - r[0]['p'][k]).max() == 0.0, (k, np.abs(ref[k] - r[0]['p'][k]).max())
