"""GPU tests of config.OPTIMIZER = 'rmsprop' / 'momentum' (DESIGN §9.5): tg_momentum_f32 and tg_rmsprop_f32 against the float64
restatement (tests/optimizer_reference.py; its forms, bounds and negative controls are checked on the CPU by
tests/test_optimizer_reference.py on the same inputs), the optimisers inside the training step, bit-identical execution modes that
follow set_hyper(lr), checkpoints and resume, and two data-parallel ranks."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import step_cifar10 as S
import gpu_common as G
import optimizer_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
NETS = ('discriminator', 'good_generator', 'classifier')
SUFFIXES = {'adam': ['/Adam_optimizer', '/Adam_optimizer_1'], 'momentum': ['/Momentum'],
            'rmsprop': ['/RMSProp_optimizer', '/RMSProp_optimizer_1']}


def _lib():
    from tg import lib
    lib.load()
    return lib


def _st():
    from tg import lib
    return lib.cur_stream()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()


def _host(t):
    return t.detach().cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------------------- 1. the kernels
def _run_kernel(kind, case, grad_scale=0.5):
    """the case's steps through the entry point, gradients divided by grad_scale (exact for 0.5) -> host arrays."""
    lib = _lib()
    h = case['hyper']
    p, lr = _dev(case['p0']), _dev([h['lr']])
    n = p.numel()
    if kind == 'momentum':
        accum = _dev(case['slots0']['accum'])
        for g in case['grads']:
            gd = _dev(g / np.float32(grad_scale))
            lib.call('tg_momentum_f32', lib.ptr(p), lib.ptr(gd), lib.ptr(accum), n, lib.ptr(lr), h['momentum'], grad_scale, _st())
        torch.cuda.synchronize()
        return dict(p=_host(p), accum=_host(accum))
    rms, mom = _dev(case['slots0']['rms']), _dev(case['slots0']['mom'])
    for g in case['grads']:
        gd = _dev(g / np.float32(grad_scale))
        lib.call('tg_rmsprop_f32', lib.ptr(p), lib.ptr(gd), lib.ptr(rms), lib.ptr(mom), n, lib.ptr(lr), h['decay'], h['momentum'], h['epsilon'],
                 grad_scale, _st())
    torch.cuda.synchronize()
    return dict(p=_host(p), rms=_host(rms), mom=_host(mom))


def _miss(kind, case, got, **variant):
    ref = R.run_reference(kind, case, **variant)
    return np.abs(got['p'].astype(np.float64) - ref['p']).max() / R.param_bound(ref, R.STEPS), ref


def test_momentum_kernel_matches_the_restatement():
    case = R.kernel_case('momentum')
    assert R.N % 4 == 3
    got = _run_kernel('momentum', case)
    miss, ref = _miss('momentum', case, got)
    slot = R.slots_close(got['accum'], ref['accum'])
    print('momentum: parameter error / bound %.3f, slot error / bound %.3f' % (miss, slot))
    assert miss <= 1.0 and slot <= 1.0
    assert _miss('momentum', case, got, nesterov=True)[0] > 10.0                   # negative control: the Nesterov form
    again = _run_kernel('momentum', case)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


@pytest.mark.parametrize("kind", ['rmsprop', 'rmsprop_small', 'rmsprop_mom'])
def test_rmsprop_kernel_matches_the_restatement(kind):
    case = R.kernel_case(kind)
    got = _run_kernel('rmsprop', case)
    miss, ref = _miss('rmsprop', case, got)
    # with momentum != 0 the sum mom*momentum + x can cancel: bounded against the largest slot value, like the parameter
    atol = R.SLOT_ATOL if kind != 'rmsprop_mom' else 1e-6 * np.abs(ref['mom']).max() * R.STEPS
    s_rms, s_mom = R.slots_close(got['rms'], ref['rms']), R.slots_close(got['mom'], ref['mom'], atol)
    print('%s: parameter error / bound %.3f, rms %.3f, mom %.3f' % (kind, miss, s_rms, s_mom))
    assert miss <= 1.0 and s_rms <= 1.0 and s_mom <= 1.0
    if kind == 'rmsprop_small':
        assert _miss('rmsprop', case, got, eps_outside=True)[0] > 10.0             # negative control: epsilon outside the root
    if kind == 'rmsprop':
        assert _miss('rmsprop', case, got, rms0=0.0)[0] > 10.0                     # negative control: rms starting at 0
    again = _run_kernel('rmsprop', case)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def test_kernels_follow_the_device_learning_rate_and_leave_their_inputs():
    """lr is read from the device at launch (a replayed plan follows set_hyper); the gradient buffer is not written."""
    lib = _lib()
    n = 1031
    rng = np.random.default_rng(5)
    p0, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    for lr_v in (3e-4, 7e-2):
        p, gd, a, lr = _dev(p0), _dev(g), torch.zeros(n, device='cuda'), _dev([lr_v])
        lib.call('tg_momentum_f32', lib.ptr(p), lib.ptr(gd), lib.ptr(a), n, lib.ptr(lr), 0.9, 1.0, _st())
        want, _ = R.momentum_step(p0, g, np.zeros(n), R.f32(lr_v), R.f32(0.9))
        assert np.abs(_host(p) - want).max() <= 1e-6 * R.f32(lr_v) * np.abs(g).max() + 2e-7 * np.abs(p0).max()
        assert _host(gd).tobytes() == g.tobytes()
        p, rms, mom = _dev(p0), torch.ones(n, device='cuda'), torch.zeros(n, device='cuda')
        lib.call('tg_rmsprop_f32', lib.ptr(p), lib.ptr(gd), lib.ptr(rms), lib.ptr(mom), n, lib.ptr(lr), 0.9, 0.0, 1e-10, 1.0, _st())
        want, _, wmom = R.rmsprop_step(p0, g, np.ones(n), np.zeros(n), R.f32(lr_v), R.f32(0.9), 0.0, R.f32(1e-10))
        assert np.abs(_host(p) - want).max() <= 1e-6 * np.abs(wmom).max() + 2e-7 * np.abs(p0).max()
        assert _host(gd).tobytes() == g.tobytes()


def test_bad_arguments_return_an_error_status():
    lib = _lib()
    h = lib.load()
    n = 64
    buf = [torch.zeros(n + 4, device='cuda') for _ in range(4)]
    lr = torch.zeros(1, device='cuda')
    ok = [lib.ptr(b) for b in buf]
    off = [lib.ptr(b[1:]) for b in buf]                                            # 4 bytes past a 16-byte boundary
    assert h.tg_momentum_f32(ok[0], ok[1], ok[2], n, lib.ptr(lr), 0.9, 1.0, _st()) == 0
    assert h.tg_rmsprop_f32(ok[0], ok[1], ok[2], ok[3], n, lib.ptr(lr), 0.9, 0.0, 1e-10, 1.0, _st()) == 0
    assert h.tg_momentum_f32(ok[0], ok[1], ok[2], 0, lib.ptr(lr), 0.9, 1.0, _st()) != 0
    assert h.tg_rmsprop_f32(ok[0], ok[1], ok[2], ok[3], 0, lib.ptr(lr), 0.9, 0.0, 1e-10, 1.0, _st()) != 0
    assert h.tg_momentum_f32(ok[0], ok[1], ok[2], n, None, 0.9, 1.0, _st()) != 0
    assert h.tg_rmsprop_f32(ok[0], ok[1], None, ok[3], n, lib.ptr(lr), 0.9, 0.0, 1e-10, 1.0, _st()) != 0
    for k in range(3):
        a = list(ok[:3])
        a[k] = off[k]
        assert h.tg_momentum_f32(a[0], a[1], a[2], n, lib.ptr(lr), 0.9, 1.0, _st()) != 0
        assert b'16-B aligned' in h.tg_last_error_string()
    for k in range(4):
        a = list(ok)
        a[k] = off[k]
        assert h.tg_rmsprop_f32(a[0], a[1], a[2], a[3], n, lib.ptr(lr), 0.9, 0.0, 1e-10, 1.0, _st()) != 0
        assert b'16-B aligned' in h.tg_last_error_string()
    with pytest.raises(lib.TgError, match='momentum'):
        lib.call('tg_momentum_f32', ok[0], ok[1], ok[2], -5, lib.ptr(lr), 0.9, 1.0, _st())
    torch.cuda.synchronize()
    assert not any(b.any().item() for b in buf[:2])                               # zero gradients moved nothing; nothing was written by the refusals


# ------------------------------------------------------------------------------------------------------------- 2. in the step
def _record_train_ops(tr):
    """wrap Train._train_op: p, g and the slots of the network before and after each optimiser application."""
    rec, orig = [], tr._train_op

    def wrapped(optimizer, store, grad_scale=1.0):
        torch.cuda.synchronize()
        before = {k: _host(getattr(store, k)) for k in 'pgmv'}
        t0 = int(store.step.item())
        orig(optimizer, store, grad_scale)
        torch.cuda.synchronize()
        rec.append(dict(net=store.name, opt=optimizer, grad_scale=grad_scale, before=before, after={k: _host(getattr(store, k)) for k in 'pgmv'},
                        steps=(t0, int(store.step.item()))))
    tr._train_op = wrapped
    return rec


def _check_application(r, lr):
    """one recorded application against the restatement applied to the before-values, within the bounds of part 1 for one step."""
    b, a, opt = r['before'], r['after'], r['opt']
    g = b['g'].astype(np.float64) * r['grad_scale']
    assert a['g'].tobytes() == b['g'].tobytes()
    tag = (r['net'], opt.kind)
    if opt.kind == 'adam':
        assert r['steps'][1] == r['steps'][0] + 1, tag                              # covered by tests/test_gpu_kernels.py and test_gpu_step.py
        return
    assert r['steps'][1] == r['steps'][0], tag                                      # no step count
    if opt.kind == 'momentum':
        p, accum = R.momentum_step(b['p'], g, b['m'], lr, R.f32(opt.momentum))
        # accum*momentum + g can cancel in a real step: the product's rounding, u * max|accum before|, is the absolute part
        assert R.slots_close(a['m'], accum, R.SLOT_ATOL + R.U * np.abs(b['m']).max()) <= 1.0, tag
        assert a['v'].tobytes() == b['v'].tobytes(), tag
    else:
        p, ms, mom = R.rmsprop_step(b['p'], g, b['v'], b['m'], lr, R.f32(opt.decay), R.f32(opt.momentum), R.f32(opt.epsilon))
        assert opt.momentum == 0.0
        assert R.slots_close(a['v'], ms) <= 1.0 and R.slots_close(a['m'], mom) <= 1.0, tag
        assert a['v'].min() > 0, tag
    ref = dict(max_update=np.abs(p - b['p']).max(), max_p=np.abs(p).max())
    err = np.abs(a['p'].astype(np.float64) - p).max()
    assert err <= R.param_bound(ref, 1), (tag, err, R.param_bound(ref, 1))
    assert ref['max_update'] > 0 and a['p'].tobytes() != b['p'].tobytes(), tag      # the network moved
    assert np.isfinite(a['p']).all(), tag


@pytest.mark.parametrize("optimizer, loss", [('rmsprop', 'GAN'), ('momentum', 'GAN'), (('rmsprop', 'adam', 'momentum'), 'GAN'), ('rmsprop', 'WGAN_GP')])
def test_two_eager_iterations_apply_the_restatement_to_every_network(optimizer, loss):
    from Training.Train_goodGAN import check_optimizer
    cfg = G.make_config(SMALL, USE_HIP_GRAPH=False, EXEC_MODE='eager', SEED=2, OPTIMIZER=optimizer, LOSS=loss)
    kinds = check_optimizer(cfg)
    tr = G.fresh_trainer(cfg)
    assert tr.optimizer_kinds == kinds and [tr.cx.stores[n].optimizer for n in NETS] == list(kinds)
    for net, kind in zip(NETS, kinds):
        st = tr.cx.stores[net]
        assert float(st.v.min()) == float(st.v.max()) == (1.0 if kind == 'rmsprop' else 0.0) and not st.m.any().item(), net
    tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
    lr, cla_lr = (float(v) for v in tr.hyper[:2].cpu().numpy())
    assert (lr, cla_lr) == (R.f32(3e-4), R.f32(3e-3))
    rec = _record_train_ops(tr)
    full = dict(S.SIZES, **SMALL)
    for it in range(2):
        tr.feed(S.synth_batch(60 + it, full))
        tr.sample_latent()
        tr.train_iteration(use_graph=False)
    torch.cuda.synchronize()
    assert [r['net'] for r in rec] == list(NETS) * 2
    for r in rec:
        assert r['opt'].kind == kinds[NETS.index(r['net'])]
        _check_application(r, cla_lr if r['net'] == 'classifier' else lr)
    assert all(np.isfinite(v) for v in tr.losses())
    if loss == 'WGAN_GP':                                                           # the penalty's gradient is in store.g before the optimiser reads it
        assert float(tr._gp_grad.abs().max()) > 0 and float(tr.wgan_terms_dev.cpu()[3]) > 0


# ------------------------------------------------------------------------------------------------------------- 3. execution modes
def _run_modes(mode, hyper4, optimizer='rmsprop', iters=4):
    tr = G.fresh_trainer(G.make_config(SMALL, USE_HIP_GRAPH=None, EXEC_MODE=mode, SEED=3, OPTIMIZER=optimizer))
    tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
    tr.feed(S.synth_batch(7, dict(S.SIZES, **SMALL)))
    snaps = []
    for it in range(iters):
        if it == iters - 1:
            tr.set_hyper(**hyper4)
        tr.sample_latent()
        tr.train_iteration()
        if it >= iters - 2:
            torch.cuda.synchronize()
            snaps.append({k: _host(st.p) for k, st in tr.cx.stores.items()})
    slots = {k: (_host(st.m), _host(st.v)) for k, st in tr.cx.stores.items()}
    return dict(after3=snaps[0], after4=snaps[1], slots=slots, losses=tr.losses())


def test_execution_modes_are_bit_identical_and_follow_set_hyper_lr():
    """three Philox iterations, then set_hyper(lr, cla_lr) and a fourth: a learning rate passed by value into a recorded plan or graph
    would leave the replayed modes on the old one.  Eager launches read the device scalar afresh (part 2 holds them to it)."""
    new = dict(lr=9e-4, cla_lr=1e-3)
    runs = {m: _run_modes(m, new) for m in ('eager', 'overlap', 'plan', 'graph')}
    ref = runs['eager']
    for m, r in runs.items():
        assert r['losses'] == ref['losses'], (m, r['losses'], ref['losses'])
        for k in ref['after4']:
            assert r['after3'][k].tobytes() == ref['after3'][k].tobytes(), (m, k)
            assert r['after4'][k].tobytes() == ref['after4'][k].tobytes(), (m, k)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r['slots'][k], ref['slots'][k])), (m, k)
    old = _run_modes('plan', dict(lr=3e-4, cla_lr=3e-3))
    for k in ref['after4']:
        assert old['after3'][k].tobytes() == ref['after3'][k].tobytes(), k
        assert old['after4'][k].tobytes() != ref['after4'][k].tobytes(), k
    # D runs first in an iteration, so from the same third iterate both fourth iterations see the same D gradient and rms; RMSProp with
    # momentum 0 steps by (g*lr)/sqrt(ms + eps), so the new step is the old one times the ratio of the rates, 3 (least squares over the
    # network: the differences of fp32 weights carry the rounding of the weights themselves)
    d3, d_new, d_old = (r['discriminator'].astype(np.float64) for r in (ref['after3'], ref['after4'], old['after4']))
    ratio = np.dot(d_new - d3, d_old - d3) / np.dot(d_old - d3, d_old - d3)
    assert abs(ratio - 3.0) <= 1e-2, ratio


# ------------------------------------------------------------------------------------------------------------- 4. checkpoints and resume
def _state(tr):
    """values, running statistics, step counts and EMA shadows as whole buffers; the slots variable by variable — the 32-float padding
    between variables is no variable and is not stored (RMSProp's rms decays there too, 0.9^t, next to a zero gradient and a zero value)."""
    out = {}
    for k, st in tr.cx.stores.items():
        for buf in ('p', 's', 'step'):
            out[k + '/' + buf] = _host(getattr(st, buf))
        for nm in st.names(True):
            out[nm + '/m'], out[nm + '/v'] = st.get(nm, 'm'), st.get(nm, 'v')
        if st.ema is not None:
            out[k + '/ema'] = _host(st.ema)
    return out


def _expected_keys(tr, kinds):
    keys = {'tg/rng_state', 'tg/rng_streams', 'tg/epoch'}
    for net, kind in zip(NETS, kinds):
        st = tr.cx.stores[net]
        keys.add('tg/adam_step/' + net)
        for nm, _shape, trainable in st.specs:
            keys.add(nm)
            if trainable:
                keys |= {nm + s for s in SUFFIXES[kind]}
                if net == 'classifier':
                    keys.add(nm + '/ExponentialMovingAverage')
    return keys


@pytest.mark.parametrize("kinds", [('rmsprop', 'momentum', 'adam'), ('momentum', 'rmsprop', 'rmsprop')])
def test_resume_continues_bit_identically_and_refuses_another_optimizer(tmp_path, kinds):
    from Training.Saver import Saver
    feeds = [S.synth_batch(40 + i, dict(S.SIZES, **SMALL)) for i in range(4)]

    def run(tr, its):
        for i in its:
            tr.feed(feeds[i])
            tr.sample_latent()
            tr.train_iteration()
        torch.cuda.synchronize()

    a = G.fresh_trainer(G.make_config(SMALL, SEED=9, USE_HIP_GRAPH=True, OPTIMIZER=kinds))
    a.set_hyper(lambda_1=0.3, lambda_2=0.5)
    run(a, [0, 1])
    saver = Saver(str(tmp_path))
    saver.set_save_path(comments='resume test')
    path = saver.save(a, 'model_0002.ckpt')
    with np.load(path) as z:
        assert set(z.files) == _expected_keys(a, kinds)
        for net, kind in zip(NETS, kinds):
            assert int(z['tg/adam_step/' + net].reshape(-1)[0]) == (2 if kind == 'adam' else 0)
            if kind == 'rmsprop':
                nm = a.cx.stores[net].names(True)[0]
                assert np.array_equal(z[nm + '/RMSProp_optimizer'], a.cx.stores[net].get(nm, 'v')) and z[nm + '/RMSProp_optimizer'].min() > 0
    run(a, [2, 3])
    want, want_losses = _state(a), a.losses()

    b = G.fresh_trainer(G.make_config(SMALL, SEED=1234, USE_HIP_GRAPH=True, OPTIMIZER=kinds))      # different seed: everything comes from the file
    b.set_hyper(lambda_1=0.3, lambda_2=0.5)
    assert Saver(str(tmp_path)).restore(b) == 2
    run(b, [2, 3])
    got = _state(b)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert b.losses() == want_losses

    c = G.fresh_trainer(G.make_config(SMALL, SEED=9, OPTIMIZER=(kinds[0], 'adam', kinds[2])))
    before = _state(c)
    with pytest.raises(KeyError) as e:
        Saver(str(tmp_path)).restore(c)
    msg = str(e.value)
    assert 'good_generator' in msg and kinds[1] in msg and 'adam' in msg
    after = _state(c)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)               # nothing zero-filled, nothing half restored


# ------------------------------------------------------------------------------------------------------------- 5. data parallel
WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, os.path.join({root!r}, "tensorflow-implementation-of-triple-gan_amd"))
import torch
import gpu_common as G
from oracle import step_cifar10 as S
sizes = {sizes!r}
tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=None, EXEC_MODE='plan', SEED=5, OPTIMIZER={optimizer!r}))
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
torch.save(dict(world=tr.world, rank=rank, sums=sums, losses=tr.losses(), p0=p0, p={{k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}},
                v={{k: st.v.cpu().numpy() for k, st in tr.cx.stores.items()}}),
           {out!r} % rank)
torch.distributed.destroy_process_group()
'''


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _one_process_average(sizes, p0, iters, optimizer):
    """one process, no replicas: per solver run each shard's gradient (its own batch and Philox seed, as rank r draws them) is computed, the
    two are summed as the all-reduce does and the optimiser steps with grad_scale 1/2."""
    tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=False, EXEC_MODE='eager', SEED=5, OPTIMIZER=optimizer))
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
    return {k: s.p.cpu().numpy() for k, s in st.items()}, {k: s.v.cpu().numpy() for k, s in st.items()}


def test_two_ranks_on_one_gpu_step_like_one_process_on_the_summed_gradient(tmp_path):
    sizes, iters, optimizer = SMALL, 2, ('rmsprop', 'momentum', 'rmsprop')
    port = _free_port()
    out = str(tmp_path / "r%d.pt")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, sizes=sizes, out=out, iters=iters, optimizer=optimizer))
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
        np.testing.assert_array_equal(r[0]['v'][k], r[1]['v'][k])
    assert r[0]['losses'] != r[1]['losses']
    ref_p, ref_v = _one_process_average(sizes, r[0]['p0'], iters, optimizer)
    for k in ref_p:
        assert np.abs(ref_p[k] - r[0]['p'][k]).max() == 0.0, (k, np.abs(ref_p[k] - r[0]['p'][k]).max())
        assert np.abs(ref_v[k] - r[0]['v'][k]).max() == 0.0, k
        assert np.abs(r[0]['p'][k] - r[0]['p0'][k]).max() > 0, k
