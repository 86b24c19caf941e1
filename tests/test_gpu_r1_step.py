"""GPU tests of the training step with config.R1_GAMMA (Training/Train_goodGAN.py), following tests/test_gpu_wgan_gp_step.py
test for test: one phase-synchronised iteration against the float64 restatement (tests/r1_reference.d_phase on the oracle's GAN step) on
CIFAR-10, MNIST and SVHN at that file's bounds; eager, overlap, plan and graph bit-identical over three iterations at the reference sizes
with a fourth after set_r1_gamma(); losses()[0] = the GAN d_loss + the penalty; isolation from a standalone penalty at another n; two
data-parallel ranks; a checkpoint taken with R1 on; and a trainer built without the option, which allocates nothing of it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nets_goodgan as NG
from oracle import step_cifar10 as S
from oracle import step_goodgan as SG
import gpu_common as G
import r1_reference as R
from test_gpu_wgan_gp_step import (GP_L2_TOL, GP_MAX_TOL, GP_TOL, HYPER, LOSS_TOL, ROOT, SMALL, _check_net, _errs, _f64, _free_port, _sync)

pytestmark = pytest.mark.gpu
GAMMA = 10.0


# ------------------------------------------------------------------------------------------------------------- one synchronised iteration
@pytest.mark.parametrize("data", ['cifar10', 'mnist', 'svhn'])
def test_synchronised_iteration_matches_the_restatement(data):
    from tg.runtime import InjectedRNG
    if data == 'cifar10':
        P = S.init_params(0)
        st = S.new_state(_f64(P))
        tr = G.fresh_trainer(G.make_config(SMALL, R1_GAMMA=GAMMA), P)
        full = dict(S.SIZES, **SMALL)
        batch, rnd = S.synth_batch(100, full), S.synth_rnd(200, full)
        arrays = G.injected_arrays(rnd)
        zca = tuple(np.asarray(a, np.float64) for a in G.zca())
    else:
        from Model.Good_GAN import Good_GAN
        P = NG.init_params(data, 0)
        st = SG.new_state(_f64(P))
        tr = G.fresh_trainer(G.make_config_goodgan(data, SMALL, R1_GAMMA=GAMMA), P, Good_GAN)
        batch, rnd = SG.synth_batch(data, 100, SMALL), SG.synth_rnd(data, 200, SMALL)
        arrays = G.injected_arrays_goodgan(rnd)
        zca = None
    n_real = SMALL['L_D'] + SMALL['U_D']
    r1_rnd = R.r1_draws(data, n_real, 300)
    arrays.update({'R1/' + k: v for k, v in r1_rnd.items()})
    rnd['D']['R1'] = r1_rnd
    b64, r64 = _f64(batch), _f64(rnd)
    tr.set_hyper(HYPER['lr'], HYPER['cla_lr'], HYPER['lambda_1'], HYPER['lambda_2'])
    cx, stores = tr.cx, tr.cx.stores
    cx.rng = InjectedRNG(arrays, cx.device)
    tr.feed(batch)
    # ---- D-update: the HIP run first, so that the restatement's discriminator sees the labels the HIP classifier gave (near-ties)
    tr._d_forward_backward()
    oh_unl, oh_unl_d = (a.numpy() for a in tr._d_labels)
    out = {}
    d_ref = R.d_phase(data, st, b64, r64['D'], HYPER, GAMMA, zca=zca, out=out, labels=dict(unl=oh_unl, unl_d=oh_unl_d))
    sd = stores['discriminator']
    assert _check_net(sd, out['head_grads']) <= 1.0, _check_net.worst                           # the D backward of the head, before the penalty is added
    # the penalty part, against the restatement at the HIP path's own kinks: evaluated at X_P itself, with [y_l_d | oh_unl_d]
    gs = tr.model.last_gp_state
    X_P = np.concatenate([batch['x_l_d'], batch['x_u_d']], axis=0)
    assert np.array_equal(gs['x'].numpy().reshape(X_P.shape), X_P) and 'alpha' not in gs
    P64 = {k: np.asarray(sd.get(k), np.float64) for k in sd.names()}
    if data == 'cifar10':
        acts = {name: a.numpy() for (name, _, _, _), a in zip(tr.model.D_CONVS, gs['acts'])}
    else:
        acts = [a.numpy() for a in gs['acts']]
    xr = X_P.reshape(n_real, -1) if data == 'mnist' else X_P
    pref = R.r1(data, P64, xr, out['Y_P'], r1_rnd, GAMMA, acts=acts)
    terms = tr.r1_terms()
    assert abs(terms['penalty'] - pref['penalty']) <= GP_TOL * pref['penalty'] and terms['penalty'] == float(tr._gp_w.cpu()[0])
    assert abs(terms['grad_sq_mean'] - pref['grad_sq_mean']) <= GP_TOL * pref['grad_sq_mean']
    gflat = tr._gp_grad.cpu().numpy()
    for k, v in pref['grads'].items():
        kind, off, n, shape = sd.index[k]
        got = gflat[off:off + n].reshape(shape)
        if not np.any(v):
            assert not got.any(), k
            continue
        l2, mx = _errs(got, v.reshape(shape))
        assert l2 <= GP_L2_TOL and mx <= GP_MAX_TOL, (k, l2, mx)
    # negative control: the penalty with y_g-like labels instead of [y_l_d | oh_unl_d] misses those bounds by more than 10x
    wrong = R.r1(data, P64, xr, np.roll(out['Y_P'], 1, axis=1), r1_rnd, GAMMA)
    worst = max(_errs(gflat[sd.index[k][1]:sd.index[k][1] + sd.index[k][2]].reshape(sd.index[k][3]), v.reshape(sd.index[k][3]))[0]
                for k, v in wrong['grads'].items() if np.any(v))
    assert worst > 10 * GP_L2_TOL, worst
    tr._add_gp_slice(sd.g)                                                     # what the D segment adds before its exchange
    total = st['last_grads']['D']
    assert _check_net(sd, total) <= 1.0, _check_net.worst
    # negative control: the D gradient WITHOUT the penalty term fails the very check the sum passes.  (These are the step's loose bounds,
    # 1e-2 / 5e-2 of a network-wide scale, and gamma = 10 weighs the penalty's gradient about as much as the head's on fresh weights — so
    # no 10x is asked here; the penalty's own gradient is held to the tight bounds above, with a control that misses those by 10x.)
    assert _check_net(sd, out['head_grads']) > 1.0
    d_got = tr.losses()[0]
    assert abs(d_got - d_ref) <= LOSS_TOL * max(1.0, abs(d_ref)), (d_got, d_ref)
    assert abs((d_got - terms['penalty']) - out['gan_d_loss']) <= LOSS_TOL * max(1.0, abs(d_ref))
    tr._train_op(tr.d_optimizer, sd)
    _sync(tr, st, 'D')
    # ---- G-update: the oracle's GAN step, untouched by the penalty
    if data == 'cifar10':
        g_ref = S.g_phase(st, b64, r64['G'], HYPER)
    else:
        g_ref = SG.g_phase(st, data, b64, r64['G'], HYPER)
    tr._g_forward_backward()
    assert _check_net(stores['good_generator'], st['last_grads']['G']) <= 1.0, _check_net.worst
    assert abs(tr.losses()[1] - g_ref) <= LOSS_TOL * max(1.0, abs(g_ref))
    tr._train_op(tr.g_optimizer, stores['good_generator'])
    _sync(tr, st, 'G')
    # ---- C-update: D(x_u_c) is applied with the discriminator that has just taken the penalised step.  The HIP run first, so that the
    # restatement labels x_u_c as the HIP classifier did (near-ties)
    tr._c_forward_backward()
    oh_c = np.eye(10)[tr._c_logits.numpy().argmax(axis=1)]
    if data == 'cifar10':
        c_ref = S.c_phase(st, b64, r64['C'], HYPER, zca, labels=dict(unl=oh_c))
    else:
        c_ref = SG.c_phase(st, data, b64, r64['C'], HYPER, labels=dict(unl=oh_c))
    assert _check_net(stores['classifier'], st['last_grads']['C']) <= 1.0, _check_net.worst
    assert abs(tr.losses()[2] - c_ref) <= LOSS_TOL * max(1.0, abs(c_ref))
    # nothing of the penalty reached G or C: its gradient buffer is the discriminator's alone, and the D-update's terms stand
    assert tr._gp_grad.numel() == sd.n_p and tr.r1_terms() == terms


# ------------------------------------------------------------------------------------------------------------- execution modes
def _trainer(sizes, mode, seed, gamma=GAMMA, **over):
    tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=None, EXEC_MODE=mode, SEED=seed, **dict(dict(R1_GAMMA=gamma) if gamma else {}, **over)))
    tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
    return tr


def _run_modes(mode, iters, sizes, gamma2):
    tr = _trainer(sizes, mode, 3)
    full = dict(S.SIZES, **sizes)
    tr.feed(S.synth_batch(7, full))
    losses, terms = [], []
    for it in range(iters):
        if it == iters - 1 and gamma2 is not None:
            tr.set_r1_gamma(gamma2)
        tr.sample_latent()
        tr.train_iteration()
        losses.append(tr.losses())
        terms.append(tr.r1_terms())
    torch.cuda.synchronize()
    return dict(losses=losses, terms=terms, p={k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()})


def test_eager_overlap_plan_graph_are_bit_identical_and_follow_set_r1_gamma():
    """three PhiloxRNG iterations at the reference sizes 100 / 50 / 50 / 20 / 80, then a new gamma and a fourth: a gamma baked into a launch
    argument of a recorded plan or graph would leave the replayed modes on the old value."""
    runs = {m: _run_modes(m, 4, {}, 2.5) for m in ('eager', 'overlap', 'plan', 'graph')}
    ref = runs['eager']
    for m, r in runs.items():
        assert r['losses'] == ref['losses'], (m, r['losses'], ref['losses'])
        assert r['terms'] == ref['terms'], (m, r['terms'], ref['terms'])
        for k in ref['p']:
            assert r['p'][k].tobytes() == ref['p'][k].tobytes(), (m, k)
    t = ref['terms']
    assert all(v['penalty'] > 0 and np.isfinite(v['penalty']) for v in t) and all(np.isfinite(v) for l in ref['losses'] for v in l)
    for v in t[:3]:
        assert abs(v['penalty'] - 0.5 * GAMMA * v['grad_sq_mean']) <= 1e-6 * v['penalty']
    assert abs(t[3]['penalty'] - 0.5 * 2.5 * t[3]['grad_sq_mean']) <= 1e-6 * t[3]['penalty']       # the fourth iteration ran at the NEW gamma
    # and gamma matters: left at the old value the fourth iteration differs
    old = _run_modes('plan', 4, {}, None)
    assert old['losses'][:3] == ref['losses'][:3] and old['losses'][3][0] != ref['losses'][3][0]


def test_d_loss_is_the_gan_d_loss_plus_the_penalty():
    """the same weights, feed and injected draws through a GAN-loss trainer and an R1 trainer: the discriminator's forward pass sees the
    same masks in both (with the Philox RNG it would not — stream ids are handed out in order of first use, and the penalty draws first),
    so the R1 trainer's d_loss is the GAN trainer's plus r1_terms()['penalty'], to the bit: one fp32 add on the device."""
    from tg.runtime import InjectedRNG
    full = dict(S.SIZES, **SMALL)
    P, batch, rnd = S.init_params(0), S.synth_batch(8, full), S.synth_rnd(9, full)
    arrays = G.injected_arrays(rnd)
    arrays.update({'R1/' + k: v for k, v in R.r1_draws('cifar10', SMALL['L_D'] + SMALL['U_D'], 10).items()})
    out = {}
    for name, over in (('gan', {}), ('r1', dict(R1_GAMMA=GAMMA))):
        tr = G.fresh_trainer(G.make_config(SMALL, USE_HIP_GRAPH=False, EXEC_MODE='eager', **over), P)
        tr.cx.rng = InjectedRNG(arrays, tr.cx.device)
        tr.feed(batch)
        tr._d_forward_backward()
        out[name] = (tr.losses()[0], tr.r1_terms()['penalty'] if over else None)
    d_gan, pen = np.float32(out['gan'][0]), np.float32(out['r1'][1])
    assert np.float32(out['r1'][0]) == d_gan + pen and pen > 0 and d_gan > 0


def test_pre_train_iterations_run_no_penalty():
    tr = _trainer(SMALL, 'eager', 2)
    tr.feed(S.synth_batch(8, dict(S.SIZES, **SMALL)))
    tr.sample_latent()
    tr.train_iteration(pre_train=True)
    torch.cuda.synchronize()
    assert tr.r1_terms() == dict(penalty=0.0, grad_sq_mean=0.0) and tr._gp_grad is None and tr.losses()[0] == 0.0


def test_plan_iterations_are_isolated_from_a_standalone_penalty():
    """a standalone _r1_penalty (phase 'r1', its own buffers) at another n between two plan iterations changes nothing and regrows none of
    the step's buffers."""
    def run(interleave):
        tr = _trainer(SMALL, 'plan', 4)
        full = dict(S.SIZES, **SMALL)
        tr.feed(S.synth_batch(9, full))
        for it in range(5):
            tr.sample_latent()
            tr.train_iteration()
            if interleave and it == 2:
                m, cx = tr.model, tr.cx
                before = {k: (v.data_ptr(), v.numel()) for k, v in cx.buffers.items()}
                b = S.synth_batch(11, dict(S.SIZES, B_G=40, L_D=20, U_D=20))
                x = np.concatenate([b['x_l_d'], b['x_u_d']])
                y = np.eye(10, dtype=np.float32)[np.arange(40) % 10]
                pen = tr._r1_penalty(cx.from_numpy(x), cx.from_numpy(y), m.discriminator, 3.0)
                assert float(pen[0].item()) > 0
                after = {k: (v.data_ptr(), v.numel()) for k, v in cx.buffers.items()}
                assert all(after[k] == v for k, v in before.items()), "a buffer of the recorded step was regrown"
                assert any(k.startswith('r1') for k in set(after) - set(before))
        torch.cuda.synchronize()
        return tr.losses(), tr.r1_terms(), {k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}
    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1]
    for k in a[2]:
        assert a[2][k].tobytes() == b[2][k].tobytes(), k


def test_a_trainer_without_the_option_has_nothing_of_it():
    """R1_GAMMA = None: no device scalar, no buffer under an R1 call site, the same launches as ever; the controls refuse."""
    from tg import lib
    tr = _trainer(SMALL, 'eager', 4, gamma=None)
    tr.feed(S.synth_batch(9, dict(S.SIZES, **SMALL)))
    calls = []
    orig = lib.call
    lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        tr.sample_latent()
        tr.train_iteration()
    finally:
        lib.call = orig
    torch.cuda.synchronize()
    assert tr.r1_dev is None and tr._r1_out is None and tr._gp_grad is None
    assert 'tg_r1_penalty_f32' not in calls and len(calls) > 100
    assert not [k for k in tr.cx.buffers if 'gpgrad' in k or 'r1gamma' in k or k.startswith('r1') or '/gpp' in k]
    with pytest.raises(lib.TgError, match='R1_GAMMA = None'):
        tr.set_r1_gamma(1.0)
    with pytest.raises(lib.TgError, match='R1_GAMMA = None'):
        tr.r1_terms()
    on = _trainer(SMALL, 'eager', 4)
    on.feed(S.synth_batch(9, dict(S.SIZES, **SMALL)))
    on.sample_latent()
    on.train_iteration()
    assert [k for k in on.cx.buffers if 'gpgrad' in k] and on.r1_dev is not None
    for bad in (0.0, -1.0, float('nan'), float('inf'), True):
        with pytest.raises(lib.TgError, match='positive finite'):
            on.set_r1_gamma(bad)


# ------------------------------------------------------------------------------------------------------------- summaries
def _one_epoch(tmp_path, monkeypatch, gamma):
    """one epoch of the CIFAR-10 entry point with --r1-gamma `gamma` -> (the epoch's record, the trainer, history.csv lines, event bytes)."""
    from tg import runtime
    from Training import Train_goodGAN as TG
    runtime.set_context(None)
    kept = []

    init = TG.Train.__init__

    def keeping(self, *a, **kw):                       # (Train.__init__ names its class: wrap the method, do not replace the class)
        init(self, *a, **kw)
        kept.append(self)

    class Flags(object):
        train_size = 4000 + 300
        sample_dir = None
        seed = 1
        r1_gamma = gamma
    monkeypatch.setattr(TG, "_root_dir", lambda: str(tmp_path))
    monkeypatch.setattr(TG.Train, "__init__", keeping)
    hist = TG._main_training_cifar10(Flags(), epochs=1)
    assert len(hist) == 1 and len(kept) == 1
    csv = events = None
    for dirpath, _, files in os.walk(str(tmp_path)):
        for f in files:
            if os.sep + 'train' + os.sep in dirpath + os.sep:
                if f == 'history.csv':
                    csv = open(os.path.join(dirpath, f)).read().splitlines()
                elif f.startswith('events.out.tfevents'):
                    events = open(os.path.join(dirpath, f), 'rb').read()
    return hist[0], kept[0], csv, events


def test_summary_and_history_carry_d_r1_only_with_the_option(tmp_path, monkeypatch):
    """Train.train through an epoch tail: with R1_GAMMA the record, the train events and history.csv gain d_r1 = the last D-update's
    penalty (r1_terms()); without it the columns are exactly the ones there always were."""
    rec, tr, csv, events = _one_epoch(tmp_path / 'plain', monkeypatch, None)
    assert 'd_r1' not in rec and tr.r1_dev is None
    assert csv == ['step,g_loss,d_loss,c_loss', '%d,' % rec['epoch'] + ','.join('%.6g' % rec[k] for k in ('g_loss', 'd_loss', 'c_loss'))]
    assert b'd_r1' not in events and all(t in events for t in (b'g_loss', b'd_loss', b'c_loss'))
    rec, tr, csv, events = _one_epoch(tmp_path / 'r1', monkeypatch, GAMMA)
    pen = tr.r1_terms()['penalty']
    assert rec['d_r1'] == pen and pen > 0 and np.isfinite(pen)
    assert csv[0] == 'step,g_loss,d_loss,c_loss,d_r1' and len(csv) == 2
    assert csv[1] == '%d,' % rec['epoch'] + ','.join('%.6g' % rec[k] for k in ('g_loss', 'd_loss', 'c_loss', 'd_r1'))
    assert events.count(b'd_r1') == 1 and b'grad_norm' not in events


# ------------------------------------------------------------------------------------------------------------- checkpoint
def test_a_checkpoint_taken_with_r1_on_continues_bit_identically(tmp_path):
    from Training.Saver import Saver
    from test_gpu_resume import SIZES, _state
    feeds = [S.synth_batch(40 + i, dict(S.SIZES, **SIZES)) for i in range(4)]

    def run(tr, its):
        for i in its:
            tr.feed(feeds[i])
            tr.sample_latent()
            tr.train_iteration()
        torch.cuda.synchronize()

    a = G.fresh_trainer(G.make_config(SIZES, SEED=9, USE_HIP_GRAPH=True, R1_GAMMA=GAMMA))
    a.set_hyper(lambda_1=0.3, lambda_2=0.5)
    run(a, [0, 1])
    saver = Saver(str(tmp_path))
    saver.set_save_path(comments='resume test, R1')
    saver.save(a, 'model_0002.ckpt')
    run(a, [2, 3])
    want, want_losses, want_terms = _state(a), a.losses(), a.r1_terms()
    b = G.fresh_trainer(G.make_config(SIZES, SEED=1234, USE_HIP_GRAPH=True, R1_GAMMA=GAMMA))   # different seed: everything must come from the file
    b.set_hyper(lambda_1=0.3, lambda_2=0.5)
    assert Saver(str(tmp_path)).restore(b) == 2
    run(b, [2, 3])
    got = _state(b)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert b.losses() == want_losses and b.r1_terms() == want_terms and want_terms['penalty'] > 0


# ------------------------------------------------------------------------------------------------------------- data parallel
WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, os.path.join({root!r}, "tensorflow-implementation-of-triple-gan_amd"))
import torch
import gpu_common as G
from oracle import step_cifar10 as S
sizes = {sizes!r}
tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=None, EXEC_MODE='plan', SEED=5, R1_GAMMA={gamma!r}))
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
torch.save(dict(world=tr.world, rank=rank, sums=sums, losses=tr.losses(), terms=tr.r1_terms(), p0=p0,
                p={{k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}}), {out!r} % rank)
torch.distributed.destroy_process_group()
'''


def _one_process_average(sizes, p0, iters):
    """one process, no replicas: per solver run each shard's gradient (its own batch and Philox seed, as rank r draws them) is computed —
    the discriminator's with its penalty gradient added —, the two are summed as the all-reduce does and the optimiser steps with
    grad_scale 1/2."""
    tr = G.fresh_trainer(G.make_config(sizes, USE_HIP_GRAPH=False, EXEC_MODE='eager', SEED=5, R1_GAMMA=GAMMA))
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
    script.write_text(WORKER.format(root=ROOT, sizes=sizes, out=out, iters=iters, gamma=GAMMA))
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
    assert r[0]['losses'] != r[1]['losses'] and r[0]['terms'] != r[1]['terms']          # each rank's penalty is its own shard's
    ref = _one_process_average(sizes, r[0]['p0'], iters)
    for k in ref:
        assert np.abs(ref[k] - r[0]['p'][k]).max() == 0.0, (k, np.abs(ref[k] - r[0]['p'][k]).max())
