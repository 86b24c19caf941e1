"""The pre-training step on the GPU: Train.train_iteration(pre_train=True) — the C solver run alone, the whole trainer of the first 30
epochs of a run with config.PRE_TRAIN (Training/schedule.py; reference Training/Train_goodGAN.py:182-226).

  1. two phase-synchronised pre-training iterations through the public entry against the float64 oracle's c_phase (MNIST, SVHN f32 and
     bf16, CIFAR-10 with ZCA and the consistency pass), with what a pre-training step must NOT do pinned byte for byte;
  2. eager, overlap, plan and graph launches of it bit-identical, alone and handing over to the full step in the same trainer;
  3. one pre-training and one full iteration, free-running, against c_phase + train_step on one oracle state;
  4. a checkpoint written after pre-training, restored into a trainer that starts with a full iteration, continues bit-identically;
  5. Train.train() crosses epoch 30 / 31 after a restore.

Every tolerance is the one the full step is held to: the tables and helpers of tests/test_gpu_step.py (CIFAR-10) and
tests/test_gpu_goodgan.py (MNIST, SVHN) by import.  The batch seeds of part 1 and 3 were chosen on the CPU, with the oracle alone: the
classifier labels x_u_c for the discriminator by arg-max, and on every x_u_c row the float64 oracle's two largest logits are further
apart than the near-tie threshold of tests/test_gpu_goodgan.py (4 * ACT_TOL * max|logit|; for bf16 with and without the operand
rounding, at the bf16 ACT_TOL) — the tests assert that, so the HIP labels have to equal the oracle's outright."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from oracle import nets_goodgan as NG
from oracle import step_cifar10 as SC
from oracle import step_goodgan as SG
import gpu_common as G
import test_gpu_goodgan as TG
import test_gpu_step as TS
from test_gpu_goodgan import oracle_prec                                  # noqa: F401  (fixture)
from test_gpu_resume import SIZES as CIFAR_SMALL, _state
from test_oracle_goodgan import scrambled

pytestmark = pytest.mark.gpu
SMALL = TG.SMALL
NETS = TS.NETS
SEED = 5
# (data, prec) -> the batch seeds of two consecutive iterations (the draws' seed is the batch's + 100); see the module docstring
SEEDS = {('mnist', 'f32'): (31, 32), ('svhn', 'f32'): (32, 33), ('svhn', 'bf16'): (36, 68), ('cifar10', 'f32'): (31, 32)}
FULL_SEED = 42                                                            # part 3: the full iteration behind mnist's 31

f64 = TS.f64


class _Case(object):
    """one data set's oracle, trainer and inputs behind one interface: the CIFAR-10 oracle takes the ZCA constants, the MNIST / SVHN one
    the data set's name."""

    def __init__(self, data, prec='f32'):
        self.data, self.prec = data, prec
        if data == 'cifar10':
            P = SC.init_params(0)
            self.st = SC.new_state(f64(P))
            self.tr = G.fresh_trainer(G.make_config(CIFAR_SMALL), P)
            self.zca = tuple(np.asarray(a, np.float64) for a in G.zca())
            self.full = dict(SC.SIZES, **CIFAR_SMALL)
            lambda_2 = 0.5
        else:
            P32 = {k: v.astype(np.float32) for k, v in scrambled(data, 11).items()}
            self.st = SG.new_state(f64(P32))
            self.tr = TG.trainer(data, f64(P32), prec=prec)
            lambda_2 = 0.0
        c = self.tr.config                       # the experiment's own rates; lambda_1 as from epoch 200 on, so that C_fake's rows count
        self.hyper = dict(lr=c.LEARNING_RATE, cla_lr=c.CLA_LEARNINIG_RATE, beta1=c.BETA1, lambda_1=c.FAKE_G_LAMBDA, lambda_2=lambda_2)
        self.tr.set_hyper(self.hyper['lr'], self.hyper['cla_lr'], self.hyper['lambda_1'], lambda_2)
        self.act_tol = TG.TOL[prec]['act']

    def inputs(self, seed):
        """(batch, draws, the draws as the InjectedRNG wants them)."""
        if self.data == 'cifar10':
            batch, rnd = SC.synth_batch(seed, self.full), SC.synth_rnd(seed + 100, self.full)
            return batch, rnd, G.injected_arrays(rnd)
        batch, rnd = SG.synth_batch(self.data, seed, SMALL), SG.synth_rnd(self.data, seed + 100, SMALL)
        return batch, rnd, G.injected_arrays_goodgan(rnd)

    def c_phase(self, st, b64, r64, labels=None):
        if self.data == 'cifar10':
            return SC.c_phase(st, b64, r64['C'], self.hyper, self.zca, labels=labels)
        return SG.c_phase(st, self.data, b64, r64['C'], self.hyper, labels=labels)

    def train_step(self, st, b64, r64):
        if self.data == 'cifar10':
            return SC.train_step(st, b64, r64, self.hyper, self.zca)
        return SG.train_step(st, self.data, b64, r64, self.hyper)

    def gaps(self, logits):
        """(top-2 gap of every row, the near-tie threshold) of oracle logits."""
        top2 = np.sort(logits, axis=1)[:, -2:]
        return top2[:, 1] - top2[:, 0], 4 * self.act_tol * np.abs(logits).max()

    def moving_close(self, got, ref):
        """a generator moving statistic at the tolerance the full step's are held to."""
        return TS.moving_stat_close(got, ref) if self.data == 'cifar10' else G.rel_err(got, ref) < TG.TOL[self.prec]['stat']


def _frozen_bytes(stores):
    return {(net, buf): getattr(stores[net], buf).detach().cpu().numpy().tobytes()
            for net in ('discriminator', 'good_generator') for buf in ('p', 'm', 'v', 'g', 'step')}


def _figures(case, st, tr, before, c_ref):
    """the errors of one iteration in the units of the tolerances they are asserted at below (a report: nothing is asserted here)."""
    cs, lr = tr.cx.stores['classifier'], case.hyper['cla_lr']
    out = dict(loss_rel=abs(tr.losses()[2] - c_ref) / max(1.0, abs(c_ref)), grad_max_rel=0.0, grad_l2_rel=0.0, adam_max_over_lr=0.0,
               adam_mean_over_lr=0.0, ema_max_over_lr=0.0, stat_rel=0.0, g_moving_rel=0.0)
    gref = st['last_grads']['C']
    floor = TG.check_grads.__defaults__[0] * max(np.abs(v).max() for v in gref.values())
    for k, ref in gref.items():
        if case.data == 'cifar10':
            if np.abs(ref).max() < floor:        # analytically zero: under the absolute floor of test_gpu_step.check_grads
                continue
            sc = n2 = None
        elif case.prec == 'bf16' and k in TG.ANALYTIC_ZERO:
            continue
        else:                                    # the scales of test_gpu_goodgan.check_grads
            sc = max(np.abs(ref).max(), floor)
            n2 = max(np.linalg.norm(ref), sc)
        d = cs.get(k, 'grad') - ref
        out['grad_max_rel'] = max(out['grad_max_rel'], np.abs(d).max() / (sc or np.abs(ref).max()))
        out['grad_l2_rel'] = max(out['grad_l2_rel'], np.linalg.norm(d) / (n2 or np.linalg.norm(ref)))
    for k in cs.names(True):
        err = np.abs(cs.get(k) - st['P'][k])
        out['adam_max_over_lr'] = max(out['adam_max_over_lr'], err.max() / lr)
        out['adam_mean_over_lr'] = max(out['adam_mean_over_lr'], err.mean() / lr)
        out['ema_max_over_lr'] = max(out['ema_max_over_lr'], np.abs(cs.get(k, 'ema') - st['ema'][k]).max() / lr)
    for k in cs.names(False):
        out['stat_rel'] = max(out['stat_rel'], G.rel_err(cs.get(k), st['P'][k]))
    gs = tr.cx.stores['good_generator']
    for k in gs.names(False):
        out['g_moving_rel'] = max(out['g_moving_rel'], G.rel_err(gs.get(k), st['P'][k]))
    return {k: float(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------- 1. oracle parity
@pytest.mark.parametrize("data,prec", sorted(SEEDS))
def test_pre_training_iterations_match_the_oracles_c_phase(data, prec, oracle_prec):
    """two consecutive pre-training iterations on two batches, each checked from identical weights: gradients, loss, Adam step, EMA,
    running statistics against c_phase; the discriminator's and the generator's p / m / v / g / step byte for byte what they were (g: the
    zeros it was allocated with — a pre-training step writes no gradient of theirs); the generator's moving statistics advanced ONCE."""
    from tg.runtime import InjectedRNG
    oracle_prec(prec)
    case = _Case(data, prec)
    st, tr, hyper, tol = case.st, case.tr, case.hyper, TG.TOL[prec]
    cx, stores = tr.cx, tr.cx.stores
    cs, gs = stores['classifier'], stores['good_generator']
    thrice = (1 - NG.BN_DECAY ** 3) / (1 - NG.BN_DECAY)      # three moving-statistics updates on one batch, in units of one
    figures = {}
    for it, seed in enumerate(SEEDS[data, prec]):
        batch, rnd, arrays = case.inputs(seed)
        b64, r64 = f64(batch), f64(rnd)
        cx.rng = InjectedRNG(arrays, cx.device)
        tr.feed(batch)
        before = {k: v.copy() for k, v in st['P'].items()}
        frozen = _frozen_bytes(stores)
        st0 = copy.deepcopy(st)
        c_ref = case.c_phase(st, b64, r64)
        tr.train_iteration(pre_train=True, use_graph=False)
        # ---- the labels of D(x_u_c, argmax C_unl)
        ref_logits, hip_logits = st['last_logits']['unl'], tr._c_logits.numpy()
        gap, near = case.gaps(ref_logits)
        mism = np.where(hip_logits.argmax(1) != ref_logits.argmax(1))[0]
        if prec == 'f32':
            assert (gap > near).all(), ('the batch seed was chosen for clear labels', it, gap, near)
            assert len(mism) == 0, ('labels', it, mism)
        else:
            assert (gap[mism] <= near).all(), ('labels differ where the oracle has no near-tie', it, mism, gap, near)
            assert len(mism) <= 1, (it, mism)
            if len(mism):
                st = copy.deepcopy(st0)
                c_ref = case.c_phase(st, b64, r64, labels=dict(unl=np.eye(ref_logits.shape[1])[hip_logits.argmax(1)]))
        figures['it%d' % it] = _figures(case, st, tr, before, c_ref)
        print('pretrain_parity_%s_%s' % (data, prec), json.dumps(figures))              # (shown with pytest -s)
        # ---- gradients and loss
        got = tr.losses()
        if data == 'cifar10':
            TS.check_grads(st, tr, 'C')
            assert abs(got[2] - c_ref) <= TS.LOSS_TOL * max(1.0, abs(c_ref)), (it, got, c_ref)
        else:
            TG.check_grads(cs, st['last_grads']['C'], tol=tol)
            assert abs(got[2] - c_ref) <= tol['loss'] * max(1.0, abs(c_ref)), (it, got, c_ref)
        # ---- running state, EMA, the Adam step; the oracle's state goes in for the next iteration
        if data != 'cifar10':
            for k in cs.names(False):
                assert G.rel_err(cs.get(k), st['P'][k]) < tol['stat'], (it, k)
                cs.set(k, st['P'][k])
        TS.check_ema_and_sync(st, tr, hyper['cla_lr'])
        # (MNIST / SVHN: Adam's envelope alone, see check_update_and_sync — measured on one MI355X, worst variable's mean error over lr:
        # mnist 0.16 on c_h0_conv0's bias, 4 of whose 32 oracle gradients are 0; svhn f32 0.33 on c_h2_bn2/beta, analytically 0; svhn
        # bf16 0.61; CIFAR-10, held to the mean bound as well, 0.007)
        TS.check_update_and_sync(st, tr, 'C', before, hyper['cla_lr'], mean=data == 'cifar10')
        if data == 'cifar10':
            TS.sync_pop_means(st, tr)
        for k in gs.names(False):
            ref, was = st['P'][k], before[k]
            assert case.moving_close(gs.get(k), ref), (it, k, np.abs(gs.get(k) - ref).max())
            assert not case.moving_close(was, ref), (it, k)                                # they did move,
            assert not case.moving_close(was + thrice * (ref - was), ref), (it, k)         # and a full step's three updates would not pass
            gs.set(k, ref)
        # ---- what must not have happened
        for key, was in frozen.items():
            assert _frozen_bytes(stores)[key] == was, (it, key)
        for net in ('discriminator', 'good_generator'):
            assert not torch.count_nonzero(stores[net].g).item() and not torch.count_nonzero(stores[net].m).item(), net
        assert [int(stores[NETS[k]].step.item()) for k in 'DGC'] == [0, 0, it + 1] == [st['t'][k] for k in 'DGC']
        assert got[0] == 0.0 and got[1] == 0.0
        assert tr._g_saved is None


# ------------------------------------------------------------------------------------------------------------- 2. replay modes
MODES = ('eager', 'overlap', 'plan', 'graph')


def _philox_config(data, **over):
    return G.make_config(CIFAR_SMALL, **over) if data == 'cifar10' else G.make_config_goodgan(data, SMALL, **over)


def _philox_trainer(data, **over):
    """a trainer on the Philox RNG with the model's own initial weights, lambda_1 as from epoch 200 on (and CIFAR-10's lambda_2 as from
    epoch 68 on): every term of c_loss counts."""
    c = _philox_config(data, **over)
    if data == 'cifar10':
        tr = G.fresh_trainer(c)
        tr.set_hyper(lambda_1=c.FAKE_G_LAMBDA, lambda_2=0.5)
    else:
        from Model.Good_GAN import Good_GAN
        tr = G.fresh_trainer(c, None, Good_GAN)
        tr.set_hyper(lambda_1=c.FAKE_G_LAMBDA)
    return tr


def _feeds(data, n):
    if data == 'cifar10':
        return [SC.synth_batch(40 + i, dict(SC.SIZES, **CIFAR_SMALL)) for i in range(n)]
    return [SG.synth_batch(data, 40 + i, SMALL) for i in range(n)]


def _recorded(tr):
    """{key: (the graph handles, the launch plans)} of the executor, as lists of their own."""
    return {key: (list(r.graphs), list(r.plans)) for key, r in tr.executor.replay.items()}


def _run_mode(data, mode, schedule, feeds, cla_lr_at=None):
    """one fresh trainer through `schedule` (pre_train of every iteration) -> per iteration (losses, every store buffer, what is recorded).
    cla_lr_at: (iteration, rate) — set_hyper in front of that iteration."""
    tr = _philox_trainer(data, USE_HIP_GRAPH=None, EXEC_MODE=mode, SEED=SEED)
    out = []
    for i, pre in enumerate(schedule):
        if cla_lr_at is not None and cla_lr_at[0] == i:
            tr.set_hyper(cla_lr=cla_lr_at[1])
        tr.feed(feeds[i])
        tr.sample_latent()
        tr.train_iteration(pre_train=pre)
        torch.cuda.synchronize()
        out.append((tr.losses(), _state(tr), _recorded(tr)))
    return out


def _assert_same_run(mode, run, ref):
    for i, ((losses, state, _), (ref_losses, ref_state, _)) in enumerate(zip(run, ref)):
        assert all(np.isfinite(ref_losses)), (i, ref_losses)
        assert losses == ref_losses, (mode, i, losses, ref_losses)
        assert set(state) == set(ref_state)
        for k in ref_state:
            assert state[k].tobytes() == ref_state[k].tobytes(), (mode, i, k)


def _all_set(handles):
    return len(handles) > 0 and all(h is not None for h in handles)


def _none_set(handles):
    return all(h is None for h in handles)


@pytest.mark.parametrize("data", ['cifar10', 'mnist'])
def test_pre_training_is_bit_identical_in_every_launch_mode_and_follows_set_hyper(data):
    """four pre-training iterations per mode, a new cla_lr in front of the fourth: a rate baked into a recorded launch would leave the
    replayed modes on the old one.  Plans are recorded and graphs captured in the second iteration, under the key 'pre' alone."""
    feeds = _feeds(data, 4)
    new_lr = 0.5 * _philox_config(data).CLA_LEARNINIG_RATE
    runs = {m: _run_mode(data, m, [True] * 4, feeds, cla_lr_at=(3, new_lr)) for m in MODES}
    for m in MODES:
        _assert_same_run(m, runs[m], runs['eager'])
        which = {'graph': 0, 'plan': 1}.get(m)
        for i, (_, state, rec) in enumerate(runs[m]):
            assert rec['full'] == ([], []), (m, i)
            for kind in (0, 1):
                if kind == which and i >= 1:
                    assert _all_set(rec['pre'][kind]), (m, i, kind)
                else:
                    assert _none_set(rec['pre'][kind]), (m, i, kind)
            assert [int(state[net + '/step'][0]) for net in (NETS[k] for k in 'DGC')] == [0, 0, i + 1]
    # and the rate matters: left at the old value, the fourth iteration ends elsewhere (c_loss is taken in front of the step: the same)
    old = _run_mode(data, 'plan', [True] * 4, feeds)
    _assert_same_run('plan, old rate', old[:3], runs['eager'][:3])
    assert old[3][0] == runs['eager'][3][0]
    assert old[3][1]['classifier/p'].tobytes() != runs['eager'][3][1]['classifier/p'].tobytes()
    assert old[3][1]['classifier/v'].tobytes() == runs['eager'][3][1]['classifier/v'].tobytes()      # same gradients, another rate


@pytest.mark.parametrize("data", ['cifar10', 'mnist'])
def test_the_full_step_takes_over_from_pre_training_in_every_launch_mode(data):
    """three pre-training iterations, then three full ones in the same trainer: the full step shares every phase-'C' call-site buffer with
    the pre-training step but records its own plans / captures its own graphs, at ITS second iteration, and leaves those of 'pre' alone."""
    feeds = _feeds(data, 6)
    schedule = [True] * 3 + [False] * 3
    runs = {m: _run_mode(data, m, schedule, feeds) for m in MODES}
    for m in MODES:
        _assert_same_run(m, runs[m], runs['eager'])
        which = {'graph': 0, 'plan': 1}.get(m)
        pre_kept = runs[m][2][2]['pre']
        for i, (_, state, rec) in enumerate(runs[m]):
            for kind in (0, 1):
                if kind != which:
                    assert _none_set(rec['pre'][kind]) and _none_set(rec['full'][kind]), (m, i, kind)
                    continue
                assert _all_set(rec['pre'][kind]) == (i >= 1), (m, i)
                assert _all_set(rec['full'][kind]) == (i >= 4) and (i >= 4 or _none_set(rec['full'][kind])), (m, i)
                if i >= 3:                       # the very handles pre-training left behind
                    assert len(rec['pre'][kind]) == len(pre_kept[kind]) and all(a is b for a, b in zip(rec['pre'][kind], pre_kept[kind])), (m, i)
            assert [int(state[net + '/step'][0]) for net in (NETS[k] for k in 'DGC')] == [max(0, i - 2), max(0, i - 2), i + 1]
    assert len(runs['graph'][5][2]['full'][0]) > len(runs['graph'][5][2]['pre'][0])                   # D, G and C segments against C's


# ------------------------------------------------------------------------------------------------------------- 3. hand-over against the oracle
def test_pre_training_then_a_full_iteration_track_the_oracle_free_running():
    """mnist, f32: one pre-training iteration, then one full iteration in the same trainer, nothing synchronised in between, against
    c_phase + train_step on one oracle state at the bounds of test_gpu_step.test_free_running_three_iterations.  What the pre-training
    step could leak into the full one — a kept generator tape, a stale filter layout, a moving-statistics update too many or too few —
    shows here: the generator's moving statistics have had 1 + 3 updates on both sides.  (They are held to the `stat` tolerance of the
    synchronised step: only the last of the four updates sees generator weights that differ between the two free trajectories, by at
    most 2.2 * lr in single elements, and it weighs 0.1.)"""
    from tg.runtime import InjectedRNG
    case = _Case('mnist')
    st, tr = case.st, case.tr
    p0 = {k: v.copy() for k, v in st['P'].items()}
    for it, (seed, pre) in enumerate(((SEEDS['mnist', 'f32'][0], True), (FULL_SEED, False))):
        batch, rnd, arrays = case.inputs(seed)
        b64, r64 = f64(batch), f64(rnd)
        tr.cx.rng = InjectedRNG(arrays, tr.cx.device)
        tr.feed(batch)
        if pre:
            ref = (0.0, 0.0, case.c_phase(st, b64, r64))
            logits = [st['last_logits']['unl']]
        else:
            st_d = copy.deepcopy(st)             # (the D-update's label logits, which train_step's C-update overwrites)
            SG.d_phase(st_d, 'mnist', b64, r64['D'], case.hyper)
            ref = case.train_step(st, b64, r64)
            logits = list(st_d['last_logits'].values()) + [st['last_logits']['unl']]
        for lg in logits:
            gap, near = case.gaps(lg)
            assert (gap > near).all(), ('the batch seed was chosen for clear labels', it, gap, near)
        tr.train_iteration(pre_train=pre, use_graph=False)
        got = tr.losses()
        print('free-running', it, 'oracle', ref, 'hip', got)
        TS.check_free_running_losses(ref, got, it)
        assert tr._g_saved is None
    TS.check_free_running_envelope(st, tr, case.hyper, dict(D=1, G=1, C=2), p0)
    assert [int(tr.cx.stores[NETS[k]].step.item()) for k in 'DGC'] == [1, 1, 2] == [st['t'][k] for k in 'DGC']
    gs = tr.cx.stores['good_generator']
    for k in gs.names(False):
        err = G.rel_err(gs.get(k), st['P'][k])
        print('free-running moving statistic', k, err)
        assert err < TG.TOL['f32']['stat'], (k, err)


# ------------------------------------------------------------------------------------------------------------- 4. resume across the boundary
@pytest.mark.parametrize("data", ['cifar10', 'mnist'])
def test_resume_behind_pre_training_continues_bit_identically(tmp_path, data):
    """a: two pre-training iterations, save, two full iterations.  b: another seed, restore, the same two full iterations.  PhiloxRNG
    numbers a stream when it is first used — a: latent, C/C, C/D, D/C, D/D, G/D; a process that starts with a full iteration: latent,
    D/C, D/D, G/D, C/C, C/D — so the checkpoint has to carry the numbering (tg/rng_streams) for b to draw what a drew."""
    from Training.Saver import Saver
    feeds = _feeds(data, 4)
    fresh = lambda seed: _philox_trainer(data, USE_HIP_GRAPH=True, SEED=seed)

    def run(tr, its, pre):
        for i in its:
            tr.feed(feeds[i])
            tr.sample_latent()
            tr.train_iteration(pre_train=pre)
        torch.cuda.synchronize()

    a = fresh(9)
    run(a, [0, 1], True)
    saver = Saver(str(tmp_path))
    saver.set_save_path(comments='resume behind pre-training')
    path = saver.save(a, 'model_0030.ckpt')
    streams_a = dict(a.cx.rng.stream_ids)
    run(a, [2, 3], False)
    want, want_losses = _state(a), a.losses()

    b = fresh(1234)                               # different seed: everything must come from the file
    assert Saver(str(tmp_path)).restore(b) == 30
    streams_b = dict(b.cx.rng.stream_ids)
    run(b, [2, 3], False)
    got = _state(b)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert b.losses() == want_losses and all(np.isfinite(want_losses))
    # how: the table as a plain string array, names in the order of their ids, and b numbered its streams by it
    assert streams_b == streams_a and b.cx.rng.stream_ids == a.cx.rng.stream_ids
    with np.load(path) as z:
        names = z['tg/rng_streams']
    assert names.dtype.kind == 'U' and [str(n) for n in names] == sorted(streams_a, key=streams_a.get)
    assert names[0].startswith('latent/') and all(n.split('/')[0] in ('latent', 'C') for n in names)


def test_a_checkpoint_without_the_stream_table_restores_as_before(tmp_path):
    """a file written before tg/rng_streams existed: everything else is restored, the numbering is left to the order of use."""
    from Training.Saver import Saver, load_state_dict
    a = _philox_trainer('mnist', USE_HIP_GRAPH=False, EXEC_MODE='eager', SEED=9)
    a.feed(_feeds('mnist', 1)[0])
    a.sample_latent()
    a.train_iteration(pre_train=True)
    saver = Saver(str(tmp_path))
    saver.set_save_path(comments='old file')
    d = dict(np.load(saver.save(a, 'model_0001.ckpt')))
    assert len(d.pop('tg/rng_streams')) == len(a.cx.rng.stream_ids) > 2
    b = _philox_trainer('mnist', USE_HIP_GRAPH=False, EXEC_MODE='eager', SEED=1234)
    assert load_state_dict(b.cx.stores, d, b.cx.rng) == []
    assert b.cx.rng.stream_ids == {} and torch.equal(b.cx.rng.state, a.cx.rng.state)
    want = _state(a)
    for k, v in _state(b).items():
        np.testing.assert_array_equal(v, want[k], err_msg=k)


# ------------------------------------------------------------------------------------------------------------- 5. train() crosses the boundary
def test_train_crosses_from_pre_training_to_the_full_step(tmp_path):
    """mnist, PRE_TRAIN: a checkpoint that restores as start_epoch = 29, then two epochs of three iterations — epoch 30 pre-trains, epoch 31
    trains fully.  The first epoch's training_statistics() runs the whole forward graph on a discriminator that has never been trained."""
    from tg import runtime
    from Training.Saver import Saver
    from Training.Train_goodGAN import Train
    from Model.Good_GAN import Good_GAN
    from Input_Pipeline.syntheticDataset import syntheticDataset
    save = str(tmp_path / 'Weight')
    os.makedirs(save)
    kw = dict(TRAIN_SIZE=3 * SMALL['B_G'], PRE_TRAIN=True, USE_HIP_GRAPH=True, SAVE_PER_EPOCH=1, SAMPLE_SIZE=16, SEED=SEED)
    first = G.fresh_trainer(G.make_config_goodgan('mnist', SMALL, **kw), None, Good_GAN)
    saver = Saver(save)
    saver.set_save_path(comments='epoch 29')
    saver.save(first, 'model_0029.ckpt')

    runtime.set_context(None)
    torch.cuda.empty_cache()
    tr = Train(G.make_config_goodgan('mnist', SMALL, RESTORE=True, EPOCHS=2, **kw), None, save, comments='crossing')
    steps = lambda: [int(tr.cx.stores[NETS[k]].step.item()) for k in 'DGC']
    seen, stats = [], tr.training_statistics
    tr.training_statistics = lambda: (seen.append(steps()), stats())[1]
    history = tr.train(syntheticDataset, Good_GAN, None)
    assert [h['epoch'] for h in history] == [30, 31]
    assert seen == [[0, 0, 3], [3, 3, 6]]                                 # epoch 30 ran the C solver alone, and its statistics pass an untrained D
    assert steps() == [3, 3, 6]
    for h in history:
        assert all(np.isfinite(h[k]) for k in ('d_loss', 'g_loss', 'c_loss', 'val_accuracy')), h
    assert all(tr.executor.replay[key].ran for key in ('pre', 'full'))
    run_dir = os.path.join(save, os.listdir(save)[0])
    assert sorted(f for f in os.listdir(run_dir) if f.startswith('model')) == ['model_%04d.ckpt.npz' % e for e in (29, 30, 31)]
