"""config.WN_INIT = 'data' in the trainer: Train.data_dependent_init on the CIFAR-10, SVHN and MNIST configurations at
the sizes of tests/test_gpu_dp.py, against the float64 whole-pass restatement (tests/wn_init_reference.py) with the trainer's own
parameters, batch and latents.

Tolerance of g and b: TOL = 2e-4 of the largest element — the forward-parity tolerance these networks are already held to against
float64 (tests/test_gpu_goodgan.py TOL['f32']['act'] = 2e-4, tests/test_gpu_nets.py ACT_TOL = 1e-4): g = init_scale / sqrt(var t)
carries half the relative error of var t, i.e. the relative error of the fp32 forward pass that produced t, and every layer hands on
an activation normalised to the same scale, so nothing amplifies.  b = -m g is compared on the scale of the terms it balances,
max|b| + init_scale (the output's standard deviation): a batch mean near zero leaves b itself near zero.  The labels the
discriminator's init sees are an arg-max of near-tied logits at initialisation, so the reference takes them from the run
(model.wn_init_labels), as Train.label_override does for the step tests."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import gpu_common as G
import wn_init_reference as R
from oracle import nets_goodgan as NG
from oracle import step_cifar10 as S
from oracle import step_goodgan as SG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
TOL = 2e-4
DATA = ['cifar10', 'svhn', 'mnist']
# the layer lists of DESIGN §9.9
COUNTS = {'cifar10': dict(good_generator=0, classifier=10, discriminator=0),
          'svhn': dict(good_generator=1, classifier=2, discriminator=7),
          'mnist': dict(good_generator=1, classifier=0, discriminator=6)}


def _params(data):
    return S.init_params(0) if data == 'cifar10' else {k: v.astype(np.float32) for k, v in NG.init_params(data, 0).items()}


def _batch(data, seed):
    return S.synth_batch(seed, dict(S.SIZES, **SIZES)) if data == 'cifar10' else SG.synth_batch(data, seed, SIZES)


def _trainer(data, seed=5, **over):
    if data == 'cifar10':
        return G.fresh_trainer(G.make_config(SIZES, SEED=seed, **over), _params(data))
    from Model.Good_GAN import Good_GAN
    return G.fresh_trainer(G.make_config_goodgan(data, SIZES, SEED=seed, **over), _params(data), Good_GAN)


def _state(tr):
    import torch
    torch.cuda.synchronize()
    out = {'rng': tr.cx.rng.state.cpu().numpy().copy()}
    for net, st in tr.cx.stores.items():
        for buf in ('p', 'g', 'm', 'v', 's', 'step'):
            out[net + '/' + buf] = getattr(st, buf).detach().cpu().numpy().copy()
        if st.ema is not None:
            out[net + '/ema'] = st.ema.detach().cpu().numpy().copy()
        for nm in st.names():
            out['var:' + nm] = st.get(nm).copy()
    return out


def _init(tr, data, seed=21):
    tr.feed(_batch(data, seed))
    tr.sample_latent()
    before = _state(tr)
    counts = tr.data_dependent_init()
    return before, counts, _state(tr)


def _reference(tr, data, seed=21):
    b = dict(_batch(data, seed), z_g=tr.z_g_ph.numpy(), y_g=tr.y_g_ph.numpy())
    if data == 'cifar10':
        new, _ = R.init_pass_cifar10(_params(data), b['x_u_c'], G.zca())
        return new
    labels = tr.model.wn_init_labels.numpy()
    assert labels.shape == (SIZES['U_D'], 10) and (labels.sum(axis=1) == 1).all() and set(np.unique(labels)) <= {0.0, 1.0}
    new, recs, _ = R.init_pass_goodgan(_params(data), data, b, labels)
    return new


@pytest.mark.parametrize("data", DATA)
def test_init_matches_float64_and_changes_nothing_else(data):
    from tg import lib
    tr = _trainer(data)
    before, counts, after = _init(tr, data)
    assert counts == COUNTS[data] == tr.wn_initialised
    assert {net: len(v) for net, v in tr.model.WN_INIT_LAYERS.items()} == COUNTS[data]
    new = _reference(tr, data)
    assert len(new) == 2 * sum(COUNTS[data].values())
    scale = {k[:-2]: R.INIT_SCALE.get(k[:-2], 1.0) for k in new}
    for k, ref in new.items():
        got = after['var:' + k]
        if k.endswith('/g'):
            assert np.abs(got - ref).max() <= TOL * np.abs(ref).max(), (k, np.abs(got - ref).max(), np.abs(ref).max())
        else:
            sc = np.abs(ref).max() + scale[k[:-2]]
            assert np.abs(got - ref).max() <= TOL * sc, (k, np.abs(got - ref).max(), sc)
        assert not np.array_equal(got, before['var:' + k]), k                          # it was assigned
    # only */g and */b of the weight-norm layers changed: every other variable, every running statistic, the gradients, the optimiser
    # slots and steps and the Philox state are bit-identical; the EMA shadows are the weights
    for k in before:
        if k.startswith('var:') and k[4:] in new:
            continue
        if k.endswith('/p') or k.endswith('/ema'):
            continue
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    np.testing.assert_array_equal(after['classifier/ema'], after['classifier/p'])
    # a second fresh trainer: bit-identical
    tr2 = _trainer(data)
    _, counts2, after2 = _init(tr2, data)
    assert counts2 == counts
    for k in after:
        np.testing.assert_array_equal(after2[k], after[k], err_msg=k)
    # refused once an iteration has run
    tr2.train_iteration()
    with pytest.raises(lib.TgError, match="iteration"):
        tr2.data_dependent_init()


def test_iterations_after_the_init_agree_across_launch_modes():
    """eager launches, the recorded launch plan and the replayed hipGraph compute bit-identical weights from the initialised state
    (three iterations: the plan replays and the graph is launched from the third / second on)."""
    import torch
    feeds = [_batch('cifar10', 60 + i) for i in range(3)]
    results = {}
    for mode in ('eager', 'plan', 'graph'):
        tr = _trainer('cifar10', seed=9, EXEC_MODE=mode, USE_HIP_GRAPH=None)
        tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
        per_iter = []
        for i, f in enumerate(feeds):
            tr.feed(f)
            tr.sample_latent()
            if i == 0:
                assert tr.data_dependent_init()['classifier'] == 10
            tr.train_iteration()
            torch.cuda.synchronize()
            per_iter.append({net: st.p.cpu().numpy().copy() for net, st in tr.cx.stores.items()})
        results[mode] = per_iter
    for mode in ('plan', 'graph'):
        for i in range(3):
            for net in results['eager'][i]:
                np.testing.assert_array_equal(results[mode][i][net], results['eager'][i][net], err_msg="%s iteration %d %s" % (mode, i + 1, net))


def test_resume_continues_bit_identically_without_reinitialising(tmp_path):
    """tests/test_gpu_resume.py's protocol on an initialised run: the checkpoint (contents unchanged) carries the assigned g and b."""
    import torch
    from Training.Saver import Saver
    feeds = [_batch('svhn', 40 + i) for i in range(4)]

    def run(tr, its):
        for i in its:
            tr.feed(feeds[i])
            tr.sample_latent()
            if i == 0:
                tr.data_dependent_init()
            tr.train_iteration()
        torch.cuda.synchronize()

    a = _trainer('svhn', seed=9)
    run(a, [0, 1])
    os.makedirs(str(tmp_path / 'a'))
    saver = Saver(str(tmp_path / 'a'))
    saver.set_save_path(comments='wn init resume')
    keys = set(np.load(saver.save(a, 'model_0002.ckpt')).files)
    run(a, [2, 3])
    want = _state(a)
    b = _trainer('svhn', seed=1234)                                                    # different seed: everything must come from the file
    os.makedirs(str(tmp_path / 'plain'))
    plain = Saver(str(tmp_path / 'plain'))
    plain.set_save_path(comments='no init')
    assert set(np.load(plain.save(b, 'model_0001.ckpt')).files) == keys                # the same variables with or without the init
    assert Saver(str(tmp_path / 'a')).restore(b) == 2
    run(b, [2, 3])
    assert b.wn_initialised is None
    got = _state(b)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_train_initialises_once_and_never_after_a_restore(tmp_path):
    import torch
    from tg import runtime
    from Training.Train_goodGAN import Train
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10
    from Input_Pipeline.syntheticDataset import syntheticDataset
    save, log = str(tmp_path / 'Weight'), str(tmp_path / 'Log')
    os.makedirs(save)
    kw = dict(TRAIN_SIZE=8 * 2, EPOCHS=1, SAMPLE_DIR=None, SAMPLE_SIZE=16, SUMMARY=False, SAVE_PER_EPOCH=1, NUM_LABEL=40, WN_INIT='data')
    calls = []

    def fresh(**over):
        runtime.set_context(None)
        torch.cuda.empty_cache()
        tr = Train(G.make_config(SIZES, **dict(kw, **over)), log, save, comments='wn')
        inner = tr.data_dependent_init
        tr.data_dependent_init = lambda: calls.append(tr.iteration) or inner()
        return tr

    tr = fresh()
    assert tr.options.wn_init == 'data'
    tr.train(syntheticDataset, Good_GAN_cifar10, None)
    assert calls == [0] and tr.iteration == 2                                         # once, on the first batch, which was iteration 1 too
    assert tr.wn_initialised == COUNTS['cifar10']
    g = tr.cx.stores['classifier'].get('classifier/conv1_1/g')
    assert not (g == 1.0).all()
    tr2 = fresh(RESTORE=True)
    tr2.train(syntheticDataset, Good_GAN_cifar10, None)
    assert calls == [0] and tr2.wn_initialised is None and tr2.iteration == 2          # a restored run never re-initialises
    tr3 = fresh(WN_INIT=None)
    del calls[:]
    tr3.train(syntheticDataset, Good_GAN_cifar10, None)
    assert calls == [] and tr3.wn_initialised is None


WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, os.path.join({root!r}, "tensorflow-implementation-of-triple-gan_amd"))
import torch
import test_gpu_wn_init_step as W
tr = W._trainer('svhn', seed=5)
rank = tr.rank
tr.feed(W._batch('svhn', 500 + 1000 * rank))
tr.sample_latent()
counts = tr.data_dependent_init()
torch.cuda.synchronize()
out = dict(world=tr.world, rank=rank, counts=counts, p={{k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}},
           s={{k: st.s.cpu().numpy() for k, st in tr.cx.stores.items()}}, ema=tr.cx.stores['classifier'].ema.cpu().numpy())
tr.train_iteration()
torch.cuda.synchronize()
out['p1'] = {{k: st.p.cpu().numpy() for k, st in tr.cx.stores.items()}}
torch.save(out, {out!r} % rank)
torch.distributed.destroy_process_group()
'''


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_hold_rank_zeros_initialisation(tmp_path):
    """two ranks on one GPU over gloo (the pattern of tests/test_gpu_dp.py): every rank runs the pass on its own batch, then holds
    rank 0's result — bit for bit what a single process initialised on rank 0's batch holds — and the replicas stay identical."""
    import torch
    port = _free_port()
    out = str(tmp_path / "r%d.pt")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, out=out))
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   TG_DIST_BACKEND="gloo", TG_DEVICE_INDEX="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-3000:]
    r = [torch.load(out % i, weights_only=False) for i in range(2)]
    assert r[0]['world'] == r[1]['world'] == 2 and r[0]['counts'] == r[1]['counts'] == COUNTS['svhn']
    single = _trainer('svhn', seed=5)
    single.feed(_batch('svhn', 500))
    single.sample_latent()
    single.data_dependent_init()
    torch.cuda.synchronize()
    for net, st in single.cx.stores.items():
        for q in r:
            np.testing.assert_array_equal(q['p'][net], st.p.cpu().numpy(), err_msg=net)
            np.testing.assert_array_equal(q['s'][net], st.s.cpu().numpy(), err_msg=net)
        np.testing.assert_array_equal(r[0]['p1'][net], r[1]['p1'][net], err_msg=net)       # and one iteration on: still replicas
    for q in r:
        np.testing.assert_array_equal(q['ema'], single.cx.stores['classifier'].ema.cpu().numpy())
