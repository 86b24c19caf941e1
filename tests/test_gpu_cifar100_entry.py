"""_main_training_cifar100 (Training/Train_goodGAN.py): the CIFAR-10 networks and algorithm with NUM_CLASSES = 100 run end to end on the
synthetic dataset for a shortened epoch — training iterations, validation, the sample grid and a checkpoint."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_cifar100_entry_point_runs_one_short_epoch(tmp_path, monkeypatch):
    from tg import runtime
    from Training import Train_goodGAN as TG
    runtime.set_context(None)

    class Flags(object):
        train_size = 10000 + 400
        sample_dir = str(tmp_path / "samples")
        seed = 1
    monkeypatch.setattr(TG, "_root_dir", lambda: str(tmp_path))
    hist = TG._main_training_cifar100(Flags(), epochs=1)
    assert len(hist) == 1 and np.isfinite([hist[0]['d_loss'], hist[0]['g_loss'], hist[0]['c_loss']]).all()
    assert 0.0 <= hist[0]['val_accuracy'] <= 1.0 and hist[0]['images_per_sec'] > 0
    files = [f for _, _, fs in os.walk(str(tmp_path)) for f in fs]
    assert 'train_01.png' in files
    assert any('Weight_cifar100' in d for d, _, fs in os.walk(str(tmp_path)) if fs), "no checkpoint written"


def _state(tr):
    out = {}
    for k, st in tr.cx.stores.items():
        for buf in ('p', 'm', 'v', 's', 'step'):
            out[k + '/' + buf] = getattr(st, buf).detach().cpu().numpy().copy()
        if st.ema is not None:
            out[k + '/ema'] = st.ema.detach().cpu().numpy().copy()
    return out


def test_cifar100_checkpoint_restores_and_continues_bit_identically(tmp_path):
    """a 100-class model (output_dense 100 wide, 100 label channels in every discriminator concat) saved after two iterations, restored
    into a trainer of another seed, continues bit-identically to the uninterrupted run: weights, Adam slots, running statistics, EMA
    shadows and losses."""
    import torch
    import gpu_common as G
    from Training.Saver import Saver
    sizes = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
    rng = np.random.default_rng(41)
    oh = lambda n: np.eye(100, dtype=np.float32)[rng.integers(0, 100, n)]
    img = lambda n: np.tanh(rng.standard_normal((n, 32, 32, 3))).astype(np.float32)
    feeds = [dict(x_l_c=img(4), y_l_c=oh(4), x_l_d=img(2), y_l_d=oh(2), x_u_d=img(6), x_u_c=img(4)) for _ in range(4)]

    def run(tr, its):
        for i in its:
            tr.feed(feeds[i])
            tr.sample_latent()
            tr.train_iteration()
        torch.cuda.synchronize()

    def trainer(seed):
        tr = G.fresh_trainer(G.make_config(sizes, SEED=seed, USE_HIP_GRAPH=True, NUM_CLASSES=100, DATA_NAME='cifar100'))
        tr.set_hyper(lambda_1=0.3, lambda_2=0.5)
        return tr

    a = trainer(9)
    assert a.cx.stores['classifier'].get('classifier/output_dense/V').shape[-1] == 100
    run(a, [0, 1])
    saver = Saver(str(tmp_path))
    saver.set_save_path(comments='cifar100 resume test')
    saver.save(a, 'model_0002.ckpt')
    run(a, [2, 3])
    want, want_losses = _state(a), a.losses()

    b = trainer(1234)                                   # another seed: everything must come from the file
    assert Saver(str(tmp_path)).restore(b) == 2
    run(b, [2, 3])
    got = _state(b)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert b.losses() == want_losses and np.isfinite(want_losses).all()
