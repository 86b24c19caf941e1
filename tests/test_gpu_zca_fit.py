"""config.ZCA = 'fit' on the GPU: tg_gram_u8_i64 bit-exact against integer-valued float64 BLAS over edge shapes and byte
patterns, the fit end to end from CIFAR-10-named TFRecords through Train.train (files, constants, reload, whitening property, a short
epoch), and two data-parallel replicas that end with the same constants and one writer."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import gpu_common as G
import zca_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 32


def _data(kind, n, d, rng):
    if kind == 'random':
        return rng.integers(0, 256, (n, d), dtype=np.uint8)
    if kind == 'zeros':
        return np.zeros((n, d), np.uint8)
    if kind == 'ones':
        return np.full((n, d), 255, np.uint8)
    return ((np.arange(n * d, dtype=np.int64) & 1) * 255).astype(np.uint8).reshape(n, d)        # alternating 0 / 255


def _want(kind, x):
    n, d = x.shape
    if kind in ('zeros', 'ones'):                                  # closed form: every x' is -128 (zeros) or 127 (ones)
        v = -128 if kind == 'zeros' else 127
        return np.full(d, v * n, np.int64), np.full((d, d), v * v * n, np.int64)
    _, s, g = R.int_moments(x)
    return s, g


SHAPES = [(1, 1), (1, 3072), (65, 100), (1000, 784), (4099, 3072), (50000, 3072), (140000, 64)]
KINDS = ['random', 'zeros', 'ones', 'alternating']


@pytest.mark.parametrize("n, d", SHAPES)
def test_gram_is_bit_exact(n, d):
    """gram and colsum equal the exact integer moments of x' = x - 128 (int64, both triangles), a second call doubles them, and the
    canaries behind gram and behind colsum are untouched.  (140000, 64) crosses the 131071-row int32 window of one workgroup."""
    import torch
    from tg import lib
    lib.load()
    rng = np.random.default_rng(n * 7 + d)
    st = lib.cur_stream()
    for kind in KINDS:
        x = _data(kind, n, d, rng)
        xd = torch.from_numpy(x).cuda()
        buf = torch.full((d * d + CANARY + d + CANARY,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device='cuda')
        gram, colsum = buf[:d * d], buf[d * d + CANARY:d * d + CANARY + d]
        gram.zero_()
        colsum.zero_()
        lib.call('tg_gram_u8_i64', lib.ptr(xd), n, d, lib.ptr(gram), lib.ptr(colsum), st)
        torch.cuda.synchronize()
        s_want, g_want = _want(kind, x)
        g1, s1 = gram.cpu().numpy().reshape(d, d), colsum.cpu().numpy()
        np.testing.assert_array_equal(s1, s_want, err_msg=kind)
        np.testing.assert_array_equal(g1, g_want, err_msg=kind)
        lib.call('tg_gram_u8_i64', lib.ptr(xd), n, d, lib.ptr(gram), lib.ptr(colsum), st)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(colsum.cpu().numpy(), 2 * s_want, err_msg=kind)
        np.testing.assert_array_equal(gram.cpu().numpy().reshape(d, d), 2 * g_want, err_msg=kind)
        b = buf.cpu().numpy()
        assert (b[d * d:d * d + CANARY] == -0x5A5A5A5A5A5A5A5B).all() and (b[d * d + CANARY + d:] == -0x5A5A5A5A5A5A5A5B).all(), kind
        del xd, buf


def test_gram_rejects_bad_arguments_and_ignores_no_rows():
    import torch
    from tg import lib
    lib.load()
    st = lib.cur_stream()
    x = torch.zeros(64, dtype=torch.uint8, device='cuda')
    g = torch.full((16,), 7, dtype=torch.int64, device='cuda')
    lib.call('tg_gram_u8_i64', lib.ptr(x), 0, 4, lib.ptr(g), lib.ptr(g), st)
    torch.cuda.synchronize()
    assert (g.cpu().numpy() == 7).all()
    for n, d in ((-1, 4), (4, 0)):
        with pytest.raises(lib.TgError, match="gram_u8_i64"):
            lib.call('tg_gram_u8_i64', lib.ptr(x), n, d, lib.ptr(g), lib.ptr(g), st)


SIZES = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
N_LAB, N_UNL, N_TEST = 300, 900, 40


def _write_files(root, seed=3):
    from tg import io as tgio
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    os.makedirs(os.path.join(root, 'Tfrecord'))
    rng = np.random.default_rng(seed)
    tr = cifar10Dataset(root, None, N_LAB, 'train')
    te = cifar10Dataset(root, None, N_LAB, 'test')
    imgs = []
    for name, n in zip(tr.get_filenames() + te.get_filenames(), (N_LAB, N_UNL, N_TEST)):
        img = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
        tgio.write_tfrecord(name, img, rng.integers(0, 10, n))
        imgs.append(img)
    return np.concatenate(imgs[:2])


def _config(root):
    return G.make_config(SIZES, DATA_DIR=root, NUM_LABEL=N_LAB, TRAIN_SIZE=2 * SIZES['B_G'], EPOCHS=1, SAMPLE_DIR=None, REPEAT=-1,
                         ZCA='fit')


def _train(cfg):
    import torch
    from tg import runtime
    from Training.Train_goodGAN import Train
    from Model.Good_GAN_cifar10 import Good_GAN_cifar10
    from Input_Pipeline.cifar10Dataset import cifar10Dataset
    runtime.set_context(None)
    torch.cuda.empty_cache()
    tr = Train(cfg, None, None)
    return tr, tr.train(cifar10Dataset, Good_GAN_cifar10, None)


def test_fit_end_to_end_from_tfrecords(tmp_path, monkeypatch):
    import torch
    from Model.zca import ZCA_EPS, cifar10_ZCA, zca_paths
    from tg.runtime import Act
    root = str(tmp_path)
    train = _write_files(root)
    cfg = _config(root)
    tr, hist = _train(cfg)
    # the files of the reference's path, float32 in NHWC flatten order
    m_path, mat_path = zca_paths(cfg)
    assert tr.zca_source == 'fit' and os.path.exists(m_path) and os.path.exists(mat_path)
    mean, mat = np.load(m_path), np.load(mat_path)
    assert mean.dtype == mat.dtype == np.float32 and mean.shape == (3072,) and mat.shape == (3072, 3072)
    assert [f for f in os.listdir(root) if f.endswith('.tmp')] == []
    assert np.array_equal(cfg.ZCA[0], mean) and np.array_equal(cfg.ZCA[1], mat)
    # the constants are the float64 restatement's, within float32 storage
    mean_r, mat_r, cov_r, s_r = R.zca(train, ZCA_EPS)
    np.testing.assert_allclose(mean, mean_r, rtol=0, atol=1e-7)
    assert np.abs(mat.astype(np.float64) - mat_r).max() <= 2e-7 * np.abs(mat_r).max()
    # one short epoch on the files, finite losses
    assert len(hist) == 1 and np.isfinite([hist[0][k] for k in ('d_loss', 'g_loss', 'c_loss')]).all()
    assert tr.iteration == 2
    # the model's zca().apply on the training images whitens them: eigenvalues of the output covariance = s / (s + eps)
    cx = tr.cx
    x = torch.from_numpy(R.scaled(train).astype(np.float32)).to(cx.device)
    out = []
    for a in range(0, len(train), 400):
        xa = x[a:a + 400].reshape(-1)
        out.append(tr.model.zca().apply(Act(xa, xa.numel() // 3072, 32, 32, 3, 3)).numpy().reshape(-1, 3072))
    y = np.concatenate(out).astype(np.float64)
    yc = y - y.mean(0)
    got = np.linalg.eigvalsh(yc.T @ yc / len(y))
    want = R.whitening_eigenvalues(s_r, ZCA_EPS)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-3)
    # a second Train.train loads the files and does not fit again
    monkeypatch.setattr(cifar10_ZCA, 'fit', staticmethod(lambda *a, **k: pytest.fail("refit")))
    cfg2 = _config(root)
    tr2, hist2 = _train(cfg2)
    assert tr2.zca_source == 'files' and np.array_equal(cfg2.ZCA[0], mean) and np.array_equal(cfg2.ZCA[1], mat)
    assert np.isfinite([hist2[0][k] for k in ('d_loss', 'g_loss', 'c_loss')]).all()


WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, os.path.join({root!r}, "tensorflow-implementation-of-triple-gan_amd"))
import torch
import test_gpu_zca_fit as T
cfg = T._config({data!r})
tr, hist = T._train(cfg)
torch.save(dict(rank=tr.rank, world=tr.world, source=tr.zca_source, mean=cfg.ZCA[0], mat=cfg.ZCA[1],
                losses=[hist[0][k] for k in ('d_loss', 'g_loss', 'c_loss')]), {out!r} % tr.rank)
torch.distributed.destroy_process_group()
'''


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_replicas_hold_identical_constants_with_one_writer(tmp_path):
    """two gloo ranks on one GPU (tests/test_gpu_dp.py): rank 0 fits and writes, rank 1 receives the constants by broadcast."""
    import torch
    from Model.zca import zca_paths
    data = str(tmp_path / 'data')
    os.makedirs(data)
    _write_files(data)
    out = str(tmp_path / "r%d.pt")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, data=data, out=out))
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   TG_DIST_BACKEND="gloo", TG_DEVICE_INDEX="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-3000:]
    r = [torch.load(out % i, weights_only=False) for i in range(2)]
    assert r[0]['world'] == r[1]['world'] == 2
    assert [q['source'] for q in r] == ['fit', 'broadcast']            # exactly one writer
    assert np.array_equal(r[0]['mean'], r[1]['mean']) and np.array_equal(r[0]['mat'], r[1]['mat'])
    assert r[0]['mean'].dtype == r[0]['mat'].dtype == np.float32 and r[0]['mat'].shape == (3072, 3072)
    cfg = _config(data)
    m_path, mat_path = zca_paths(cfg)
    assert np.array_equal(np.load(m_path), r[0]['mean']) and np.array_equal(np.load(mat_path), r[0]['mat'])
    assert sorted(f for f in os.listdir(data) if f != 'Tfrecord') == ['cifar10_zca_mat.npy', 'cifar10_zca_mean.npy']
    assert all(np.isfinite(q['losses']).all() for q in r)
