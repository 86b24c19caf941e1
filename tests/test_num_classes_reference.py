"""CPU: config.NUM_CLASSES is checked on the host (Training/Train_goodGAN.check_num_classes), and the float64 oracle's classifier-loss
terms, which the K-class GPU tests compare against, are the derivatives of the reference's loss at K != 10: oracle/tf_ops.py's
softmax_ce_mean, entropy, balance_entropy, c_unl_loss and mse_mean, and tests/loss_heads_k_reference.c_loss, against a torch float64
autograd restatement of train_base.py:43-57,75-79,130-152 at K in {2, 7, 100}."""
import numpy as np
import pytest
import torch

from oracle import tf_ops as T
import loss_heads_k_reference as R


def cfg(k):
    return type('C', (), dict(NUM_CLASSES=k))()


@pytest.mark.parametrize("k", [2, 3, 10, 100, 1000, 1024, np.int64(7)])
def test_check_num_classes_accepts_the_range(k):
    from Training.Train_goodGAN import check_num_classes
    assert check_num_classes(cfg(k)) == int(k)


@pytest.mark.parametrize("k", [None, 0, 1, -3, 1025, 4096, 10.0, "10", True])
def test_check_num_classes_rejects_the_rest(k):
    from Training.Train_goodGAN import check_num_classes
    with pytest.raises(ValueError, match="1024"):
        check_num_classes(cfg(k))


def _torch_terms(l_real, l_unl, l_rep, l_fake, y_real, y_fake, d_unl):
    """the reference's classifier terms as torch float64 expressions of the logits."""
    k = l_unl.shape[1]
    ce = lambda l, y: (torch.logsumexp(l, 1) * y.sum(1) - (y * l).sum(1)).mean()
    p = torch.softmax(l_unl, 1)
    h = (torch.logsumexp(l_unl, 1) - (p * l_unl).sum(1)).mean()
    bal = -(torch.log(p.mean(0) + 1e-12) / k).sum()
    pm = p.max(1).values
    r = torch.nn.functional.softplus(-d_unl)              # BCE(d, 1)
    c_unl = (pm * r).mean()
    mse = ((l_rep - l_unl) ** 2).mean()
    return [ce(l_real, y_real), c_unl, h, bal, ce(l_fake, y_fake), mse]


@pytest.mark.parametrize("k", [2, 7, 100])
def test_oracle_c_loss_terms_match_autograd(k):
    rng = np.random.default_rng(k)
    n_real, n_unl, n_fake = 6, 9, 5
    arr = lambda n: rng.standard_normal((n, k)) * 2.0
    l = [arr(n_real), arr(n_unl), arr(n_unl), arr(n_fake)]
    y_real, y_fake = np.eye(k)[rng.integers(0, k, n_real)], np.eye(k)[rng.integers(0, k, n_fake)]
    d_unl = rng.standard_normal(n_unl)
    tl = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in l]
    terms = _torch_terms(*tl, torch.tensor(y_real), torch.tensor(y_fake), torch.tensor(d_unl))

    def grads(t):
        return [g if g is not None else torch.zeros_like(a) for g, a in zip(torch.autograd.grad(t, tl, allow_unused=True, retain_graph=True), tl)]
    close = lambda a, b: np.testing.assert_allclose(a, b.detach().numpy() if torch.is_tensor(b) else b, rtol=1e-10, atol=1e-12)
    v, g = T.softmax_ce_mean(l[0], y_real)
    close(v, terms[0]); close(g, grads(terms[0])[0])
    v, g = T.c_unl_loss(l[1], d_unl[:, None])
    close(v, terms[1]); close(g, grads(terms[1])[1])
    v, g = T.entropy(l[1])
    close(v, terms[2]); close(g, grads(terms[2])[1])
    v, g = T.balance_entropy(l[1])
    close(v, terms[3]); close(g, grads(terms[3])[1])
    v, g = T.softmax_ce_mean(l[3], y_fake)
    close(v, terms[4]); close(g, grads(terms[4])[3])
    v, g_unl, g_rep = T.mse_mean(l[1], l[2])
    close(v, terms[5]); close(g_unl, grads(terms[5])[1]); close(g_rep, grads(terms[5])[2])
    # the restatement the GPU head tests use: weighted sum and gradient of the concatenated rows
    w6 = [1.0, 0.5, 0.3, 0.7, 0.4, 0.6]
    loss, got_terms, g = R.c_loss(*l, y_real, y_fake, d_unl, w6)
    total = sum(w * t for w, t in zip(w6, terms))
    for a, b in zip(got_terms, terms):
        close(a, b)
    close(loss, total)
    close(g, torch.cat(grads(total)))
