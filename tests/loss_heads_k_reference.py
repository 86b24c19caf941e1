"""float64 NumPy restatement of the classifier's loss heads for any class count K (csrc/loss.hip; Training/train_base.py:43-57,75-79,
113-154,162-166): value and d(value)/d(logits) of c_loss / c_loss_terms, true_fake_loss, softmax_ce and entropy_terms.  Logits are
[n, K] (the padding columns already cut off), labels dense [n, K]."""
import numpy as np


def softmax(l):
    m = l.max(axis=1, keepdims=True)
    e = np.exp(l - m)
    s = e.sum(axis=1, keepdims=True)
    return e / s, (m + np.log(s))[:, 0]


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def ce(l, y):
    """mean_n softmax-CE(y, l) and its gradient."""
    p, lse = softmax(l)
    n = len(l)
    ysum = y.sum(axis=1)
    return float(np.mean(lse * ysum - (y * l).sum(axis=1))), (p * ysum[:, None] - y) / n


def entropy(l):
    """H = mean_n(lse - sum_k p_k l_k) and dH/dl."""
    p, lse = softmax(l)
    pl = (p * l).sum(axis=1, keepdims=True)
    n = len(l)
    return float(np.mean(lse - pl[:, 0])), (p - p * (1.0 + l - pl)) / n


def balance(l):
    """Bal = -sum_k (1/K) log(mean_n p_k + 1e-12) and dBal/dl."""
    p, _ = softmax(l)
    n, k = l.shape
    q = p.mean(axis=0)
    dq = -1.0 / (k * (q + 1e-12)) / n
    pdq = (p * dq).sum(axis=1, keepdims=True)
    return float(-np.sum(np.log(q + 1e-12)) / k), p * (dq - pdq)


def c_loss(real, unl, rep, fake, y_real, y_fake, d_unl, w6):
    """rows [real | unl | rep (or None) | fake (may have 0 rows)]; w6 = {CE(real), c_unl, H, Bal, CE(fake), MSE}.  Returns
    (loss, the six unweighted terms, gradient of the concatenated rows)."""
    n_unl, k = unl.shape
    t_real, g_real = ce(real, y_real)
    p, _ = softmax(unl)
    j = np.argmax(p, axis=1)
    pm = p[np.arange(n_unl), j]
    rr = softplus(-d_unl) if d_unl is not None else np.zeros(n_unl)       # BCE(d, 1)
    t_unl = float(np.mean(pm * rr))
    oh = np.eye(k)[j]
    g_cunl = (rr * pm)[:, None] * (oh - p) / n_unl
    t_h, g_h = entropy(unl)
    t_bal, g_bal = balance(unl)
    g_unl = w6[1] * g_cunl + w6[2] * g_h + w6[3] * g_bal
    grads = [w6[0] * g_real, g_unl]
    t_mse = 0.0
    if rep is not None:
        d = rep - unl
        t_mse = float(np.sum(d * d) / (n_unl * k))
        gm = 2.0 * d / (n_unl * k)
        grads[1] = g_unl - w6[5] * gm
        grads.append(w6[5] * gm)
    t_fake = 0.0
    if len(fake):
        t_fake, g_fake = ce(fake, y_fake)
        grads.append(w6[4] * g_fake)
    terms = [t_real, t_unl, t_h, t_bal, t_fake, t_mse]
    loss = sum(w * t for w, t in zip(w6, terms))
    return loss, terms, np.concatenate(grads, axis=0)


def true_fake(unl, fake, w_unl, w_fake):
    _, lu = softmax(unl)
    _, lf = softmax(fake)
    pu, _ = softmax(unl)
    pf, _ = softmax(fake)
    t_u = float(np.mean(-0.5 * lu + 0.5 * softplus(lu)))
    t_f = float(0.5 * np.mean(softplus(lf)))
    gu = (w_unl * (-0.5 + 0.5 * sigmoid(lu)) / len(unl))[:, None] * pu
    gf = (w_fake * 0.5 * sigmoid(lf) / len(fake))[:, None] * pf
    return [w_unl * t_u + w_fake * t_f, t_u, t_f], gu, gf
