"""Whole-network gradients of the float32 HIP path against the float64 oracle BEHIND IDENTICAL KINKS.

tests/test_gpu_nets.py, test_gpu_goodgan.py and test_gpu_step.py compare the un-injected runs and have to allow 1e-2 .. 6e-2 per variable:
a handful of activations sit closer to a ReLU / leaky-ReLU / max-pool kink than the float32 forward error and take the other branch.  Here
the oracle's backward pass is given the decisions the HIP path took — read from the activation buffers its forward pass stored
(tests/kink_capture.py), which is what every kink decision of the HIP backward kernels is a function of — so that what is compared is the
backward tape itself: closure order, gradient accumulation and aliasing, per-application statistics of batched calls, the label channels
cut off concat gradients.  The bounds (kink_reference.BOUNDS) are 10 x the error of the oracle's own float32 twin, never what the HIP
path produces; profiles/kink_parity.txt has every number and how each bound was set.

The networks run alone (batched applications of unequal size, a gradient seeded on the classifier's feature as well as on its logits)
and inside one phase-synchronised iteration per model family, where the pseudo-labels are injected too.

In every test: each oracle kink site is matched to a logged buffer by shape, order and value (a site without a match fails); the buffers
are equal before and after the backward pass (backward overwrites no kink carrier); the injected kinks differ from the oracle's own only
where the oracle itself is within ACT_TOL of a kink, in at most 1e-3 of a site's decisions (injection cannot hide a wrong forward pass)."""
import os

import numpy as np
import pytest

import gpu_common as G
import kink_reference as K
from kink_capture import Capture, match

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cifar():
    c = K.case('cifar10/C')[0]
    return G.fresh_trainer(G.make_config(dict(B_G=6, L_C=3, U_C=2, L_D=2, U_D=4)), c.P)


_GOODGAN = {}


def goodgan(data):
    from test_gpu_goodgan import trainer
    if data not in _GOODGAN:
        _GOODGAN.clear()                                   # one live trainer at a time
        _GOODGAN[data] = trainer(data, K.case(data + '/G')[0].P)
    return _GOODGAN[data]


def hip_run(c, tr, tag):
    """the case's forward + backward on the HIP path -> (out, {variable: gradient}, arrays after forward, arrays after backward)."""
    from tg.runtime import InjectedRNG
    cx, m = tr.cx, tr.model
    net = {'C': 'classifier', 'D': 'discriminator', 'G': 'good_generator'}[c.net]
    cat = lambda parts: np.concatenate(parts)
    cx.rng = InjectedRNG({'%s/%s/%s' % (tag, c.net, k): v for k, v in G.cat_rnd(*c.rnd).items()}, cx.device)
    seed = c.dl if hasattr(c, 'dl') else c.do
    inp = None
    with Capture(cx) as cap:
        with cx.phase_scope(tag, train_nets=(net,)):
            with cx.rng_scoped('%s/%s' % (tag, c.net)):
                if c.net == 'C':
                    out, feat = m.classifier(cx.from_numpy(cat(c.x)), True, segments=list(c.segs))
                elif c.net == 'D':
                    inp = cx.from_numpy(cat(c.x))
                    inp.requires_grad = True
                    _, out = m.discriminator(inp, cx.from_numpy(cat(c.y)))
                else:
                    out = m.good_generator(cx.from_numpy(c.z if hasattr(c, 'z') else c.x[0]), cx.from_numpy(c.y[0] if isinstance(c.y, list) else c.y))
            fwd = cap.snapshot()
            out_host = out.numpy().copy()
            out.grad = cx.from_numpy(seed.reshape(out_host.shape), ld=None if c.net == 'G' else 32)
            if c.net == 'C' and c.df is not None:
                feat.grad = cx.from_numpy(c.df, ld=feat.ld)
            cx.backward()
        bwd = cap.snapshot(len(fwd))
    st = cx.stores[net]
    grads = {k: st.get(k, 'grad') for k in st.names(True)}
    if inp is not None:
        grads['d_input'] = inp.grad.numpy()
    return out_host, grads, fwd, bwd


def check(name, tr, tag, report):
    c, st, g_own = K.case(name)
    out, grads, fwd, bwd = hip_run(c, tr, tag)
    lines = ['%s  (%s)' % (name, tag)]
    assert G.rel_err(out.reshape(st['out'].shape), st['out']) < c.act_tol
    per_app = c.sites(st)
    sites = K.cat_sites(per_app)
    acts, where = match(sites, fwd, c.act_tol)
    for key, j in where.items():
        assert np.array_equal(fwd[j], bwd[j]), ('the backward pass overwrote a kink carrier', key, j)
    moved = sum(1 for a, b in zip(fwd, bwd) if a is not None and not np.array_equal(a, b))
    kinks = K.kinks_from_acts(sites, acts)
    fl = K.flips(sites, kinks, c.act_tol)
    lines.append('  kink sites %d, all matched; buffers logged %d, changed by backward %d (none a kink carrier); flipped/decisions: %s'
                 % (len(sites), len(fwd), moved, ' '.join('%s:%d/%d' % (k, a, b) for k, (a, b) in fl.items())))
    g_ref = c.backward(st, K.split_kinks(kinks, per_app))
    if 'd_input' in g_ref:
        rows = (slice(2, 5) if name == 'cifar10/D' else slice(None))
        grads['d_input'] = grads['d_input'][rows].reshape(g_ref['d_input'].shape)
    assert set(g_ref) <= set(grads), set(g_ref) - set(grads)
    errs = K.grad_errors(grads, g_ref, c.zero)
    own = K.grad_errors(grads, g_own, c.zero)
    bmx, bl2 = K.BOUNDS[name]
    over = lambda k: errs[k][0] > K.bound(name, k)[0] or errs[k][1] > K.bound(name, k)[1]
    for k, (mx, l2) in errs.items():
        lines.append('  %-64s max %.2e  L2 %.2e   (against the oracle\'s own kinks: %.2e %.2e)%s'
                     % (k, mx, l2, own[k][0], own[k][1], '   <-- over the bound' if over(k) else ''))
    for k in c.zero:
        lines.append('  %-64s analytically 0: max|g_hip| %.2e   floor %.1e' % (k, np.abs(grads[k]).max(), K.ZERO_FLOORS[name][k]))
    lines.append('  worst %.2e %.2e   bound %.2e %.2e' % (K.worst(errs) + (bmx, bl2)))
    print('\n'.join(lines))
    report(lines)
    bad = {k: e for k, e in errs.items() if over(k)}
    assert not bad, (name, 'bound', (bmx, bl2), bad)
    for k in c.zero:
        assert np.abs(grads[k]).max() <= K.ZERO_FLOORS[name][k], ('analytically zero gradient', k, np.abs(grads[k]).max())


@pytest.fixture(scope="module")
def report():
    """collects the measured figures; with KINK_PARITY_REPORT=<file> they are appended there (the record in profiles/kink_parity.txt is
    made from it — a record, not the source of any bound)."""
    path = os.environ.get('KINK_PARITY_REPORT')

    def add(lines):
        if path:
            with open(path, 'a') as f:
                f.write('\n'.join(lines) + '\n')
    return add


@pytest.mark.parametrize("policy", [0, 1])
def test_cifar10_classifier_two_segments_with_feature_seed(cifar, report, policy):
    """segments [3, 2], dlogits and a dfeat seed on the pooled feature; under both routings of the 3x3 layers (tg_conv3x3_policy)."""
    from tg import lib
    was = lib.call('tg_conv3x3_policy', policy)
    try:
        check('cifar10/C', cifar, 'KC%d' % policy, report)
    finally:
        lib.call('tg_conv3x3_policy', was)


def test_cifar10_discriminator_three_applications(cifar, report):
    """applications [2, 3, 2] in one batched call, weight gradients summed over them, the image gradient of the middle (fake) rows."""
    check('cifar10/D', cifar, 'KD', report)


def test_cifar10_generator(cifar, report):
    check('cifar10/G', cifar, 'KG', report)


@pytest.mark.parametrize("net", ['G', 'D', 'C'])
@pytest.mark.parametrize("data", ['mnist', 'svhn'])
def test_goodgan_networks(data, net, report):
    """MNIST / SVHN models, float32: G and D on 5 images, C on segments [3, 2] (batch norms with per-application statistics, max-pools)."""
    check('%s/%s' % (data, net), goodgan(data), 'K' + net, report)


# ------------------------------------------------------------------------------------------------ one phase-synchronised iteration
def run_step(c, st, tr, report, after):
    """tests/test_gpu_step.run_synchronised for one iteration, with every solver run of the oracle given the HIP run's kinks and pseudo-
    labels: HIP phase -> capture -> oracle phase with injection -> gradients -> `after(phase, before)` (optimiser step, state sync)."""
    from oracle import tf_ops as T
    cx, prev, ref_losses = tr.cx, [], []
    lines = ['%s step %s' % (c.family, c.sizes)]
    for ph, hip in (('D', tr._d_forward_backward), ('G', tr._g_forward_backward), ('C', tr._c_forward_backward)):
        before = {k: v.copy() for k, v in st['P'].items()}
        with Capture(cx) as cap:
            hip()
        arrays = cap.snapshot()
        labels = None
        if ph == 'D':
            labels = {'unl': tr._d_labels[0].numpy(), 'unl_d': tr._d_labels[1].numpy()}
        elif ph == 'C':
            labels = {'unl': T.argmax_onehot(tr._c_logits.numpy().astype(np.float64))}
        pool = prev + arrays if ph == 'G' else arrays          # the G-update re-uses the D-update's generator forward pass
        fl = {}

        def inject(key, sites):
            acts, _ = match(sites, pool, c.act_tol, c.rows[ph][key])
            kk = K.kinks_from_acts(sites, acts)
            fl[key] = K.flips(sites, kk, c.act_tol)
            return kk
        ref_losses.append(c.phase(st, ph, np.float64, inject, labels))
        assert set(fl) == set(c.rows[ph]), (set(fl), set(c.rows[ph]))          # every application that has a backward pass was injected
        moved = 0
        for k, lg in (st['last_logits'].items() if labels else ()):
            mism = np.where(labels[k].argmax(1) != lg.argmax(1))[0]           # the near-tie rule of tests/test_gpu_goodgan.py
            top2 = np.sort(lg, axis=1)[:, -2:]
            assert ((top2[mism, 1] - top2[mism, 0]) <= 4 * c.act_tol * np.abs(lg).max()).all(), ('labels differ where the oracle has no near-tie', k, mism)
            moved += len(mism)
        store = cx.stores[K.STEP_NETS[ph]]
        g_ref = st['last_grads'][ph]
        zero = K.STEP_ZERO[c.family] if ph == 'C' else ()
        grads = {k: store.get(k, 'grad') for k in g_ref}
        errs = K.grad_errors(grads, g_ref, zero)
        bmx, bl2, _ = K.STEP_BOUNDS[c.family][ph]
        lines.append('  %s-update: kinks flipped %s; pseudo-labels moved %d' % (ph, ' '.join(
            '%s:%d/%d' % (key, sum(a for a, _ in f.values()), sum(b for _, b in f.values())) for key, f in fl.items()), moved))
        for k, (mx, l2) in errs.items():
            lines.append('    %-62s max %.2e  L2 %.2e%s' % (k, mx, l2, '   <-- over the bound' if mx > bmx or l2 > bl2 else ''))
        for k in zero:
            lines.append('    %-62s analytically 0: max|g_hip| %.2e   floor %.1e' % (k, np.abs(grads[k]).max(), K.STEP_ZERO_FLOORS[c.family][k]))
        lines.append('    worst %.2e %.2e   bound %.2e %.2e' % (K.worst(errs) + (bmx, bl2)))
        print('\n'.join(lines[-len(errs) - len(zero) - 2:]))
        bad = {k: e for k, e in errs.items() if e[0] > bmx or e[1] > bl2}
        if bad:
            report(lines)
        assert not bad, (c.family, ph, (bmx, bl2), bad)
        for k in zero:
            assert np.abs(grads[k]).max() <= K.STEP_ZERO_FLOORS[c.family][k], ('analytically zero gradient', k, np.abs(grads[k]).max())
        after(ph, before)
        prev = arrays
    got = tr.losses()
    for ph, r, g in zip('DGC', ref_losses, got):
        lines.append('  %s loss: oracle %.8f  HIP %.8f  relative %.2e   bound %.1e' % (ph, r, g, abs(r - g) / max(1.0, abs(r)), K.STEP_BOUNDS[c.family][ph][2]))
    print('\n'.join(lines[-3:]))
    report(lines)
    for ph, r, g in zip('DGC', ref_losses, got):
        assert abs(r - g) <= K.STEP_BOUNDS[c.family][ph][2] * max(1.0, abs(r)), (ph, r, g)


def test_cifar10_synchronised_iteration(report):
    import test_gpu_step as TS
    from tg.runtime import InjectedRNG
    c = K.Step('cifar10')
    st, tr, _ = TS.setup(c.sizes, c.hyper)
    stores = tr.cx.stores
    tr.cx.rng = InjectedRNG(G.injected_arrays(c.rnd), tr.cx.device)
    tr.feed(c.batch)

    def after(ph, before):
        if ph == 'C':
            tr._c_apply()
        else:
            tr._train_op(tr.d_optimizer if ph == 'D' else tr.g_optimizer, stores[K.STEP_NETS[ph]])
        TS.check_update_and_sync(st, tr, ph, before, c.hyper['cla_lr' if ph == 'C' else 'lr'])
        if ph != 'G':
            TS.sync_pop_means(st, tr)
    run_step(c, st, tr, report, after)


def test_svhn_synchronised_iteration(report):
    from test_gpu_goodgan import trainer, f64
    from tg.runtime import InjectedRNG
    c = K.Step('svhn')
    st = c.new_state(np.float64)
    _GOODGAN.clear()
    tr = trainer('svhn', f64(c.P), sizes=c.sizes)
    tr.set_hyper(c.hyper['lr'], c.hyper['cla_lr'], c.hyper['lambda_1'], 0.0)
    stores = tr.cx.stores
    tr.cx.rng = InjectedRNG(G.injected_arrays_goodgan(c.rnd), tr.cx.device)
    tr.feed(c.batch)

    def after(ph, before):
        if ph == 'C':
            tr._c_apply()
            return
        tr._train_op(tr.d_optimizer if ph == 'D' else tr.g_optimizer, stores[K.STEP_NETS[ph]])
        for net in K.STEP_NETS.values():                   # each solver run starts from identical weights and moving statistics
            for k in stores[net].names():
                stores[net].set(k, st['P'][k])
    run_step(c, st, tr, report, after)
