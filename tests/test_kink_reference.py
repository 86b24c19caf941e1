"""CPU tests of the kink-control machinery (tests/kink_reference.py, oracle.nets_*.apply_kinks) that tests/test_gpu_kink_parity.py
stands on: injecting a network's own kinks changes nothing (bit for bit); what an injected kink MEANS is pinned against torch float64
autograd of the frozen-mask network; the float32 twin gives the scale the GPU bounds are set from; and every negative control — one
single-site mistake of the kind a backward-tape bug makes — exceeds the bound at least three times.  The twin and control numbers are
written to profiles/kink_parity.txt."""
import os

import numpy as np
import pytest
import torch

from oracle import nets_cifar10 as NC
from oracle import nets_goodgan as NG
from oracle import step_cifar10 as SC
from oracle import step_goodgan as SG
import kink_reference as K
from test_oracle_ops import tconv
import test_oracle_nets as TN
import test_oracle_goodgan as TG

torch.set_num_threads(4)
tt = TN.tt
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'kink_parity.txt')


def write_section(title, lines):
    """replace (or append) the section '== title ==' of profiles/kink_parity.txt; a read-only checkout is left alone."""
    head = '== %s ==' % title
    try:
        old = open(PROFILE).read().split('\n') if os.path.exists(PROFILE) else []
        new = [head] + list(lines) + ['']
        if head in old:                                      # in place: the sections keep their order
            i = old.index(head)
            j = next((k for k in range(i + 1, len(old)) if old[k].startswith('== ')), len(old))
            out = old[:i] + new + old[j:]
        else:
            while old and not old[-1]:
                old.pop()
            out = old + ([''] if old else []) + new
        while out and not out[-1]:
            out.pop()
        with open(PROFILE, 'w') as f:
            f.write('\n'.join(out) + '\n')
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------ own kinks: bit for bit
@pytest.mark.parametrize("name", list(K.CASES))
def test_own_kinks_reproduce_the_gradients_bit_for_bit(name):
    c, st, g = K.case(name)
    per_app = c.sites(st)
    own = [K.kinks_of(s) for s in per_app]
    # the helper's decisions are the cache's own (same arg-max rule), per application and through the batched round trip
    cat = K.kinks_of(K.cat_sites(per_app))
    for a, b in zip(K.split_kinks(cat, per_app), own):
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    g2 = c.backward(st, own)
    assert set(g2) == set(g)
    for k in g:
        assert np.array_equal(g[k], g2[k]), k
    assert all(n == 0 for n, _ in K.flips(K.cat_sites(per_app), cat, c.act_tol).values())
    gmax = max(np.abs(v).max() for k, v in g.items() if k != 'd_input')
    for k in c.zero:                                            # the variables excluded from relative bounds ARE zero in exact arithmetic
        assert np.abs(g[k]).max() < 1e-9 * gmax, k


# ------------------------------------------------------------------------------------------------ what an injected kink means
def frozen_act(x, mask, slope):
    """value of the (leaky) ReLU, derivative where(mask, 1, slope): the injected decision replaces the derivative, never a value."""
    one = torch.ones((), dtype=x.dtype)
    lin = x * torch.where(torch.as_tensor(mask), one, slope * one)
    return torch.where(x > 0, x, slope * x).detach() + lin - lin.detach()


def frozen_pool2(x, idx):
    n, h, w, c = x.shape
    v = x.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4, c)
    g = v.gather(3, torch.as_tensor(idx)[:, :, :, None, :]).squeeze(3)
    return v.amax(3).detach() + g - g.detach()


def frozen_gpool(x, idx):
    n, h, w, c = x.shape
    v = x.reshape(n, h * w, c)
    g = v.gather(1, torch.as_tensor(idx)[:, None, :]).squeeze(1)
    return v.amax(1).detach() + g - g.detach()


def t_classifier_frozen(P, x, rnd, kk):
    x = x + tt(rnd['noise'])
    for name, cout, pad in NC.C_CONVS:
        p = 'classifier/%s/' % name
        x = tconv(x, TN.wn(P[p + 'V'], P[p + 'g']), 1, pad)
        x = frozen_act(x - x.mean(dim=(0, 1, 2)) + P[p + 'b'], kk[name + '/y'], 0.2)
        if name in NC.C_POOL_AFTER:
            x = frozen_pool2(x, kk[name + '/pool_idx']) * tt(rnd[NC.C_POOL_AFTER[name]]) / 0.5
    for name in ('NiN1', 'NiN2'):
        p = 'classifier/%s/%s/' % (name, name)
        s = x.shape
        x2 = x.reshape(-1, s[-1]) @ P[p + 'V'] * (P[p + 'g'] / torch.sqrt((P[p + 'V'] ** 2).sum(0)))
        x = frozen_act(x2 - x2.mean(0) + P[p + 'b'], kk[name + '/y'], 0.2).reshape(s[0], s[1], s[2], -1)
    feat = frozen_gpool(x, kk['gpool/idx'])
    p = 'classifier/output_dense/'
    x2 = feat @ P[p + 'V'] * (P[p + 'g'] / torch.sqrt((P[p + 'V'] ** 2).sum(0)))
    return x2 - x2.mean(0) + P[p + 'b'], feat


def t_generator_frozen(P, z, y, kk):
    g = 'good_generator/'
    h = frozen_act(torch.cat([z, y], 1) @ P[g + 'gg_h0_lin/gg_h0_lin/kernel'] + P[g + 'gg_h0_lin/gg_h0_lin/bias'], kk['r0'], 0.0)
    h = TN.cc(TN.bn(h, P[g + 'gg_bn0/gamma'], P[g + 'gg_bn0/beta']).reshape(-1, 4, 4, 512), y)
    for i, (name, cout) in enumerate(NC.G_DECONVS):
        p = g + '%s/%s/' % (name, name)
        h = TN.t_deconv(h, P[p + 'kernel']) + P[p + 'bias']
        if i < 2:
            h = TN.cc(TN.bn(frozen_act(h, kk['r%d' % (i + 1)], 0.0), P[g + 'gg_bn%d/gamma' % (i + 1)], P[g + 'gg_bn%d/beta' % (i + 1)]), y)
    return torch.tanh(h)


def t_discriminator_frozen(P, img, y, rnd, kk):
    h = img * tt(rnd['drop0']) / 0.8
    for name, cout, s, drop in NC.D_CONVS:
        p = 'discriminator/%s/%s/' % (name, name)
        h = frozen_act(tconv(TN.cc(h, y), P[p + 'kernel'], s, 'SAME') + P[p + 'bias'], kk[name + '/y'], 0.2)
        if drop:
            h = h * tt(rnd[drop]) / 0.8
    h = torch.cat([h.mean(dim=(1, 2)), y], 1)
    return h @ P['discriminator/lin/lin/kernel'] + P['discriminator/lin/lin/bias']


def t_seq_frozen(P, layers, x, y, rnd, kk):
    """test_oracle_goodgan.t_seq layer by layer, with the kink layers frozen."""
    feat = None
    for i, l in enumerate(layers):
        if l[0] == 'act' and l[1] in ('relu', 'lrelu'):
            x = frozen_act(x, kk[i], 0.2 if l[1] == 'lrelu' else 0.0)
        elif l[0] == 'maxpool':
            x = frozen_pool2(x, kk[i])
        elif l[0] == 'feature':
            feat = x
        else:
            x, _ = TG.t_seq(P, [l], x, y, rnd)
    return x, feat


def perturbed(kinks, sites):
    """the net's own kinks with a few chosen decisions changed: three signs per activation, three windows per pool."""
    out = {}
    for key, kind, y in sites:
        k = np.array(kinks[key])
        where = [0, k.size // 2 + 1, k.size - 1]
        if kind == 'sign':
            k.flat[where] = ~k.flat[where]
        else:
            k.flat[where] = (k.flat[where] + 1) % (4 if kind == 'pool2' else y.shape[1] * y.shape[2])
        out[key] = k
    return out


def _cmp(G, tgrads, zero=()):
    gmax = max(np.abs(v).max() for v in tgrads.values())
    for k, ref in tgrads.items():
        sc = gmax if k in zero else np.abs(ref).max()
        assert np.abs(G[k] - ref).max() <= 1e-10 * sc, (k, np.abs(G[k] - ref).max() / sc)


D64 = np.float64


@pytest.mark.parametrize("net", ['C', 'D', 'G'])
def test_injected_kink_is_the_frozen_mask_network_cifar10(net):
    """two images; against torch float64 autograd of the network whose activations are x * where(mask, 1, slope) and whose pools gather
    at the given indices (values as in the real forward pass), masks differing from the net's own in a few chosen elements."""
    P = TN._params64(0)
    sizes = dict(SC.SIZES, L_C=2, B_G=2)
    b, rnd = SC.synth_batch(2, sizes, D64), SC.synth_rnd(1, sizes, D64)
    rng = np.random.default_rng(3)
    TP = {k: tt(v, True) for k, v in P.items()}
    if net == 'C':
        r = rnd['C']['C_real']
        logits, feat, cache = NC.classifier_fwd(P, b['x_l_c'], True, r)
        sites = K.sites_cifar('C', cache)
        kk = perturbed(K.kinks_of(sites), sites)
        dl, df = rng.standard_normal(logits.shape), rng.standard_normal(feat.shape)
        G = NC.classifier_bwd(P, NC.apply_kinks(cache, kk), dl, r, dfeat=df)
        tl, tf_ = t_classifier_frozen(TP, tt(b['x_l_c']), r, kk)
        np.testing.assert_allclose(tl.detach().numpy(), logits, rtol=1e-9, atol=1e-11)
        ((tl * tt(dl)).sum() + (tf_ * tt(df)).sum()).backward()
        zero = ()
    elif net == 'D':
        r = rnd['G']['D_fake']
        img = np.tanh(rng.standard_normal((2, 32, 32, 3)))
        logits, cache = NC.discriminator_fwd(P, img, b['y_g'], r)
        sites = K.sites_cifar('D', cache)
        kk = perturbed(K.kinks_of(sites), sites)
        dl = rng.standard_normal(logits.shape)
        G, dimg = NC.discriminator_bwd(P, NC.apply_kinks(cache, kk), dl, r, True, True)
        ti = tt(img, True)
        tl = t_discriminator_frozen(TP, ti, tt(b['y_g']), r, kk)
        np.testing.assert_allclose(tl.detach().numpy(), logits, rtol=1e-9, atol=1e-11)
        (tl * tt(dl)).sum().backward()
        assert np.abs(dimg - ti.grad.numpy()).max() <= 1e-10 * np.abs(dimg).max()
        zero = ()
    else:
        out, cache = NC.generator_fwd(P, b['z_g'], b['y_g'])
        sites = K.sites_cifar('G', cache)
        kk = perturbed(K.kinks_of(sites), sites)
        do = rng.standard_normal(out.shape)
        G = NC.generator_bwd(P, NC.apply_kinks(cache, kk), do)
        to = t_generator_frozen(TP, tt(b['z_g']), tt(b['y_g']), kk)
        np.testing.assert_allclose(to.detach().numpy(), out, rtol=1e-8, atol=1e-10)
        (to * tt(do)).sum().backward()
        zero = ()
    assert any(not np.array_equal(G[k], g0) for k, g0 in _own_grads(net, P, cache, locals()).items())     # the changed decisions do matter
    _cmp(G, {k: TP[k].grad.numpy() for k in G}, zero)


def _own_grads(net, P, cache, v):
    if net == 'C':
        return NC.classifier_bwd(P, cache, v['dl'], v['r'], dfeat=v['df'])
    if net == 'D':
        return NC.discriminator_bwd(P, cache, v['dl'], v['r'], True, True)[0]
    return NC.generator_bwd(P, cache, v['do'])


@pytest.mark.parametrize("net", ['G', 'D', 'C'])
@pytest.mark.parametrize("data", ['mnist', 'svhn'])
def test_injected_kink_is_the_frozen_mask_network_goodgan(data, net):
    P = TG.scrambled(data, 3)
    n = 2
    sizes = dict(B_G=n, L_C=n, U_C=n, L_D=1, U_D=n - 1)
    b, rnd = SG.synth_batch(data, 5, sizes, D64), SG.synth_rnd(data, 6, sizes, D64)
    if net == 'G':
        layers, x, y, r = NG.generator_layers(data), b['z_g'], b['y_g'], {}
    elif net == 'D':
        layers, x, y, r = NG.discriminator_layers(data), b['x_l_c'], b['y_l_c'], rnd['G']['D_fake']
    else:
        layers, x, y, r = NG.classifier_layers(data), b['x_l_c'], None, rnd['C']['C_real']
    out, caches, feat = NG.seq_fwd(P, layers, x, y, r, True)
    sites = K.sites_goodgan(P, layers, caches)
    kk = perturbed(K.kinks_of(sites), sites)
    rng = np.random.default_rng(7)
    do = rng.standard_normal(out.shape)
    df = rng.standard_normal(feat.shape) if feat is not None else None
    G, dx = NG.seq_bwd(P, layers, NG.apply_kinks(layers, caches, kk), do, y, r, dfeat=df)
    names = list(G)
    TP = {k: tt(v, k in names) for k, v in P.items()}
    tx = tt(x, True)
    to, tf_ = t_seq_frozen(TP, layers, tx, None if y is None else tt(y), r, kk)
    np.testing.assert_allclose(to.detach().numpy(), out, rtol=1e-8, atol=1e-10)
    loss = (to * tt(do)).sum()
    if df is not None:
        loss = loss + (tf_ * tt(df)).sum()
    loss.backward()
    if sites:
        G0, _ = NG.seq_bwd(P, layers, caches, do, y, r, dfeat=df)
        assert any(not np.array_equal(G[k], G0[k]) for k in G)
    gmax = max(np.abs(TP[k].grad.numpy()).max() for k in names)
    for k in names:
        ref = TP[k].grad.numpy()
        sc = np.abs(ref).max() if np.abs(ref).max() >= 1e-6 * gmax else gmax      # a shift in front of a batch norm: analytically zero, pure noise
        assert np.abs(G[k] - ref).max() <= 1e-10 * sc, (k, np.abs(G[k] - ref).max() / sc)
    assert np.abs(dx - tx.grad.numpy()).max() <= 1e-10 * np.abs(dx).max()


# ------------------------------------------------------------------------------------------------ the twin, the controls, the bounds
@pytest.mark.parametrize("name", list(K.CASES))
def test_float32_twin_sets_the_bound_and_every_control_exceeds_it(name):
    c, st, g = K.case(name)
    errs, out_err, residue = K.twin_errors(name)
    special = {v: b for (n, v), b in K.BOUNDS_VAR.items() if n == name}
    tw = K.worst({k: e for k, e in errs.items() if k not in special})
    bmx, bl2 = K.BOUNDS[name]
    lines = ['shapes: applications %s; %d variables, analytically zero and held to an absolute floor instead: %s'
             % (c.segs, len(errs), ', '.join(c.zero) or 'none'),
             'float32 twin (the oracle on float32 arrays, the float64 run\'s kinks injected) against float64, worst variable:',
             '  max error / max|g| %.2e   L2 error / ||g|| %.2e   (output: %.2e)' % (tw + (out_err,))]
    for k, (mx, l2) in special.items():
        lines.append('  apart from %s: twin %.2e %.2e -> 10 x that is looser than 1e-3: held to that ceiling, %.1e %.1e'
                     % ((k,) + errs[k] + (mx, l2)))
        assert errs[k][0] <= mx and errs[k][1] <= l2
    for k, r in residue.items():
        fl = K.ZERO_FLOORS[name][k]
        lines.append('  analytically zero %s: twin leaves max|g| %.2e -> floor %.1e' % (k, r, fl))
        assert 0.5 * 10 * r <= fl <= 2 * 10 * r, (k, r, fl)
    lines.append('bound = 10 x twin, rounded up: max %.1e  L2 %.1e' % (bmx, bl2))
    # the constants in kink_reference.BOUNDS follow the rule (BLAS builds differ in float32 summation order: a factor 2 either way)
    assert 0.5 * 10 * tw[0] <= bmx <= 2 * 10 * tw[0] and 0.5 * 10 * tw[1] <= bl2 <= 2 * 10 * tw[1], (tw, (bmx, bl2))
    assert bmx <= 1e-3 and bl2 <= 1e-3                       # no looser than the un-injected tests' no-flip GRAD_TOL
    ctl = K.controls(name)
    assert ctl
    lines.append('negative controls (float64 oracle against itself), smallest effect over the variables touched:')
    smallest = [np.inf, np.inf]
    for label, eff in ctl:
        mx, l2 = K.smallest_effect(eff)
        lines.append('  %-78s max %.2e  L2 %.2e  (%d of %d variables)' % (label, mx, l2, sum(e[0] > 1e-10 for e in eff.values()), len(eff)))
        assert mx >= 3 * bmx and l2 >= 3 * bl2, (label, (mx, l2), (bmx, bl2))
        smallest = [min(smallest[0], mx), min(smallest[1], l2)]
    lines.append('smallest control effect / bound: max %.0fx  L2 %.0fx' % (smallest[0] / bmx, smallest[1] / bl2))
    for k, (mx, l2) in special.items():
        assert mx <= smallest[0] / 3 * 1.01 and l2 <= smallest[1] / 3 * 1.01, (k, (mx, l2), smallest)
    write_section('float32 twin and controls, CPU: ' + name, lines)


@pytest.mark.parametrize("family", ['cifar10', 'svhn'])
def test_step_twin_sets_the_bounds_of_the_synchronised_iteration(family):
    """one iteration at the GPU test's batch sizes: every solver run of the float32 twin from the float64 run's weights, kinks and
    pseudo-labels.  The bounds of tests/test_gpu_kink_parity.py's step tests follow the same rule as the networks'."""
    tw = K.step_twin(family)
    lines = ['batch sizes %s' % (K.STEP_SIZES[family],)]
    for ph in 'DGC':
        errs, loss_err, residue = tw[ph]
        w = K.worst(errs)
        bmx, bl2, bloss = K.STEP_BOUNDS[family][ph]
        lines.append('%s-update: twin worst variable max %.2e  L2 %.2e  loss %.2e  ->  bounds %.1e %.1e, loss %.1e'
                     % ((ph,) + w + (loss_err, bmx, bl2, bloss)))
        assert 0.5 * 10 * w[0] <= bmx <= 2 * 10 * w[0] and 0.5 * 10 * w[1] <= bl2 <= 2 * 10 * w[1], (ph, w, (bmx, bl2))
        assert bmx <= 1e-3 and bl2 <= 1e-3
        want = max(K.LOSS_FLOOR, 10 * loss_err)
        assert 0.5 * want <= bloss <= 2 * want and bloss <= K.LOSS_CEILING, (ph, loss_err, bloss)
        smallest = [K.smallest_effect(eff) for _, eff in K.controls('%s/%s' % (family, ph))]
        assert bmx <= min(s[0] for s in smallest) / 3 and bl2 <= min(s[1] for s in smallest) / 3, (ph, smallest)
        for k, r in residue.items():
            fl = K.STEP_ZERO_FLOORS[family][k]
            lines.append('  analytically zero %s: twin leaves max|g| %.2e -> floor %.1e' % (k, r, fl))
            assert fl == 1e-7 if 10 * r <= 1e-7 else 0.5 * 10 * r <= fl <= 2 * 10 * r, (k, r, fl)
    write_section('float32 twin of one synchronised iteration, CPU: ' + family, lines)
