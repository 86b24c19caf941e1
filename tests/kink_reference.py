"""Kink control for whole-network gradient parity (the ordinary backward pass; tests/wgan_gp_reference.py does the same for the penalty).

The networks are full of kinks — ReLU / leaky-ReLU signs, 2x2 and global max-pool arg-max — and a float32 forward pass takes the other
branch for the handful of activations that sit closer to a kink than its rounding error.  Every such decision of the oracle's backward
pass is read from its cache, so a test can hand the oracle the decisions the implementation under test took
(oracle.nets_cifar10.apply_kinks, oracle.nets_goodgan.apply_kinks) and compare gradients behind IDENTICAL decisions: what is left is
float32 arithmetic, a 1e-5 effect (profiles/kink_parity.txt), not the 1e-2 flip budget of the un-injected tests.

A kink SITE is (key, kind, y): the oracle's cache key, 'sign' | 'pool2' | 'gpool', and the oracle's tensor the decision is taken on
(the activation output; the pre-pool tensor).  The decision rule is the oracle's own (tf_ops.maxpool2 / global_maxpool: FIRST maximum,
row-major), which is also the rule of the HIP backward kernels (csrc/elementwise.hip)."""
import contextlib

import numpy as np

from oracle import nets_cifar10 as NC
from oracle import nets_goodgan as NG
from oracle import tf_ops as T


# ------------------------------------------------------------------------------------------------ sites
def sites_cifar(net, cache):
    """forward-ordered kink sites of one application of a CIFAR-10 network ('C', 'D', 'G')."""
    out = []
    if net == 'C':
        for name, _, _ in NC.C_CONVS:
            out.append((name + '/y', 'sign', cache[name + '/y']))
            if name in NC.C_POOL_AFTER:
                out.append((name + '/pool_idx', 'pool2', cache[name + '/y']))
        for name in ('NiN1', 'NiN2'):
            out.append((name + '/y', 'sign', cache[name + '/y']))
        out.append(('gpool/idx', 'gpool', cache['NiN2/y'].reshape(cache['gpool/shape'])))
    elif net == 'D':
        out = [(name + '/y', 'sign', cache[name + '/y']) for name, _, _, _ in NC.D_CONVS]
    else:
        out = [('r%d' % i, 'sign', cache['r%d' % i]) for i in range(3)]
    return out


def sites_goodgan(P, layers, caches):
    """the same for a layer list of oracle.nets_goodgan.  The pre-pool tensor of a max-pool is the batch norm's output in front of it."""
    out = []
    for i, kind in NG.kink_sites(layers).items():
        if kind == 'sign':
            out.append((i, 'sign', caches[i]))
        else:
            assert layers[i - 1][0] == 'bn', layers[i - 1]
            name = layers[i - 1][1]
            out.append((i, 'pool2', P[name + '/gamma'] * caches[i - 1][0] + P[name + '/beta']))
    return out


def cat_sites(per_app):
    """sites of a batched call: the applications' tensors concatenated along the rows (image-major in every layout used here)."""
    return [(s[0][0], s[0][1], np.concatenate([a[2] for a in s], axis=0)) for s in zip(*per_app)]


def decide(kind, y):
    if kind == 'sign':
        return y > 0
    return (T.maxpool2(y) if kind == 'pool2' else T.global_maxpool(y))[1]


def kinks_of(sites):
    """the oracle's own kinks."""
    return {key: decide(kind, y) for key, kind, y in sites}


def kinks_from_acts(sites, acts):
    """kinks from host copies of the implementation's activations: acts[key] has the elements of the site's tensor in the same order."""
    return {key: decide(kind, np.asarray(acts[key]).reshape(y.shape)) for key, kind, y in sites}


def split_kinks(kinks, per_app):
    """kinks of a batched call -> one kink dict per application (rows in application order)."""
    out, off = [], {}
    for sites in per_app:
        k = {}
        for key, kind, y in sites:
            rows = decide(kind, y).shape[0]
            o = off.get(key, 0)
            k[key] = kinks[key][o:o + rows]
            off[key] = o + rows
        out.append(k)
    for key, o in off.items():
        assert o == kinks[key].shape[0], (key, o, kinks[key].shape)
    return out


def _windows(kind, y):
    n, h, w, c = y.shape
    if kind == 'pool2':
        return y.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4, c), 3
    return y.reshape(n, h * w, c), 1


FLIP_SHARE_CAP = 1e-3


def flips(sites, injected, act_tol):
    """Where the injected kinks differ from the oracle's own, and the oracle's distance to the kink there.  Injection must not hide a wrong
    forward pass: a sign may differ only where |y_ref| <= act_tol max|y_ref|, a pool index only where the oracle's two candidates differ by
    <= 2 act_tol max|y_ref|, and at most FLIP_SHARE_CAP of a site's decisions may differ at all.  Returns {key: (n flipped, n decisions)}."""
    out = {}
    for key, kind, y in sites:
        own, inj = decide(kind, y), np.asarray(injected[key])
        assert own.shape == inj.shape, (key, own.shape, inj.shape)
        diff = own != inj
        scale = np.abs(y).max()
        if kind == 'sign':
            dist = np.abs(y)[diff]
            lim = act_tol * scale
        else:
            v, ax = _windows(kind, y)
            take = lambda idx: np.take_along_axis(v, np.expand_dims(idx, ax), axis=ax).squeeze(ax)
            dist = (take(own) - take(inj.astype(own.dtype)))[diff]
            lim = 2 * act_tol * scale
        assert dist.size == 0 or dist.max() <= lim, ('kink moved where the oracle is not near one', key, kind, float(dist.max()), float(lim))
        assert diff.sum() <= FLIP_SHARE_CAP * diff.size, ('too many kinks moved', key, int(diff.sum()), diff.size)
        out[key] = (int(diff.sum()), int(diff.size))
    return out


# ------------------------------------------------------------------------------------------------ comparing gradients
def grad_errors(got, ref, zero=()):
    """{variable: (max error / max|g|, L2 error / ||g||)} over the variables of `ref` not named in `zero` (analytically zero gradients)."""
    out = {}
    for k, r in ref.items():
        if k in zero:
            continue
        r = np.asarray(r, np.float64)
        d = np.asarray(got[k], np.float64) - r
        out[k] = (np.abs(d).max() / np.abs(r).max(), np.linalg.norm(d) / np.linalg.norm(r))
    return out


def worst(errs):
    return max(e[0] for e in errs.values()), max(e[1] for e in errs.values())


def smallest_effect(errs):
    """smallest per-variable effect over the variables touched at all, per norm."""
    hit = [e for e in errs.values() if e[0] > 1e-10]          # float64 re-association noise (1e-16) is not an effect
    assert hit, 'the control changed no gradient'
    return min(e[0] for e in hit), min(e[1] for e in hit)


# ------------------------------------------------------------------------------------------------ negative controls
# Each is ONE single-site mistake of the kind a backward-tape bug makes, applied to the float64 oracle's backward pass `run()` (a closure
# returning {variable: gradient}) by re-routing one call of an oracle/tf_ops.py function.

@contextlib.contextmanager
def rerouted(fn_name, calls, bad):
    """inside the block the calls of tf_ops.<fn_name> whose ordinal (0-based, in execution order) is in `calls` go to bad(orig, *args)."""
    orig, n = getattr(T, fn_name), [0]

    def wrapper(*a, **kw):
        i = n[0]
        n[0] += 1
        return bad(orig, *a, **kw) if i in calls else orig(*a, **kw)
    setattr(T, fn_name, wrapper)
    try:
        yield n
    finally:
        setattr(T, fn_name, orig)


def control_slope(run, call, leaky=True):
    """(a) the activation gradient of one layer uses slope 0.21 for 0.2 (a ReLU: 0.01 for 0) — in that layer's backward only."""
    if leaky:
        with rerouted('lrelu_bwd_from_out', {call}, lambda orig, y, dy, alpha=0.2: orig(y, dy, alpha + 0.01)):
            return run()
    with rerouted('relu_bwd_from_out', {call}, lambda orig, y, dy: T.lrelu_bwd_from_out(y, dy, 0.01)):
        return run()


def control_dropout_scale(run, call):
    """(b) one dropout layer's backward applies the keep mask without the 1/keep scale."""
    with rerouted('dropout_bwd', {call}, lambda orig, dy, mask, rate: dy * mask):
        return run()


def control_mobn_joint(run, calls):
    """(c) the mean-only-BN backward of ONE layer of a two-application call (`calls`: that layer's ordinal in each application's
    backward) is centred over both applications' rows together instead of per application."""
    seen = []

    def spy(orig, dy):
        seen.append((dy.sum(axis=tuple(range(dy.ndim - 1))), dy.size // dy.shape[-1]))
        return orig(dy)
    with rerouted('mobn_train_bwd', set(calls), spy):
        run()
    mean = sum(s for s, _ in seen) / sum(c for _, c in seen)
    with rerouted('mobn_train_bwd', set(calls), lambda orig, dy: (dy - mean, orig(dy)[1])):
        return run()


def control_concat_leak(run, fn_name, call, ncls=10):
    """(d) the input gradient of one layer in front of a label concat is not cut cleanly: the label channels' gradient is added onto the
    last `ncls` channels that are kept."""
    def bad(orig, *a, **kw):
        d = np.array(orig(*a, **kw))
        c = d.shape[-1]
        d[..., c - 2 * ncls:c - ncls] += d[..., c - ncls:]
        return d
    with rerouted(fn_name, {call}, bad):
        return run()


def control_pool_routing(sites, kinks, hip_acts=None, share=0.01, seed=0):
    """(e) kinks whose pool gradients go to the LAST maximum in windows where the implementation's values tie, and otherwise to the
    second-largest element in `share` of the windows (at least one per pool)."""
    out = dict(kinks)
    rng = np.random.default_rng(seed)
    for key, kind, y in sites:
        if kind == 'sign':
            continue
        v, ax = _windows(kind, y if hip_acts is None else np.asarray(hip_acts[key]).reshape(y.shape))
        idx = np.array(kinks[key])
        last = v.shape[ax] - 1 - np.flip(v, ax).argmax(axis=ax)
        second = np.argsort(v, axis=ax, kind='stable').take(-2, axis=ax)
        pick = rng.random(idx.shape) < share
        pick.flat[rng.integers(pick.size)] = True
        out[key] = np.where(last != idx, last, np.where(pick, second, idx))
    return out


# ------------------------------------------------------------------------------------------------ float32 twin
def cast(d, dtype):
    if isinstance(d, dict):
        return {k: cast(v, dtype) for k, v in d.items()}
    return None if d is None else np.asarray(d, dtype)


# ------------------------------------------------------------------------------------------------ the cases both test files run
class Case(object):
    """One network at the shapes of tests/test_gpu_kink_parity.py: float32-representable parameters, inputs, randomness and gradient seeds,
    and the oracle's forward / backward over its applications in a chosen dtype.  forward() -> state; sites(state) -> per-application site
    lists; backward(state, kinks) -> {variable: gradient summed over the applications} (+ 'd_input' where an input gradient is asked)."""
    zero = ()

    def run(self, dtype=np.float64, kinks=None):
        st = self.forward(dtype)
        return st, self.backward(st, kinks)


class CifarC(Case):
    name, net, segs, act_tol = 'cifar10/C', 'C', [3, 2], 1e-4
    zero = ()     # NiN2/b, analytically 0 under dlogits alone (tests/test_gpu_step.py), is not under the feature seed this case adds

    def __init__(self):
        from test_gpu_nets import scrambled_params
        from oracle import step_cifar10 as S
        self.P = scrambled_params(0)
        sizes = dict(S.SIZES, L_C=3, U_C=2)
        rnd, b = S.synth_rnd(1, sizes), S.synth_batch(2, sizes)
        self.rnd, self.x = [rnd['C']['C_real'], rnd['C']['C_unl']], [b['x_l_c'], b['x_u_c']]
        rng = np.random.default_rng(3)
        self.dl, self.df = rng.standard_normal((5, 10)).astype(np.float32), rng.standard_normal((5, 128)).astype(np.float32)

    def forward(self, dtype):
        P, pops, apps = cast(self.P, dtype), {}, []
        for x, r in zip(self.x, self.rnd):
            apps.append(NC.classifier_fwd(P, x.astype(dtype), True, cast(r, dtype), pops))
        return dict(P=P, apps=apps, dtype=dtype, out=np.concatenate([a[0] for a in apps]), feat=np.concatenate([a[1] for a in apps]))

    def sites(self, st):
        return [sites_cifar('C', a[2]) for a in st['apps']]

    def backward(self, st, kinks=None, dfeat=True):
        G, o = {}, 0
        for i, (a, r) in enumerate(zip(st['apps'], self.rnd)):
            n = a[0].shape[0]
            c = a[2] if kinks is None else NC.apply_kinks(a[2], kinks[i])
            g = NC.classifier_bwd(st['P'], c, self.dl[o:o + n].astype(st['dtype']), cast(r, st['dtype']),
                                  dfeat=self.df[o:o + n].astype(st['dtype']) if dfeat else None)
            o += n
            for k, v in g.items():
                G[k] = G.get(k, 0) + v
        return G


class CifarD(Case):
    name, net, segs, act_tol = 'cifar10/D', 'D', [2, 3, 2], 1e-4

    def __init__(self):
        from test_gpu_nets import scrambled_params
        from oracle import step_cifar10 as S
        self.P = scrambled_params(0)
        rng = np.random.default_rng(8)
        self.rnd = [S.synth_rnd(7 + i, dict(S.SIZES, B_G=n))['G']['D_fake'] for i, n in enumerate(self.segs)]
        self.y = [np.eye(10, dtype=np.float32)[rng.integers(0, 10, n)] for n in self.segs]
        self.x = [np.tanh(rng.standard_normal((n, 32, 32, 3))).astype(np.float32) for n in self.segs]
        self.dl = rng.standard_normal((7, 1)).astype(np.float32)

    def forward(self, dtype):
        P = cast(self.P, dtype)
        apps = [NC.discriminator_fwd(P, x.astype(dtype), y.astype(dtype), cast(r, dtype)) for x, y, r in zip(self.x, self.y, self.rnd)]
        return dict(P=P, apps=apps, dtype=dtype, out=np.concatenate([a[0] for a in apps]))

    def sites(self, st):
        return [sites_cifar('D', a[1]) for a in st['apps']]

    def backward(self, st, kinks=None):
        G, o = {}, 0
        for i, (a, r) in enumerate(zip(st['apps'], self.rnd)):
            n = a[0].shape[0]
            c = a[1] if kinks is None else NC.apply_kinks(a[1], kinks[i])
            g, dimg = NC.discriminator_bwd(st['P'], c, self.dl[o:o + n].astype(st['dtype']), cast(r, st['dtype']), True, i == 1)
            o += n
            for k, v in g.items():
                G[k] = G.get(k, 0) + v
            if i == 1:
                G['d_input'] = dimg          # the fake rows' image gradient (what the G-update takes from D)
        return G


class CifarG(Case):
    name, net, segs, act_tol = 'cifar10/G', 'G', [6], 1e-4

    def __init__(self):
        from test_gpu_nets import scrambled_params
        from oracle import step_cifar10 as S
        self.P = scrambled_params(0)
        b = S.synth_batch(4, dict(S.SIZES, B_G=6))
        self.z, self.y, self.rnd = b['z_g'], b['y_g'], [{}]
        self.do = np.random.default_rng(5).standard_normal((6, 32, 32, 3)).astype(np.float32)

    def forward(self, dtype):
        P = cast(self.P, dtype)
        out, c = NC.generator_fwd(P, self.z.astype(dtype), self.y.astype(dtype))
        return dict(P=P, apps=[(out, c)], dtype=dtype, out=out)

    def sites(self, st):
        return [sites_cifar('G', st['apps'][0][1])]

    def backward(self, st, kinks=None):
        c = st['apps'][0][1]
        return NC.generator_bwd(st['P'], c if kinks is None else NC.apply_kinks(c, kinks[0]), self.do.astype(st['dtype']))


class GoodganNet(Case):
    """G, D (one application of 5 images) or C (two applications [3, 2]: its batch norms take per-application statistics) of the MNIST /
    SVHN models, parameters as tests/test_gpu_goodgan.py scrambles them."""
    act_tol = 2e-4

    def __init__(self, data, net):
        from test_oracle_goodgan import scrambled
        from oracle import step_goodgan as S
        self.name, self.data, self.net = '%s/%s' % (data, net), data, net
        self.P = {k: v.astype(np.float32) for k, v in scrambled(data, 3).items()}
        self.segs = [3, 2] if net == 'C' else [5]
        sizes = dict(B_G=5, L_C=3, U_C=2, L_D=1, U_D=4)
        b, rnd = S.synth_batch(data, 5, sizes), S.synth_rnd(data, 6, sizes)
        rng = np.random.default_rng(7)
        if net == 'G':
            self.layers, self.x, self.y, self.rnd = NG.generator_layers(data), [b['z_g']], [b['y_g']], [{}]
        elif net == 'D':
            self.layers, self.rnd = NG.discriminator_layers(data), [rnd['G']['D_fake']]
            self.x, self.y = [np.concatenate([b['x_l_c'], b['x_u_c']])], [b['y_g']]
        else:
            self.layers, self.x, self.y = NG.classifier_layers(data), [b['x_l_c'], b['x_u_c']], [None, None]
            self.rnd = [rnd['C']['C_real'], rnd['C']['C_unl']]
            # a shift in front of a batch norm with only linear maps in between (tests/test_gpu_goodgan.py ANALYTIC_ZERO; MNIST's last
            # hidden batch norm is c_h2_bn1): |g| < 1e-9 max|g| in the exact float64 oracle, asserted in tests/test_kink_reference.py
            self.zero = ('classifier/c_h2_bn%d/beta' % (1 if data == 'mnist' else 2), 'classifier/c_h2_lin/c_h2_lin/bias')
        st = self.forward(np.float64)
        self.do = rng.standard_normal(st['out'].shape).astype(np.float32)
        self.df = None                                # the feature seed is the CIFAR-10 classifier's case

    def forward(self, dtype):
        P, bnu, apps = cast(self.P, dtype), {}, []
        for x, y, r in zip(self.x, self.y, self.rnd):
            apps.append(NG.seq_fwd(P, self.layers, x.astype(dtype), None if y is None else y.astype(dtype), cast(r, dtype), True, bnu))
        st = dict(P=P, apps=apps, dtype=dtype, out=np.concatenate([a[0] for a in apps]), bnu=bnu)
        if self.net == 'C':
            st['feat'] = np.concatenate([a[2] for a in apps])
        return st

    def sites(self, st):
        return [sites_goodgan(st['P'], self.layers, a[1]) for a in st['apps']]

    def backward(self, st, kinks=None, dfeat=True):
        G, o, dt = {}, 0, st['dtype']
        for i, (a, y, r) in enumerate(zip(st['apps'], self.y, self.rnd)):
            n = a[0].shape[0]
            c = a[1] if kinks is None else NG.apply_kinks(self.layers, a[1], kinks[i])
            df = self.df[o:o + n].astype(dt) if (self.df is not None and dfeat) else None
            g, dx = NG.seq_bwd(st['P'], self.layers, c, self.do[o:o + n].astype(dt), None if y is None else y.astype(dt), cast(r, dt), dfeat=df)
            o += n
            for k, v in g.items():
                G[k] = G.get(k, 0) + v
            if self.net == 'D':
                G['d_input'] = dx
        return G


# (max error / max|g|, L2 error / ||g||) per variable, HIP float32 against the float64 oracle with the HIP path's kinks injected.
# Each is 10 x the worst per-variable error of the network's float32 twin at these shapes (twin_errors; the margin of 10 is for summation
# order: NumPy sums pairwise, the MFMA chains and split-K partials sequentially), rounded up to two digits.  tests/test_kink_reference.py
# re-measures the twin and the negative controls and holds every entry to: at most a third of the network's smallest control effect, and
# no looser than 1e-3.  profiles/kink_parity.txt has the numbers.  Nothing here comes from what the HIP path produces.
BOUNDS = {
    'cifar10/C': (7.3e-5, 6.0e-5), 'cifar10/D': (1.1e-5, 7.3e-6), 'cifar10/G': (2.4e-4, 2.3e-4),
    'mnist/G': (5.6e-5, 4.2e-5), 'mnist/D': (4.4e-5, 4.4e-5), 'mnist/C': (3.2e-4, 1.9e-4),
    'svhn/G': (6.3e-5, 4.5e-5), 'svhn/D': (1.3e-5, 1.1e-5), 'svhn/C': (5.4e-4, 3.5e-4),
}
# The one variable the twin cannot hold with the margin of 10: the MNIST generator's first bias sits in front of softplus -> batch norm,
# which removes nearly all of a shift — its gradient (7.7e-2, beside 16 for the kernel of the same layer) is what is left of a cancelling
# sum, and the float32 twin is off by 8.9e-4 / 1.8e-4 there (5.5e-6 for every other variable of that network, which BOUNDS['mnist/G'] is
# taken from).  10 x that would be looser than 1e-3, the no-flip GRAD_TOL of the un-injected tests, so this variable is held to exactly
# that ceiling — far below a third of the network's smallest control effect (7e-2 / 2e-2), which is all the rule would ask here.
BOUNDS_VAR = {('mnist/G', 'good_generator/gg_h0_lin/gg_h0_lin/bias'): (1e-3, 1e-3)}
# Gradients that are analytically 0 (Case.zero) have no relative error: max|g_hip| is held to 10 x the residue the float32 twin leaves
# there.  (tests/test_gpu_step.py's absolute 1e-7 belongs to its gradient scale: loss means over the batch.  These cases seed unit-normal
# dlogits, their largest gradients are 23 .. 125, and the residue of a cancelling float32 sum scales with its terms.)
ZERO_FLOORS = {
    'mnist/C': {'classifier/c_h2_bn1/beta': 1.6e-4, 'classifier/c_h2_lin/c_h2_lin/bias': 1.2e-3},
    'svhn/C': {'classifier/c_h2_bn2/beta': 2.1e-5, 'classifier/c_h2_lin/c_h2_lin/bias': 1.4e-4},
}


def bound(name, var):
    return BOUNDS_VAR.get((name, var), BOUNDS[name])


CASES = {'cifar10/C': CifarC, 'cifar10/D': CifarD, 'cifar10/G': CifarG}
for _d in ('mnist', 'svhn'):
    for _n in ('G', 'D', 'C'):
        CASES['%s/%s' % (_d, _n)] = (lambda d, n: (lambda: GoodganNet(d, n)))(_d, _n)

_CACHE = {}


def case(name):
    """the case with its float64 reference run, computed once per process and left unchanged."""
    if name not in _CACHE:
        c = CASES[name]()
        st, g = c.run(np.float64)
        _CACHE[name] = (c, st, g)
    return _CACHE[name]


def twin_errors(name):
    """the float32 twin: the same oracle functions on float32 arrays with the float64 run's kinks injected, against float64."""
    c, st, g = case(name)
    own = [kinks_of(s) for s in c.sites(st)]
    st32, g32 = c.run(np.float32, own)
    residue = {k: float(np.abs(g32[k]).max()) for k in c.zero}
    return grad_errors(g32, g, c.zero), abs(float(np.abs(st32['out'] - st['out']).max()) / float(np.abs(st['out']).max())), residue


def controls(name):
    """[(label, {variable: (max, L2) effect})]: the negative controls that apply to the case, each against the float64 reference."""
    c, st, g = case(name)
    run = lambda: c.backward(st)
    per_app = c.sites(st)
    own = [kinks_of(s) for s in per_app]
    leaky = any(l[0] == 'act' and l[1] == 'lrelu' for l in getattr(c, 'layers', ())) or c.net in ('C', 'D')
    has_act = bool(per_app[0])
    out = []
    if has_act and any(k == 'sign' for _, k, _ in per_app[0]):
        out.append(('(a) one layer\'s activation slope +0.01 in backward', control_slope(run, 2, leaky)))
    if any('drop' in k for k in c.rnd[0]):
        out.append(('(b) one dropout backward without its scale', control_dropout_scale(run, 1 if name.endswith('/D') else 0)))
    if name == 'cifar10/C':
        out.append(('(c) mean-only-BN backward of one layer centred over both applications', control_mobn_joint(run, (4, 14))))
        out.append(('(f) the feature seed dropped (dfeat)', c.backward(st, dfeat=False)))
    leak = {'cifar10/D': ('conv2d_bwd_input', 1), 'svhn/D': ('conv2d_bwd_input', 1), 'cifar10/G': ('conv2d_transpose_bwd_input', 1),
            'svhn/G': ('conv2d_transpose_bwd_input', 1), 'mnist/G': ('matmul', 3), 'mnist/D': ('matmul', 3)}.get(name)
    if leak:
        out.append(('(d) one concat gradient not cut: label channels leak into dx', control_concat_leak(run, *leak)))
    if any(k != 'sign' for _, k, _ in per_app[0]):
        bad = [control_pool_routing(s, k, seed=i) for i, (s, k) in enumerate(zip(per_app, own))]
        out.append(('(e) pool gradient to the second-largest element in 1 % of windows', c.backward(st, bad)))
    return [(label, grad_errors(gb, g, c.zero)) for label, gb in out]


# ------------------------------------------------------------------------------------------------ one phase-synchronised iteration
STEP_SIZES = {'cifar10': dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6), 'svhn': dict(B_G=6, L_C=4, U_C=4, L_D=2, U_D=4)}
STEP_NETS = {'D': 'discriminator', 'G': 'good_generator', 'C': 'classifier'}
STEP_ZERO = {'cifar10': ('classifier/NiN2/NiN2/b',),                                    # tests/test_gpu_step.py
             'svhn': ('classifier/c_h2_bn2/beta', 'classifier/c_h2_lin/c_h2_lin/bias')}     # tests/test_gpu_goodgan.py ANALYTIC_ZERO
# 10 x the float32 twin of each solver run at STEP_SIZES (step_twin; tests/test_kink_reference.py holds them to the rule, to a third of
# the networks' smallest control effect and to 1e-3), as BOUNDS above; the third entry is the loss (relative to max(1, |loss|), ceiling
# tests/test_gpu_step.py LOSS_TOL = 2e-4).
# The loss is never held tighter than LOSS_FLOOR: it comes back as ONE float32 (2^-24 = 6e-8 relative for the value alone) reduced from
# at most 20 float32 log-sum-exp terms, ~16 roundings = 1e-6; the twin's own loss error (2e-10 .. 2e-7) is below what the format can show.
LOSS_FLOOR, LOSS_CEILING = 1e-6, 2e-4
STEP_BOUNDS = {
    'cifar10': {'D': (1.9e-4, 1.4e-4, 1e-6), 'G': (2.3e-4, 2.0e-4, 1e-6), 'C': (6.6e-5, 7.3e-5, 1.6e-6)},
    'svhn': {'D': (2.1e-4, 1.9e-4, 1e-6), 'G': (3.1e-4, 1.4e-4, 1e-6), 'C': (9.3e-5, 9.6e-5, 1e-6)},
}
# analytically zero gradients of the C-update: the absolute 1e-7 of tests/test_gpu_step.py, or 10 x the twin's residue where that is larger
STEP_ZERO_FLOORS = {'cifar10': {'classifier/NiN2/NiN2/b': 1e-7},
                    'svhn': {'classifier/c_h2_bn2/beta': 1.9e-6, 'classifier/c_h2_lin/c_h2_lin/bias': 1.4e-5}}


class Step(object):
    """One Triple-GAN iteration (D-, G-, C-update) of a model family on float32-representable weights, batch and randomness, phase by phase
    through the step oracle in a chosen dtype, with the hooks of oracle/step_*.py: kinks(key, sites) -> kink dict, labels."""

    def __init__(self, family):
        self.family, self.sizes = family, STEP_SIZES[family]
        if family == 'cifar10':
            from oracle import step_cifar10 as S
            self.S, full = S, dict(S.SIZES, **self.sizes)
            self.P = S.init_params(0)
            self.batch, self.rnd = S.synth_batch(100, full), S.synth_rnd(200, full)
            self.hyper = dict(lr=3e-4, cla_lr=3e-3, beta1=0.5, lambda_1=0.3, lambda_2=0.5)
            self.zca = S.synth_zca()
            self.act_tol = 1e-4
        else:
            from oracle import step_goodgan as S
            from test_oracle_goodgan import scrambled
            self.S = S
            self.P = {k: v.astype(np.float32) for k, v in scrambled(family, 11).items()}
            self.batch, self.rnd = S.synth_batch(family, 21, self.sizes), S.synth_rnd(family, 22, self.sizes)
            self.hyper = dict(lr=1e-3, cla_lr=3e-4, beta1=0.5, lambda_1=0.1, lambda_2=0.0)
            self.act_tol = 2e-4
        s = self.sizes
        # application key -> (first row, rows, rows of the batched call) in the HIP path's batching order (gpu_common.injected_arrays*)
        nd = s['L_D'] + s['U_D'] + s['B_G'] + s['U_C']
        self.rows = {'D': {'D_real': (0, s['L_D'] + s['U_D'], nd), 'D_fake': (s['L_D'] + s['U_D'], s['B_G'], nd),
                           'D_unl': (s['L_D'] + s['U_D'] + s['B_G'], s['U_C'], nd)},
                     'G': {'D_fake': (0, s['B_G'], s['B_G']), 'G': (0, s['B_G'], s['B_G'])}}
        keys = ['C_real', 'C_unl'] + (['C_unl_rep'] if family == 'cifar10' else []) + ['C_fake']
        ns = [s['L_C'], s['U_C']] + ([s['U_C']] if family == 'cifar10' else []) + [s['B_G']]
        self.rows['C'] = {k: (sum(ns[:i]), n, sum(ns)) for i, (k, n) in enumerate(zip(keys, ns))}

    def new_state(self, dtype):
        return self.S.new_state(cast(self.P, dtype))

    def sites(self, st, key, *cache):
        """kink sites of application `key` from what the oracle's hook is handed (a cache; or layers, caches)."""
        net = 'G' if key == 'G' else key[0]
        if self.family == 'cifar10':
            return sites_cifar(net, cache[0])
        return sites_goodgan(st['P'], cache[0], cache[1])

    def phase(self, st, ph, dtype, kinks=None, labels=None):
        """runs solver run `ph` on `st` -> loss.  kinks: callable (key, sites) -> kink dict."""
        S, b, r = self.S, cast(self.batch, dtype), cast(self.rnd[ph], dtype)
        hook = None if kinks is None else (lambda key, *cache: kinks(key, self.sites(st, key, *cache)))
        kw = dict(kinks=hook) if ph == 'G' else dict(kinks=hook, labels=labels)
        if self.family == 'cifar10':
            z = tuple(np.asarray(a, dtype) for a in self.zca)
            return {'D': lambda: S.d_phase(st, b, r, self.hyper, z, **kw), 'G': lambda: S.g_phase(st, b, r, self.hyper, **kw),
                    'C': lambda: S.c_phase(st, b, r, self.hyper, z, **kw)}[ph]()
        return getattr(S, ph.lower() + '_phase')(st, self.family, b, r, self.hyper, **kw)


def step_twin(family):
    """{phase: (per-variable errors, loss error, residue on the analytically zero variables)} of the float32 twin: every solver run from
    the float64 run's weights, with its kinks and pseudo-labels injected."""
    from oracle import tf_ops
    c = Step(family)
    st64, st32 = c.new_state(np.float64), c.new_state(np.float32)
    out = {}
    for ph in 'DGC':
        rec = {}

        def own(key, sites):
            rec[key] = kinks_of(sites)
            return rec[key]
        l64 = c.phase(st64, ph, np.float64, own)
        labels = None if ph == 'G' else {k: tf_ops.argmax_onehot(v) for k, v in st64['last_logits'].items()}
        l32 = c.phase(st32, ph, np.float32, lambda key, sites: rec[key], labels)
        g64, g32 = st64['last_grads'][ph], st32['last_grads'][ph]
        zero = STEP_ZERO[family] if ph == 'C' else ()
        out[ph] = (grad_errors(g32, g64, zero), abs(l32 - l64) / max(1.0, abs(l64)), {k: float(np.abs(g32[k]).max()) for k in zero})
        for k in ('P', 'm', 'v', 'ema'):                       # the next solver run starts from identical weights on both sides
            st32[k] = cast(st64[k], np.float32)
    return out
