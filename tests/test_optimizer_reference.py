"""CPU checks behind config.OPTIMIZER: the float64 restatement of momentum SGD and RMSProp (tests/optimizer_reference.py)
against torch-CPU and in closed form; the bounds of the GPU kernel tests shown to hold for a correctly rounded fp32 implementation and
to fail by more than 10x for the three wrong forms, on the very inputs the GPU test uses; check_optimizer; and the checkpoint key
sets, cross-optimiser refusal and slot initialisation on host ParamStores."""
import numpy as np
import pytest
import torch

import optimizer_reference as R


def _torch_run(make_opt, p0, grads, seed_state=None):
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = make_opt([p])
    if seed_state is not None:
        p.grad = torch.zeros_like(p)
        opt.step()                                   # a zero-gradient step creates the state and moves nothing
        assert torch.equal(p.detach(), torch.tensor(p0, dtype=torch.float64))
        for k, v in seed_state.items():
            opt.state[p][k].copy_(torch.tensor(v, dtype=torch.float64))
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
    return p.detach().numpy()


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_momentum_equals_torch_sgd_over_five_steps():
    rng = np.random.default_rng(0)
    p0, grads = rng.standard_normal(257), [rng.standard_normal(257) for _ in range(5)]
    for lr, mu in ((3e-4, 0.9), (0.1, 0.5)):
        want = _torch_run(lambda ps: torch.optim.SGD(ps, lr=lr, momentum=mu, dampening=0, nesterov=False), p0, grads)
        p, accum = p0, np.zeros(257)
        for g in grads:
            p, accum = R.momentum_step(p, g, accum, lr, mu)
        assert _rel(p - p0, want - p0) <= 1e-12 and _rel(p, want) <= 1e-12
        pn, an = p0, np.zeros(257)
        for g in grads:
            pn, an = R.momentum_step(pn, g, an, lr, mu, nesterov=True)
        assert _rel(pn - p0, want - p0) > 0.1                  # the flag computes something else


def test_rmsprop_equals_torch_when_the_forms_coincide():
    """epsilon = 0 and rms0 = 0 remove both differences between TensorFlow's form and torch's (no gradient element is zero: 0/0)."""
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal(257)
    grads = [rng.standard_normal(257) for _ in range(5)]
    assert all(np.all(g != 0) for g in grads)
    want = _torch_run(lambda ps: torch.optim.RMSprop(ps, lr=3e-4, alpha=0.9, eps=0, momentum=0), p0, grads)
    p, ms, mom = p0, np.zeros(257), np.zeros(257)
    for g in grads:
        p, ms, mom = R.rmsprop_step(p, g, ms, mom, 3e-4, decay=0.9, momentum=0.0, epsilon=0.0)
    assert _rel(p - p0, want - p0) <= 1e-12 and _rel(p, want) <= 1e-12


def test_rmsprop_tf_defaults_differ_from_torch_defaults():
    rng = np.random.default_rng(2)
    p0 = rng.standard_normal(64)
    # (a) rms0 = 1 against torch's square_avg = 0, ordinary gradients: the first step is lr*g/sqrt(.9 + .1 g^2) against lr*sqrt(10)*sign(g)
    g = rng.standard_normal(64)
    want = _torch_run(lambda ps: torch.optim.RMSprop(ps, lr=3e-4, alpha=0.9, eps=1e-10, momentum=0), p0, [g])
    p, _, _ = R.rmsprop_step(p0, g, np.ones(64), np.zeros(64), 3e-4)
    assert _rel(p - p0, want - p0) > 0.5
    # (b) the same slot value on both sides, ms near 1e-10 = epsilon, g*g << ms: sqrt(ms + eps) = 1.4e-5 against sqrt(ms) + eps = 1e-5
    g = rng.standard_normal(64) * 1e-7
    ms0 = np.full(64, 1e-10 / 0.9)
    want = _torch_run(lambda ps: torch.optim.RMSprop(ps, lr=3e-4, alpha=0.9, eps=1e-10, momentum=0), p0, [g], seed_state=dict(square_avg=ms0))
    p, ms, _ = R.rmsprop_step(p0, g, ms0, np.zeros(64), 3e-4)
    assert np.all(np.abs(ms - 1e-10) < 1e-13)
    assert 0.25 < _rel(p - p0, want - p0) < 0.35               # 1 - 1/sqrt(2) = 0.293
    po, _, _ = R.rmsprop_step(p0, g, ms0, np.zeros(64), 3e-4, eps_outside=True)
    assert _rel(po - p0, want - p0) <= 1e-9                    # and eps_outside is torch's form


def test_closed_form_single_steps():
    p, accum = R.momentum_step(1.0, 2.0, 0.5, 0.1, 0.9)
    assert abs(accum - 2.45) <= 1e-15 and abs(p - 0.755) <= 1e-15
    p, ms, mom = R.rmsprop_step(1.0, 2.0, 1.0, 0.0, 0.1, decay=0.9, momentum=0.0, epsilon=0.0)
    assert abs(ms - 1.3) <= 1e-15 and abs(mom - 0.2 / np.sqrt(1.3)) <= 1e-15 and abs(p - (1 - 0.2 / np.sqrt(1.3))) <= 1e-15
    p, ms, mom = R.rmsprop_step(1.0, 3.0, 0.0, 0.25, 0.1, decay=0.5, momentum=0.5, epsilon=4.0 - 4.5)
    assert ms == 4.5 and abs(mom - (0.125 + 0.3 / 2.0)) <= 1e-15 and abs(p - (1 - 0.275)) <= 1e-15       # sqrt(4.5 - 0.5) = 2: eps is inside


# ---- the GPU kernel test's bounds, on its inputs, for a correctly rounded fp32 implementation and for the wrong forms -------------------
def _miss(kind, case, got, **variant):
    ref = R.run_reference(kind, case, **variant)
    return np.abs(got['p'].astype(np.float64) - ref['p']).max() / R.param_bound(ref, R.STEPS), ref


@pytest.mark.parametrize("kind", ['momentum', 'rmsprop', 'rmsprop_small', 'rmsprop_mom'])
def test_fp32_emulation_meets_the_kernel_bounds(kind):
    base = 'momentum' if kind == 'momentum' else 'rmsprop'
    case = R.kernel_case(kind)
    got = R.run_f32(base, case)
    miss, ref = _miss(base, case, got)
    print(kind, 'parameter error / bound', miss)
    assert miss <= 1.0
    if base == 'momentum':
        assert R.slots_close(got['accum'], ref['accum']) <= 1.0
    else:
        assert R.slots_close(got['rms'], ref['rms']) <= 1.0
        # with momentum != 0 the sum mom*momentum + x can cancel: bounded against the largest slot value, like the parameter
        atol = R.SLOT_ATOL if kind != 'rmsprop_mom' else 1e-6 * np.abs(ref['mom']).max() * R.STEPS
        assert R.slots_close(got['mom'], ref['mom'], atol) <= 1.0


def test_negative_controls_miss_the_parameter_bound_by_more_than_10x():
    case = R.kernel_case('rmsprop_small')
    got = R.run_f32('rmsprop', case)
    assert _miss('rmsprop', case, got, eps_outside=True)[0] > 10.0
    case = R.kernel_case('rmsprop')
    got = R.run_f32('rmsprop', case)
    assert _miss('rmsprop', case, got, rms0=0.0)[0] > 10.0
    case = R.kernel_case('momentum')
    got = R.run_f32('momentum', case)
    assert _miss('momentum', case, got, nesterov=True)[0] > 10.0


# ---- check_optimizer ---------------------------------------------------------------------------------------------------------------------
def test_check_optimizer():
    from config import Config
    from Training.Train_goodGAN import check_optimizer

    class Cfg(Config):
        BATCH_SIZE = 1

    c = Cfg()
    assert Config.OPTIMIZER == 'adam' and Config.MOMENTUM == 0.9
    assert check_optimizer(c) == ('adam', 'adam', 'adam')
    assert check_optimizer(object()) == ('adam', 'adam', 'adam')              # no attribute: the default
    c.OPTIMIZER = 'rmsprop'
    assert check_optimizer(c) == ('rmsprop',) * 3
    c.OPTIMIZER = ('rmsprop', 'adam', 'momentum')
    assert check_optimizer(c) == ('rmsprop', 'adam', 'momentum')
    c.OPTIMIZER = ['momentum', 'momentum', 'adam']
    assert check_optimizer(c) == ('momentum', 'momentum', 'adam')
    for bad in ('sgd', 'Adam', '', ('adam', 'adam'), ('adam',) * 4, (), ('adam', 'adam', 'nesterov'), ('adam', 'adam', None), None, 3):
        c.OPTIMIZER = bad
        with pytest.raises(ValueError, match='OPTIMIZER'):
            check_optimizer(c)


def test_optimizer_flag_flows_through_customize_config():
    from config import Config
    from Training.Train_goodGAN import _customize_config, check_optimizer

    class Cfg(Config):
        BATCH_SIZE = 1

    class Flags(object):
        optimizer = 'rmsprop'
        momentum = None

    c = Cfg()
    _customize_config(c, Flags())
    assert check_optimizer(c) == ('rmsprop',) * 3 and c.MOMENTUM == 0.9


# ---- checkpoints and slot initialisation on host stores ---------------------------------------------------------------------------------
SPECS = {'discriminator': [('discriminator/a/kernel', (3, 5), True), ('discriminator/a/bias', (5,), True)],
         'good_generator': [('good_generator/b/kernel', (4, 4), True), ('good_generator/b/moving_mean', (4,), False)],
         'classifier': [('classifier/c/V', (2, 3), True), ('classifier/c/pop_mean', (3,), False)]}
SUFFIXES = {'adam': ['/Adam_optimizer', '/Adam_optimizer_1'], 'momentum': ['/Momentum'],
            'rmsprop': ['/RMSProp_optimizer', '/RMSProp_optimizer_1']}


def _stores(kinds, seed=0):
    from tg.runtime import ParamStore
    from Training.train_base import Train_base
    tb = Train_base()
    lr = torch.zeros(1)
    make = {'adam': lambda: tb._Adam_optimizer(lr, 0.5), 'momentum': lambda: tb._SGD_w_Momentum_optimizer(lr, 0.9),
            'rmsprop': lambda: tb._RMSProp_optimizer(lr)}
    rng = np.random.default_rng(seed)
    stores = {}
    for (net, specs), kind in zip(SPECS.items(), kinds):
        st = stores[net] = ParamStore(net, specs, 'cpu')
        if net == 'classifier':
            st.enable_ema()
        make[kind]().bind(st)
        for buf in (st.p, st.s) + ((st.m, st.v) if seed else ()):
            buf.copy_(torch.from_numpy(rng.standard_normal(buf.numel()).astype(np.float32)))
    return stores


def _expected_keys(kinds):
    keys = {'tg/epoch'}
    for (net, specs), kind in zip(SPECS.items(), kinds):
        keys.add('tg/adam_step/' + net)
        for nm, _shape, trainable in specs:
            keys.add(nm)
            if trainable:
                keys |= {nm + s for s in SUFFIXES[kind]}
                if net == 'classifier':
                    keys.add(nm + '/ExponentialMovingAverage')
    return keys


@pytest.mark.parametrize("kinds", [('adam',) * 3, ('rmsprop',) * 3, ('momentum',) * 3, ('rmsprop', 'adam', 'momentum')])
def test_state_dict_keys_follow_each_networks_optimizer(kinds):
    from Training.Saver import load_state_dict, state_dict
    a = _stores(kinds, seed=5)
    d = state_dict(a, epoch=4)
    assert set(d) == _expected_keys(kinds)
    b = _stores(kinds, seed=6)
    assert load_state_dict(b, d) == []
    for net, kind in zip(SPECS, kinds):
        for nm, _shape, trainable in SPECS[net]:                       # (variable by variable: the padding between them is not stored)
            for which in ('value',) + ((('m', 'v') if kind != 'momentum' else ('m',)) if trainable else ()):
                assert np.array_equal(a[net].get(nm, which), b[net].get(nm, which)), (nm, which)
    # which buffer goes under which name
    da = a['discriminator']
    nm = 'discriminator/a/kernel'
    if kinds[0] == 'rmsprop':
        assert np.array_equal(d[nm + '/RMSProp_optimizer'], da.get(nm, 'v')) and np.array_equal(d[nm + '/RMSProp_optimizer_1'], da.get(nm, 'm'))
    if kinds[0] == 'momentum':
        assert np.array_equal(d[nm + '/Momentum'], da.get(nm, 'm'))


def test_restore_across_optimizers_raises_and_fills_nothing():
    from Training.Saver import load_state_dict, state_dict
    d = state_dict(_stores(('rmsprop', 'adam', 'adam'), seed=5))
    b = _stores(('adam', 'adam', 'adam'), seed=6)
    before = {k: getattr(b['discriminator'], k).clone() for k in 'pmv'}
    for strict in (True, False):
        with pytest.raises(KeyError) as e:
            load_state_dict(b, d, strict=strict)
        msg = str(e.value)
        assert 'discriminator' in msg and 'rmsprop' in msg and 'adam' in msg
    for k, v in before.items():
        assert torch.equal(getattr(b['discriminator'], k), v), k
    d = state_dict(_stores(('adam', 'adam', 'momentum'), seed=5))
    with pytest.raises(KeyError) as e:
        load_state_dict(_stores(('adam', 'adam', 'rmsprop'), seed=6), d)
    assert 'classifier' in str(e.value) and 'momentum' in str(e.value) and 'rmsprop' in str(e.value)


def test_rms_slot_is_one_wherever_it_comes_to_exist():
    from tg.runtime import ParamStore
    from Training.Saver import load_state_dict, state_dict
    from Training.train_base import Train_base
    st = _stores(('rmsprop', 'momentum', 'adam'))
    d, g, c = st['discriminator'], st['good_generator'], st['classifier']
    assert d.optimizer == 'rmsprop' and g.optimizer == 'momentum' and c.optimizer == 'adam'
    assert torch.all(d.v == 1) and not d.m.any() and not g.m.any() and not g.v.any() and not c.v.any() and not c.m.any()
    # a store that grows (Context.get_variable): inside its reserve, then beyond it (re-allocation)
    s = ParamStore('discriminator', [], 'cpu', capacity=64)
    Train_base()._RMSProp_optimizer(torch.zeros(1)).bind(s)
    s.extend([('discriminator/x', (40,), True)])
    assert s.v.numel() == 64 and torch.all(s.v == 1) and not s.m.any()
    s.v[:40].fill_(0.25)
    s.extend([('discriminator/y', (1000,), True)])
    assert s.n_p == 64 + 1024 and torch.all(s.v[:40] == 0.25) and torch.all(s.v[40:] == 1) and not s.m.any() and not s.p.any()
    # a restore that does not supply the slot (strict=False): ones again, never zeros and never what happened to be there
    dd = state_dict(st)
    del dd['discriminator/a/kernel/RMSProp_optimizer']
    d.v.fill_(0.0)
    missing = load_state_dict(st, dd, strict=False)
    assert missing == ['discriminator/a/kernel/RMSProp_optimizer']
    kernel = d._slice(d.v, 'discriminator/a/kernel')
    assert torch.all(kernel == 1)
    with pytest.raises(KeyError):
        load_state_dict(st, dd)
    # Adam bound to a store that RMSProp had: zeros again
    Train_base()._Adam_optimizer(torch.zeros(1), 0.5).bind(d)
    assert d.optimizer == 'adam' and not d.v.any()


def test_train_base_factories_keep_the_reference_signatures():
    import inspect
    from Training.train_base import MomentumOptimizer, RMSPropOptimizer, Train_base
    assert list(inspect.signature(Train_base._SGD_w_Momentum_optimizer).parameters) == ['self', 'lr', 'momentum']
    sig = inspect.signature(Train_base._RMSProp_optimizer)
    assert list(sig.parameters) == ['self', 'lr', 'name'] and sig.parameters['name'].default == 'RMSProp_optimizer'
    r = Train_base()._RMSProp_optimizer('lr')
    assert isinstance(r, RMSPropOptimizer) and (r.decay, r.momentum, r.epsilon) == (0.9, 0.0, 1e-10)
    m = Train_base()._SGD_w_Momentum_optimizer('lr', 0.8)
    assert isinstance(m, MomentumOptimizer) and m.momentum == 0.8
