"""CPU self-checks of tests/wn_init_reference.py, the float64 restatement the GPU tests of the data-dependent weight-norm initialisation
 compare against: the rule does what Salimans & Kingma ask of it, the whole pass is idempotent, and the tolerance the kernel
test uses tells a two-pass fp64 accumulation from a one-pass fp32 one (the negative control, needing no GPU)."""
import numpy as np
import pytest

import wn_init_reference as R
from oracle import nets_goodgan as NG
from oracle import step_cifar10 as S
from oracle import step_goodgan as SG

SIZES = dict(B_G=8, L_C=4, U_C=4, L_D=2, U_D=6)
LAYERS = {'cifar10': 10, 'mnist': 1 + 6, 'svhn': 1 + 2 + 7}


def _check_records(recs):
    """after the pass each layer's g t + b over the init batch has per-channel mean 0 and variance init_scale^2 v / (v + eps)."""
    for r in recs:
        y = r.g * r.t + r.b
        v = np.square(r.t - r.t.mean(axis=0)).mean(axis=0)
        scale = np.abs(r.g) * np.abs(r.t).max(axis=0) + np.abs(r.b)
        assert (np.abs(y.mean(axis=0)) <= 1e-12 * scale).all(), r.name
        np.testing.assert_allclose(y.var(axis=0), r.init_scale ** 2 * v / (v + r.eps), rtol=1e-10, atol=0, err_msg=r.name)
        np.testing.assert_allclose(r.g, r.init_scale / np.sqrt(v + r.eps), rtol=1e-13, err_msg=r.name)


@pytest.mark.parametrize("eps,scale", [(1e-8, 1.0), (1e-10, 0.1)])
def test_rule_normalises_the_batch(eps, scale):
    rng = np.random.default_rng(3)
    t = rng.standard_normal((257, 5)) * np.array([1e-3, 1.0, 30.0, 1.0, 0.0]) + np.array([0.0, -2.0, 7.0, 1e3, 4.0])
    m, v, g, b = R.rule(t, eps, scale)
    _check_records([R.Record('rule', t, g, b, eps, scale)])
    assert g[4] == scale / np.sqrt(eps) and b[4] == -4.0 * g[4]                 # a constant channel: v = 0 exactly


@pytest.fixture(scope="module")
def cifar_pass():
    P = S.init_params(0)
    b = S.synth_batch(11, dict(S.SIZES, **SIZES))
    new, recs = R.init_pass_cifar10(P, b['x_u_c'], S.synth_zca())
    return P, b, new, recs


def test_cifar10_pass(cifar_pass):
    P, b, new, recs = cifar_pass
    assert len(recs) == LAYERS['cifar10'] and len(new) == 2 * LAYERS['cifar10']
    assert [r.eps for r in recs] == [1e-8] * 7 + [1e-10] * 3
    assert all(k in P and P[k].shape == v.shape for k, v in new.items())
    _check_records(recs)
    again, _ = R.init_pass_cifar10(dict(P, **new), b['x_u_c'], S.synth_zca())   # idempotent: t does not depend on g, b
    for k in new:
        np.testing.assert_array_equal(again[k], new[k], err_msg=k)


@pytest.mark.parametrize("data", ['mnist', 'svhn'])
def test_goodgan_pass(data):
    P = NG.init_params(data, 0)
    b = SG.synth_batch(data, 12, SIZES)
    new, recs, labels = R.init_pass_goodgan(P, data, b)
    assert len(recs) == LAYERS[data] and len(new) == 2 * LAYERS[data]
    assert all(k in P and P[k].shape == v.shape for k, v in new.items())
    assert labels.shape == (SIZES['U_D'], 10) and (labels.sum(axis=1) == 1).all()
    assert {r.init_scale for r in recs} == ({1.0} if data == 'mnist' else {0.1, 1.0})
    _check_records(recs)
    again, _, _ = R.init_pass_goodgan(dict(P, **new), data, b, labels)
    for k in new:
        np.testing.assert_array_equal(again[k], new[k], err_msg=k)
    # the pass is a function of the variables and the batch: moving statistics play no part
    P2 = dict(P, **{k: v + 1.0 for k, v in P.items() if 'moving_' in k})
    other, _, _ = R.init_pass_goodgan(P2, data, b, labels)
    for k in new:
        np.testing.assert_array_equal(other[k], new[k], err_msg=k)


@pytest.mark.parametrize("eps", [1e-8, 1e-10])
def test_the_bound_tells_a_two_pass_fp64_kernel_from_a_one_pass_fp32_one(eps):
    """the negative control of the kernel's tolerance (K_G, K_B), on the fixed ill-conditioned channels the GPU test feeds the kernel:
    mean 1e3, standard deviation 1e-2."""
    t = R.ill_conditioned(1023, 3)
    assert abs(float(t.mean()) - 1e3) < 1e-2 and 0.5e-2 < float(t.astype(np.float64).std()) < 2e-2
    m, v, g64, b64 = R.rule(t, np.float64(np.float32(eps)))
    assert R.within(g64, b64, t, eps)                                            # the float64 reference itself
    assert R.within(*R.kernel_model(t, eps), t, eps)                             # fp64 accumulation, one rounding each: inside
    g1, b1 = R.one_pass_fp32_model(t, eps)
    assert not R.within(g1, b1, t, eps)                                          # fp32 E[x^2] - m^2: outside ...
    assert (np.abs(g1.astype(np.float64) - g64) > 1e3 * R.K_G * R.U * np.abs(g64)).all()      # ... by orders of magnitude, in every channel
    # and on well-conditioned data the fp32 shortcut would have passed unnoticed at a loose tolerance: the control needs these inputs
    easy = np.random.default_rng(5).standard_normal((1023, 3)).astype(np.float32)
    ge, _ = R.one_pass_fp32_model(easy, eps)
    assert np.allclose(ge, R.rule(easy, eps)[2], rtol=1e-4)
