"""CPU checks behind config.CLIP_NORM: the float64 restatement of tf.clip_by_global_norm (tests/clip_reference.py) against
torch.nn.utils.clip_grad_norm_ on CPU float64 and in closed form; then, on the very inputs tests/test_gpu_clip.py uses, the bounds of
the GPU tests shown to hold for a correctly rounded float32 implementation and to fail for three wrong forms — fixed here, before a
kernel ran."""
import numpy as np
import pytest
import torch

import clip_reference as CR
import optimizer_reference as R


# ------------------------------------------------------------------------------------------------------------- against torch, float64
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_differs_from_torch_clip_grad_norm_by_its_epsilon_only(scale):
    """torch clips by clip/(norm + 1e-6) clamped to 1: wherever it clips, its gradients are ours times norm/(norm + 1e-6), i.e. differ by the
    relative 1e-6/(norm + 1e-6) and by nothing else."""
    rng = np.random.default_rng(31)
    grads = [rng.standard_normal(s) * scale / 10.0 for s in (57, 300, 5)]
    norm = CR.global_norm(grads)
    assert 0.3 * scale < norm < 3.0 * scale
    for clip in (norm * 0.25, norm * 0.9):
        ps = [torch.zeros(g.shape, dtype=torch.float64, requires_grad=True) for g in grads]
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(g, dtype=torch.float64)
        total = torch.nn.utils.clip_grad_norm_(ps, clip)
        assert abs(float(total) - norm) <= 1e-14 * norm
        ours, n2, factor = CR.clip_by_global_norm(grads, clip)
        assert n2 == norm and abs(factor - clip / norm) <= 1e-15 * factor
        predicted = 1e-6 / (norm + 1e-6)
        for p, o in zip(ps, ours):
            t = p.grad.numpy()
            nz = o != 0
            rel = (o[nz] - t[nz]) / o[nz]
            assert np.abs(rel - predicted).max() <= 1e-12 + 1e-9 * predicted, (scale, clip)
        eps_form = CR.clip_by_global_norm(grads, clip, form='torch_eps')[0]
        for p, e in zip(ps, eps_form):
            assert np.abs(e - p.grad.numpy()).max() <= 1e-14 * np.abs(e).max()          # and the 'torch_eps' control IS torch's form
    ps = [torch.zeros(g.shape, dtype=torch.float64, requires_grad=True) for g in grads]      # above the norm: neither clips
    for p, g in zip(ps, grads):
        p.grad = torch.tensor(g, dtype=torch.float64)
    torch.nn.utils.clip_grad_norm_(ps, norm * 4.0)
    ours, _, factor = CR.clip_by_global_norm(grads, norm * 4.0)
    assert np.float32(factor) == np.float32(1.0)
    for p, g in zip(ps, grads):
        assert np.array_equal(p.grad.numpy(), g)


# ------------------------------------------------------------------------------------------------------------- closed form
def test_closed_form_cases():
    g = np.array([3.0, 4.0, 0.0])
    out, norm, factor = CR.clip_by_global_norm(g, 1.0)
    assert norm == 5.0 and abs(factor - 0.2) <= 1e-16 and np.allclose(out[0], [0.6, 0.8, 0.0], rtol=1e-15, atol=0)
    _, factor, n32, f32 = CR.norm_and_factor(g, 5.0)                         # norm == clip exactly
    assert n32 == np.float32(5.0) and f32 == np.float32(1.0) and abs(factor - 1.0) <= 2.0 ** -52
    for clip in (5.0000001, 7.0, 1e30):                                      # norm < clip: clip*(1/clip) may be 1 - 2^-53, float32 1.0f
        _, factor, _, f32 = CR.norm_and_factor(g, clip)
        assert f32.tobytes() == np.float32(1.0).tobytes() and abs(factor - 1.0) <= 2.0 ** -52
        assert np.array_equal(CR.used_gradient(g.astype(np.float32), clip, 1.0), g)       # the bits of the unclipped path
    bad = np.array([1.0, np.inf, -2.0], np.float32)
    norm, factor, n32, f32 = CR.norm_and_factor(bad, 1.0)
    assert np.isinf(norm) and np.isnan(factor) and np.isnan(f32)
    assert np.isnan(CR.used_gradient(bad, 1.0, 1.0)).all() and np.isnan(CR.f32_used_gradient(bad, 1.0, 1.0)[0]).all()
    assert np.isnan(CR.norm_and_factor(np.array([1.0, np.nan], np.float32), 1.0)[3])
    z = CR.norm_and_factor(np.zeros(5, np.float32), 1.0)                     # a zero gradient: 1/0 = inf loses the min, factor 1
    assert z[0] == 0.0 and z[3] == np.float32(1.0)
    rng = np.random.default_rng(32)
    grads = [rng.standard_normal(40), rng.standard_normal(9)]
    half = CR.clip_by_global_norm(grads, 0.7, grad_scale=0.5)
    pre = CR.clip_by_global_norm([a * 0.5 for a in grads], 0.7, grad_scale=1.0)            # halving is exact
    assert half[1] == pre[1] and half[2] == pre[2]
    assert all(np.array_equal(a, b) for a, b in zip(half[0], pre[0]))


# ------------------------------------------------------------------------------------------------------------- the GPU bounds, on the CPU
def _forms_out(g, clip):
    """{form: (norm, factor)} in float64 of the restatement and the wrong forms for the stored buffer g (quarters = 'variables')."""
    out = {}
    for form in CR.FORMS:
        _, norm, factor = CR.clip_by_global_norm(np.array_split(g, 4) if g.size >= 4 else [g[:1], g[1:]], clip, CR.GRAD_SCALE, form)
        out[form] = (norm, factor)
    return out


def test_kernel_output_bounds_hold_for_the_emulation_and_fail_for_the_wrong_forms():
    """tests/test_gpu_clip.py part 3 on its own inputs: {norm, factor} rounded to float32 once are within OUT_RTOL of the restatement, and
    exactly 1.0f where norm <= clip.  Negative controls, worst |value - restatement| / (OUT_RTOL |restatement|) where each misses most
    (1 passes), as measured when the bounds were fixed:
        'unscaled_norm'  8.3e6   the norm is 2x the restatement's in every case (grad_scale 0.5)
        'torch_eps'      1.7e4   the factor on 'n3' (norm 2.5e-4) with the clip below the norm; inside the bound on the cases whose norm
                                 is >> 1, which is why 'n3' is small
        'per_variable'   8.8e6   the first variable's norm instead of the buffer's"""
    worst = {f: 0.0 for f in CR.FORMS}
    for name in CR.NORM_CASES:
        g = CR.stored(CR.norm_case(name))
        assert g.size % 4 in ((3,) if name in ('tail', 'n3') else (0, 1, 2, 3))
        if name != 'n3':
            mags = np.abs(g[g != 0])
            assert mags.min() < 1e-8 and mags.max() > 1e3 and (g == 0).sum() >= g.size // 11
        for k, clip in enumerate(CR.thresholds(g)):
            norm, factor, n32, f32 = CR.norm_and_factor(g, clip, CR.GRAD_SCALE)
            assert CR.out_close(n32, norm) <= 0.51 and CR.out_close(f32, factor) <= 0.51          # one rounding: half an ulp
            if norm <= clip:
                assert f32.tobytes() == np.float32(1.0).tobytes(), (name, clip)
            if k == 0:
                assert f32 < 0.011
            if k == 2:
                assert norm < clip
            for form, (wn, wf) in _forms_out(g, clip).items():
                miss = max(CR.out_close(wn, norm), CR.out_close(wf, factor))
                worst[form] = max(worst[form], miss)
                if form == 'tf':
                    assert miss <= 1e-6                     # the same form summed variable by variable: float64 order only
    print('worst miss / bound:', {k: '%.3g' % v for k, v in worst.items()})
    assert worst['unscaled_norm'] > 1e6 and worst['torch_eps'] > 1e4 and worst['per_variable'] > 1e5


@pytest.mark.parametrize("kind", CR.OPT_KINDS)
def test_clipped_optimizer_bounds_hold_for_the_emulation_and_fail_for_the_wrong_forms(kind):
    """tests/test_gpu_clip.py part 4 on its own inputs: three clipped steps of the float32 emulation stay inside the parameter bound of
    tests/optimizer_reference.py and the slot bound widened by one rounding per step (clip_reference.SLOT_RTOL), and each step's factor
    is a different number below 1.  Negative controls (parameter error / bound, 1 passes), as measured when the bounds were fixed:
        adam      unscaled_norm 2.2     torch_eps 1e-5   per_variable 14     (Adam divides the gradient's scale out again)
        momentum  unscaled_norm 918     torch_eps 5e-5   per_variable 1.8e3
        rmsprop   unscaled_norm 453     torch_eps 2e-5   per_variable 688
    so a factor of the wrong scale is caught by momentum and RMSProp by more than 400x; torch's epsilon is 3e-8 relative at this norm of
    ~33 and cannot be seen here — the kernel-output test above catches it by 1.7e4x.  The emulation itself uses 0.40 - 0.44 of the
    parameter bound and 0.17 - 0.18 of the slot bound."""
    case = CR.optimizer_case(kind)
    ref = CR.run_reference(kind, case)
    assert len(set(ref['factors'])) == R.STEPS and all(0.2 < f < 0.5 for f in ref['factors'])
    miss, slot = CR.optimizer_miss(kind, CR.run_f32(kind, case), ref)
    print('%s: emulation parameter error / bound %.3f, slot error / bound %.3f' % (kind, miss, slot))
    assert miss <= 1.0 and slot <= 1.0
    wrong = {}
    for form in CR.FORMS[1:]:
        w = CR.run_reference(kind, case, form=form)
        wrong[form] = np.abs(w['p'] - ref['p']).max() / R.param_bound(ref, R.STEPS)
    print('%s: wrong forms, parameter error / bound: %s' % (kind, {k: '%.3g' % v for k, v in wrong.items()}))
    if kind != 'adam':
        assert wrong['unscaled_norm'] > 100.0 and wrong['per_variable'] > 100.0


def test_used_gradient_emulation_is_within_three_roundings():
    for name in ('tail', 'n3'):
        g = CR.stored(CR.norm_case(name))
        for clip in CR.thresholds(g):
            want = CR.used_gradient(g, clip, CR.GRAD_SCALE)
            got, _, f32 = CR.f32_used_gradient(g, clip, CR.GRAD_SCALE)
            nz = np.abs(want) > 1e-37                                                   # above the subnormals
            assert (np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max() <= CR.USED_RTOL
            if f32 == np.float32(1.0):
                assert got.tobytes() == (g * np.float32(CR.GRAD_SCALE)).tobytes()       # the bits of the unclipped path
