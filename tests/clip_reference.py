"""float64 NumPy restatement of config.CLIP_NORM: tf.clip_by_global_norm(grads, clip_norm) over a solver's var_list as
TensorFlow 1.x computes it, as recalled [UNVERIFIED-TF: TensorFlow is not importable here], with the data-parallel grad_scale as an
argument.  `g` is the stored gradient (after the all-reduce, and under LOSS = 'WGAN_GP' with the penalty's gradient added):

    norm   = grad_scale * sqrt(sum_i g_i^2)            sum and root in float64, rounded to float32 once
    factor = clip * min(1/norm, 1/clip)                in float64 from the float64 norm, rounded to float32 once;
                                                       NaN when the norm is not finite (TensorFlow poisons every gradient then)
    g_used = (g * grad_scale) * factor                 two float32 roundings, in this order; then the optimiser's own form

tests/test_clip_reference.py pins it against torch.nn.utils.clip_grad_norm_ on CPU float64 and in closed form.  `form` selects the
forms the kernels must NOT compute (negative controls): 'unscaled_norm' (the factor from the norm of the unscaled buffer, applied
before grad_scale), 'torch_eps' (torch's clip/(norm + 1e-6) clamped to 1) and 'per_variable' (tf.clip_by_norm per variable).
`f32_*` round to float32 where the kernels do — what a correct implementation computes, used on the CPU to show that the bounds of the
GPU tests hold for it, and fail for the wrong forms, before any kernel runs.  `norm_case` / `optimizer_case` build the inputs the CPU
and the GPU tests share."""
import numpy as np

import optimizer_reference as R

U = R.U                              # unit round-off of float32, 2^-24
FORMS = ('tf', 'unscaled_norm', 'torch_eps', 'per_variable')


def global_norm(grads, grad_scale=1.0):
    """grad_scale * sqrt(sum over every array of `grads` (one array or a list) of g^2), float64."""
    arrays = grads if isinstance(grads, (list, tuple)) else [grads]
    with np.errstate(over='ignore', invalid='ignore'):
        total = sum(float(np.sum(np.square(np.asarray(a, np.float64)))) for a in arrays)
        return float(grad_scale) * float(np.sqrt(total))


def clip_factor(norm, clip):
    """clip * min(1/norm, 1/clip) in float64; NaN for a norm that is not finite."""
    if not np.isfinite(norm):
        return float('nan')
    with np.errstate(divide='ignore'):
        return float(clip) * min(np.float64(1.0) / np.float64(norm), 1.0 / float(clip))


def norm_and_factor(grads, clip, grad_scale=1.0):
    """-> (norm, factor, norm32, factor32): the float64 values and their single float32 roundings — what tg_grad_norm_clip_f32 writes."""
    norm = global_norm(grads, grad_scale)
    factor = clip_factor(norm, clip)
    with np.errstate(over='ignore'):
        return norm, factor, np.float32(norm), np.float32(factor)


def clip_by_global_norm(grads, clip, grad_scale=1.0, form='tf'):
    """-> (list of used gradients in float64, norm, factor).  The used gradient is g*grad_scale*factor without intermediate rounding;
    `factor` is the restatement's float64 one (form 'tf') or a wrong form's."""
    arrays = [np.asarray(a, np.float64) for a in (grads if isinstance(grads, (list, tuple)) else [grads])]
    assert form in FORMS, form
    if form == 'per_variable':                                   # tf.clip_by_norm on each variable: no global norm at all
        out = []
        for a in arrays:
            nv = global_norm(a, grad_scale)
            out.append(a * grad_scale * clip_factor(nv, clip))
        return out, global_norm(arrays[0], grad_scale), clip_factor(global_norm(arrays[0], grad_scale), clip)
    if form == 'unscaled_norm':                                  # clip the summed gradient, average afterwards
        norm = global_norm(arrays, 1.0)
        factor = clip_factor(norm, clip)
    elif form == 'torch_eps':                                    # torch.nn.utils.clip_grad_norm_
        norm = global_norm(arrays, grad_scale)
        factor = min(float(clip) / (norm + 1e-6), 1.0) if np.isfinite(norm) else float('nan')
    else:
        norm = global_norm(arrays, grad_scale)
        factor = clip_factor(norm, clip)
    return [a * grad_scale * factor for a in arrays], norm, factor


def used_gradient(g32, clip, grad_scale):
    """what the optimiser is specified to see, in float64, for float32 gradients g32: (g*grad_scale) * factor32 — the factor IS the
    float32 number the formulas define, the two products are exact here and carry one float32 rounding each in the kernel."""
    _, _, _, f32 = norm_and_factor(g32, clip, grad_scale)
    return np.asarray(g32, np.float64) * float(grad_scale) * float(f32)


def f32_used_gradient(g32, clip, grad_scale):
    """the kernels' arithmetic: float64 sum, norm and factor rounded to float32 once each, then two float32 products."""
    F = np.float32
    _, _, n32, f32 = norm_and_factor(g32, clip, grad_scale)
    with np.errstate(invalid='ignore'):
        return (np.asarray(g32, F) * F(grad_scale)) * f32, n32, f32


# ---- the bounds, fixed from the rounding count before any kernel ran ----------------------------------------------------
OUT_RTOL = 1.2e-7                   # {norm, factor}: one float32 rounding of a float64 value is <= u = 6e-8 relative; 1 ulp = 2u allows the
                                    # float64 sum's own order (error < 1e-12 for n <= 1e7) to move the value across one rounding boundary
USED_RTOL = 2e-7                    # g_used against used_gradient(): two roundings, (1+u)^2 - 1 = 1.2e-7, and one more ulp of the factor
                                    # itself (above): 3u = 1.8e-7
SLOT_RTOL = R.SLOT_RTOL + R.STEPS * U
"""the slot bound of tests/test_gpu_optimizers.py, 1e-6 ~ 17u for <= 4 roundings per step over 3 steps (12u, 5u to spare), widened by ONE
rounding per step: the product with the factor.  Worst case that rounding enters RMSProp's rms and Adam's v through gg*gg twice, 6u over
three steps: 18u against the 20u = 1.19e-6 allowed.  The parameter bound (optimizer_reference.param_bound) is kept as it is."""


def out_close(got, ref):
    """|got - ref| / (OUT_RTOL |ref|) of a float32 result against the float64 restatement; <= 1 passes (0 for two zeros)."""
    got, ref = float(got), float(ref)
    return 0.0 if got == ref else abs(got - ref) / (OUT_RTOL * abs(ref))


def slots_close(got, ref, atol=R.SLOT_ATOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (SLOT_RTOL * np.abs(ref) + atol)).max())


# ---- inputs shared by tests/test_clip_reference.py (CPU) and tests/test_gpu_clip.py -------------------------------------------------
GRAD_SCALE = 0.5
STORE_N = 327520                    # the CIFAR-10 discriminator's flat buffer (tools/bench_optim.py store_sizes)
NORM_CASES = ('tail', 'n3', 'store', 'capped')


def norm_case(name):
    """float32 gradients of the direct kernel test.
      'tail'    n = 10 007 (n % 4 = 3): magnitudes log-uniform over 1e-9 .. 1e3, every 11th exactly zero
      'n3'      n = 3 < one 16-byte unit, norm ~ 2.5e-4: only the scalar tail runs (and torch's + 1e-6 is 0.4 % of this norm)
      'store'   n = 327 520, the discriminator's store: 40 workgroups
      'capped'  n = 1024 * 8192 + 3 * 8192 + 5: more chunks than the grid's cap, some workgroups sum two chunks"""
    rng = np.random.default_rng({'tail': 21, 'n3': 22, 'store': 23, 'capped': 24}[name])
    if name == 'n3':
        return np.array([3e-4, -4e-4, 0.0], np.float32)
    n = {'tail': 10007, 'store': STORE_N, 'capped': 1024 * 8192 + 3 * 8192 + 5}[name]
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-9.0, 3.0, n)).astype(np.float32)
    g[::11] = 0
    return g


def thresholds(g32, grad_scale=GRAD_SCALE):
    """clip thresholds below, equal to (the float32 nearest the norm) and above the norm of g32."""
    norm = global_norm(g32, grad_scale)
    return [float(np.float32(norm * 0.01)), float(np.float32(norm)), float(np.float32(norm * 7.0))]


OPT_KINDS = ('adam', 'momentum', 'rmsprop')
ADAM_HYPER = dict(lr=R.f32(3e-4), beta1=0.5, beta2=R.f32(0.999), epsilon=R.f32(1e-8))


def optimizer_case(kind):
    """tests/optimizer_reference.kernel_case (n = 10 007, three steps; Adam: the inputs of 'rmsprop' with zero slots) plus a clip
    threshold of a third of the first step's norm, so every step is clipped by a different factor."""
    case = R.kernel_case('rmsprop' if kind == 'adam' else kind)
    if kind == 'adam':
        case = dict(case, slots0=dict(m=np.zeros(R.N, np.float32), v=np.zeros(R.N, np.float32)), hyper=ADAM_HYPER)
    case['clip'] = float(np.float32(global_norm(case['grads'][0], 1.0) / 3.0))
    return case


def stored(g, grad_scale=GRAD_SCALE):
    """the buffer a test hands the kernel for a case's gradient g: divided by grad_scale (exact for 0.5)."""
    return g / np.float32(grad_scale)


def run_reference(kind, case, grad_scale=GRAD_SCALE, form='tf'):
    """float64: clip (form 'tf': with the float32 factor, used_gradient) composed with the optimiser's restatement, over the case's steps.
    -> dict(p, slots..., max_update, max_p, factors)."""
    from oracle import tf_ops as T
    p = case['p0'].astype(np.float64)
    h = case['hyper']
    slots = {k: v.astype(np.float64) for k, v in case['slots0'].items()}
    max_update, factors = 0.0, []
    for t, g in enumerate(case['grads'], 1):
        gs = stored(g, grad_scale)
        if form == 'tf':
            gu = used_gradient(gs, case['clip'], grad_scale)
            factors.append(float(norm_and_factor(gs, case['clip'], grad_scale)[3]))
        else:
            quarters = np.array_split(gs, 4)
            gu = np.concatenate(clip_by_global_norm(quarters, case['clip'], grad_scale, form)[0])
        if kind == 'adam':
            q, slots['m'], slots['v'] = T.adam_update(p, gu, slots['m'], slots['v'], t, h['lr'], h['beta1'], h['beta2'], h['epsilon'])
        elif kind == 'momentum':
            q, slots['accum'] = R.momentum_step(p, gu, slots['accum'], h['lr'], h['momentum'])
        else:
            q, slots['rms'], slots['mom'] = R.rmsprop_step(p, gu, slots['rms'], slots['mom'], h['lr'], h['decay'], h['momentum'], h['epsilon'])
        max_update, p = max(max_update, np.abs(q - p).max()), q
    return dict(slots, p=p, max_update=max_update, max_p=np.abs(p).max(), factors=factors)


def run_f32(kind, case, grad_scale=GRAD_SCALE):
    """the float32 emulation of the *_clip_* kernels over the case's steps."""
    from oracle import tf_ops as T
    F = np.float32
    p = case['p0']
    h = case['hyper']
    slots = dict(case['slots0'])
    for t, g in enumerate(case['grads'], 1):
        gu, _, _ = f32_used_gradient(stored(g, grad_scale), case['clip'], grad_scale)
        if kind == 'adam':
            p, slots['m'], slots['v'] = T.adam_update(p, gu, slots['m'], slots['v'], t, h['lr'], F(h['beta1']), F(h['beta2']), h['epsilon'])
        elif kind == 'momentum':
            p, slots['accum'] = R.f32_momentum_step(p, gu, slots['accum'], h['lr'], h['momentum'])
        else:
            p, slots['rms'], slots['mom'] = R.f32_rmsprop_step(p, gu, slots['rms'], slots['mom'], h['lr'], h['decay'], h['momentum'], h['epsilon'])
    return dict(slots, p=p)


def optimizer_miss(kind, got, ref):
    """(parameter error / bound, worst slot error / bound) of a run's results against run_reference's; both <= 1 pass.  Slot atol as in
    tests/test_gpu_optimizers.py: exact zeros and subnormal products only — except Adam's m, a signed sum that can cancel, bounded against the largest value like the parameter."""
    miss = np.abs(np.asarray(got['p'], np.float64) - ref['p']).max() / R.param_bound(ref, R.STEPS)
    worst = 0.0
    for k in ref:
        if k in ('p', 'max_update', 'max_p', 'factors'):
            continue
        cancels = k == 'm'                                     # (the 'rmsprop' case keeps the reference factory's momentum 0)
        atol = 1e-6 * np.abs(ref[k]).max() * R.STEPS if cancels else R.SLOT_ATOL
        worst = max(worst, slots_close(got[k], ref[k], atol))
    return float(miss), worst
