"""float64 NumPy restatement of the two optimisers behind config.OPTIMIZER = 'momentum' / 'rmsprop' (DESIGN §9.5), written from the
update rules of TensorFlow 1.x's ApplyMomentum / ApplyRMSProp kernels as recalled [UNVERIFIED-TF: TensorFlow is not importable here]:

    tf.train.MomentumOptimizer(lr, momentum), use_nesterov=False      accum = accum*momentum + g;  p -= lr*accum
    tf.train.RMSPropOptimizer(lr, decay, momentum, epsilon)           ms += (g*g - ms)*(1 - decay)
                                                                      mom = mom*momentum + (g*lr)/sqrt(ms + epsilon);  p -= mom

The initial slots are ARGUMENTS (TensorFlow: accum 0, mom 0, ms ONE).  tests/test_optimizer_reference.py pins both against torch-CPU in
float64 and in closed form.  The flags `nesterov`, `eps_outside` select the forms the kernels must NOT compute (negative controls);
`f32_*` are the same updates with every operation rounded to float32 once, in the kernels' operation order — what a correct fp32
implementation computes, used on the CPU to show that the bounds of the GPU tests hold for it and fail for the wrong forms before
any kernel is run.  `kernel_case` builds the inputs the CPU and the GPU test share."""
import numpy as np

U = 2.0 ** -24                      # unit round-off of float32


def f32(x):
    """the float32 value of a hyper-parameter as a Python float: the kernels receive lr / momentum / decay / epsilon as float32, and
    that rounding is part of the input, not an error of the kernel."""
    return float(np.float32(x))


def momentum_step(p, g, accum, lr, momentum, nesterov=False):
    """-> (p, accum).  nesterov=True: TensorFlow's use_nesterov form p -= lr*g + lr*momentum*accum (negative control only)."""
    p, g, accum = (np.asarray(a, np.float64) for a in (p, g, accum))
    accum = accum * momentum + g
    if nesterov:
        return p - (lr * g + lr * momentum * accum), accum
    return p - lr * accum, accum


def rmsprop_step(p, g, ms, mom, lr, decay=0.9, momentum=0.0, epsilon=1e-10, eps_outside=False):
    """-> (p, ms, mom).  eps_outside=True: sqrt(ms) + epsilon, the form of torch.optim.RMSprop (negative control only)."""
    p, g, ms, mom = (np.asarray(a, np.float64) for a in (p, g, ms, mom))
    ms = ms + (g * g - ms) * (1.0 - decay)
    den = np.sqrt(ms) + epsilon if eps_outside else np.sqrt(ms + epsilon)
    mom = mom * momentum + (g * lr) / den
    return p - mom, ms, mom


def f32_momentum_step(p, g, accum, lr, momentum, grad_scale=1.0):
    F = np.float32
    p, g, accum = (np.asarray(a, F) for a in (p, g, accum))
    gg = g * F(grad_scale)
    accum = accum * F(momentum) + gg
    return p - F(lr) * accum, accum


def f32_rmsprop_step(p, g, ms, mom, lr, decay=0.9, momentum=0.0, epsilon=1e-10, grad_scale=1.0):
    F = np.float32
    p, g, ms, mom = (np.asarray(a, F) for a in (p, g, ms, mom))
    gg = g * F(grad_scale)
    ms = ms + (gg * gg - ms) * (F(1.0) - F(decay))
    mom = mom * F(momentum) + (gg * F(lr)) / np.sqrt(ms + F(epsilon))
    return p - mom, ms, mom


# ---- the inputs of the kernel tests (tests/test_gpu_optimizers.py part 1; the CPU file checks the bounds on them first) ----------------
N, STEPS = 10007, 3                 # n % 4 = 3: the scalar tail runs


def kernel_case(kind):
    """kind -> dict(p0, slots0, grads [STEPS], hyper).  Gradients as tests/test_gpu_kernels.py's Adam test draws them: standard normal,
    every 7th scaled by 1e-9, every 11th exactly zero.
      'momentum'      the sign of an element's gradient is the same in every step, so accum = accum*momentum + g never cancels and a
                      RELATIVE bound on the slot is meaningful (with mixed signs the sum can be arbitrarily smaller than its terms)
      'rmsprop'       TensorFlow's initial slots: rms = 1, mom = 0
      'rmsprop_small' everything at the scale of epsilon: gradients ~1e-5 (g*g ~ 1e-10 = epsilon), rms seeded log-uniformly over
                      1e-14 .. 1e-6, values ~1e-3 — sqrt(ms + eps) and sqrt(ms) + eps differ by up to 10x here
      'rmsprop_mom'   momentum 0.5 (the kernel's argument; the reference's factory leaves it 0)"""
    rng = np.random.default_rng({'momentum': 11, 'rmsprop': 12, 'rmsprop_small': 13, 'rmsprop_mom': 14}[kind])
    small = kind == 'rmsprop_small'
    p0 = (rng.standard_normal(N) * (1e-3 if small else 1.0)).astype(np.float32)
    sign = np.where(rng.random(N) < 0.5, -1.0, 1.0)
    grads = []
    for _ in range(STEPS):
        g = rng.standard_normal(N)
        if kind == 'momentum':
            g = np.abs(g) * sign
        if small:
            g = g * 1e-5
        g = g.astype(np.float32)
        g[::7] *= np.float32(1e-9)
        g[::11] = 0
        grads.append(g)
    if kind == 'momentum':
        return dict(p0=p0, slots0=dict(accum=np.zeros(N, np.float32)), grads=grads, hyper=dict(lr=f32(3e-4), momentum=f32(0.9)))
    rms0 = np.exp(rng.uniform(np.log(1e-14), np.log(1e-6), N)).astype(np.float32) if small else np.ones(N, np.float32)
    return dict(p0=p0, slots0=dict(rms=rms0, mom=np.zeros(N, np.float32)), grads=grads,
                hyper=dict(lr=f32(3e-4), decay=f32(0.9), momentum=f32(0.5 if kind == 'rmsprop_mom' else 0.0), epsilon=f32(1e-10)))


def run_reference(kind, case, **variant):
    """the float64 restatement over the case's steps -> dict(p, slots..., max_update, max_p).  variant: nesterov / eps_outside / rms0."""
    p = case['p0'].astype(np.float64)
    h = case['hyper']
    max_update = 0.0
    if kind == 'momentum':
        accum = case['slots0']['accum'].astype(np.float64)
        for g in case['grads']:
            q, accum = momentum_step(p, g, accum, h['lr'], h['momentum'], nesterov=variant.get('nesterov', False))
            max_update, p = max(max_update, np.abs(q - p).max()), q
        return dict(p=p, accum=accum, max_update=max_update, max_p=np.abs(p).max())
    ms = case['slots0']['rms'].astype(np.float64) if 'rms0' not in variant else np.full(p.shape, float(variant['rms0']))
    mom = case['slots0']['mom'].astype(np.float64)
    for g in case['grads']:
        q, ms, mom = rmsprop_step(p, g, ms, mom, h['lr'], h['decay'], h['momentum'], h['epsilon'], eps_outside=variant.get('eps_outside', False))
        max_update, p = max(max_update, np.abs(q - p).max()), q
    return dict(p=p, rms=ms, mom=mom, max_update=max_update, max_p=np.abs(p).max())


def run_f32(kind, case, grad_scale=0.5):
    """the float32 emulation over the case's steps, fed grad_scale and gradients divided by it the way the GPU test feeds the kernels."""
    p = case['p0']
    h = case['hyper']
    if kind == 'momentum':
        accum = case['slots0']['accum']
        for g in case['grads']:
            p, accum = f32_momentum_step(p, g / np.float32(grad_scale), accum, h['lr'], h['momentum'], grad_scale)
        return dict(p=p, accum=accum)
    ms, mom = case['slots0']['rms'], case['slots0']['mom']
    for g in case['grads']:
        p, ms, mom = f32_rmsprop_step(p, g / np.float32(grad_scale), ms, mom, h['lr'], h['decay'], h['momentum'], h['epsilon'], grad_scale)
    return dict(p=p, rms=ms, mom=mom)


# ---- the bounds: from the rounding count, u = 2^-24 -------------------------------------------------------------------
SLOT_RTOL = 1e-6                    # ~17 u: a slot update is at most 4 roundings per step, 3 steps, nothing cancels (see kernel_case)
SLOT_ATOL = 1e-30                   # exact zeros and subnormal products only


def param_bound(ref, steps):
    """|p - p_ref| <= 1e-6 * max|update| * steps + 2e-7 * max|p|: an update carries its slot's relative error (<= 17 u) in every step,
    and the subtraction from p is one rounding per step, 3 u |p| = 1.8e-7 |p| over three."""
    return 1e-6 * ref['max_update'] * steps + 2e-7 * ref['max_p']


def slots_close(got, ref, atol=SLOT_ATOL):
    """worst |got - ref| / (SLOT_RTOL |ref| + atol); <= 1 passes."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (SLOT_RTOL * np.abs(ref) + atol)).max())
