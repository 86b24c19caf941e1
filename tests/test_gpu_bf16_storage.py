"""bf16-stored activations (config.ACT_DTYPE = 'bf16'): the batch norms in front of the SVHN classifier's 3x3 convolutions store RNE(y) as
bf16 and those convolutions read it as it is.  Every MFMA operand is the bit pattern the fp32-input *_bf16 launches round to, so the
results must be IDENTICAL, bit for bit — per entry point here, and over a whole D+G+C step below."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_common as G

pytestmark = pytest.mark.gpu

BF16 = 'bf16'          # the fp32-input reference launches are named 'tg_igemm_' + BF16 etc.


def _lib():
    from tg import lib
    lib.load()
    return lib


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    """bit patterns (NaN payloads included) of a float32 / float64 / bfloat16 tensor."""
    t = t.detach().contiguous()
    v = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16}[t.dtype]
    return t.view(v).cpu().numpy()


def rtz_bf16(x):
    """truncation toward zero to bf16 (the wrong rounding mode of the negative control)."""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def special_input(shape, seed):
    """normal values with +-0, fp32 denormals and exact bf16 rounding ties (both parities) sprinkled in, and one +Inf and one -Inf."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=min(flat.size // 8, 4096), replace=False)
    ties = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x40A28000], np.uint32).view(np.float32)
    den = np.array([1e-40, -1e-40, 3e-39, -5e-42], np.float32)
    special = np.concatenate([np.array([0.0, -0.0], np.float32), den, ties])
    flat[idx] = special[rng.integers(0, special.size, idx.size)]
    flat[idx[:2]] = [np.inf, -np.inf]              # two pixels: their 3x3 neighbourhoods go Inf / NaN, the rest stays finite
    return x


BN_TRAIN = {'f32': 'tg_bn_train_f32', 'bf16': 'tg_bn_train_bf16'}
BN_APPLY = {'f32': 'tg_bn_train_apply_f32', 'bf16': 'tg_bn_train_apply_bf16'}


def _bn_args(rows, c, nseg):
    rng = np.random.default_rng(5)
    g = torch.from_numpy(rng.standard_normal(c).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.standard_normal(c).astype(np.float32)).cuda()
    segs = [rows // nseg] * (nseg - 1) + [rows - rows // nseg * (nseg - 1)]
    return g, b, segs


@pytest.mark.parametrize("n,hw,c,ld,nseg", [(8, 32, 128, 128, 2), (4, 16, 256, 256, 3), (3, 8, 96, 128, 1)])
def test_bn_apply_bf16_output_is_the_rne_of_the_fp32_output(n, hw, c, ld, nseg):
    """tg_bn_train_bf16 (statistics + apply) and tg_bn_train_apply_bf16 against tg_bn_train_apply_f32 from the SAME batch sums (the
    statistics launch adds with fp64 atomics, so two statistics launches may differ in the last bit): y16 = torch's RNE of y32, bit for
    bit; mean / inv-std and the moving statistics identical; the padding channels c..ld stay zero."""
    lib = _lib()
    rows = n * hw * hw
    rng = np.random.default_rng(11)
    x = torch.zeros(rows, ld, device='cuda')
    x[:, :c] = torch.from_numpy((rng.standard_normal((rows, c)) * 3 + 1).astype(np.float32)).cuda()
    gamma, beta, segs = _bn_args(rows, c, nseg)
    sa = (C.c_int32 * nseg)(*segs)

    def fresh():
        return (torch.zeros(2 * nseg * c, device='cuda'), torch.full((c,), 0.25, device='cuda'), torch.full((c,), 2.0, device='cuda'))

    sums = torch.zeros(16 * nseg * c, device='cuda', dtype=torch.float64)
    y_st = torch.zeros(rows, ld, device='cuda', dtype=torch.bfloat16)
    st_st = fresh()
    lib.call(BN_TRAIN['bf16'], lib.ptr(x), ld, lib.ptr(y_st), ld, rows, c, sa, nseg, lib.ptr(gamma), lib.ptr(beta), 1e-5, 0.9, lib.ptr(st_st[1]),
             lib.ptr(st_st[2]), lib.ptr(sums), 0, lib.ptr(st_st[0]), st())
    out = {}
    for sfx in ('f32', 'bf16'):
        y = torch.zeros(rows, ld, device='cuda', dtype=torch.float32 if sfx == 'f32' else torch.bfloat16)
        sta = fresh()
        lib.call(BN_APPLY[sfx], lib.ptr(x), ld, lib.ptr(y), ld, rows, c, sa, nseg, lib.ptr(gamma), lib.ptr(beta), 1e-5, 0.9, lib.ptr(sta[1]),
                 lib.ptr(sta[2]), lib.ptr(sums), lib.ptr(sta[0]), st())
        out[sfx] = (y,) + sta
    torch.cuda.synchronize()
    ref16 = bits(out['f32'][0].to(torch.bfloat16))
    for y16, stats in ((out['bf16'][0], out['bf16'][1:]), (y_st, st_st)):
        assert (bits(y16) == ref16).all(), "bf16 output is not the RNE of the fp32 output"
        assert (bits(y16[:, c:]) == 0).all(), "padding channels written"
        assert not (bits(y16[:, :c]) == 0).all()
        for a, b in zip(out['f32'][1:], stats):
            assert (bits(a) == bits(b)).all(), "statistics / moving statistics differ"


def _conv_case(n, hw, ci, co, x_np, act='lrelu'):
    from tg import geom
    rng = np.random.default_rng(31)
    x32 = torch.from_numpy(x_np).cuda()
    w = torch.from_numpy((rng.standard_normal((co, 9, ci)) * 0.05).astype(np.float32)).cuda()
    bias = torch.from_numpy(rng.standard_normal(co).astype(np.float32)).cuda()
    d = geom.conv_fwd(n, hw, hw, ci, co, 3, 1, 'SAME', act=act)
    return x32, w, bias, d


# the four SVHN classifier edges (c_h0_bn0 -> c_h0_conv1 and c_h0_bn1 -> c_h0_conv2 at 32x32x128, c_h1_bn* -> c_h1_conv* at 16x16x256) at
# sizes that take the halo kernel whole, cut into a halo head + generic tail (130 = 128 + 2 images of 32x32), and the generic kernel alone
CONV_SHAPES = [(64, 32, 128, 128), (130, 32, 128, 128), (3, 32, 128, 128), (130, 16, 256, 256), (64, 16, 256, 256), (2, 16, 256, 256)]


@pytest.mark.parametrize("n,hw,ci,co", CONV_SHAPES)
def test_conv_forward_with_bf16_stored_input_is_bit_identical(n, hw, ci, co):
    """tg_igemm_bnstat_bf16in_bf16 on x16 = RNE(x) (made by the bf16 batch-norm apply kernel) against the fp32-input bf16 launch on x: the
    stored activation and the batch-norm statistics identical bit for bit.  Negative control: x truncated toward zero must differ."""
    lib = _lib()
    rng = np.random.default_rng(7)
    rows = n * hw * hw
    xpre = torch.from_numpy(rng.standard_normal((rows, ci)).astype(np.float32) * 2).cuda()
    gamma, beta, _ = _bn_args(rows, ci, 1)
    segs = [n // 2 * hw * hw, (n - n // 2) * hw * hw] if n >= 2 else [rows]
    x32 = torch.zeros(rows, ci, device='cuda')
    x16 = torch.zeros(rows, ci, device='cuda', dtype=torch.bfloat16)
    one = (C.c_int32 * 1)(rows)
    bsums = torch.zeros(16 * ci, device='cuda', dtype=torch.float64)
    lib.call(BN_TRAIN['bf16'], lib.ptr(xpre), ci, lib.ptr(x16), ci, rows, ci, one, 1, lib.ptr(gamma), lib.ptr(beta), 1e-5, 0.9, None, None,
             lib.ptr(bsums), 0, lib.ptr(torch.zeros(2 * ci, device='cuda')), st())
    lib.call(BN_APPLY['f32'], lib.ptr(xpre), ci, lib.ptr(x32), ci, rows, ci, one, 1, lib.ptr(gamma), lib.ptr(beta), 1e-5, 0.9, None, None,
             lib.ptr(bsums), lib.ptr(torch.zeros(2 * ci, device='cuda')), st())          # the same batch sums
    torch.cuda.synchronize()
    assert (bits(x16) == bits(x32.to(torch.bfloat16))).all()
    _, w, bias, d = _conv_case(n, hw, ci, co, np.zeros((1,), np.float32))
    sa = (C.c_int32 * len(segs))(*segs)

    def run(name, xin):
        y = torch.full((rows, co), 7.0, device='cuda')
        sums = torch.full((32 * len(segs) * co,), 7.0, device='cuda', dtype=torch.float64)
        lib.call_igemm(name, d, lib.ptr(xin), lib.ptr(w), lib.ptr(bias), lib.ptr(y), sa, len(segs), lib.ptr(sums), 0, st())
        torch.cuda.synchronize()
        return bits(y), bits(sums)

    ref = run('tg_igemm_bnstat_' + BF16, x32)
    got = run('tg_igemm_bnstat_bf16in_bf16', x16)
    assert (ref[0] == got[0]).all(), "conv output differs"
    assert (ref[1] == got[1]).all(), "batch-norm statistics differ"
    bad = run('tg_igemm_bnstat_bf16in_bf16', rtz_bf16(x32))
    assert (bad[0] != ref[0]).any(), "negative control: truncated operands gave the same result"


@pytest.mark.parametrize("n,hw,ci,co", [(64, 32, 128, 128), (130, 32, 128, 128), (130, 16, 256, 256), (2, 16, 256, 256)])
def test_conv_forward_with_bf16_stored_input_special_values(n, hw, ci, co):
    """tg_igemm_bf16in_bf16 (no statistics) on RNE(x) against the fp32-input bf16 launch on x, x holding +-0, fp32 denormals, bf16 rounding
    ties and +-Inf: identical bits (NaN included).  RTZ input must differ."""
    lib = _lib()
    x_np = special_input((n, hw, hw, ci), 3)
    x32, w, bias, d = _conv_case(n, hw, ci, co, x_np)

    def run(name, xin):
        y = torch.full((n * hw * hw, co), 7.0, device='cuda')
        lib.call_igemm(name, d, lib.ptr(xin), lib.ptr(w), lib.ptr(bias), lib.ptr(y), st())
        torch.cuda.synchronize()
        return bits(y)

    ref = run('tg_igemm_' + BF16, x32)
    got = run('tg_igemm_bf16in_bf16', x32.to(torch.bfloat16))
    assert (ref == got).all()
    assert (run('tg_igemm_bf16in_bf16', rtz_bf16(x32)) != ref).any()


@pytest.mark.parametrize("n,hw,ci,co,special", [(64, 32, 128, 128, False), (64, 16, 256, 256, False), (96, 32, 128, 128, True),
                                                (64, 16, 256, 256, True)])
def test_filter_gradient_with_bf16_stored_input_is_bit_identical(n, hw, ci, co, special):
    """tg_wgrad_bf16in_bf16 on RNE(x) against tg_wgrad_bf16 on x at the split tg_wgrad_splits_bf16 picks (wgrad3x3_kernel both): the
    slabs identical bit for bit; dy stays fp32.  RTZ input must differ."""
    lib = _lib()
    from tg import geom
    rng = np.random.default_rng(9)
    x_np = special_input((n, hw, hw, ci), 4) if special else rng.standard_normal((n, hw, hw, ci)).astype(np.float32)
    x32 = torch.from_numpy(x_np).cuda()
    dy = torch.from_numpy(rng.standard_normal((n, hw, hw, co)).astype(np.float32)).cuda()
    desc = geom.conv_wgrad(n, hw, hw, ci, co, 3, 1, 'SAME')
    ns = geom.wgrad_splits(desc, True)
    assert ns > 0

    def run(name, xin):
        slab = torch.full((geom.wgrad_slab_floats(desc, ns),), 7.0, device='cuda')
        lib.call(name, desc, lib.ptr(xin), lib.ptr(dy), lib.ptr(slab), ns, st())
        torch.cuda.synchronize()
        return bits(slab)

    ref = run('tg_wgrad_' + BF16, x32)
    got = run('tg_wgrad_bf16in_bf16', x32.to(torch.bfloat16))
    assert (ref == got).all()
    assert (run('tg_wgrad_bf16in_bf16', rtz_bf16(x32)) != ref).any()


def test_conv_forward_reads_bf16_input_with_channel_padding():
    """ld > c on the bf16-stored input: the padding channels are zero in bf16 (what the apply kernel leaves) and the result equals the
    fp32-input launch on the same padded tensor."""
    lib = _lib()
    n, hw, c, ld, co = 8, 16, 200, 256, 128
    rng = np.random.default_rng(12)
    x = np.zeros((n, hw, hw, ld), np.float32)
    x[..., :c] = rng.standard_normal((n, hw, hw, c))
    x32, w, bias, d = _conv_case(n, hw, ld, co, x)
    x16 = x32.to(torch.bfloat16)
    assert (bits(x16.reshape(-1, ld)[:, c:]) == 0).all()
    outs = []
    for name, xin in (('tg_igemm_' + BF16, x32), ('tg_igemm_bf16in_bf16', x16)):
        y = torch.full((n * hw * hw, co), 7.0, device='cuda')
        lib.call_igemm(name, d, lib.ptr(xin), lib.ptr(w), lib.ptr(bias), lib.ptr(y), st())
        torch.cuda.synchronize()
        outs.append(bits(y))
    assert (outs[0] == outs[1]).all()


def test_unsupported_layer_is_refused_not_reinterpreted():
    """a bf16-stored input at a shape no bf16-input kernel serves (1x1 conv) is TG_ERR_INVALID."""
    lib = _lib()
    from tg import geom
    d = geom.conv_fwd(4, 16, 16, 128, 128, 1, 1, 'SAME')
    x = torch.zeros(4 * 16 * 16 * 128, device='cuda', dtype=torch.bfloat16)
    y = torch.zeros(4 * 16 * 16 * 128, device='cuda')
    with pytest.raises(lib.TgError):
        lib.call_igemm('tg_igemm_bf16in_bf16', d, lib.ptr(x), lib.ptr(y), None, lib.ptr(y), st())


# ---- whole step ---------------------------------------------------------------------------------------------------------------------------
SIZES3 = dict(B_G=100, L_C=50, U_C=50, L_D=20, U_D=80)          # BASELINE configs[3]


def _step_state(act, mode, iters=3):
    from Model.Good_GAN import Good_GAN
    cfg = G.make_config_goodgan('svhn', SIZES3, MFMA_DTYPE='bf16', ACT_DTYPE=act, EXEC_MODE=mode, USE_HIP_GRAPH=None, SEED=3)
    tr = G.fresh_trainer(cfg, Model=Good_GAN)
    tr.set_hyper(lambda_1=0.1, lambda_2=0.5)
    rng = np.random.default_rng(1234)
    img = lambda k: rng.uniform(-1, 1, (k, 32, 32, 3)).astype(np.float32)
    oh = lambda k: np.eye(10, dtype=np.float32)[rng.integers(0, 10, k)]
    losses = []
    for _ in range(iters):
        tr.feed(dict(x_l_c=img(50), y_l_c=oh(50), x_l_d=img(20), y_l_d=oh(20), x_u_d=img(80), x_u_c=img(50)))
        tr.sample_latent()
        tr.train_iteration()
        losses.append(np.asarray(tr.losses(), np.float32))
    torch.cuda.synchronize()
    state = {'losses': np.stack(losses)}
    for net, s in tr.cx.stores.items():
        for k in ('p', 'm', 'v', 's', 'ema'):
            t = getattr(s, k)
            if t is not None:
                state['%s/%s' % (net, k)] = t.detach().cpu().numpy().copy()
    return state, tr.bf16_act_edges


@pytest.mark.parametrize("mode", ['eager', 'plan', 'graph'])
def test_whole_step_is_bit_identical_with_bf16_stored_activations(mode):
    """configs[3] (SVHN, MFMA_DTYPE 'bf16', 100 / 50 / 50 / 20 / 80, same seed and Philox stream): three D+G+C iterations with ACT_DTYPE
    'f32' and 'bf16' — losses, every parameter, Adam slot, EMA shadow and BN moving statistic identical bit for bit, in eager launches,
    replayed launch plans and hipGraph replay.  The four classifier edges were really stored as bf16."""
    ref, e_ref = _step_state('f32', mode)
    got, e_got = _step_state('bf16', mode)
    assert e_ref == 0 and e_got == 4, (e_ref, e_got)
    assert set(ref) == set(got)
    for k in sorted(ref):
        a, b = ref[k], got[k]
        assert a.shape == b.shape and (a.view(np.int32) == b.view(np.int32)).all(), (mode, k, np.abs(a.astype(np.float64) - b).max())
