"""CPU guard of tests/test_gpu_halo_tiles.py's reach (no GPU needed: the descriptors and the library's host queries run without a device).

launch_pipe in csrc/conv3x3_bf16.hip names the conv3x3_pipe_kernel<W, COLSUM, BF16, STAT2, IN16> instantiations, conv3x3_bf16_launch the
widths it dispatches to; launch in csrc/wgrad3x3.hip names the wgrad3x3_kernel<W, BF16, IN16> ones, wgrad3x3_launch its widths.  The
test module's entry-point maps must name exactly these instantiations, every (W, instantiation, epilogue branch) must be reached by a case
of HALO_CASES (policy 1), every (W, instantiation) by a case of WGRAD3_CASES, and every case must have the kernel's shape
(include/tg_kernels.h: 3x3 / stride 1 / SAME, width 16 / 32 / 64, whole 256-pixel tiles of image rows, 64 | ld_in with bf16 operands and
32 | ld_in with fp32 ones, 128 | c_out, at most 8 segments of whole images) and meet its tiles-per-workgroup regime on the 256 compute units
of an MI355X.  A new instantiation, or a case that stops reaching its kernel, fails here."""
import ctypes as C
import os
import re

import pytest

from tg import lib

import test_gpu_halo_tiles as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflow-implementation-of-triple-gan_amd", "csrc")
CONV_HIP = os.path.join(CSRC, "conv3x3_bf16.hip")
WGRAD_HIP = os.path.join(CSRC, "wgrad3x3.hip")
CUS = 256                                  # MI355X compute units (the library's fallback without a device is the same)
WIDTHS = (16, 32, 64)


def _flag(s):
    return {'true': True, 'false': False}[s.strip()]


def _function(text, head):
    """the text of the function that starts at `head` (up to the closing brace in column 0)."""
    i = text.index(head)
    return text[i:text.index("\n}\n", i)]


def conv_instantiations(text=None):
    """{(W, (COLSUM, BF16, STAT2, IN16))} that launch_pipe dispatches, W from conv3x3_bf16_launch's launch_pipe<16 / 32 / 64> calls."""
    text = open(CONV_HIP).read() if text is None else text
    body = _function(text, "void launch_pipe(")
    flags = set()
    for args in re.findall(r"hipLaunchKernelGGL\(\(conv3x3_pipe_kernel<W,([^>]*)>\)", body):
        f = [_flag(a) for a in args.split(",")]
        flags.add(tuple(f + [False] * (4 - len(f))))             # STAT2, IN16 default to false
    widths = {int(w) for w in re.findall(r"launch_pipe<(\d+)>\(p, s\)", _function(text, "int conv3x3_bf16_launch("))}
    return {(w, f) for w in widths for f in flags}


def wgrad_instantiations(text=None):
    """{(W, (BF16, IN16))} that wgrad3x3.hip's launch dispatches, W from wgrad3x3_launch's launch<16 / 32 / 64> calls."""
    text = open(WGRAD_HIP).read() if text is None else text
    body = _function(text, "void launch(const WParams& p")
    flags = set()
    for args in re.findall(r"hipLaunchKernelGGL\(\(wgrad3x3_kernel<W,([^>]*)>\)", body):
        f = [_flag(a) for a in args.split(",")]
        flags.add(tuple(f + [False] * (2 - len(f))))
    widths = {int(w) for w in re.findall(r"launch<(\d+)>\(p, bf16, in16, s\)", _function(text, "int wgrad3x3_launch("))}
    return {(w, f) for w in widths for f in flags}


def required(insts):
    """(W, flags, branch) keys every instantiation must reach.  Per width: plain forward / input gradient / forward without bias
    (COLSUM = 0; the bf16-stored input: forward), colsum and actsum (COLSUM, not STAT2), bnstat and bnbwdstat (STAT2; IN16: bnstat only).
    Per instantiation over the widths: the activations none / relu / leaky relu of plain and bnstat and of actsum's multiplier."""
    keys = set()
    for w, f in insts:
        colsum, _, stat2, in16 = f
        if not colsum:
            keys |= {(w, f, 'plain-fwd')} | (set() if in16 else {(w, f, 'plain-dgrad'), (w, f, 'plain-nobias')})
            keys |= {(None, f, 'plain-' + a) for a in H.ACTS}
        elif not stat2:
            keys |= {(w, f, 'colsum'), (w, f, 'actsum')} | {(None, f, 'actsum-' + a) for a in H.ACTS}
        else:
            keys |= {(w, f, 'bnstat')} | (set() if in16 else {(w, f, 'bnbwdstat')}) | {(None, f, 'bnstat-' + a) for a in H.ACTS}
    return keys


def reached(cases):
    """{key: [case ids]} of the policy-1 cases (the routing cases also run generic tails: they do not count)."""
    out = {}
    for c in cases:
        if c['policy'] != 1:
            continue
        w, f, fam = c['W'], H.ENTRY_KERNEL[c['entry']], c['family']
        if fam == 'plain':
            keys = [(w, f, 'plain-' + ('nobias' if not c['bias'] else c['op'])), (None, f, 'plain-' + (c['act'] or 'none'))]
            if not c['bias']:
                keys.append((w, f, 'plain-' + c['op']))
        elif fam == 'actsum':
            keys = [(w, f, 'actsum'), (None, f, 'actsum-' + (c['ymul_act'] or 'none'))]
        elif fam == 'bnstat':
            keys = [(w, f, 'bnstat'), (None, f, 'bnstat-' + (c['act'] or 'none'))]
        else:
            keys = [(w, f, fam)]
        for k in keys:
            out.setdefault(k, []).append(c['id'])
    return out


def _name(key):
    w, (colsum, bf16, stat2, in16), branch = key
    inst = "conv3x3_pipe_kernel<%s, %s, %s, %s, %s>" % ('W' if w is None else w, *('true' if b else 'false' for b in (colsum, bf16, stat2, in16)))
    return "%s %s" % (inst, branch)


def uncovered(cases, insts=None):
    insts = conv_instantiations() if insts is None else insts
    r = reached(cases)
    return sorted(_name(k) for k in required(insts) if k not in r)


def shape_errors(c, cus=CUS):
    """why case c does not have the halo kernel's shape or regime ([] when it does)."""
    n = H.n_images(c, cus)
    d = H.descriptor(c, n)
    bad = []
    if not (d.n_taps == 9 and d.n_group == 0 and d.s_y == d.s_x == 1 and d.os_y == d.os_x == 1 and d.oo_y == d.oo_x == 0):
        bad.append("not a 3x3 / stride-1 window")
    if not (d.h_v == d.h_in == d.h_out and d.w_v == d.w_in == d.w_out and d.w_in in WIDTHS):
        bad.append("not SAME on a width of 16 / 32 / 64")
    if sorted((int(d.dy[t]), int(d.dx[t])) for t in range(9)) != [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]:
        bad.append("taps are not the nine offsets of a 3x3 window")
    if d.h_in % (H.TILE_PX // d.w_in):
        bad.append("h = %d is not whole 256-pixel tiles" % d.h_in)
    if d.ld_in % (32 if c['prec'] == H.F32 else 64) or d.c_out % H.BN:
        bad.append("ld_in %d / c_out %d not whole channel chunks / column tiles" % (d.ld_in, d.c_out))
    if lib.ACT[c['act']] not in (lib.ACT['none'], lib.ACT['relu'], lib.ACT['lrelu']) or (c['ymul_act'] or 'none') not in H.ACTS:
        bad.append("an activation the register epilogue does not apply")
    segs = H.segments(c, n)
    if (c['family'] == 'plain') != (len(segs) == 0) or len(segs) > 8 or (segs and (sum(segs) != n or min(segs) < 1)):
        bad.append("segments %s of %d images" % (segs, n))
    if c['live'] and not c['live'] <= d.n_store:
        bad.append("live channels beyond n_store")
    if c['policy'] == 1 and not H.regime_holds(c['regime'], H.tiles_per_workgroup(n * H.tiles_per_image(c), cus)):
        bad.append("regime %s does not hold on %d CUs" % (c['regime'], cus))
    if c['policy'] == 0 and not 0 < H.head_images(n, H.tiles_per_image(c), cus, c['prec'] != H.F32) < n:
        bad.append("the launch is not cut into a halo head and a generic tail")
    return bad


# ---- tests ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_maps_name_exactly_the_dispatched_instantiations():
    conv = conv_instantiations()
    assert {w for w, _ in conv} == set(WIDTHS) and len(conv) == 24, sorted(conv)
    assert {f for _, f in conv} == set(H.ENTRY_KERNEL.values()), "conv3x3_pipe_kernel instantiations %s vs ENTRY_KERNEL %s" % (
        sorted({f for _, f in conv}), sorted(set(H.ENTRY_KERNEL.values())))
    wg = wgrad_instantiations()
    assert {w for w, _ in wg} == set(WIDTHS) and len(wg) == 9, sorted(wg)
    assert {f for _, f in wg} == set(H.WGRAD_ENTRY_KERNEL.values())


def test_every_instantiation_and_epilogue_branch_is_covered():
    missing = uncovered(H.HALO_CASES)
    assert not missing, "without a case in tests/test_gpu_halo_tiles.py: %s" % ", ".join(missing)
    assert len({c['id'] for c in H.HALO_CASES}) == len(H.HALO_CASES)


def test_every_family_and_operand_type_meets_the_three_regimes():
    seen = {}
    for c in H.HALO_CASES:
        if c['policy'] == 1:
            seen.setdefault((c['family'], c['prec']), set()).add(c['regime'])
    assert all(seen.get((f, p)) == set(H.REGIMES) for f in H.FAMILIES for p in (H.F32, H.BF16)), seen
    assert seen[('plain', H.BF16IN)] == seen[('bnstat', H.BF16IN)] == set(H.REGIMES), seen
    # routing: every column-sum family cut into a head and a tail, with a segment boundary in each part somewhere
    route = {(c['family'], c['regime']) for c in H.HALO_CASES if c['policy'] == 0}
    assert {f for f, _ in route} == set(H.FAMILIES[1:]) and {r for _, r in route} == {'head', 'tail'}


def test_shapes_the_cases_need():
    lib.load()
    wide = {(c['W'], c['family']) for c in H.HALO_CASES if c['c_out'] == 256 and c['policy'] == 1}
    assert wide == {(w, f) for w in WIDTHS for f in H.FAMILIES}, "families without a case of two column tiles: %s" % sorted(
        {(w, f) for w in WIDTHS for f in H.FAMILIES} - wide)
    assert any(c['live_in'] for c in H.HALO_CASES) and any(c['nseg'] == 8 for c in H.HALO_CASES)
    assert any(c['ld_out'] and c['ld_out'] > c['c_out'] and c['n_store'] < c['c_out'] for c in H.HALO_CASES)


@pytest.mark.parametrize("case", H.HALO_CASES, ids=[c['id'] for c in H.HALO_CASES])
def test_every_case_has_the_kernel_shape(case):
    lib.load()
    was = lib.call('tg_conv3x3_policy', 1)
    try:
        bad = shape_errors(case)
        assert not bad, "%s: %s" % (case['id'], "; ".join(bad))
        if case['prec'] != H.F32 and case['policy'] == 1:
            # the library's own routing: a bf16 launch of the halo kernel asks for exactly its packed filter as scratch
            d = H.descriptor(case, H.n_images(case, CUS))
            segs = [s * case['h'] * case['W'] for s in H.segments(case, d.n_img)]
            sa = (C.c_int32 * len(segs))(*segs) if segs else None
            ws = lib.call('tg_igemm_workspace_bytes', C.byref(d), 1, sa, len(segs), 2 if case['prec'] == H.BF16IN else 1)
            assert ws == (d.c_out // 128) * (d.ld_in // 64) * 9 * 128 * 128, "%s: the library does not route it to the halo kernel" % case['id']
    finally:
        lib.call('tg_conv3x3_policy', was)


def test_every_wgrad3x3_instantiation_is_covered_at_its_shape():
    lib.load()
    was = lib.call('tg_conv3x3_policy', 1)
    try:
        got = set()
        for c in H.WGRAD3_CASES:
            bf16, in16 = H.WGRAD_ENTRY_KERNEL[c[1]]
            d = H.wgrad3_desc(c)
            bmw = 128 if bf16 else 64
            assert d.w_in in WIDTHS and (d.h_in * d.w_in) % bmw == 0 and bmw % d.w_in == 0 and d.ld_in % 32 == 0 and d.c_out % 128 == 0, c[0]
            assert d.ld_out >= d.c_out
            T = d.n_img * d.h_in * d.w_in // bmw
            ragged, empty = H.wgrad3_splits(T)
            assert T % ragged and (empty - 1) * -(-T // empty) >= T, c[0]
            assert lib.call('tg_wgrad_splits_bf16' if bf16 else 'tg_wgrad_splits', C.byref(d)) >= 1, "%s: not a wgrad3x3 layer" % c[0]
            got.add((d.w_in, (bf16, in16)))
    finally:
        lib.call('tg_conv3x3_policy', was)
    assert got == wgrad_instantiations(), sorted(wgrad_instantiations() - got)
    assert any(c[5] == 32 for c in H.WGRAD3_CASES) and any(c[5] > 32 for c in H.WGRAD3_CASES)
    assert any(c[6] == 256 for c in H.WGRAD3_CASES) and any(c[7] and c[7] > c[6] for c in H.WGRAD3_CASES)


def test_the_guard_sees_a_new_dispatch_line_and_a_missing_case():
    text = open(CONV_HIP).read()
    line = "    else hipLaunchKernelGGL((conv3x3_pipe_kernel<W, false, true, false, true>), grid, dim3(512), 0, s, p);\n"
    assert line in text
    fake = text.replace(line, line.replace("else hip", "if (p.act == 7) hip").replace("false, true, false, true", "true, true, false, true"))
    insts = conv_instantiations(fake)
    assert (16, (True, True, False, True)) in insts and (16, (True, True, False, True)) not in conv_instantiations()
    assert any(m.startswith("conv3x3_pipe_kernel<16, true, true, false, true> ") for m in uncovered(H.HALO_CASES, insts))
    # a case that is the sole cover of a key: without it that key is reported
    r = reached(H.HALO_CASES)
    sole = {ids[0] for k, ids in r.items() if len(ids) == 1 and k in required(conv_instantiations())}
    assert sole
    for cid in sorted(sole):
        assert uncovered([c for c in H.HALO_CASES if c['id'] != cid]), cid
