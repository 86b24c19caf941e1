"""CPU guard of tests/test_gpu_packed_tiles.py's reach (no GPU needed: the source text and the library's host queries).

The launchers of csrc/packed_conv.hip name packed_fwd<1|2> and packed_wgrad<1|2> (each at wgrad_rows 4 and 8), those of csrc/narrow.hip
narrow_dgrad<1..4> and, through the TG_NARROW_WGRAD macro, narrow_wgrad<1..4, 4|8>.  Every one of them must be reached by a case of
PACKED_CASES / NARROW_CASES or be listed in UNREACHABLE with the arithmetic that shows no supported shape gets there; every case must be
a shape the library serves and reach the instantiation it claims; tg_*_supported must agree with this module's restatement of shape_ok
(LDS sizes recomputed from the constants parsed out of the .hip files) around every boundary; and the edges the suite was written for
(EDGES) must be present in the tables.  A new dispatch line, or a case that goes missing, fails here."""
import os
import re

import numpy as np
import pytest

from tg import lib

import test_gpu_packed_tiles as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflow-implementation-of-triple-gan_amd", "csrc")
PACKED_HIP = os.path.join(CSRC, "packed_conv.hip")
NARROW_HIP = os.path.join(CSRC, "narrow.hip")
LDS_LIMIT = 64 * 1024


def constants(path):
    return {k: int(v) for k, v in re.findall(r"^constexpr int (\w+) = (\d+);", open(path).read(), flags=re.M)}


PK, NR = constants(PACKED_HIP), constants(NARROW_HIP)


def packed_instantiations(text=None):
    text = open(PACKED_HIP).read() if text is None else text
    out = set()
    for name, nt in re.findall(r"hipLaunchKernelGGL\((packed_fwd|packed_wgrad)<(\d+)>", text):
        out |= {(name, int(nt))} if name == 'packed_fwd' else {(name, int(nt), rows) for rows in (4, 8)}
    return out


def narrow_instantiations(text=None):
    text = open(NARROW_HIP).read() if text is None else text
    out = {('narrow_dgrad', int(co)) for co in re.findall(r"hipLaunchKernelGGL\(narrow_dgrad<(\d+)>", text)}
    macro = text[text.index("#define TG_NARROW_WGRAD(CO_)"):text.index("#undef TG_NARROW_WGRAD")]
    xus = {int(xu) for xu in re.findall(r"hipLaunchKernelGGL\(\(narrow_wgrad<CO_, (\d+)>\)", macro)}
    cos = {int(co) for co in re.findall(r"TG_NARROW_WGRAD\((\d+)\);", macro)}
    return out | {('narrow_wgrad', co, xu) for co in cos for xu in xus}


# ---- shape_ok restated (csrc/packed_conv.hip, csrc/narrow.hip), LDS sizes from the parsed constants --------------------------------------
def packed_kpad(c_in):
    return (9 * c_in + 1) & ~1


def packed_fwd_lds(c_in, c_out):
    return (packed_kpad(c_in) * c_out + (PK['FROWS'] + 2) * PK['PCOLS'] * c_in + packed_kpad(c_in)) * 4


def packed_wgrad_lds(w, c_in, c_out):
    return (3 * (w + 2) * c_in + w * c_out) * 4


def packed_ok(n, h, w, c_in, c_out):
    return (n > 0 and h > 0 and w > 0 and 1 <= c_in <= PK['MAX_CIN'] and c_out in (32, 64) and w % 16 == 0 and w <= 32 and h % 4 == 0
            and packed_fwd_lds(c_in, c_out) <= LDS_LIMIT and packed_wgrad_lds(w, c_in, c_out) <= LDS_LIMIT)


def narrow_kpad(co):
    return (NR['TAPS'] * co + 1) & ~1


def narrow_dgrad_lds(c_out, ci_p):
    return (narrow_kpad(c_out) * ci_p + (2 * NR['DROWS'] + 3) * NR['PC'] * c_out + narrow_kpad(c_out)) * 4


def narrow_wgrad_lds(w, c_out, ci_p):
    return (w * ci_p + 5 * (2 * w + 3) * c_out) * 4


def narrow_ok(n, h, w, c_out, ci_p):
    return (n > 0 and h > 0 and w > 0 and 1 <= c_out <= 4 and 32 <= ci_p <= 32 * NR['MAXQ'] and ci_p % 32 == 0 and w % 16 == 0 and w <= 32
            and h % NR['RB'] == 0 and narrow_dgrad_lds(c_out, ci_p) <= LDS_LIMIT and narrow_wgrad_lds(w, c_out, ci_p) <= LDS_LIMIT)


def narrow_max_ci_p(c_out):
    return max(q for q in range(32, 32 * NR['MAXQ'] + 1, 32) if narrow_ok(1, 4, 16, c_out, q))


# instantiation -> why no supported shape launches it (checked below, not taken on trust)
UNREACHABLE = {
    ('narrow_wgrad', 4, 8): "XU = 8 needs w * ci_p / 4 > 1024, i.e. w = 32 and ci_p >= 160; dgrad_lds_bytes(4, 160) = (100 * 160 + 19 * 35 * 4 + 100) * 4 "
                            "= 75040 > 65536: shape_ok admits c_out = 4 up to ci_p = 128 only",
}


def reached(packed=None, narrow=None):
    out = {}
    for c in (P.PACKED_CASES if packed is None else packed):
        for k in P.packed_reach(c):
            out.setdefault(k, []).append(c['id'])
    for c in (P.NARROW_CASES if narrow is None else narrow):
        for k in P.narrow_reach(c):
            out.setdefault(k, []).append(c['id'])
    return out


def uncovered(insts=None, packed=None, narrow=None):
    insts = packed_instantiations() | narrow_instantiations() if insts is None else insts
    r = reached(packed, narrow)
    return sorted(k for k in insts if k not in r and k not in UNREACHABLE)


# ---- the edges the tables must hold: name -> predicate over (packed cases, narrow cases) ---------------------------------------------------
def _any(cases, f):
    return any(f(c) for c in cases)


def _edges():
    E = {}
    pk = lambda name, f: E.__setitem__('packed: ' + name, lambda p, n, f=f: _any(p, f))
    nr = lambda name, f: E.__setitem__('narrow: ' + name, lambda p, n, f=f: _any(n, f))
    for v in (1, 2, 13, 16):
        pk('c_in = %d' % v, lambda c, v=v: c['c_in'] == v)
    pk('an odd c_in with an odd K (kpad rounds up)', lambda c: c['c_in'] % 2 == 1 and c['c_in'] not in (1, 13))
    for co in (32, 64):
        for w in (16, 32):
            pk('c_out %d at w = %d' % (co, w), lambda c, co=co, w=w: c['c_out'] == co and c['w'] == w)
        for ln in (1, 10):
            pk('c_out %d with lab_n = %d' % (co, ln), lambda c, co=co, ln=ln: c['c_out'] == co and c['lab_n'] == ln)
    for h in (4, 8, 12, 20):
        pk('h = %d' % h, lambda c, h=h: c['h'] == h)
        nr('h = %d' % h, lambda c, h=h: c['h'] == h)
    pk('n = 1', lambda c: c['n'] == 1)
    pk('n >= 3', lambda c: c['n'] >= 3)
    pk('no activation', lambda c: c['act'] == 'none')
    pk('relu', lambda c: c['act'] == 'relu')
    pk('leaky relu with a slope other than 0.2', lambda c: c['act'] == 'lrelu' and c['alpha'] not in (0.0, 0.2, 1.0))
    pk('bias NULL', lambda c: not c['bias'])
    pk('bias', lambda c: c['bias'])
    pk('labels NULL', lambda c: c['lab_n'] is None)
    pk('labels NULL with channels to zero behind the convolution', lambda c: c['lab_n'] is None and c['ld_y'] > c['c_out'])
    pk('ld_y = c_out', lambda c: c['ld_y'] == c['c_out'])
    pk('ld_y = c_out + lab_n, not a multiple of 32', lambda c: c['lab_n'] and c['ld_y'] == c['c_out'] + c['lab_n'] and c['ld_y'] % 32)
    pk('ld_y wider than pad32(c_out + lab_n)', lambda c: c['lab_n'] and c['ld_y'] > P.pad32(c['c_out'] + c['lab_n']))
    pk('ld_x = c_in, odd', lambda c: c['ld_x'] == c['c_in'] and c['c_in'] % 2 == 1)
    pk('ld_x = 32', lambda c: c['ld_x'] == 32)
    pk('ld_x = 64', lambda c: c['ld_x'] == 64)
    pk('ld_dy = c_out', lambda c: c['ld_dy'] == c['c_out'])
    pk('ld_dy = c_out + 4', lambda c: c['ld_dy'] == c['c_out'] + 4)
    for co in (1, 2, 3, 4):
        nr('c_out = %d' % co, lambda c, co=co: c['c_out'] == co)
    nr('ci_p = 32', lambda c: c['ci_p'] == 32)
    nr('ci_p = 256', lambda c: c['ci_p'] == 32 * NR['MAXQ'])
    nr('the largest ci_p of c_out = 4', lambda c: c['c_out'] == 4 and c['ci_p'] == narrow_max_ci_p(4))
    nr('the largest ci_p of c_out = 3', lambda c: c['c_out'] == 3 and c['ci_p'] == narrow_max_ci_p(3))
    nr('c_in = ci_p', lambda c: c['c_in'] == c['ci_p'])
    nr('c_in well below ci_p', lambda c: c['c_in'] <= c['ci_p'] - 16)
    nr('w = 16', lambda c: c['w'] == 16)
    nr('w = 32', lambda c: c['w'] == 32)
    nr('n = 1', lambda c: c['n'] == 1)
    nr('n >= 3', lambda c: c['n'] >= 3)
    nr('scale_a NULL', lambda c: not c['scale'])
    nr('scale_a', lambda c: c['scale'])
    nr('ld_dy = c_out', lambda c: c['ld_dy'] == c['c_out'])
    nr('ld_dy = 32', lambda c: c['ld_dy'] == 32)
    nr('ld_dy = 64', lambda c: c['ld_dy'] == 64)
    nr('ld_dx = ci_p', lambda c: c['ld_dx'] == c['ci_p'])
    nr('ld_dx wider than ci_p', lambda c: c['ld_dx'] > c['ci_p'])
    nr('ld_x = ci_p', lambda c: c['ld_x'] == c['ci_p'])
    nr('ld_x wider than ci_p', lambda c: c['ld_x'] > c['ci_p'])
    nr('an x row of exactly 1024 units (the last shape of XU = 4)', lambda c: c['w'] * (c['ci_p'] // 4) == 1024)
    nr('the first shape of XU = 8 (w = 32, ci_p = 160)', lambda c: c['w'] == 32 and c['ci_p'] == 160)
    return E


EDGES = _edges()


def missing_edges(packed=None, narrow=None):
    packed, narrow = P.PACKED_CASES if packed is None else packed, P.NARROW_CASES if narrow is None else narrow
    return sorted(name for name, f in EDGES.items() if not f(packed, narrow))


# ---- tests ------------------------------------------------------------------------------------------------------------------------------------
def test_the_parsed_dispatch_is_what_the_suite_was_written_for():
    assert packed_instantiations() == {('packed_fwd', 1), ('packed_fwd', 2)} | {('packed_wgrad', nt, r) for nt in (1, 2) for r in (4, 8)}
    assert narrow_instantiations() == {('narrow_dgrad', co) for co in (1, 2, 3, 4)} | {('narrow_wgrad', co, xu) for co in (1, 2, 3, 4) for xu in (4, 8)}
    assert set(PK) >= {'MAX_CIN', 'FROWS', 'PCOLS'} and set(NR) >= {'TAPS', 'MAXQ', 'PC', 'DROWS', 'RB'}
    # the predicates the cases' reach is computed from are the launchers' own
    assert "int wgrad_rows(int h) { return h % 8 == 0 ? 8 : 4; }" in open(PACKED_HIP).read()
    assert "const bool big = w * (ci_p / 4) > 1024;" in open(NARROW_HIP).read()


def test_every_instantiation_is_covered_or_shown_unreachable():
    missing = uncovered()
    assert not missing, "without a case in tests/test_gpu_packed_tiles.py: %s" % missing
    ids = [c['id'] for c in P.PACKED_CASES + P.NARROW_CASES]
    assert len(set(ids)) == len(ids)
    r = reached()
    for k, why in UNREACHABLE.items():
        assert k in narrow_instantiations() and k not in r and why
    # the arithmetic behind UNREACHABLE: no shape shape_ok admits has c_out = 4 and more than 1024 units per x row
    for w in (16, 32):
        for ci_p in range(32, 32 * NR['MAXQ'] + 1, 32):
            if narrow_ok(1, 4, w, 4, ci_p):
                assert w * (ci_p // 4) <= 1024
    assert narrow_dgrad_lds(4, 160) == 75040 > LDS_LIMIT and narrow_max_ci_p(4) == 128
    # and XU = 8 is reachable for the others
    assert all(narrow_ok(1, 4, 32, co, 160) for co in (1, 2, 3))


def test_every_case_is_served_and_reaches_what_it_names():
    lib.load()
    for c in P.PACKED_CASES:
        assert lib.call('tg_conv3x3_packed_supported', c['n'], c['h'], c['w'], c['c_in'], c['c_out']) == 1, c['id']
        assert c['ld_x'] >= c['c_in'] and c['ld_y'] >= c['c_out'] + (c['lab_n'] or 0) and c['ld_dy'] >= c['c_out'] and c['ld_dy'] % 4 == 0, c['id']
        nt, rows = c['c_out'] // 32, (8 if c['h'] % 8 == 0 else 4)
        assert P.packed_reach(c) == [('packed_fwd', nt), ('packed_wgrad', nt, rows)]
        # the workspace is one slab per (image, block of wgrad_rows rows): the library's size names the row count it launches with
        need = lib.call('tg_conv3x3_packed_wgrad_workspace_bytes', c['n'], c['h'], c['w'], c['c_in'], c['c_out'])
        assert need == c['n'] * (c['h'] // rows) * 9 * c['c_in'] * c['c_out'] * 4, c['id']
    for c in P.NARROW_CASES:
        assert lib.call('tg_deconv5x5s2_narrow_supported', c['n'], c['h'], c['w'], c['c_out'], c['ci_p']) == 1, c['id']
        assert 1 <= c['c_in'] <= c['ci_p'] <= min(c['ld_dx'], c['ld_x']) and c['ld_dy'] >= c['c_out'] and c['ld_x'] % 4 == 0, c['id']
        big = c['w'] * (c['ci_p'] // 4) > 1024
        assert P.narrow_reach(c) == [('narrow_dgrad', c['c_out']), ('narrow_wgrad', c['c_out'], 8 if big else 4)]
        assert ('big' in c['id']) == big, c['id']


def test_supported_queries_agree_with_shape_ok_around_every_boundary():
    lib.load()
    ns, hs, ws = (0, 1, 3), (0, 2, 4, 6, 8, 12, 20), (0, 8, 16, 24, 32, 48, 64)
    for n in ns:
        for h in hs:
            for w in ws:
                for c_in in (0, 1, 2, 13, 15, 16, 17, 32):
                    for c_out in (0, 16, 32, 48, 64, 96, 128):
                        assert lib.call('tg_conv3x3_packed_supported', n, h, w, c_in, c_out) == int(packed_ok(n, h, w, c_in, c_out)), (n, h, w, c_in, c_out)
                for c_out in (0, 1, 2, 3, 4, 5):
                    for ci_p in (0, 16, 32, 48, 64, 96, 128, 160, 192, 224, 256, 288):
                        assert lib.call('tg_deconv5x5s2_narrow_supported', n, h, w, c_out, ci_p) == int(narrow_ok(n, h, w, c_out, ci_p)), (n, h, w, c_out, ci_p)
    # the LDS terms: those of packed_conv.hip and narrow.hip's filter gradient never bind inside the other terms (largest shape below)
    assert packed_fwd_lds(PK['MAX_CIN'], 64) == 48960 <= LDS_LIMIT and packed_wgrad_lds(32, PK['MAX_CIN'], 64) == 14720 <= LDS_LIMIT
    assert narrow_wgrad_lds(32, 4, 32 * NR['MAXQ']) == 38128 <= LDS_LIMIT
    # narrow.hip's input gradient: binds for c_out = 3 and 4
    assert [narrow_max_ci_p(co) for co in (1, 2, 3, 4)] == [256, 256, 160, 128]
    assert narrow_dgrad_lds(3, 160) <= LDS_LIMIT < narrow_dgrad_lds(3, 192) and narrow_dgrad_lds(4, 128) <= LDS_LIMIT < narrow_dgrad_lds(4, 160)


def test_the_envelope_tables_sit_on_the_boundaries():
    lib.load()
    text = {'packed': open(PACKED_HIP).read(), 'narrow': open(NARROW_HIP).read()}
    for which, table, ok in (('packed', P.PACKED_ENVELOPE, packed_ok), ('narrow', P.NARROW_ENVELOPE, narrow_ok)):
        body = text[which][text[which].index("bool shape_ok("):]
        body = body[:body.index("\n}\n")]
        for term, inside, outside in table:
            assert ok(*inside) and not ok(*outside), (term, inside, outside)
            assert term.split('(')[0].split(' ')[0] in body, "%s is not a term of %s's shape_ok" % (term, which)
        # every term of shape_ok has a pair, except the LDS terms shown above to be out of reach
        terms = [t.strip() for t in re.split(r"&&", body[body.index("return") + 6:].rstrip(';'))]
        unbound = {'packed': ('fwd_lds_bytes', 'wgrad_lds_bytes'), 'narrow': ('wgrad_lds_bytes',)}[which]
        named = {t for t, _, _ in table}
        for t in terms:
            t = t.strip('() ;\n')
            if any(t.startswith(u) for u in unbound):
                continue
            assert any(t.startswith(nm.split('(')[0]) or nm in t for nm in named), "shape_ok term %r of %s has no envelope pair" % (t, which)


def test_the_edges_are_in_the_tables():
    assert not missing_edges(), missing_edges()


def test_controls_are_told_apart_by_the_float64_reference_alone():
    """a sample of cases on the CPU (the GPU test asserts it for every case): both wrong references differ from the float64 reference by
    more than 10 x TOL x sum|terms| somewhere."""
    from kernel_check import rejected
    for c in (P.PACKED_CASES[0], P.PACKED_CASES[2], P.PACKED_CASES[4]):
        x, wt, bias, lab, dy = P.packed_inputs(c)
        for ref, sabs, bf, cut in (P.packed_fwd_refs(c, x, wt, bias), P.packed_wgrad_refs(c, x, dy)):
            assert rejected(ref, bf, sabs) and rejected(ref, cut, sabs), c['id']
            assert not rejected(ref, ref, sabs)
    for c in (P.NARROW_CASES[0], P.NARROW_CASES[8]):
        x, wt, dy, scale = P.narrow_inputs(c)
        for ref, sabs, bf, cut in (P.narrow_dgrad_refs(c, wt, dy, scale), P.narrow_wgrad_refs(c, x, dy)):
            assert rejected(ref, bf, sabs) and rejected(ref, cut, sabs), c['id']


def test_the_guard_sees_a_new_dispatch_line_and_a_missing_case():
    text = open(NARROW_HIP).read()
    line = "    case 3: TG_NARROW_WGRAD(3); break;\n"
    assert line in text
    insts = narrow_instantiations(text.replace(line, line + "    case 5: TG_NARROW_WGRAD(5); break;\n"))
    assert ('narrow_wgrad', 5, 8) in insts and ('narrow_wgrad', 5, 8) in uncovered(insts | packed_instantiations())
    ptext = open(PACKED_HIP).read()
    line = "  else hipLaunchKernelGGL(packed_fwd<2>, grid"
    assert line in ptext
    insts = packed_instantiations(ptext.replace(line, "  else if (c_out == 96) hipLaunchKernelGGL(packed_fwd<3>, grid", 1))
    assert ('packed_fwd', 3) in uncovered(insts | narrow_instantiations())
    # a case that is the sole cover of an instantiation: without it the instantiation is reported
    sole = {ids[0]: k for k, ids in reached().items() if len(ids) == 1}
    assert sole
    for cid, k in sole.items():
        left = uncovered(packed=[c for c in P.PACKED_CASES if c['id'] != cid], narrow=[c for c in P.NARROW_CASES if c['id'] != cid])
        assert k in left, cid
    # a case that is the sole cover of an edge: without it the edge is reported
    n_sole = 0
    for cid in [c['id'] for c in P.PACKED_CASES + P.NARROW_CASES]:
        gone = missing_edges([c for c in P.PACKED_CASES if c['id'] != cid], [c for c in P.NARROW_CASES if c['id'] != cid])
        n_sole += bool(gone)
    assert n_sole >= 3
