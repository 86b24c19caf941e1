"""CPU guard of tests/test_gpu_gemm_tiles.py's reach (no GPU needed: the library's host queries run without a device).

The dispatch lines of csrc/igemm.hip (launch_igemm<BM, BN, ...> / launch_wgrad<CT, NT, ...>) name the tile instantiations the generic
kernels can run.  Every dispatched igemm tile x operand type x schedule (uncut / cut along K) x epilogue family (plain, colsum, actsum,
bnstat, bnbwdstat) must be reached by a case of IGEMM_CASES, as tg_igemm_tile and tg_igemm_workspace_bytes evaluate it, or be listed in UNREACHABLE
with the reason the cost model can never pick it; every dispatched wgrad tile must be reached by a case of WGRAD_CASES (tg_wgrad_tile) in
both operand types.  A tile added to the dispatch, or a case that stops reaching what it names, fails here."""
import os
import re

from tg import lib

import test_gpu_gemm_tiles as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGEMM_HIP = os.path.join(ROOT, "tensorflow-implementation-of-triple-gan_amd", "csrc", "igemm.hip")

SCHEDULES = (False, True)          # cut along K
PRECS = (G.F32, G.BF16)

# (BM, BN, operand type) -> why tg::igemm_pick_tile never picks it (every schedule, every family)
UNREACHABLE = {
    (128, 128, G.F32): "fp32 64x64 efficiency 1.02 > 1.00: 64x64 is allowed wherever 128x128 is and needs at most 4x the rounds at a quarter "
                       "of the area, so its charged cost is always lower",
    (64, 128, G.F32): "fp32 64x64 efficiency 1.02 > 0.97: 64x64 is allowed wherever 64x128 is and needs at most 2x the rounds at half the "
                      "area, so its charged cost is always lower",
}


def dispatched(kind, text=None):
    """{(BM, BN)} of the launch_igemm<...> / launch_wgrad<...> calls in igemm.hip's dispatch (template definitions excluded)."""
    text = open(IGEMM_HIP).read() if text is None else text
    tiles = set(re.findall(r"\b%s<(\d+),\s*(\d+),[^>]*>\s*\(p," % kind, text))
    return {(int(a), int(b)) for a, b in tiles}


def reached_igemm():
    lib.load()
    out = {}
    for c in G.IGEMM_CASES:
        bm, bn, cut = G.query_tile(G.descs_of(c), c['segs'], c['prec'] == G.BF16)
        out.setdefault((bm, bn, c['prec'], cut, c['family']), []).append(c['id'])
    return out


def uncovered_igemm(tiles, reached):
    return ["%dx%d %s %s %s" % (bm, bn, p, 'cut' if cut else 'uncut', fam)
            for (bm, bn) in sorted(tiles) for p in PRECS for cut in SCHEDULES for fam in G.FAMILIES
            if (bm, bn, p) not in UNREACHABLE and (bm, bn, p, cut, fam) not in reached]


def test_every_case_reaches_the_tile_and_schedule_it_names():
    lib.load()
    wrong = []
    for c in G.IGEMM_CASES:
        got = G.query_tile(G.descs_of(c), c['segs'], c['prec'] == G.BF16)
        if got != tuple(c['tile']) + (c['cut'],):
            wrong.append("%s: names %s cut=%s, the cost model picks %s cut=%s" % (c['id'], c['tile'], c['cut'], got[:2], got[2]))
    for c in G.WGRAD_CASES:
        got = G.query_wgrad_tile(G.wgrad_desc(c))
        if got != c[1]:
            wrong.append("wgrad %s: names %s, tg_wgrad_tile picks %s" % (c[0], c[1], got))
    assert not wrong, "\n".join(wrong)
    assert len({c['id'] for c in G.IGEMM_CASES}) == len(G.IGEMM_CASES) and len({c[0] for c in G.WGRAD_CASES}) == len(G.WGRAD_CASES)


def test_every_dispatched_igemm_tile_is_covered():
    tiles = dispatched("launch_igemm")
    assert len(tiles) >= 5, tiles
    missing = uncovered_igemm(tiles, reached_igemm())
    assert not missing, "igemm tile x operand type x schedule x family without a case in tests/test_gpu_gemm_tiles.py (and not in " \
                        "UNREACHABLE): %s" % ", ".join(missing)
    # nothing covered is listed as unreachable
    reached = {k[:3] for k in reached_igemm()}
    assert not set(UNREACHABLE) & reached, "UNREACHABLE lists tiles a case reaches: %s" % (set(UNREACHABLE) & reached)


def test_unreachable_entries_name_dispatched_tiles():
    tiles = dispatched("launch_igemm")
    for (bm, bn, p), reason in UNREACHABLE.items():
        assert (bm, bn) in tiles, "UNREACHABLE lists %dx%d, which igemm.hip no longer dispatches" % (bm, bn)
        assert p in PRECS and reason


def test_every_dispatched_wgrad_tile_is_covered():
    tiles = dispatched("launch_wgrad")
    assert len(tiles) == 9, tiles
    reached = {G.query_wgrad_tile(G.wgrad_desc(c)) for c in G.WGRAD_CASES}
    missing = sorted(tiles - reached)
    assert not missing, "wgrad tiles without a case in tests/test_gpu_gemm_tiles.py: %s" % ", ".join("%dx%d" % t for t in missing)
    # the wgrad test runs every case in both operand types
    assert "@pytest.mark.parametrize(\"prec\", [F32, BF16])" in open(G.__file__).read()


def test_the_guard_sees_a_new_dispatch_line():
    """a launch_igemm<32, 64, ...> line added to the dispatch is reported as uncovered (the parser reads what igemm.hip dispatches)."""
    text = open(IGEMM_HIP).read()
    line = "  else if (bm == 64 && bn == 64) launch_igemm<64, 64, 2, 2>(p, s, bf16);\n"
    assert line in text
    fake = text.replace(line, line + "  else if (bm == 32 && bn == 64) launch_igemm<32, 64, 1, 2>(p, s, bf16);\n")
    tiles = dispatched("launch_igemm", fake)
    assert (32, 64) in tiles and (32, 64) not in dispatched("launch_igemm")
    assert any(m.startswith("32x64 ") for m in uncovered_igemm(tiles, reached_igemm()))
