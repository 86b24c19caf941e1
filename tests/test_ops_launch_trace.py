"""Which launches tg/ops.py issues, with which arguments, into which call-site buffers, in which order — checked without a GPU.

tests/launch_trace.py runs every route of ops.conv2d / deconv2d / filter_grad, the filter-prep cache and plan, the pieces tg/grad_penalty.py
shares with them and one small case of every other op on a device-less Context, with tg.lib.call recording the launch entry points instead
of issuing them.  Each case first asserts the launch names its route is made of (a shape that falls to another route fails there), then the
whole trace is compared with tests/golden/ops_launch_traces.json, recorded from tg/ops.py as it was BEFORE its conv2d was split into routed
stages.  A restructuring of the host code must leave the fixture byte-for-byte unchanged.  Regenerating it
(`python tests/launch_trace.py --record`) is a change of behaviour — another route, argument, buffer or launch order — and is to be named
as such in the commit message."""
import json

import pytest

import launch_trace as LT
from tg import ops


@pytest.fixture(scope='module')
def golden():
    with open(LT.FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('name', sorted(LT.CASES))
def test_launch_trace(name, golden, monkeypatch):
    trace = LT.run_case(name, monkeypatch)
    LT.check_route(name, trace)
    assert name in golden, "no recorded trace for %s" % name
    want = golden[name]
    for k, (got, exp) in enumerate(zip(trace, want)):
        assert got == exp, "%s: entry %d differs\n  got      %s\n  recorded %s" % (name, k, got, exp)
    assert len(trace) == len(want), "%s: %d entries, %d recorded: %s" % (name, len(trace), len(want), LT.names(trace))


def test_fixture_has_no_stale_case(golden):
    assert sorted(golden) == sorted(LT.CASES)


def test_lib_call_is_restored():
    from tg import lib, runtime
    assert lib.call.__module__ == 'tg.lib' and not isinstance(runtime._CTX, LT.TraceContext)


def test_every_launch_literal_of_ops_is_traced(golden):
    """every tg_* launch name written out in tg/ops.py occurs in at least one recorded trace — no exemptions"""
    seen = {n for trace in golden.values() for n in LT.names(trace)}
    missing = sorted(LT.launch_literals() - seen)
    assert not missing, "launches of tg/ops.py that no recorded trace issues: %s" % missing


def test_filter_prep_plan_keeps_the_call_site_buffers(golden):
    """the recording pass, the tg_filter_prep_multi_f32 pass and the one after name the same buffers in every launch they share"""
    trace = golden['filter_prep_plan']
    cuts = [k for k, e in enumerate(trace) if isinstance(e, str) and e.startswith('pass ')] + [len(trace)]
    passes = [trace[a + 1:b] for a, b in zip(cuts, cuts[1:])]
    assert len(passes) == 3
    prep = ('tg_wn_scale_f32', 'tg_filter_prep_f32', 'tg_filter_prep_multi_f32')
    assert [n for n in LT.names(passes[0]) if n in prep] == ['tg_wn_scale_f32', 'tg_filter_prep_f32', 'tg_filter_prep_f32']
    rest = [[e for e in p if e[0] not in prep] for p in passes]
    assert rest[0] == rest[1] == rest[2] and len(rest[0]) >= 10
    for p in passes[1:]:
        assert [n for n in LT.names(p) if n in prep] == ['tg_filter_prep_multi_f32']
        jobs = p[0][1]
        layers = [e for e in passes[0] if e[0] == 'tg_filter_prep_f32']
        assert [(j['src'], j['dst_same'], j['dst_tr']) for j in jobs] == [(e[1], e[9], e[10]) for e in layers]
    assert passes[1] == passes[2]


def test_require_f32_names_the_op():
    import torch
    from tg import lib
    from tg.runtime import Act
    a = Act(torch.zeros(64, dtype=torch.bfloat16), 1, 1, 2, 32, 32, dtype='bf16')
    for op in (ops.global_avgpool, lambda x: ops.global_avgpool_concat(x, None, 10)):
        with pytest.raises(lib.TgError, match=r'ops\.global_avgpool(_concat)?:'):
            op(a)
    with pytest.raises(lib.TgError, match=r'ops\.global_avgpool: '):
        ops.global_avgpool(a)
