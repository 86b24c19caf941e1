"""CPU tests of tg/executor.py: the launch-mode decision of Train.train_iteration as a table, and the measurement schedule of
config.EXEC_MODE = 'auto' with a fake clock.  No device, no extension."""
import pytest

from tg import executor as X

# config.EXEC_MODE, use_graph (train_iteration's argument merged with config.USE_HIP_GRAPH), the RNG replays (PhiloxRNG), the exchange
# backend allows captures (tg.dist.graphs_allowed), what auto_pick returns (None: it must not be called) -> how, graph_refused.
# Written out row by row from the decision the step has made since EXEC_MODE = 'auto' exists: a change of behaviour is a change of a row.
LAUNCH_TABLE = [
    ('auto',    None,  True,  True,  'plan',  'plan',    False),
    ('auto',    None,  True,  True,  'graph', 'graph',   False),
    ('auto',    None,  True,  False, None,    'plan',    False),
    ('auto',    None,  False, True,  None,    'overlap', False),
    ('auto',    None,  False, False, None,    'overlap', False),
    ('auto',    False, True,  True,  None,    'overlap', False),
    ('auto',    False, True,  False, None,    'overlap', False),
    ('auto',    False, False, True,  None,    'overlap', False),
    ('auto',    False, False, False, None,    'overlap', False),
    ('auto',    True,  True,  True,  None,    'graph',   False),
    ('auto',    True,  True,  False, None,    'eager',   True),
    ('auto',    True,  False, True,  None,    'eager',   False),
    ('auto',    True,  False, False, None,    'eager',   False),
    ('eager',   None,  True,  True,  None,    'eager',   False),
    ('eager',   None,  True,  False, None,    'eager',   False),
    ('eager',   None,  False, True,  None,    'eager',   False),
    ('eager',   None,  False, False, None,    'eager',   False),
    ('eager',   False, True,  True,  None,    'eager',   False),
    ('eager',   False, True,  False, None,    'eager',   False),
    ('eager',   False, False, True,  None,    'eager',   False),
    ('eager',   False, False, False, None,    'eager',   False),
    ('eager',   True,  True,  True,  None,    'graph',   False),
    ('eager',   True,  True,  False, None,    'eager',   True),
    ('eager',   True,  False, True,  None,    'eager',   False),
    ('eager',   True,  False, False, None,    'eager',   False),
    ('overlap', None,  True,  True,  None,    'overlap', False),
    ('overlap', None,  True,  False, None,    'overlap', False),
    ('overlap', None,  False, True,  None,    'overlap', False),
    ('overlap', None,  False, False, None,    'overlap', False),
    ('overlap', False, True,  True,  None,    'overlap', False),
    ('overlap', False, True,  False, None,    'overlap', False),
    ('overlap', False, False, True,  None,    'overlap', False),
    ('overlap', False, False, False, None,    'overlap', False),
    ('overlap', True,  True,  True,  None,    'graph',   False),
    ('overlap', True,  True,  False, None,    'overlap', True),
    ('overlap', True,  False, True,  None,    'overlap', False),
    ('overlap', True,  False, False, None,    'overlap', False),
    ('plan',    None,  True,  True,  None,    'plan',    False),
    ('plan',    None,  True,  False, None,    'plan',    False),
    ('plan',    None,  False, True,  None,    'overlap', False),
    ('plan',    None,  False, False, None,    'overlap', False),
    ('plan',    False, True,  True,  None,    'plan',    False),
    ('plan',    False, True,  False, None,    'plan',    False),
    ('plan',    False, False, True,  None,    'overlap', False),
    ('plan',    False, False, False, None,    'overlap', False),
    ('plan',    True,  True,  True,  None,    'graph',   False),
    ('plan',    True,  True,  False, None,    'overlap', True),
    ('plan',    True,  False, True,  None,    'overlap', False),
    ('plan',    True,  False, False, None,    'overlap', False),
    ('graph',   None,  True,  True,  None,    'graph',   False),
    ('graph',   None,  True,  False, None,    'eager',   True),
    ('graph',   None,  False, True,  None,    'eager',   False),
    ('graph',   None,  False, False, None,    'eager',   False),
    ('graph',   False, True,  True,  None,    'eager',   False),
    ('graph',   False, True,  False, None,    'eager',   False),
    ('graph',   False, False, True,  None,    'eager',   False),
    ('graph',   False, False, False, None,    'eager',   False),
    ('graph',   True,  True,  True,  None,    'graph',   False),
    ('graph',   True,  True,  False, None,    'eager',   True),
    ('graph',   True,  False, True,  None,    'eager',   False),
    ('graph',   True,  False, False, None,    'eager',   False),
]


def test_the_launch_table_is_complete():
    inputs = [r[:4] for r in LAUNCH_TABLE]
    assert len(LAUNCH_TABLE) == 61 and len(set(inputs)) == 60                 # 5 modes x 3 x 2 x 2, the one row with a choice twice
    assert {r[0] for r in LAUNCH_TABLE} == {'auto', 'eager', 'overlap', 'plan', 'graph'}
    assert [r[:5] for r in LAUNCH_TABLE if r[4] is not None] == [('auto', None, True, True, 'plan'), ('auto', None, True, True, 'graph')]


@pytest.mark.parametrize('mode,use_graph,replayable,allowed,pick,how,refused', LAUNCH_TABLE)
def test_resolve_launch_reproduces_the_table(mode, use_graph, replayable, allowed, pick, how, refused):
    calls = []

    def auto_pick():
        calls.append(1)
        if pick is None:
            raise AssertionError("auto_pick called for %r" % ((mode, use_graph, replayable, allowed),))
        return pick
    got = X.resolve_launch(mode, use_graph, replayable, allowed, auto_pick)
    assert got == (how, refused) and type(got[1]) is bool
    assert len(calls) == (0 if pick is None else 1)       # AutoMode.next counts iterations and synchronises the device: once, and only there


@pytest.mark.parametrize('use_graph', [None, False, True])
@pytest.mark.parametrize('replayable', [True, False])
@pytest.mark.parametrize('allowed', [True, False])
def test_an_unknown_mode_launches_like_eager(use_graph, replayable, allowed):
    assert X.resolve_launch('bogus', use_graph, replayable, allowed, None) == X.resolve_launch('eager', use_graph, replayable, allowed, None)


def test_auto_schedule_with_the_shipped_constants():
    from Training.Train_goodGAN import Train
    assert (X.AUTO_SETTLE, X.AUTO_TIMED, X.AUTO_BLOCKS, X.AUTO_ITERS) == (3, 5, 3, 49)
    assert (Train.AUTO_SETTLE, Train.AUTO_TIMED, Train.AUTO_BLOCKS, Train.AUTO_ITERS) == (3, 5, 3, 49)
    for n in range(X.AUTO_ITERS):
        mode, opens, closes, decides = X.auto_schedule(n, X.AUTO_SETTLE, X.AUTO_TIMED, X.AUTO_BLOCKS)
        b, k = divmod(n, 8)
        assert mode == ('plan', 'graph')[b % 2], n                      # plan, graph, plan, ... in blocks of 8
        assert opens == (k == 3 and n < 48), n                          # after the 3 settling iterations of each block
        assert closes == (k == 0 and n > 0), n                          # 5 timed iterations later, at offset 0 of the next block
        assert decides == (n == 48), n                                  # AUTO_ITERS = 49 iterations including the deciding one
    assert sum(X.auto_schedule(n, 3, 5, 3)[1] for n in range(49)) == 6 == sum(X.auto_schedule(n, 3, 5, 3)[2] for n in range(49))
    # other shapes: blocks of settle + timed, 2 * blocks of them, then the decision
    assert [X.auto_schedule(n, 1, 2, 1) for n in range(7)] == [
        ('plan', False, False, False), ('plan', True, False, False), ('plan', False, False, False),
        ('graph', False, True, False), ('graph', True, False, False), ('graph', False, False, False), ('plan', False, True, True)]


class FakeClock(object):
    """the test moves `now` on by what each iteration costs; a reading (device synchronisation + host time in the trainer) is counted."""

    def __init__(self):
        self.now, self.reads = 100.0, 0

    def __call__(self):
        self.reads += 1
        return self.now


def test_auto_mode_times_blocks_takes_the_fastest_and_stops_reading_the_clock():
    clock = FakeClock()
    decided = []

    def decide(times):
        decided.append(dict(times))
        pick = min(times, key=times.get)
        return pick, dict(times)
    auto = X.AutoMode(clock, decide)
    assert auto.chosen() == (None, {}) and auto.n == 0
    # seconds per iteration of (candidate, its block number): the first block of each is slow (page-ins), the rest differ a little
    cost = {('plan', 0): 0.028, ('plan', 1): 0.0146, ('plan', 2): 0.0150, ('graph', 0): 0.020, ('graph', 1): 0.0152, ('graph', 2): 0.0149}
    ran = []
    for n in range(X.AUTO_ITERS + 20):
        mode = auto.next()
        ran.append(mode)
        if n < 48:
            assert mode == X.auto_schedule(n, 3, 5, 3)[0] and auto.chosen()[0] is None
            clock.now += cost[(mode, n // 16)]                    # the iteration itself
        if n == 20:                                               # one block of each timed so far: partial timings, nothing chosen
            pick, partial = auto.chosen()
            assert pick is None and partial == {'plan': pytest.approx(0.028), 'graph': pytest.approx(0.020)}
    assert len(decided) == 1 and decided[0] == {'plan': pytest.approx(0.0146), 'graph': pytest.approx(0.0149)}      # fastest block / timed
    assert {k: [round(x, 6) for x in v] for k, v in auto.times.items()} == {'plan': [0.028, 0.0146, 0.015], 'graph': [0.02, 0.0152, 0.0149]}
    assert list(decided[0]) == ['plan', 'graph']                  # ties go to the first candidate in tg.dist.decide_together
    assert auto.chosen() == ('plan', decided[0]) and auto.pick == 'plan' and auto.n == 49
    assert ran[48:] == ['plan'] * 21                              # the deciding iteration already runs the choice, and so does every later one
    assert clock.reads == 12                                      # two per block in the first AUTO_ITERS iterations, none afterwards


def test_the_executor_module_needs_no_device():
    import subprocess
    import sys
    import os
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(X.__file__)))
    code = ("import sys; sys.path.insert(0, %r); import tg.executor, torch; assert not torch.cuda.is_initialized(); "
            "assert 'tg.runtime' not in sys.modules" % pkg)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES=''))
    assert r.returncode == 0, r.stderr[-2000:]
