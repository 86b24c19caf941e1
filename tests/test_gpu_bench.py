"""bench.py on one GPU, each run a fresh process: a plain run prints the headline line and nothing that needs work of its own beyond the
timed steps; --full adds those measurements and checks (bench.FULL_ONLY) after the timed steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1'] + list(extra),
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_leaves_out_the_full_fields():
    import bench
    out = _bench()
    assert out['unit'] == 'images/sec' and out['higher_is_better'] is True and out['dtype'] == 'f32' and out['steps'] == 3
    assert out['metric'].startswith('Triple-GAN train images/sec') and out['ms_per_step'] > 0
    assert abs(out['value'] * out['ms_per_step'] - 100 * 1e3) <= 1e-3 * 100 * 1e3       # images/s = 100 images / step time
    assert not set(bench.FULL_ONLY) & set(out), sorted(set(bench.FULL_ONLY) & set(out))


def test_full_run_adds_the_issue_time_and_the_roofline():
    import bench
    out = _bench('--full', '--no-cpu-baseline', '--soak-seconds', '0', '--prof-iters', '1')
    assert set(bench.FULL_ONLY) - {'cpu_baseline'} <= set(out) and 'cpu_baseline' not in out
    assert out['replicas_identical'] is None and out['exchange_exposed_ms'] is None          # N = 1: nothing to compare or expose
    assert out['host_issue_ms_per_step'] > 0
    roof = out['roofline']
    assert 0 < roof['frac'] < 1 and roof['class_ms_per_step']['igemm_f32'] > 0 and roof['launches_per_step'] > 0
