"""bench.py plain vs --full on the GPU: a plain run prints the headline figure alone; --full adds the host issue time, the roofline, the optimiser leg
and the CPU baseline + loss parity, on the same JSON contract."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'n_gpus')
FULL_ONLY = ('roofline', 'model_flops_frac', 'with_optimizer', 'cpu_baseline', 'parity')


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'ALM_BENCH_LAUNCH_CHECK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--config', 'coarse1024', '--steps', '2', '--warmup', '1', *args],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_has_the_headline_alone_and_full_adds_the_other_legs():
    plain = _bench()
    assert all(k in plain for k in HEADLINE), sorted(plain)
    assert not any(k in plain for k in FULL_ONLY), sorted(plain)
    assert 'eager_issue_ms' not in plain['host'] and plain['steps'] == 2 and plain['value'] > 0
    full = _bench('--full')
    assert all(k in full for k in HEADLINE + FULL_ONLY), sorted(full)
    assert 'eager_issue_ms' in full['host'] and full['parity']['ok']
    assert full['roofline']['launches_per_step'] > 0 and full['with_optimizer']['ms_per_step'] > 0 and full['cpu_baseline']['value'] > 0
    assert plain['metric'] == full['metric'] and plain['config']['seq_len'] == full['config']['seq_len']
