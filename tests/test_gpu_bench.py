"""bench.py on one GPU without a launcher: a plain run prints its line from setup, warm-up and the timed steps alone; --full
adds the CPU-oracle baseline, the parity leg and the roofline leg to the same line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
           '--positives', '2000'] + list(extra)
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2500:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines          # stdout carries the one JSON line and nothing else
    return json.loads(lines[0])


def test_plain_run_leaves_the_side_legs_to_full():
    plain = run_bench()
    assert plain['cpu_baseline'] is None and plain['parity_check'] is None
    assert plain['roofline'] is None and plain['roofline_detail'] == {} and plain['roofline_k4'] is None
    assert plain['ms_per_step'] > 0 and plain['loss_is_finite'] is True

    full = run_bench('--full', '--cpu-seconds', '5', '--profile-steps', '1')
    assert full['cpu_baseline']['value'] > 0 and full['cpu_baseline']['steps'] >= 2
    assert full['parity_check']['passed'] is True
    assert full['roofline'] is not None and full['roofline_detail']
    for key in ('metric', 'unit', 'higher_is_better', 'dtype', 'steps', 'warmup'):
        assert plain[key] == full[key], key
    assert plain['config'] == full['config']
    # the legs of --full run outside the timed regions, which start from the same weights and random state either way
    assert abs(plain['final_loss'] - full['final_loss']) <= 1e-5 * abs(full['final_loss'])
