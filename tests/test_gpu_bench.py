"""bench.py's two modes on one GPU: a plain run prints the headline line of the timed update-steps and nothing it does not need;
--full adds the isolated-kernel rooflines, the CPU-oracle baseline and the figures of the committed profiles after them."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--steps', '2', '--warmup', '1', '--batch', '32', '--height', '48', '--width', '64']


def _bench(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + SMALL + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.rstrip().splitlines()[-1]
    assert last.startswith('{"metric"'), r.stdout[-2000:]
    return json.loads(last)


@pytest.mark.gpu
def test_bench_plain_and_full():
    plain = _bench([])
    assert plain['steps'] == 2 and plain['warmup'] == 1 and plain['n_gpus'] == 1 and plain['unit'] == 'update-steps/s'
    assert plain['higher_is_better'] and plain['value'] > 0 and abs(plain['value'] - 1e3 / plain['ms_per_step']) < 1e-2 * plain['value']
    assert plain['kernel_rooflines'] is None and plain['mfma'] is None and plain['dominant_kernel'] is None
    assert 'cpu_baseline' not in plain and 'secondary' not in plain

    full = _bench(['--full', '--cpu-sample-batch', '8', '--cpu-threads', '8'])
    assert set(plain) <= set(full) and full['metric'] == plain['metric'] and full['dtype'] == plain['dtype']
    assert full['kernel_rooflines'] and all(k['us'] > 0 for k in full['kernel_rooflines'])
    assert full['mfma'] is not None                          # the committed PMC run (profiles/rNN_pmc_mfma.json)
    assert full['cpu_baseline']['value'] and full['cpu_baseline']['timed_steps'] >= 1
    assert 'secondary' not in full                           # configs[2] is measured next to the default shape only
