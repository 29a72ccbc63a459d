"""The planner's parameter tables do not depend on the path switches: names, shapes, trainable flags and offsets of the three models
(checkpoints and the data-parallel bucket offsets hang on them) are the same list under the default switches and under every switch
set tests/test_gpu_paths.py and tests/test_gpu_bf16_storage.py run.  The switches are read once per process, hence one subprocess per
setting.  No GPU."""
import functools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ('CDRL_FUSED_DW', 'CDRL_FUSED_PW', 'CDRL_FUSED_STEM', 'CDRL_FUSED_PASS', 'CDRL_FUSED_BB', 'CDRL_FUSED_BWD', 'CDRL_FIN_ON_LOAD',
            'CDRL_PW_X3', 'CDRL_SIDE_STREAM')
ALL_OFF = dict(CDRL_FUSED_DW=0, CDRL_FUSED_PW=0, CDRL_FUSED_STEM=0, CDRL_FUSED_PASS=0, CDRL_FUSED_BB=0, CDRL_SIDE_STREAM=0, CDRL_PW_X3=0)
SETTINGS = {
    'all_off': ALL_OFF,
    'fused_bwd_0': dict(CDRL_FUSED_BWD=0),
    'fin_on_load_0': dict(CDRL_FIN_ON_LOAD=0),
    'pw_x3_0': dict(CDRL_PW_X3=0),
    'pw_x3_0_fused_bwd_0': dict(CDRL_PW_X3=0, CDRL_FUSED_BWD=0),
    'fin_on_load_0_fused_bwd_1': dict(CDRL_FIN_ON_LOAD=0, CDRL_FUSED_BWD=1),
}
# bf16 storage has no unfused depthwise / stem / identity-half kernels: with everything off the learner does not build (checked below)
NO_BF16S = {'all_off'}

DUMP = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
from carla_driving_rl_agent_amd import _lib
from carla_driving_rl_agent_amd.engine import LearnerEngine
out = {}
for compute in ('f32', 'bf16s'):
    try:
        e = LearnerEngine(4, device=None, H=48, W=64, compute=compute)
    except _lib.CdrlError as ex:
        out[compute] = None
        continue
    out[compute] = dict(tables={m: [[x['name'], list(x['shape']), x['trainable'], x['offset']] for x in t.entries] for m, t in e.tables.items()},
                        tail=e.tail_offset(), params=e.params_total, grads=e.grads_total)
print(json.dumps(out))
'''


@functools.lru_cache(maxsize=None)
def _tables(setting):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update({k: str(v) for k, v in SETTINGS.get(setting, {}).items()})
    r = subprocess.run([sys.executable, '-c', DUMP, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


@pytest.mark.parametrize('setting', sorted(SETTINGS))
def test_parameter_tables_do_not_depend_on_the_path_switches(setting):
    ref, got = _tables('default'), _tables(setting)
    assert ref['f32'] is not None and ref['bf16s'] is not None
    assert set(ref['f32']['tables']) == {'trunk', 'policy', 'value'} and len(ref['f32']['tables']['trunk']) > 300
    computes = ['f32'] if setting in NO_BF16S else ['f32', 'bf16s']
    if setting in NO_BF16S:
        assert got['bf16s'] is None, 'bf16 storage builds under this setting now: compare its tables too'
    for compute in computes:
        assert got[compute] is not None, (setting, compute)
        for m in ('trunk', 'policy', 'value'):
            assert got[compute]['tables'][m] == ref[compute]['tables'][m], (setting, compute, m)
        for k in ('tail', 'params', 'grads'):
            assert got[compute][k] == ref[compute][k], (setting, compute, k)
