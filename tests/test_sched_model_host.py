"""The stream scheduler's ordering contract on the CPU: tests/host/sched_model.cpp drives csrc/sched.h against a model
of the runtime's record / wait semantics.  Plain host C++, not linked against the HIP runtime; no GPU, no Python in the program."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'sched_model.cpp')
# --break=N: the edge it disables, and the point of the contract that has to notice
BREAKS = {1: ('the wait of a claim', 'FAIL 1 claim'), 2: ('the record of done_side', 'FAIL 1 claim'), 3: ('the flush of fork_side', 'FAIL 2 fork')}


def _hipcc():
    spec = importlib.util.spec_from_file_location('cdrl_build', os.path.join(ROOT, 'carla-driving-rl-agent_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._hipcc()


def _compile(out, *extra):
    hipcc = _hipcc()
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc))) if os.path.isabs(hipcc) else '/opt/rocm'
    cmd = [hipcc, '-no-hip-rt', '-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-D__HIP_PLATFORM_AMD__',
           '-I' + os.path.join(rocm, 'include'), *extra, SRC, '-o', out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f'{" ".join(cmd)}\n{r.stdout}\n{r.stderr}'
    return out


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp('sched_model') / 'sched_model'))


def test_contract_holds(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('OK'), r.stdout + r.stderr


@pytest.mark.parametrize('n', sorted(BREAKS))
def test_a_missing_edge_is_noticed(program, n):
    edge, point = BREAKS[n]
    r = subprocess.run([program, f'--break={n}'], capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout.startswith(point), f'without {edge}: {r.stdout}{r.stderr}'


def test_contract_holds_under_sanitizers(tmp_path):
    exe = _compile(str(tmp_path / 'sched_model_san'), '-fsanitize=address,undefined', '-fno-sanitize-recover=all')
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('OK'), r.stdout + r.stderr
