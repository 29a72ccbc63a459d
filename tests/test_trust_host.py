"""Trust-region guard of the policy steps (cdrl_config.trust, PPOAgent(target_kl=..., kl_penalty=...)) on the host: the
float64 restatement of the Beta KL (tests/trust_ref.py, which the GPU tests compare the kernel against) against numerical
integration and its own properties, the closed-form gradient against autograd, the constructors' validation, and the layout of the
C ABI structs -- in ctypes, and in a stand-alone host program (tests/host/trust_layout.cpp) that also runs under sanitizers.  No GPU."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import integrate
from scipy.special import betaln

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import trust_ref  # noqa: E402
from tests.test_optimizers_host import _engine, _host_agent  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'trust_layout.cpp')


# ---------------------------------------------------------------------------------------------------------------- restatement
def _kl_by_integration(a0, b0, a, b):
    """integral of p0 log(p0 / p) over the unit interval, p0 and p through their log-densities (no overflow at large parameters);
    the break points put the quadrature's intervals where p0 has its mass."""
    def f(x):
        l0 = (a0 - 1.0) * np.log(x) + (b0 - 1.0) * np.log1p(-x) - betaln(a0, b0)
        l1 = (a - 1.0) * np.log(x) + (b - 1.0) * np.log1p(-x) - betaln(a, b)
        return np.exp(l0) * (l0 - l1)
    mean, std = a0 / (a0 + b0), np.sqrt(a0 * b0 / ((a0 + b0) ** 2 * (a0 + b0 + 1.0)))
    pts = sorted({min(max(mean + k * std, 1e-12), 1.0 - 1e-12) for k in (-8, -4, -2, -1, 0, 1, 2, 4, 8)})
    value, err = integrate.quad(f, 0.0, 1.0, points=pts, limit=400, epsabs=1e-13, epsrel=1e-11)
    return value, err


@pytest.mark.parametrize('a0,b0,a,b', [(1.01, 1.01, 1.5, 2.5), (1.01, 3.0, 1.011, 2.9), (2.0, 5.0, 5.0, 2.0), (1.3, 1.01, 40.0, 7.0),
                                       (50.0, 50.0, 1.01, 1.01), (1e3, 1e3, 990.0, 1010.0), (1e3, 3.0, 900.0, 3.5),
                                       (7.5, 1e3, 8.0, 1100.0)])
def test_restatement_matches_numerical_integration(a0, b0, a, b):
    ref, err = _kl_by_integration(a0, b0, a, b)
    got = float(trust_ref.kl_beta(a0, b0, a, b))
    assert ref > 0.0
    assert abs(got - ref) <= 1e-8 * max(1.0, abs(ref)) + 10.0 * err, (got, ref, err)


def test_kl_is_zero_at_equal_parameters():
    rng = np.random.default_rng(0)
    a = np.concatenate([[1.01, 1.01, 1e3, 1e3], rng.uniform(1.01, 60.0, 200)])
    b = np.concatenate([[1.01, 1e3, 1.01, 1e3], rng.uniform(1.01, 60.0, 200)])
    assert np.array_equal(trust_ref.kl_beta(a, b, a, b), np.zeros_like(a))


def test_kl_is_not_negative_on_random_draws():
    rng = np.random.default_rng(1)
    draw = lambda: np.exp(rng.uniform(np.log(1.01), np.log(1e3), 20000))
    a0, b0, a, b = draw(), draw(), draw(), draw()
    kl = trust_ref.kl_beta(a0, b0, a, b)
    assert np.isfinite(kl).all() and kl.min() > 0.0
    near = trust_ref.kl_beta(a0, b0, a0 * (1.0 + 1e-6), b0 * (1.0 - 1e-6))      # quadratic in the distance: tiny, and rounding may
    assert near.min() > -1e-9 and near.max() < 1e-6                             # put it slightly below zero (the kernel clamps)


@pytest.mark.parametrize('B,A', [(1, 1), (5, 2), (9, 8)])
def test_closed_form_gradient_matches_autograd(B, A):
    rng = np.random.default_rng(10 * B + A)
    lin = rng.standard_normal((B, 2 * A + 2)) * 2.0
    anchor = np.exp(rng.uniform(np.log(1.01), np.log(80.0), (B, 2, A)))
    out = trust_ref.kl_from_lin(lin, anchor)
    lt = torch.tensor(lin, dtype=torch.float64, requires_grad=True)
    kl = trust_ref.kl_torch(lt, torch.tensor(anchor, dtype=torch.float64))
    kl.backward()
    assert abs(float(kl.detach()) - out["kl"]) <= 1e-12 * max(1.0, abs(out['kl']))
    g = lt.grad.numpy()
    assert np.abs(g - out['dlin']).max() <= 1e-12 * max(1.0, np.abs(g).max())
    assert not out['dlin'][:, 2 * A:].any() and not g[:, 2 * A:].any()          # the auxiliary columns carry no KL
    assert out['rows'].shape == (B,) and abs(out['rows'].mean() - out['kl']) < 1e-15 * max(1.0, out['kl'])
    assert out['metrics'][0] == out['kl'] and out['metrics'][1] == out['rows'].max() and out['metrics'][2] == out['kl'] / A


def test_restatement_reports_nan_for_a_broken_anchor():
    lin = np.zeros((3, 6))
    anchor = np.full((3, 2, 2), 2.0)
    anchor[1, 0, 1] = np.nan
    m = trust_ref.kl_from_lin(lin, anchor)['metrics']
    assert np.isnan(m).all()


# ---------------------------------------------------------------------------------------------------------------- engine / C ABI
def test_struct_layouts_keep_the_old_fields():
    from carla_driving_rl_agent_amd import _lib
    off = lambda s, n: getattr(s, n).offset
    assert off(_lib.Config, 'skip_nonfinite') == 112 and off(_lib.Config, 'clip_mode') == 108 and off(_lib.Config, 'polyak') == 100
    assert off(_lib.Config, 'trust') == 116 and C.sizeof(_lib.Config) == 120
    assert C.sizeof(_lib.HParams) == 44 and off(_lib.HParams, 'clip_norm_dynamics') == 40        # the guard's values: TrustParams
    assert off(_lib.PolicyBatch, 'du_dbeta') == 80 and off(_lib.PolicyBatch, 'anchor') == 88 and C.sizeof(_lib.PolicyBatch) == 96
    assert C.sizeof(_lib.TrustParams) == 12 and C.sizeof(_lib.TrustStats) == 48 and off(_lib.TrustStats, 'kl_sum') == 40
    assert [n for n, _ in _lib.TrustStats._fields_][:3] == [n for n, _ in _lib.TrustParams._fields_]


def test_header_declares_and_library_exports_the_trust_calls():
    from carla_driving_rl_agent_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cdrl.h')).read()
    lib = _lib.load()
    for name in ('cdrl_learner_set_trust_params', 'cdrl_learner_trust_stats', 'cdrl_learner_trust_reset', 'cdrl_beta_kl'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in _lib.PROTOTYPES and getattr(lib.raw, name) is not None
    for word in ('int32_t trust;', 'const float *anchor;', 'cdrl_trust_params', 'cdrl_trust_stats'):
        assert word in header, word
    cfg = _lib.Config()
    cfg.trust = 1
    lib.cdrl_config_default(C.byref(cfg))
    assert cfg.trust == 0


def test_host_engine_builds_with_trust():
    from carla_driving_rl_agent_amd import _lib
    d, e = _engine(), _engine(trust=True)
    assert e.trust and e.cfg.trust == 1 and not d.trust and not e.gated
    assert e.hp['target_kl'] == 0.0 and e.hp['kl_stop_factor'] == 1.5 and e.hp['kl_coef'] == 0.0 and 'target_kl' not in d.hp
    for m in ('trunk', 'policy', 'value'):          # the parameter tables and arenas do not depend on the option
        assert e.tables[m].entries == d.tables[m].entries
    assert (e.params_total, e.grads_total) == (d.params_total, d.grads_total)
    assert e.workspace_bytes > d.workspace_bytes            # the gate block and the trust block
    assert _engine(4, share_with=e).trust and not _engine(4, share_with=d).trust
    with pytest.raises(_lib.CdrlError, match='trust must be 0 or 1'):
        _engine(trust=2)
    with pytest.raises(_lib.CdrlError, match='device=None'):
        e.trust_stats()
    with pytest.raises(_lib.CdrlError, match='device=None'):
        e.trust_reset()


# ---------------------------------------------------------------------------------------------------------------- agents
@pytest.mark.parametrize('cls', ['CARLAgent', 'PPOAgent'])
def test_agents_validate_and_carry_the_options(monkeypatch, cls):
    agent, made = _host_agent(monkeypatch, cls)
    assert not agent.trust and agent.target_kl is None and made and all(not e.trust for e in made)
    assert 'target_kl' not in agent.hyper_parameters()
    agent, made = _host_agent(monkeypatch, cls, target_kl=0.02)
    assert agent.trust and made and all(e.trust for e in made) and agent.network.engine_for(5).trust
    hp = agent.hyper_parameters()
    assert (hp['target_kl'], hp['kl_stop_factor'], hp['kl_coef']) == (0.02, 1.5, 0.0)
    agent, made = _host_agent(monkeypatch, cls, kl_penalty=0.5, kl_stop_factor=2.0)
    assert agent.trust and agent.target_kl is None and all(e.trust for e in made)
    hp = agent.hyper_parameters()
    assert (hp['target_kl'], hp['kl_stop_factor'], hp['kl_coef']) == (0.0, 2.0, 0.5)
    assert not _host_agent(monkeypatch, cls, kl_penalty=0.0)[0].trust
    for kw in (dict(target_kl=-1e-3), dict(kl_penalty=-0.1), dict(target_kl=0.01, kl_stop_factor=0.0),
               dict(target_kl=float('nan')), dict(kl_penalty=float('nan'))):
        with pytest.raises(ValueError, match='target_kl'):
            _host_agent(monkeypatch, cls, **kw)
    with pytest.raises(ValueError, match='joint_update'):
        _host_agent(monkeypatch, cls, target_kl=0.01, joint_update=True)
    with pytest.raises(ValueError, match='joint_update'):
        _host_agent(monkeypatch, cls, kl_penalty=0.1, joint_update=True)


def test_options_are_not_written_to_the_config(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    agent, _ = _host_agent(monkeypatch, 'CARLAgent', target_kl=0.02, kl_penalty=0.1, weights_dir=str(tmp_path), name='t')
    agent.save_config()
    text = ' '.join(open(os.path.join(r, f)).read() for r, _, fs in os.walk(tmp_path) for f in fs if f.endswith('.json'))
    assert text and 'target_kl' not in text and 'kl_penalty' not in text and 'kl_stop_factor' not in text


def test_an_initialised_process_group_is_refused(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a: 1)
    monkeypatch.setattr(dist, 'get_rank', lambda *a: 0)
    with pytest.raises(ValueError, match='one process'):
        _host_agent(monkeypatch, 'CARLAgent', target_kl=0.01)


# ---------------------------------------------------------------------------------------------------------------- host program
def _hipcc():
    spec = importlib.util.spec_from_file_location('cdrl_build', os.path.join(ROOT, 'carla-driving-rl-agent_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._hipcc()


def _compile(out, *extra):
    cmd = [_hipcc(), '-no-hip-rt', '-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', *extra, SRC, '-o', out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f'{" ".join(cmd)}\n{r.stdout}\n{r.stderr}'
    return out


@pytest.mark.parametrize('flags', [(), ('-fsanitize=address,undefined', '-fno-sanitize-recover=all')], ids=['plain', 'sanitizers'])
def test_layout_program(tmp_path, flags):
    exe = _compile(str(tmp_path / 'trust_layout'), *flags)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('OK'), r.stdout + r.stderr
