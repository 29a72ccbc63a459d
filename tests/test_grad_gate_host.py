"""Gradient gate (cdrl_config.clip_mode / skip_nonfinite, PPOAgent(clip_mode=..., skip_nonfinite=...)) on the host: the options reach
the planner and are validated, the C ABI declares and exports the statistics calls, shared engines and agents carry the options,
CARLAgent hands the trunk's threshold on, and the numpy restatement (tests/grad_gate_ref.py, which the GPU tests compare the
kernels against) has the properties the header states.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.grad_gate_ref import F, clip_by_global_norm, global_scale, list_sqnorm, should_skip  # noqa: E402
from tests.test_optimizers_host import _engine, _host_agent  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- engine / C ABI
def test_host_engine_builds_with_both_options():
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    e = LearnerEngine(2, device=None, clip_mode='global', skip_nonfinite=True)
    assert e.clip_mode == 'global' and e.skip_nonfinite and e.gated
    assert (e.cfg.clip_mode, e.cfg.skip_nonfinite) == (1, 1)
    d = LearnerEngine(2, device=None)
    assert d.clip_mode == 'tensor' and not d.skip_nonfinite and not d.gated
    assert d.hp['clip_norm_dynamics'] == 0.0
    # the parameter tables and arenas do not depend on the options
    for m in ('trunk', 'policy', 'value'):
        assert e.tables[m].entries == d.tables[m].entries
    assert (e.params_total, e.grads_total) == (d.params_total, d.grads_total)
    assert LearnerEngine(2, device=None, clip_mode='GLOBAL').clip_mode == 'global'
    assert LearnerEngine(2, device=None, skip_nonfinite=True).gated


def test_unknown_mode_raises():
    from carla_driving_rl_agent_amd import _lib
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    with pytest.raises(ValueError, match='clip_mode'):
        LearnerEngine(2, device=None, clip_mode='norm')
    for kw, match in ((dict(clip_mode=2), 'clip_mode'), (dict(clip_mode=-1), 'clip_mode'), (dict(skip_nonfinite=2), 'skip_nonfinite')):
        with pytest.raises(_lib.CdrlError, match=match):
            _engine(**kw)


def test_config_defaults_are_off():
    from carla_driving_rl_agent_amd import _lib
    cfg = _lib.Config()
    cfg.clip_mode, cfg.skip_nonfinite = 1, 1
    _lib.load().cdrl_config_default(C.byref(cfg))
    assert (cfg.clip_mode, cfg.skip_nonfinite) == (_lib.CLIP_TENSOR, 0)
    assert _lib.CLIP_MODES == ('tensor', 'global') and _lib.CLIP_GLOBAL == 1


def test_header_declares_and_library_exports_the_gate_calls():
    from carla_driving_rl_agent_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cdrl.h')).read()
    lib = _lib.load()
    for name in ('cdrl_learner_gate_stats', 'cdrl_learner_gate_reset'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in _lib.PROTOTYPES and getattr(lib.raw, name) is not None
    for word in ('CDRL_CLIP_TENSOR = 0', 'CDRL_CLIP_GLOBAL = 1', 'int32_t clip_mode', 'int32_t skip_nonfinite', 'float clip_norm_dynamics',
                 'cdrl_gate_stats'):
        assert word in header, word
    assert C.sizeof(_lib.GateStats) == 4 * 12 and C.sizeof(_lib.HParams) == 4 * 11


def test_gate_calls_refuse_a_host_only_engine():
    from carla_driving_rl_agent_amd import _lib
    e = _engine(clip_mode='global')
    with pytest.raises(_lib.CdrlError, match='device=None'):
        e.gate_stats()
    with pytest.raises(_lib.CdrlError, match='device=None'):
        e.gate_reset()


def test_shared_engines_inherit_the_options():
    owner = _engine(32, clip_mode='global', skip_nonfinite=True)
    shared = _engine(8, share_with=owner)
    assert shared.clip_mode == 'global' and shared.skip_nonfinite
    plain = _engine(8, share_with=_engine(32))
    assert plain.clip_mode == 'tensor' and not plain.skip_nonfinite


# ---------------------------------------------------------------------------------------------------------------- agents
@pytest.mark.parametrize('clip_norm,expected', [((1.0, 2.0, 0.5), 0.5), (0.25, 0.25), (None, 0.0), ((1.0, 1.0), 0.0),
                                                ((1.0, 1.0, None), 0.0)])
def test_agent_hands_on_the_dynamics_threshold(monkeypatch, clip_norm, expected):
    agent, _ = _host_agent(monkeypatch, clip_norm=clip_norm)
    hp = agent.hyper_parameters()
    assert hp['clip_norm_dynamics'] == expected
    heads = (0.0, 0.0) if clip_norm is None else ((clip_norm, clip_norm) if isinstance(clip_norm, float) else clip_norm[:2])
    assert (hp['clip_norm_policy'], hp['clip_norm_value']) == heads


@pytest.mark.parametrize('cls', ['CARLAgent', 'PPOAgent'])
def test_agents_carry_the_options_to_every_engine(monkeypatch, cls):
    agent, made = _host_agent(monkeypatch, cls, clip_mode='Global', skip_nonfinite=True)
    assert agent.clip_mode == 'global' and agent.skip_nonfinite
    assert made and all(e.clip_mode == 'global' and e.skip_nonfinite for e in made)
    ragged = agent.network.engine_for(5)
    assert ragged.clip_mode == 'global' and ragged.skip_nonfinite
    agent, made = _host_agent(monkeypatch, cls)
    assert agent.clip_mode == 'tensor' and not agent.skip_nonfinite and all(not e.gated for e in made)
    with pytest.raises(ValueError, match='clip_mode'):
        _host_agent(monkeypatch, cls, clip_mode='value')


# ---------------------------------------------------------------------------------------------------------------- restatement
def _list(seed, n=5000, scale=1e-3):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(n) * scale).astype(F)
    return g, [(0, 1500), (1504, 1023), (2528, n - 2528)]          # three tensors with padding between them


def test_scale_is_one_at_or_below_the_threshold():
    g, segs = _list(1)
    S = list_sqnorm(g, segs)
    norm32 = float(F(np.sqrt(S)))
    for c in (norm32 * 4.0, 1e30, float(np.nextafter(F(np.sqrt(S)), F(np.inf)))):
        assert float(F(c)) >= np.sqrt(S)
        s = global_scale(S, c)
        assert s.dtype == np.float32 and s == F(1.0)
        out, norm, s2 = clip_by_global_norm(g, segs, c, dt=np.float32)
        assert s2 == F(1.0) and np.array_equal(out, g) and norm == np.sqrt(S)
    for c in (0.0, -1.0, None):                                       # off: not scaled
        assert global_scale(S, c) == F(1.0)
    assert global_scale(0.0, 1.0) == F(1.0)                           # an all-zero list


@pytest.mark.parametrize('scale', [1e-3, 1.0, 1e15])
def test_scaled_list_has_at_most_the_threshold_norm(scale):
    g, segs = _list(2, scale=scale)
    S = list_sqnorm(g, segs)
    for frac in (0.5, 0.01):
        c = float(F(np.sqrt(S) * frac))
        for dt in (np.float32, np.float64):
            out, norm, s = clip_by_global_norm(g, segs, c, dt=dt)
            assert 0.0 < s < 1.0 and norm == np.sqrt(S)
            scaled = np.sqrt(list_sqnorm(out.astype(F), segs))
            assert scaled <= c * (1.0 + 1e-6), (scale, frac, scaled / c)
            assert scaled >= c * (1.0 - 1e-6)
            assert np.array_equal(out[:10], g[:10].astype(dt) * dt(s))      # one multiply per element; the direction is kept


def test_padding_is_not_part_of_the_list():
    g, segs = _list(3)
    S = list_sqnorm(g, segs)
    g[1500:1504] = np.nan
    g[2527] = np.inf
    assert list_sqnorm(g, segs) == S and not should_skip([S])


def test_skip_decision():
    g, segs = _list(4)
    S = list_sqnorm(g, segs)
    assert not should_skip([S, 0.0])
    for bad in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[2526] = bad                                                # last element of the second tensor
        assert should_skip([list_sqnorm(h, segs)]) and should_skip([S, list_sqnorm(h, segs)])
    h = g.copy()
    h[:3] = 1e30                                                     # float32 squares overflow, the double sum does not
    Sh = list_sqnorm(h, segs)
    assert np.isfinite(Sh) and not should_skip([Sh])
    s = global_scale(Sh, 1.0)
    assert 0.0 < s < 1e-29 and np.isfinite(h * s).all()
