"""Host side of scoring on held-out traces (engine.read_score_block, CARLAgent.score_traces / imitate(validation_dir=...);
DESIGN.md 6.17): the restatement's PIT against a quadrature of the Beta density, the histogram and coverage rules on hand-made
values, the derived figures of a hand-made block, the declarations, and every refusal decided before anything touches a device."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
from scipy import integrate, special

from carla_driving_rl_agent_amd import _lib
from carla_driving_rl_agent_amd.core import CARLAgent
from carla_driving_rl_agent_amd.engine import SCORE_BINS, SCORE_LAYOUT, read_score_block, score_block, score_block_size
from carla_driving_rl_agent_amd.rl.agents.ppo import PPOAgent
from tests import score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD, ACTION = SCORE_LAYOUT['head'], SCORE_LAYOUT['action']


@pytest.mark.parametrize('a,b,x', [(1.01, 1.01, 0.5), (2.0, 5.0, 0.1), (5.0, 2.0, 0.9), (30.0, 40.0, 0.45), (1.5, 300.0, 0.004),
                                   (120.0, 3.0, 0.99)])
def test_pit_is_the_integral_of_the_density(a, b, x):
    got = float(score_ref.pit(np.float32(a), np.float32(b), np.float32(x)))
    # the float32 roundings of a, b and x move F by up to ~1e-5 relative at these parameters: integrate at the rounded arguments
    a32, b32, x32 = float(np.float32(a)), float(np.float32(b)), float(np.float32(x))
    density = lambda t: np.exp((a32 - 1.0) * np.log(t) + (b32 - 1.0) * np.log1p(-t) - special.betaln(a32, b32))
    want, _ = integrate.quad(density, 0.0, x32, epsabs=1e-13, epsrel=1e-13, limit=200)
    assert abs(got - want) < 1e-10, (got, want)


def test_pit_at_the_clip_edges():
    assert score_ref.clip(np.float32(0.0)) == float(score_ref.EPS) and score_ref.clip(np.float32(1.0)) == 1.0 - float(score_ref.EPS)
    F = score_ref.pit(np.float32([2.0, 2.0]), np.float32([3.0, 3.0]), np.float32([0.0, 1.0]))
    assert 0.0 < F[0] < 1e-12 and 1.0 - 1e-12 < F[1] <= 1.0


def test_histogram_and_coverage_rules():
    F = [0.0, 0.05, 0.0999, 0.1, 0.25, 0.5, 0.75, 0.95, 0.9999, 1.0]
    hist, c50, c90 = score_ref.pit_counts(F)
    assert hist.tolist() == [3, 1, 1, 0, 0, 1, 0, 1, 0, 3]          # 1.0 falls in the last bin, 0.1 opens the second
    assert hist.sum() == len(F) and len(hist) == SCORE_BINS
    assert c50 == 3 and c90 == 7                                    # both bounds belong to the interval
    assert score_ref.pit_counts([0.2499999, 0.7500001])[1] == 0 and score_ref.pit_counts([0.0499999, 0.9500001])[2] == 0
    d = score_ref.edge_distance(np.array([0.1, 0.25, 0.3000005, 0.62, 1.0, 0.0]))
    assert np.allclose(d, [0.0, 0.0, 5e-7, 0.02, 0.05, 0.05], atol=1e-12)


def test_read_score_block_derives_the_figures():
    rng = np.random.default_rng(3)
    n, A = 6, 2
    alpha, beta = rng.uniform(1.5, 9.0, (n, A)).astype(np.float32), rng.uniform(1.5, 9.0, (n, A)).astype(np.float32)
    u = rng.uniform(0.05, 0.95, (n, A)).astype(np.float32)
    returns = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 2, n)], axis=1).astype(np.float32)
    speed = (rng.integers(0, 128, n) / 64.0).astype(np.float32)                         # multiples of 1 / 64: the offsets are exact
    similarity = (rng.integers(-64, 64, n) / 64.0).astype(np.float32)
    value =np.concatenate([returns, (speed + np.float32(0.5))[:, None], (similarity - np.float32(0.25))[:, None]], axis=1)     # V = R
    block = score_ref.block(alpha, beta, value, u, returns, speed, similarity)
    assert block.shape == (score_block_size(A),) == (16 + 19 * A,)
    out = read_score_block(torch.as_tensor(block), A)
    al, be, x = alpha.astype(np.float64), beta.astype(np.float64), u.astype(np.float64)
    logp = (al - 1) * np.log(x) + (be - 1) * np.log1p(-x) - special.betaln(al, be)
    mean, mode = al / (al + be), (al - 1) / (al + be - 2)
    var = al * be / ((al + be) ** 2 * (al + be + 1))
    close = lambda got, want: np.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert out['rows'] == n and out['nonfinite'] == 0 and out['pit_unconverged'] == 0
    assert close(out['log_prob'], logp.mean()) and close(out['log_prob_per_action'], logp.mean(axis=0))
    assert close(out['mode_error'], np.abs(mode - x).mean()) and close(out['mode_error_per_action'], np.abs(mode - x).mean(axis=0))
    assert close(out['bias'], (mean - x).mean()) and close(out['bias_per_action'], (mean - x).mean(axis=0))
    assert close(out['rmse'], np.sqrt(((mean - x) ** 2).mean())) and close(out['rmse_per_action'], np.sqrt(((mean - x) ** 2).mean(axis=0)))
    assert close(out['predicted_std'], np.sqrt(var.mean())) and close(out['predicted_std_per_action'], np.sqrt(var.mean(axis=0)))
    ent = special.betaln(al, be) - (al - 1) * special.digamma(al) - (be - 1) * special.digamma(be) + (al + be - 2) * special.digamma(al + be)
    assert close(out['entropy'], ent.mean()) and close(out['entropy_per_action'], ent.mean(axis=0))
    F = special.betainc(al, be, x)
    assert out['pit_histogram'].shape == (A, SCORE_BINS) and out['pit_histogram'].dtype.kind == 'i'
    for a in range(A):
        hist, c50, c90 = score_ref.pit_counts(F[:, a])
        assert out['pit_histogram'][a].tolist() == hist.tolist()
        assert out['coverage_50'][a] == c50 / n and out['coverage_90'][a] == c90 / n
    assert out['value_bias'] == 0.0 and out['value_rmse'] == 0.0 and out['explained_variance'] == 1.0           # V = R
    assert close(out['speed_rmse'], 0.5) and close(out['similarity_rmse'], 0.25)
    assert np.array_equal(out['block'], block)
    # a value head that predicts the mean return explains nothing; without returns / aux targets the figures are None
    R = score_ref.decode(returns)
    flat = value.copy()
    flat[:, 0], flat[:, 1] = np.float32(R.mean()), 0.0
    ev = read_score_block(torch.as_tensor(score_ref.block(alpha, beta, flat, u, returns)), A)
    assert abs(ev['explained_variance']) < 1e-6 and ev['speed_rmse'] is None and ev['similarity_rmse'] is None
    bare = read_score_block(torch.as_tensor(score_ref.block(alpha, beta, value, u)), A)
    assert all(bare[k] is None for k in ('value_bias', 'value_rmse', 'explained_variance', 'speed_rmse', 'similarity_rmse'))
    # a stack of blocks -> a list; the empty block has no mean
    two = read_score_block(torch.as_tensor(np.stack([block, np.zeros_like(block)])), A)
    assert two[0]['log_prob'] == out['log_prob'] and two[1]['rows'] == 0 and np.isnan(two[1]['log_prob'])
    assert bool((score_block(A, 'cpu') == 0).all()) and score_block(A, 'cpu').dtype == torch.float64
    for bad in (torch.zeros(5, dtype=torch.float64), torch.zeros(score_block_size(A))):
        with pytest.raises(ValueError, match='read_score_block'):
            read_score_block(bad, A)
    with pytest.raises(ValueError, match='score_block'):
        score_block(9, 'cpu')


def _macro(text, name):
    m = re.search(r'^#define %s(?:\(A\))? (.+)$' % name, text, re.M)
    assert m, name
    return m.group(1)


def test_header_binding_and_layout_agree():
    with open(os.path.join(ROOT, 'include', 'cdrl.h')) as f:
        header = f.read()
    assert re.search(r'^int cdrl_beta_score\(', header, re.M)
    assert 'cdrl_beta_score' in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES['cdrl_beta_score']
    assert len(args) == 12                                          # six inputs, three ints, block, pit, stream
    names = {n: _macro(header, n) for n in ('CDRL_SCORE_BINS', 'CDRL_SCORE_HEAD', 'CDRL_SCORE_PER_ACTION', 'CDRL_SCORE_BLOCK')}
    env = {}
    for n in ('CDRL_SCORE_BINS', 'CDRL_SCORE_HEAD', 'CDRL_SCORE_PER_ACTION'):
        env[n] = int(eval(names[n], {}, dict(env)))
    assert env['CDRL_SCORE_BINS'] == SCORE_BINS and env['CDRL_SCORE_HEAD'] == SCORE_LAYOUT['head_size']
    assert env['CDRL_SCORE_PER_ACTION'] == SCORE_LAYOUT['action_size']
    for A in range(1, 9):
        assert int(eval(names['CDRL_SCORE_BLOCK'], {}, dict(env, A=A))) == score_block_size(A) == score_ref.block(
            np.ones((1, A), np.float32) * 2, np.ones((1, A), np.float32) * 2, np.zeros((1, 4), np.float32), np.full((1, A), 0.5, np.float32)).size
    # the enumerators of the device's own table (csrc/score_block.h), in order
    with open(os.path.join(ROOT, 'carla-driving-rl-agent_amd', 'csrc', 'score_block.h')) as f:
        table = f.read()
    order = re.findall(r'^\s+SCORE_A_(\w+?)(?: = 0)?,', table, re.M)
    assert [o.lower() for o in order] == ['count', 'logp', 'mode_err', 'err', 'err2', 'var', 'entropy', 'cover50', 'cover90', 'hist']
    assert sorted(ACTION.values()) == list(range(10)) and list(ACTION) == ['count', 'log_prob', 'mode_error', 'error', 'error2', 'variance',
                                                                          'entropy', 'cover_50', 'cover_90', 'histogram']
    assert max(HEAD.values()) < SCORE_LAYOUT['head_size'] and len(set(HEAD.values())) == len(HEAD)
    assert 'score' in _build_sources()


def _build_sources():
    import importlib.util
    spec = importlib.util.spec_from_file_location('cdrl_build_for_test', os.path.join(ROOT, 'carla-driving-rl-agent_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SOURCES


# ------------------------------------------------------------------------------------------------ refusals, no device
def _stub(**kw):
    """A CARLAgent that was never constructed: the attributes the host-side checks read, and no network."""
    agent = object.__new__(CARLAgent)
    agent.num_actions, agent.data_parallel, agent.polyak_coeff, agent.batch_size, agent.device = 2, False, 1.0, 8, 'cpu'
    agent.__dict__.update(kw)
    return agent


def test_score_traces_refusals(tmp_path):
    with pytest.raises(ValueError, match='traces_dir'):
        _stub().score_traces()
    with pytest.raises(RuntimeError, match='one GPU'):
        _stub(data_parallel=True).score_traces(str(tmp_path))
    for chunk in (0, -4, 65536, 2.5, True):
        with pytest.raises(ValueError, match=r'^score_traces: chunk = %s: 1 to 65535 rows per forward$' % re.escape(str(chunk))):
            _stub().score_traces(str(tmp_path / 'never-listed'), chunk=chunk)
    with pytest.raises(ValueError, match='chunk = 0'):
        _stub(batch_size=0).score_traces(str(tmp_path))              # the default is the batch size
    with pytest.raises(ValueError, match='no trace'):
        _stub().score_traces(str(tmp_path))
    with pytest.raises(ValueError, match='no trace'):
        _stub(traces_dir=str(tmp_path)).score_traces()               # the agent's own directory
    with pytest.raises(NotImplementedError, match='CARLAgent'):
        PPOAgent.score_traces(_stub())


def test_imitate_validation_refusals(tmp_path):
    with pytest.raises(ValueError, match='polyak=0.5'):
        _stub(polyak_coeff=0.5).imitate(traces_dir=str(tmp_path), validation_dir=str(tmp_path), close=False)
    with pytest.raises(ValueError, match='patience=2.* without validation_dir'):
        _stub().imitate(traces_dir=str(tmp_path), patience=2, close=False)
    for kw in (dict(validation_every=0), dict(validation_every=1.5), dict(patience=0), dict(patience=-1)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            _stub().imitate(traces_dir=str(tmp_path), validation_dir=str(tmp_path), close=False, **kw)
    with pytest.raises(RuntimeError, match='one GPU'):
        _stub(data_parallel=True).imitate(traces_dir=str(tmp_path), validation_dir=str(tmp_path), close=False)
    assert _stub()._validation is None


def test_signatures_and_the_pass_through(monkeypatch):
    params = inspect.signature(CARLAgent.imitate).parameters
    new = {k: params[k] for k in ('validation_dir', 'validation_every', 'patience')}
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in new.values())
    assert {k: p.default for k, p in new.items()} == dict(validation_dir=None, validation_every=1, patience=None)
    params = list(inspect.signature(PPOAgent.score_traces).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [('traces_dir', None), ('max_traces', None), ('chunk', None), ('value', True),
                                                     ('aux', True), ('per_trace', False)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[1:])
    assert inspect.signature(CARLAgent.score_traces) == inspect.signature(PPOAgent.score_traces)
    assert PPOAgent.imitation_epoch_end(_stub(), 1) is False and CARLAgent.imitation_epoch_end(_stub(), 1) is False
    seen = {}
    monkeypatch.setattr(CARLAgent, 'imitate', lambda self, **kw: seen.update(kw) or 'done')
    assert _stub().imitation_learning(traces_dir='x', validation_dir='v', validation_every=2, patience=3) == 'done'
    assert (seen['validation_dir'], seen['validation_every'], seen['patience']) == ('v', 2, 3)
