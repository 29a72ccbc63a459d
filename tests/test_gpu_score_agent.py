"""Scoring on held-out traces on the GPU, agent level (CARLAgent.score_traces, imitate(validation_dir=...)):
FakeCARLAEnvironment at 48x64, time_horizon 2, two actions, a short learn() first; two traces of 37 and 50 rows of seeded random
data.  score_traces against the restatement (tests/score_ref.py) applied to what the same inference engine gives for the same
rows; that scoring between two learn() calls and validating inside imitate() leave training bit for bit where it was."""
import json
import os

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import traces
from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
from carla_driving_rl_agent_amd.engine import read_score_block
from tests import score_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
T, A, BATCH = 2, 2, 8
KEYS = ('state_image', 'state_road', 'state_vehicle', 'state_navigation')
BOUND = 1e-9
FIGURES = ('log_prob', 'mode_error', 'bias', 'rmse', 'predicted_std', 'entropy', 'value_bias', 'value_rmse', 'explained_variance',
           'speed_rmse', 'similarity_rmse')
VALIDATION = ('validation_log_prob', 'validation_mode_error', 'validation_rmse', 'validation_coverage_90', 'validation_value_rmse')


def _env(**kw):
    cfg = dict(image_shape=(48, 64, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=A)
    cfg.update(kw)
    return FakeCARLAEnvironment(**cfg)


def _agent(root, **kw):
    cfg = dict(batch_size=BATCH, log_mode=None, seed=5, skip_data=0, shuffle=True, policy_lr=3e-4, value_lr=3e-4, dynamics_lr=3e-4,
               aug_intensity=0.0, weights_dir=os.path.join(str(root), 'weights'), name='score')
    cfg.update(kw)
    return CARLAgent(_env(seed=1, episode_length=None), **cfg)


def _write(path, episode, n, seed, reward=True, info=True):
    """One trace of seeded random data, rows with the time_horizon axis."""
    rng = np.random.default_rng(seed)
    data = dict(state_image=rng.random((n, T, 48, 64, 3), dtype=np.float32), state_road=rng.random((n, T, 9), dtype=np.float32),
                state_vehicle=rng.random((n, T, 4), dtype=np.float32), state_navigation=rng.random((n, T, 5), dtype=np.float32))
    actions = rng.uniform(-1.0, 1.0, (n, A)).astype(np.float32)
    actions[0, 0], actions[1, 1] = -1.0, 1.0                                   # the unit action at both ends of the interval
    inf = dict(speed=rng.uniform(0.0, 30.0, n), similarity=rng.uniform(-1.0, 1.0, n)) if info else None
    if reward:
        return traces.write_trace(path, episode, data, actions, rng.uniform(0.0, 1.0, n).astype(np.float32), np.zeros(n, np.float32), inf)
    os.makedirs(path, exist_ok=True)                                           # (write_trace always writes the rewards)
    name = os.path.join(path, f'trace-{episode}-bare.npz')
    np.savez_compressed(name, action=actions, done=np.zeros(n, np.float32), **data)
    return name


@pytest.fixture(scope='module')
def held_out(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('held_out'))
    _write(path, 1, 37, seed=31)
    _write(path, 2, 50, seed=32)
    return path


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """An agent after a few learn() steps: the moving statistics are no longer at their initial values."""
    agent = _agent(tmp_path_factory.mktemp('score'))
    agent.learn(episodes=1, timesteps=12, close=False)
    return agent


def _reference(agent, path, chunk, per_trace=False):
    """The restatement on what rollout_for(chunk) gives for the traces' rows, `chunk` at a time, the last chunk filled up by
    repeating the last row.  -> (block or list of blocks, the smallest distance of a reference PIT to an edge)."""
    net = agent.network
    eng = net.rollout_for(chunk)
    blocks, prior, distance = [], None, np.inf
    for trace in traces.load_traces(path):
        data = agent._trace_tensors(trace, None, True, 1.0)
        n = data['u'].shape[0]
        alpha, beta, value = np.empty((n, A), np.float32), np.empty((n, A), np.float32), np.empty((n, 4), np.float32)
        for start in range(0, n, chunk):
            m = min(chunk, n - start)
            index = torch.arange(start, start + chunk, device=DEV).clamp_(max=n - 1)
            eng.predict({k: data['states'][k].index_select(0, index) for k in KEYS})
            dist, val = eng._pred_out[0].cpu().numpy(), eng._pred_out[1].cpu().numpy()
            alpha[start:start + m], beta[start:start + m], value[start:start + m] = dist[:m, 0], dist[:m, 1], val[:m]
        got = [x.cpu().numpy() for x in net.distribution_and_value(data['states'], chunk=chunk)]
        assert np.array_equal(got[0], alpha) and np.array_equal(got[1], beta) and np.array_equal(got[2], value[:, :2])
        u = data['u'].cpu().numpy()
        distance = min(distance, float(score_ref.edge_distance(score_ref.pit(alpha, beta, u)).min()))
        block = score_ref.block(alpha, beta, value, u, data['returns'].cpu().numpy(), data['speed'].cpu().numpy(),
                                data['similarity'].cpu().numpy(), prior=None if per_trace else prior)
        prior = block
        blocks.append(block)
    return (blocks if per_trace else prior), distance


@pytest.mark.parametrize('chunk', [4, 32])
def test_score_traces_against_the_restatement(trained, held_out, chunk):
    agent = trained
    index = agent.network.action_index
    out = agent.score_traces(held_out, chunk=chunk)
    assert agent.network.action_index == index
    want, distance = _reference(agent, held_out, chunk)
    assert distance >= 1e-6, 'a reference PIT lies on an edge: draw the traces from another seed'
    assert out['rows'] == 87 == want[0]                                        # 37 + 50: no padded row is counted
    exact, err = score_ref.compare(out['block'], want, A)
    ref = read_score_block(torch.as_tensor(want), A)
    worst = max(abs(out[k] - ref[k]) / max(1.0, abs(ref[k])) for k in FIGURES)
    print(f'score_traces chunk={chunk}: worst sum error / max(1, |ref|) {err:.3e}, worst figure error {worst:.3e}; '
          f'log_prob {out["log_prob"]:.4f}, rmse {out["rmse"]:.4f}, coverage_90 {out["coverage_90"]}, value_rmse {out["value_rmse"]:.4f}')
    assert exact and err < BOUND and worst < BOUND
    assert np.array_equal(out['pit_histogram'], ref['pit_histogram']) and out['pit_histogram'].sum() == 87 * A
    assert out['coverage_50'] == ref['coverage_50'] and out['coverage_90'] == ref['coverage_90']
    assert out['nonfinite'] == 0 and out['pit_unconverged'] == 0
    assert len(out['log_prob_per_action']) == A and all(np.isfinite(out[k]) for k in FIGURES)
    assert np.array_equal(agent.score_traces(held_out, chunk=chunk)['block'], out['block'])         # the same rows: the same bits


def test_per_trace_blocks_add_up(trained, held_out):
    total = trained.score_traces(held_out, chunk=8)
    out = trained.score_traces(held_out, chunk=8, per_trace=True)
    assert [t['rows'] for t in out['traces']] == [37, 50] and out['rows'] == 87              # sorted file order
    assert np.array_equal(out['block'], out['traces'][0]['block'] + out['traces'][1]['block'])
    exact, err = score_ref.compare(out['block'], total['block'], A)
    assert exact and err < BOUND
    want, _ = _reference(trained, held_out, 8, per_trace=True)
    for t, w in zip(out['traces'], want):
        exact, err = score_ref.compare(t['block'], w, A)
        assert exact and err < BOUND
    first = trained.score_traces(held_out, chunk=8, max_traces=1)
    assert first['rows'] == 37 and np.array_equal(first['block'], out['traces'][0]['block'])


def test_traces_without_reward_or_info(trained, tmp_path, capsys):
    bare, plain = str(tmp_path / 'bare'), str(tmp_path / 'plain')
    _write(bare, 1, 11, seed=41, reward=False, info=False)
    _write(bare, 2, 9, seed=42, reward=False, info=False)
    _write(plain, 1, 11, seed=41)
    _write(plain, 2, 9, seed=42)
    capsys.readouterr()
    out = trained.score_traces(bare)
    printed = capsys.readouterr().out
    assert printed.count('has no reward') == 1 and printed.count('has no info_speed') == 1          # one line each, not one per trace
    assert out['rows'] == 20 and all(out[k] is None for k in FIGURES[6:]) and all(np.isfinite(out[k]) for k in FIGURES[:6])
    full = trained.score_traces(plain)
    assert 'has no' not in capsys.readouterr().out
    assert all(full[k] is not None and np.isfinite(full[k]) for k in FIGURES)
    head = 16
    assert np.array_equal(out['block'][head:], full['block'][head:]) and (out['block'][1:3] == 0).all()     # the actions score alike
    off = trained.score_traces(plain, value=False, aux=False)
    assert np.array_equal(off['block'], out['block']) and 'has no' not in capsys.readouterr().out


def _learner_state(agent):
    torch.cuda.synchronize()
    s = agent.network.engine.export_state()
    return s['params'], s['adam_m'], s['adam_v'], s['optimizer']


def _batch(agent, seed):
    return agent.observe([_env(seed=seed).reset()], agent.preprocess())


def test_scoring_between_two_learn_calls_changes_nothing(tmp_path, held_out):
    def run(with_score):
        agent = _agent(tmp_path / f'run{int(with_score)}')
        agent.learn(episodes=1, timesteps=12, close=False)
        if with_score:
            agent.score_traces(held_out, chunk=16)
            agent.score_traces(held_out, per_trace=True, value=False)
        agent.learn(episodes=1, timesteps=12, close=False)
        sample = agent.predict(_batch(agent, seed=71))
        return _learner_state(agent), agent.network.action_index, sample

    (p0, m0, v0, o0), i0, s0 = run(False)
    (p1, m1, v1, o1), i1, s1 = run(True)
    assert i0 == i1 and o0 == o1
    assert np.array_equal(p0, p1) and np.array_equal(m0, m1) and np.array_equal(v0, v1)     # parameters, moving statistics, slots
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))                                     # the next sampled predict
    assert np.isfinite(p0).all()


def _lines(root, name, key):
    return [l for l in (json.loads(s) for s in open(os.path.join(str(root), 'logs', name, 'summary.jsonl'))) if l['key'] == key]


@pytest.fixture(scope='module')
def training(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('training'))
    _write(path, 1, 19, seed=51)
    _write(path, 2, 16, seed=52)
    return path


def test_validation_leaves_imitate_bit_for_bit(tmp_path, monkeypatch, training, held_out):
    monkeypatch.chdir(tmp_path)                                          # Summary writes under ./logs/<name>
    plain, checked = _agent(tmp_path / 'a', log_mode='summary', name='plain'), _agent(tmp_path / 'b', log_mode='summary', name='checked')
    plain.imitate(epochs=3, traces_dir=training, value_weight=0.5, close=False)
    checked.imitate(epochs=3, traces_dir=training, value_weight=0.5, close=False, validation_dir=held_out)
    (p0, m0, v0, o0), (p1, m1, v1, o1) = _learner_state(plain), _learner_state(checked)
    assert o0 == o1 and np.array_equal(p0, p1) and np.array_equal(m0, m1) and np.array_equal(v0, v1)
    assert (plain._sample_offset, plain.network.action_index) == (checked._sample_offset, checked.network.action_index)
    assert checked._validation is None
    for key in VALIDATION:
        lines = _lines(tmp_path, 'checked', key)
        assert len(lines) == 3 and all(l['n'] == 1 and np.isfinite(l['mean']) for l in lines), key
        assert not _lines(tmp_path, 'plain', key)
    print('validation_log_prob per epoch:', [round(l['mean'], 4) for l in _lines(tmp_path, 'checked', 'validation_log_prob')])
    assert len(_lines(tmp_path, 'checked', 'imitation_loss_clone')) == len(_lines(tmp_path, 'plain', 'imitation_loss_clone')) == 6
    # every second epoch: one validation in three epochs
    third = _agent(tmp_path / 'c', log_mode='summary', name='third')
    third.imitate(epochs=3, traces_dir=training, close=False, validation_dir=held_out, validation_every=2)
    assert len(_lines(tmp_path, 'third', 'validation_log_prob')) == 1


def _epochs_the_rule_allows(values, patience, epochs):
    best, stale = -np.inf, 0
    for i, v in enumerate(values):
        best, stale = (v, 0) if v > best else (best, stale + 1)
        if stale >= patience:
            return i + 1
    return epochs


def test_patience_stops_a_run_that_cannot_improve(tmp_path, monkeypatch, training, held_out, capsys):
    """patience=1 ends a run at the second validation when the metric cannot improve: exactly 2 of 5 epochs.
    A run with lr=0.0 is NOT such a run: the weights stand still, but the clone passes still move the BatchNorm moving statistics,
    which the acting network reads -- measured here, validation_log_prob over five epochs at lr=0.0: -0.332219, -0.331550, -0.331037,
    -0.330634, -0.330290, every one a new best.  So that run is held against the rule applied to its own logged values, and the run
    that cannot improve is one whose epochs read no training file (max_traces=0): nothing the acting network reads changes."""
    monkeypatch.chdir(tmp_path)
    still = _agent(tmp_path / 'a', log_mode='summary', name='still')
    still.imitate(epochs=5, traces_dir=training, max_traces=0, lr=0.0, close=False, validation_dir=held_out, patience=1)
    lines = _lines(tmp_path, 'still', 'validation_log_prob')
    assert len(lines) == 2 and lines[0]['mean'] == lines[1]['mean']     # the first is the best so far, the second is no better
    assert capsys.readouterr().out.count('no new best validation_log_prob') == 1
    still.imitate(epochs=5, traces_dir=training, max_traces=0, lr=0.0, close=False, validation_dir=held_out, patience=2)
    assert len(_lines(tmp_path, 'still', 'validation_log_prob')) == 2 + 3
    assert capsys.readouterr().out.count('no new best validation_log_prob') == 1
    agent = _agent(tmp_path / 'b', log_mode='summary', name='patient')
    agent.imitate(epochs=5, traces_dir=training, lr=0.0, close=False, validation_dir=held_out, patience=1)
    values = [l['mean'] for l in _lines(tmp_path, 'patient', 'validation_log_prob')]
    print('validation_log_prob at lr=0.0:', values)
    assert len(values) == _epochs_the_rule_allows(values, 1, 5)
    assert len(_lines(tmp_path, 'patient', 'imitation_loss_clone')) == 2 * len(values)               # no epoch behind the stop
    assert ('no new best validation_log_prob' in capsys.readouterr().out) == (len(values) < 5)
