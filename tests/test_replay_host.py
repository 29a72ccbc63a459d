"""Reuse of recent rollouts on the host (PPOAgent(replay_rollouts=K), rl/replay.py): the store's bookkeeping on CPU tensors, the
trajectory table that store() / store_segments() feed through trajectory_stored, the refusals, and the header.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd.rl.agents.ppo import PPOAgent, Rollout
from carla_driving_rl_agent_amd.rl.replay import ReplayPeriod, RolloutReplay, TrajectoryTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 2


def _period(tag, trajectories):
    n = sum(rows for rows, _ in trajectories)
    truncated = sum(1 for _, terminal in trajectories if not terminal)
    states = dict(state_image=torch.full((n, 3), float(tag)), state_road=torch.zeros((n, 2)))
    finals = dict(state_image=torch.full((truncated, 3), float(tag)), state_road=torch.zeros((truncated, 2))) if truncated else None
    return ReplayPeriod(states, torch.zeros((n, A)), torch.zeros((n, A)), torch.arange(n, dtype=torch.float32), trajectories, finals,
                        info=dict(speed=torch.zeros(n), similarity=torch.zeros(n)))


def test_store_evicts_the_oldest_period():
    store = RolloutReplay(2)
    first, second, third = _period(1, [(3, True)]), _period(2, [(2, False), (4, True)]), _period(3, [(5, False)])
    assert store.add(first) is None and store.add(second) is None
    assert len(store) == 2 and store.rows == 9
    assert store.add(third) is first                                    # full: the oldest leaves
    assert list(store.periods) == [second, third] and store.rows == 11
    store.clear()
    assert len(store) == 0 and store.rows == 0 and store.last_refresh is None
    with pytest.raises(ValueError, match='at least one period'):
        RolloutReplay(0)


def test_period_checks_its_table_and_lays_out_the_padded_index():
    p = _period(7, [(3, True), (1, False), (2, False)])
    assert p.rows == 6 and p.lengths == [3, 1, 2] and p.truncated == [1, 2]
    rows, boots = p.padded_index()
    assert rows.tolist() == [0, 1, 2, 4, 6, 7] and boots.tolist() == [3, 5, 8]          # every trajectory, then its bootstrap entry
    assert sorted(rows.tolist() + boots.tolist()) == list(range(p.rows + len(p.trajectories)))
    with pytest.raises(ValueError, match='final observations'):
        ReplayPeriod(p.states, p.actions, p.log_probs, p.rewards, [(3, True), (1, False), (2, False)], None)
    with pytest.raises(ValueError, match='counts 7 rows, states holds 6'):
        ReplayPeriod(p.states, p.actions, p.log_probs, p.rewards, [(3, True), (4, True)], None)
    with pytest.raises(ValueError, match='at least one row'):
        ReplayPeriod(p.states, p.actions, p.log_probs, p.rewards, [(6, True), (0, True)], None)


class _Memory:
    def __init__(self):
        self.rows = 0

    def extend(self, states, actions, rewards, values, log_probs):
        self.rows += int(actions.shape[0])

    def extend_trajectories(self, trajectories, last_values, gamma, lambda_, scale, append=False):
        trajectories = list(trajectories)
        for t in trajectories:
            self.extend(*t)
        return tuple([None] * len(trajectories) for _ in range(3))

    def drop_bootstrap(self):
        pass


class _Network:
    def predict_last_value(self, state, is_terminal, **kw):
        return torch.zeros((1, 2)) if is_terminal else torch.zeros((state['state_image'].shape[0], 2))


def _bare_agent(replay_rollouts=2):
    """A PPOAgent that never ran __init__ (no engine): what store() / store_segments() and the table need."""
    agent = object.__new__(PPOAgent)
    agent.replay = RolloutReplay(replay_rollouts) if replay_rollouts else None
    agent._replay_table, agent._replay_active = TrajectoryTable(), []
    agent.memory, agent.network, agent.device = _Memory(), _Network(), 'cpu'
    agent.update_frequency, agent.gamma, agent.lambda_ = 1, 0.99, 0.95
    agent.adv_scale = lambda: 2.0
    agent.adv_scale.value = 2.0
    agent.log = lambda **kw: None
    agent.end_episode = lambda last_value, append=False: None
    return agent


def _rollout(E, steps, lengths=None):
    """A recorded rollout of E environments: environment e's image rows hold 100 * e + step, its final observation 100 * e + 99."""
    r = Rollout(E, steps, 'cpu')
    for t in range(steps):
        running = [e for e in range(E) if lengths is None or t < lengths[e]]
        image = torch.tensor([[100.0 * e + t] * 3 for e in range(E)])
        r.record(dict(state_image=image), torch.zeros((E, A)), torch.zeros((E, A)), torch.zeros((E, 2)), running)
        for e in running:
            r.rewards[e].append(0.0)
    r.final = dict(state_image=torch.tensor([[100.0 * e + 99] * 3 for e in range(E)]))
    return r


def test_store_feeds_the_trajectory_table():
    agent = _bare_agent()
    rollout = _rollout(3, 6, lengths=[4, 6, 6])
    rollout.terminal = [True, False, True]
    agent.store(rollout, timesteps=6, keep_open=False)
    table = agent._replay_table
    assert table.entries == [(4, True), (6, False), (6, True)] and agent.memory.rows == 16
    finals = table.stacked_finals()
    assert finals['state_image'].tolist() == [[199.0] * 3]             # kept for the truncated trajectory only: environment 1's row


def test_store_segments_feeds_the_trajectory_table_across_two_stores():
    agent = _bare_agent()
    agent.update_frequency = 2
    for k in range(2):
        rollout = _rollout(2, 6)
        for t in range(6):                      # environment 0: trajectories of 4 (terminal) and 2 (truncated); environment 1: 6, terminal
            for e in range(2):
                rollout.length[e] = t + 1
                rollout.env_steps[e] = t + 1
                if (e == 0 and t == 3) or t == 5:
                    rollout.close_segment(e, terminal=(e == 1 or t == 3))
        agent.store(rollout, timesteps=6, keep_open=(k == 0), auto_reset=True)
    table = agent._replay_table
    assert table.entries == [(4, True), (2, False), (6, True)] * 2 and agent.memory.rows == 24
    assert table.stacked_finals()['state_image'].tolist() == [[99.0] * 3] * 2
    agent.discard_period()
    assert len(agent._replay_table) == 0


def test_without_replay_nothing_is_recorded():
    agent = _bare_agent(replay_rollouts=0)
    rollout = _rollout(1, 3)
    agent.store(rollout, timesteps=3, keep_open=False)
    assert len(agent._replay_table) == 0
    fresh = torch.zeros(3)
    assert agent.with_replay(fresh, 'advantages') is fresh
    agent.clear_replay()                        # a no-op without a store


def test_with_replay_puts_the_kept_rows_behind_the_fresh_ones():
    agent = _bare_agent()
    kept = _period(4, [(2, True), (1, False)])
    kept.targets = dict(advantages=torch.tensor([1.0, 2.0, 3.0]), returns_be=torch.ones((3, 2)))
    kept.info['speed'] = torch.tensor([7.0, 8.0, 9.0])
    agent._replay_active = [kept]
    assert agent.with_replay(torch.zeros(2), 'advantages').tolist() == [0.0, 0.0, 1.0, 2.0, 3.0]
    assert agent.with_replay(torch.zeros(2), 'speed').tolist() == [0.0, 0.0, 7.0, 8.0, 9.0]
    states = agent.with_replay(dict(state_image=torch.zeros((2, 3)), state_road=torch.zeros((2, 2))), 'states')
    assert states['state_image'][:, 0].tolist() == [0.0, 0.0, 4.0, 4.0, 4.0] and states['state_road'].shape == (5, 2)
    agent.replay.add(kept)
    agent.clear_replay()
    assert len(agent.replay) == 0 and agent._replay_active == []


# ---------------------------------------------------------------------------------------------------------------- refusals
def _host_agent(monkeypatch, **kw):
    """A real CARLAgent whose learner engines are host-only (planned, never bound)."""
    from carla_driving_rl_agent_amd.core import networks, CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    monkeypatch.setattr(networks, 'LearnerEngine',
                        lambda B, device=None, share_with=None, **cfg: LearnerEngine(B, device=None, share_with=share_with, **cfg))
    monkeypatch.setattr(networks, 'init_engine_parameters', lambda *a, **k: None)
    env = FakeCARLAEnvironment(image_shape=(48, 64, 3), time_horizon=4, num_waypoints=5, vehicle_features=4, num_actions=A)
    return CARLAgent(env, batch_size=8, log_mode=None, seed=3, device='cpu', aug_intensity=0.0, **kw)


def test_accepted_options(monkeypatch, tmp_path):
    agent = _host_agent(monkeypatch, replay_rollouts=2, replay_rho_clip=2.0, replay_c_clip=0.0, resample_actions=False,
                        weights_dir=str(tmp_path))
    assert agent.replay.capacity == 2 and (agent.replay_rho_clip, agent.replay_c_clip) == (2.0, 0.0)
    agent.save_config()
    assert not any('replay' in k for k in agent.config)                 # not written to config.json
    assert _host_agent(monkeypatch).replay is None                      # the default keeps nothing


def test_resampled_loss_is_refused(monkeypatch):
    with pytest.raises(ValueError, match='resample_actions=False'):
        _host_agent(monkeypatch, replay_rollouts=1)                     # resample_actions defaults to True
    assert _host_agent(monkeypatch, replay_rollouts=0).replay is None   # ... and stays usable without replay


@pytest.mark.parametrize('kw', [dict(replay_rollouts=-1), dict(replay_rollouts=1.5), dict(replay_rollouts=1, replay_rho_clip=-0.1),
                                dict(replay_rollouts=1, replay_c_clip=-1.0), dict(replay_rollouts=1, replay_rho_clip=float('nan'))])
def test_negative_count_or_clips_are_refused(monkeypatch, kw):
    with pytest.raises(ValueError, match='>= 0'):
        _host_agent(monkeypatch, resample_actions=False, **kw)


def test_data_parallel_run_is_refused(monkeypatch):
    from carla_driving_rl_agent_amd.core import carla_agent, networks
    built = []
    monkeypatch.setattr(carla_agent.dist, 'is_available', lambda: True)
    monkeypatch.setattr(carla_agent.dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(carla_agent.dist, 'get_world_size', lambda: 2)
    monkeypatch.setattr(carla_agent.dist, 'get_rank', lambda: 0)
    monkeypatch.setattr(networks, 'LearnerEngine', lambda *a, **k: built.append(a))
    env = carla_agent.FakeCARLAEnvironment(image_shape=(48, 64, 3), time_horizon=4, num_waypoints=5, vehicle_features=4, num_actions=A)
    with pytest.raises(RuntimeError, match='replay_rollouts=0'):
        carla_agent.CARLAgent(env, batch_size=8, log_mode=None, device='cpu', replay_rollouts=1, resample_actions=False)
    assert not built                                                    # refused before any engine was planned


def test_header_declares_both_functions():
    header = open(os.path.join(ROOT, 'include', 'cdrl.h')).read()
    assert re.search(r'\bint\s+cdrl_vtrace_segments\s*\(', header)
    assert re.search(r'\bint64_t\s+cdrl_vtrace_segments_scratch_doubles\s*\(\s*int N,\s*int S\s*\)', header)
    from carla_driving_rl_agent_amd import _lib
    lib = _lib.load()
    assert len(lib.cdrl_vtrace_segments.argtypes) == 22
    assert int(lib.cdrl_vtrace_segments_scratch_doubles(10, 3)) == 40
    assert lib.cdrl_version() == 1
