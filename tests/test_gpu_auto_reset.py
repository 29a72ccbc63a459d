"""learn(..., auto_reset=True): an environment that terminates before `timesteps` is reset on the spot and starts a new trajectory,
every environment records every step, and store() closes ALL trajectories of the rollout with one segmented returns / GAE launch.
Every trajectory's returns / advantages in the memory must be, bit for bit, what the single-trajectory path
(utils.returns_and_advantages on that trajectory's slice, bootstrap built the way PPOMemory.end_trajectory builds it) gives."""
import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
from carla_driving_rl_agent_amd.rl import utils

pytestmark = pytest.mark.gpu

GAMMA, LAMBDA = 0.99, 0.95


def _env(**kw):
    cfg = dict(image_shape=(48, 64, 3), time_horizon=4, num_waypoints=5, vehicle_features=4, num_actions=2)
    cfg.update(kw)
    return FakeCARLAEnvironment(**cfg)


def _agent(env, tmp_path, **kw):
    return CARLAgent(env, batch_size=8, log_mode=None, seed=5, skip_data=0, shuffle=True, policy_lr=3e-4, value_lr=3e-4,
                     dynamics_lr=3e-4, gamma=GAMMA, lambda_=LAMBDA, aug_intensity=0.0, weights_dir=str(tmp_path), name='reset', **kw)


class _Probe:
    """Wraps what the test observes: update() (the memory, the info targets), predict_last_value (the value estimates), the
    environments' reset (counts) and the two utils entry points (counts; the originals stay reachable for the comparisons)."""

    def __init__(self, agent, envs, monkeypatch):
        self.agent, self.updates, self.estimates, self.resets = agent, [], [], [0] * len(envs)
        self.calls = dict(single=0, segments=0, stores=0)
        self.single, segments = utils.returns_and_advantages, utils.returns_and_advantages_segments
        orig_update, orig_last, orig_store = agent.update, agent.network.predict_last_value, agent.store

        def update():
            m = agent.memory
            self.updates.append(dict(n=len(m), returns=m.returns.clone(), adv=m.advantages.clone(), values=m.values.clone(),
                                     rewards=m.rewards.clone(), image=m.states['state_image'].clone(),
                                     info=[x.clone() for x in agent._info(len(m))], segments=list(agent._info_segments),
                                     buffers=[{k: list(v) for k, v in env.info_buffer.items()} for env in envs]))
            orig_update()

        def predict_last_value(state, is_terminal, **kw):
            out = orig_last(state, is_terminal=is_terminal, **kw)
            if not is_terminal:
                self.estimates.append(out.clone())
            return out

        def store(*a, **kw):
            self.calls['stores'] += 1
            return orig_store(*a, **kw)

        def counted(key, fn):
            def call(*a, **kw):
                self.calls[key] += 1
                return fn(*a, **kw)
            return call

        def counted_reset(e, fn):
            def reset():
                self.resets[e] += 1
                return fn()
            return reset

        agent.update, agent.store = update, store
        agent.network.predict_last_value = predict_last_value
        for e, env in enumerate(envs):
            env.reset = counted_reset(e, env.reset)
        monkeypatch.setattr(utils, 'returns_and_advantages', counted('single', self.single))
        monkeypatch.setattr(utils, 'returns_and_advantages_segments', counted('segments', segments))

    def check_trajectories(self, seen, trajectories):
        """`trajectories`: (rows, terminal, estimate row or None) in memory order; the bootstrap is built the old way."""
        r, v = seen['rewards'], seen['values']
        off = 0
        for s, (n, terminal, estimate) in enumerate(trajectories):
            lv = v.new_zeros((1, 2)) if terminal else estimate.reshape(1, 2)
            boot = float((lv[0, 0] * torch.pow(torch.tensor(10.0, device=lv.device), lv[0, 1])).item())
            re, ve = torch.cat([r[off:off + n], r.new_tensor([boot])]), torch.cat([v[off:off + n], lv])
            out = self.single(re, ve, GAMMA, 0.0, 1.0)
            assert torch.equal(out['returns_be'], seen['returns'][off:off + n]), s
            out = self.single(re, ve, GAMMA, LAMBDA, self.agent.adv_scale())
            assert torch.equal(out['advantages'], seen['adv'][off:off + n]), s
            off += n
        assert off == seen['n'] == seen['returns'].shape[0] == seen['adv'].shape[0]


def test_shard_with_auto_reset(tmp_path, monkeypatch):
    E, steps = 3, 12
    envs = [_env(seed=10 + e, episode_length=length) for e, length in enumerate((5, None, 12))]
    agent = _agent(envs[0], tmp_path)
    probe = _Probe(agent, envs, monkeypatch)
    predicts = agent.network.action_index
    before = agent.network.engine.params.clone()
    agent.learn(episodes=1, timesteps=steps, close=False, envs=envs, auto_reset=True)
    assert agent.network.action_index - predicts == steps                    # one batched predict per step
    assert E in agent.network._rollouts
    assert probe.resets == [3, 1, 1]                                         # env 0: at the start and behind steps 5 and 10
    assert len(probe.updates) == 1 and len(probe.estimates) == 1 and probe.estimates[0].shape == (E, 2)
    seen, estimate = probe.updates[0], probe.estimates[0]
    assert seen['n'] == 36 and seen['image'].shape[0] == 36
    assert seen['returns'].shape == (36, 2) and seen['adv'].shape == (36,)
    assert seen['rewards'].shape[0] == 37 and seen['values'].shape == (37, 2)     # + the LAST trajectory's bootstrap entry
    # env 0: 5, 5 terminal + 2 truncated; env 1: 12 truncated; env 2: 12 terminal (not reset)
    probe.check_trajectories(seen, [(5, True, None), (5, True, None), (2, False, estimate[0]), (12, False, estimate[1]),
                                    (12, True, None)])
    assert float(seen['rewards'][36]) == 0.0 and not seen['values'][36].any()     # the terminal last trajectory's bootstrap
    # info targets: cut per trajectory out of the environments' buffers
    segments = [(0, 0, 5), (0, 5, 5), (0, 10, 2), (1, 0, 12), (2, 0, 12)]
    assert seen['segments'] == segments
    for k, key in enumerate(('speed', 'similarity')):
        want = np.concatenate([np.asarray(seen['buffers'][e][key][start:start + rows], dtype=np.float32) for e, start, rows in segments])
        want = torch.as_tensor(want, device=seen['info'][k].device)
        assert torch.equal(seen['info'][k], want / 100.0 if key == 'speed' else want), key
    assert all(len(b['speed']) == steps for b in seen['buffers'])
    after = agent.network.engine.params
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    # ONE segmented launch per store(), none of the single-trajectory ones
    assert probe.calls == dict(single=0, segments=1, stores=1)


def test_same_shard_without_auto_reset_is_unchanged(tmp_path, monkeypatch):
    envs = [_env(seed=10 + e, episode_length=length) for e, length in enumerate((5, None, 12))]
    agent = _agent(envs[0], tmp_path)
    probe = _Probe(agent, envs, monkeypatch)
    agent.learn(episodes=1, timesteps=12, close=False, envs=envs, auto_reset=False)
    seen = probe.updates[0]
    assert seen['n'] == 5 + 12 + 12 and seen['rewards'].shape[0] == 30
    assert seen['segments'] == [(0, 0, 5), (1, 0, 12), (2, 0, 12)]
    assert probe.resets == [1, 1, 1]              # the environment that ended after 5 steps sat idle
    assert probe.calls == dict(single=6, segments=0, stores=1)


def test_one_environment_across_two_stores(tmp_path, monkeypatch):
    """E = 1, episodes of 4 steps, 10 timesteps, update every 2 rollouts: the memory of an update holds 20 rows = trajectories of
    4, 4, 2, 4, 4, 2 (the `append` / `keep_open` path: the first rollout's last bootstrap entry was dropped again)."""
    env = _env(seed=3, episode_length=4)
    agent = _agent(env, tmp_path, update_frequency=2)
    probe = _Probe(agent, [env], monkeypatch)
    before = agent.network.engine.params.clone()
    agent.learn(episodes=4, timesteps=10, close=False, auto_reset=True)
    assert len(probe.updates) == 2 and len(probe.estimates) == 4
    for k, seen in enumerate(probe.updates):
        assert seen['n'] == 20 and seen['rewards'].shape[0] == 21 and seen['segments'] == []
        first, second = probe.estimates[2 * k][0], probe.estimates[2 * k + 1][0]
        probe.check_trajectories(seen, [(4, True, None), (4, True, None), (2, False, first),
                                        (4, True, None), (4, True, None), (2, False, second)])
        assert torch.equal(seen['values'][20], second)                        # the open bootstrap entry is the second rollout's
    assert probe.calls == dict(single=0, segments=4, stores=4)
    assert probe.resets == [12]                                                # 3 per rollout
    after = agent.network.engine.params
    assert torch.isfinite(after).all() and not torch.equal(before, after)
