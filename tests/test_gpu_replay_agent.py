"""CARLAgent(replay_rollouts=K): update() keeps the last K update-periods and trains on them again behind the fresh rows, with
V-trace targets from ONE cdrl_vtrace_segments launch on the acting network's re-evaluation of the kept rows.  Smallest agent of
the agent tests: 48x64 images, batch_size 8, a shard of two synthetic environments of which one ends its trajectory early,
resample_actions=False.  Row counts are multiples of the batch size, so no ragged engine is planned."""
import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
from tests import vtrace_ref as VR

pytestmark = pytest.mark.gpu

GAMMA, LAMBDA, B, STEPS = 0.99, 0.95, 8, 12
ORDER = ('rewards', 'values_be', 'alpha', 'beta', 'actions', 'log_prob_old')


def _envs():
    """Environment 0 ends every trajectory after 4 steps, environment 1 never: 4 + 12 = 16 rows per episode, and with auto-reset
    4 + 4 + 4 + 12 = 24."""
    cfg = dict(image_shape=(48, 64, 3), time_horizon=4, num_waypoints=5, vehicle_features=4, num_actions=2)
    return [FakeCARLAEnvironment(seed=10, episode_length=4, **cfg), FakeCARLAEnvironment(seed=11, episode_length=None, **cfg)]


def _agent(env, tmp_path, **kw):
    kw.setdefault('log_mode', None)
    return CARLAgent(env, batch_size=B, seed=5, skip_data=0, shuffle=True, policy_lr=3e-4, value_lr=3e-4, dynamics_lr=3e-4, gamma=GAMMA,
                     lambda_=LAMBDA, aug_intensity=0.0, weights_dir=str(tmp_path), name='replay', resample_actions=False, **kw)


class _Run:
    """learn() for `episodes` episodes, observing every update(): the memory before it, the batch tensors it formed, the refresh it
    ran, the optimizer step counters behind it and what it logged."""

    def __init__(self, tmp_path, episodes, learn_kw=None, **kw):
        envs = _envs()
        self.agent = agent = _agent(envs[0], tmp_path, **kw)
        self.updates, self.logged = [], []
        update, policy, value, joint, log = (agent.update, agent.policy_batch_tensors, agent.value_batch_tensors,
                                             agent.joint_batch_tensors, agent.log)

        def observed_update():
            m = agent.memory
            seen = dict(n=len(m), actions=m.actions.clone(), log_probs=m.log_probabilities.clone(), advantages=m.advantages.clone(),
                        returns=m.returns.clone(), rewards=m.rewards[:len(m)].clone(), info=[x.clone() for x in agent._info(len(m))],
                        kept=[p.rows for p in agent.replay.periods] if agent.replay is not None else [])
            self.updates.append(seen)
            update()
            seen['steps'] = agent.network.engine.get_optimizer_state()
            seen['refresh'] = agent.replay.last_refresh if agent.replay is not None else None

        def keep(name, fn):
            def call():
                out = fn()
                self.updates[-1][name] = out
                return out
            return call

        def observed_log(**entries):
            self.logged.append(entries)
            log(**entries)

        agent.update, agent.log = observed_update, observed_log
        agent.policy_batch_tensors, agent.value_batch_tensors = keep('policy', policy), keep('value', value)
        agent.joint_batch_tensors = keep('joint', joint)
        agent.learn(episodes=episodes, timesteps=STEPS, close=False, envs=envs, **(learn_kw or {}))
        torch.cuda.synchronize()
        self.params = agent.network.engine.params.clone()

    def steps(self, k):
        s = self.updates[k]['steps']
        return s['t_policy'], s['t_value']


def _check_refresh(refresh, rows):
    """The refresh's targets against the float64 restatement on the inputs the refresh itself produced."""
    h = {k: refresh[k].cpu().numpy() for k in ORDER}
    assert h['alpha'].shape == (rows, 2) and np.isfinite(h['alpha']).all() and (h['alpha'] > 0).all() and (h['beta'] > 0).all()
    ref = VR.segments(*(h[k] for k in ORDER), refresh['lengths'], GAMMA, LAMBDA, 1.0, 1.0, refresh['scale'])
    span = max(1.0, float(np.abs(ref['returns']).max()))
    g = {k: refresh[k].cpu().numpy().astype(np.float64) for k in ('advantages', 'advantages_raw', 'returns', 'returns_be', 'rho')}
    fig = dict(adv_raw=np.abs(g['advantages_raw'] - ref['adv_raw']).max() / span, returns=np.abs(g['returns'] - ref['returns']).max() / span,
               returns_be=np.abs(g['returns_be'][:, 0] * 10.0 ** g['returns_be'][:, 1] - ref['returns']).max() / span,
               adv=np.abs(g['advantages'] - ref['adv']).max() / refresh['scale'], rho=(np.abs(g['rho'] - ref['rho']) / ref['rho']).max())
    print('replay refresh bounds:', ' '.join(f'{k}={v:.3e}' for k, v in fig.items()), f'span={span:.4g}')
    for k, v in fig.items():
        assert v <= 1e-5, (k, v)


def _check_second_update(run, trajectories, joint=False):
    """Update 1 runs today's steps on its fresh rows; update 2 trains on fresh + kept rows: the kept period's rows sit behind the fresh
    ones with the stored actions / behaviour log-probabilities / info targets and the refresh's V-trace targets."""
    first, second = run.updates
    n = first['n']
    assert n == second['n'] == sum(rows for rows, _ in trajectories) and n % B == 0
    assert first['kept'] == [] and second['kept'] == [n]
    assert first['refresh'] is None
    assert run.steps(0) == (n // B, n // B)                         # the step count of today
    assert run.steps(1) == (n // B + 2 * n // B,) * 2               # + the steps of fresh and kept rows
    refresh = second['refresh']
    assert refresh['lengths'] == [rows for rows, _ in trajectories]
    _check_refresh(refresh, n)
    # what the refresh read is what the first period stored; terminal trajectories bootstrap from zero, truncated ones do not
    assert torch.equal(refresh['actions'], first['actions']) and torch.equal(refresh['log_prob_old'], first['log_probs'])
    row = 0
    for s, (rows, terminal) in enumerate(trajectories):
        pad = row + s
        assert torch.equal(refresh['rewards'][pad:pad + rows], first['rewards'][row:row + rows]), s
        assert bool(refresh['values_be'][pad + rows].any()) == (not terminal), s
        row += rows
    # the batches: fresh rows keep the GAE kernel's values bit for bit, kept rows follow
    batch = second['joint'] if joint else second['policy']
    states, adv, actions, log_probs, speed, similarity = batch[:6]
    assert states['state_image'].shape[0] == 2 * n
    assert torch.equal(adv[:n], second['advantages']) and torch.equal(adv[n:], refresh['advantages'])
    assert torch.equal(actions[:n], second['actions']) and torch.equal(actions[n:], first['actions'])
    assert torch.equal(log_probs[:n], second['log_probs']) and torch.equal(log_probs[n:], first['log_probs'])
    for got, k in ((speed, 0), (similarity, 1)):
        assert torch.equal(got[:n], second['info'][k]) and torch.equal(got[n:], first['info'][k])
    returns = batch[6] if joint else second['value'][1]
    assert torch.equal(returns[:n], second['returns']) and torch.equal(returns[n:], refresh['returns_be'])
    assert torch.isfinite(run.params).all()
    store = run.agent.replay
    assert len(store) == 1 and store.periods[0].rows == n and store.periods[0].targets is None
    assert torch.equal(store.periods[0].actions, second['actions'])         # the second period replaced the first


SHARD = [(4, True), (12, False)]
SHARD_AUTO_RESET = [(4, True), (4, True), (4, True), (12, False)]


def test_zero_kept_rollouts_is_the_agent_of_today(tmp_path):
    plain = _Run(tmp_path / 'a', 2)
    zero = _Run(tmp_path / 'b', 2, replay_rollouts=0)
    assert zero.agent.replay is None
    assert torch.equal(plain.params, zero.params)
    assert plain.steps(1) == zero.steps(1) == (4, 4)


def test_one_kept_rollout(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                                     # (the summary file of log_mode goes under the working directory)
    run = _Run(tmp_path, 2, replay_rollouts=1, log_mode='summary')
    _check_second_update(run, SHARD)
    logged = [e for e in run.logged if 'replay_rows' in e]
    assert len(logged) == 1 and logged[0]['replay_rows'] == 16      # logged by the update that reused rows, once
    rho = run.updates[1]['refresh']['rho'].double()
    assert logged[0]['replay_rho_mean'] == pytest.approx(float(rho.mean()), rel=1e-12)
    assert logged[0]['replay_rho_clipped'] == pytest.approx(float((rho > 1.0).double().mean()), rel=1e-12)
    again = _Run(tmp_path / 'again', 2, replay_rollouts=1, log_mode='summary')
    assert torch.equal(run.params, again.params)                    # learn, learn with replay: the same bits run to run
    plain = _Run(tmp_path / 'plain', 2, log_mode='summary')
    assert not torch.equal(run.params, plain.params)                # ... and the kept rows did train


def test_one_kept_rollout_with_auto_reset(tmp_path):
    _check_second_update(_Run(tmp_path, 2, learn_kw=dict(auto_reset=True), replay_rollouts=1), SHARD_AUTO_RESET)


def test_one_kept_rollout_with_the_joint_update(tmp_path):
    _check_second_update(_Run(tmp_path, 2, replay_rollouts=1, joint_update=True), SHARD, joint=True)


def test_two_kept_rollouts_hold_the_last_two_periods(tmp_path, capsys):
    run = _Run(tmp_path, 3, replay_rollouts=2, replay_rho_clip=2.0, replay_c_clip=1.5)
    store = run.agent.replay
    assert [u['kept'] for u in run.updates] == [[], [16], [16, 16]]
    assert len(store) == 2
    for period, seen in zip(store.periods, run.updates[1:]):        # periods 2 and 3, oldest first
        assert torch.equal(period.actions, seen['actions']) and torch.equal(period.log_probs, seen['log_probs'])
    assert run.updates[2]['refresh']['lengths'] == [4, 12, 4, 12]   # ONE launch covered both kept periods
    assert run.steps(2) == (2 + 4 + 6, 2 + 4 + 6)
    capsys.readouterr()
    run.agent.save_state()
    assert '32 kept rollout rows of the replay store (2 periods) are not saved' in capsys.readouterr().out
    run.agent.clear_replay()
    assert len(store) == 0


def test_a_padded_last_chunk_gives_the_rows_of_a_full_one(tmp_path):
    """distribution_and_value on 11 rows in chunks of 8: rows 8..10 come from a chunk filled up with repeats of row 10; the same rows
    at other positions of a full chunk (rows 3..10) give the same numbers."""
    envs = _envs()
    agent = _agent(envs[0], tmp_path, replay_rollouts=1)
    rng = np.random.default_rng(0)
    spec = agent.state_spec
    states = {k: torch.as_tensor(rng.uniform(0, 1, (11, 4) + tuple(spec[k])).astype(np.float32)).cuda()
              for k in ('state_image', 'state_road', 'state_vehicle', 'state_navigation')}
    alpha, beta, value = agent.network.distribution_and_value(states, chunk=B)
    assert alpha.shape == (11, 2) and value.shape == (11, 2)
    full = agent.network.distribution_and_value({k: v[3:11] for k, v in states.items()}, chunk=B)
    for got, want in zip((alpha, beta, value), full):
        assert torch.isfinite(got).all()
        assert torch.allclose(got[8:11], want[5:8], rtol=1e-5, atol=1e-6)
    assert set(agent.network._rollouts) == {1, B}                   # one inference engine more, whatever the row count
