"""Host logic of auto-reset rollouts on the CPU: Rollout's per-environment segment bookkeeping and memory order, and
PPOMemory.extend_trajectories (all trajectories closed by ONE segmented returns / GAE call) against the existing per-trajectory loop
(extend + end_trajectory + compute_returns + compute_advantages + update_index + drop_bootstrap, what PPOAgent.store / end_episode
run today).  The device helpers have no CPU form: oracle/gae.py stands in for both, the segmented stand-in runs per segment."""
import numpy as np
import pytest
import torch

from oracle import gae as OG

GAMMA, LAMBDA, SCALE = 0.99, 0.95, 2.0
STEPS = 12
# (start_step, stop_step, terminal, env_steps_at_start) per environment: episode lengths (5, None, 12) over 12 steps
SEGMENTS = [[(0, 5, True, 0), (5, 10, True, 5), (10, 12, False, 10)], [(0, 12, False, 0)], [(0, 12, True, 0)]]
STATE_SPEC = dict(state_a=(3,), state_b=(2, 2))


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _one(rewards, values_be, gamma, lambda_, scale):
    r, v = _np(rewards).astype(np.float32), _np(values_be).astype(np.float32)
    ret, ret_be = OG.compute_returns(r, gamma)
    _, adv_raw, adv = OG.compute_advantages(r, v, gamma, lambda_, scale)
    f = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32))
    return dict(returns=f(ret), returns_be=f(ret_be).reshape(-1, 2), advantages_raw=f(adv_raw), advantages=f(adv))


@pytest.fixture
def calls(monkeypatch):
    """Both utils entry points replaced by oracle stand-ins that count their calls."""
    from carla_driving_rl_agent_amd.rl import utils
    count = dict(single=0, segments=0)

    def returns_and_advantages(rewards, values_be, gamma, lambda_, scale=2.0, device='cpu'):
        count['single'] += 1
        return _one(rewards, values_be, gamma, lambda_, scale)

    def returns_and_advantages_segments(rewards, values_be, lengths, gamma, lambda_, scale=2.0, device='cpu'):
        count['segments'] += 1
        assert sum(lengths) + len(lengths) == rewards.shape[0] == values_be.shape[0]
        outs, off = [], 0
        for n in lengths:
            outs.append(_one(rewards[off:off + n + 1], values_be[off:off + n + 1], gamma, lambda_, scale))
            off += n + 1
        return {k: torch.cat([o[k] for o in outs], dim=0) for k in outs[0]}

    monkeypatch.setattr(utils, 'returns_and_advantages', returns_and_advantages)
    monkeypatch.setattr(utils, 'returns_and_advantages_segments', returns_and_advantages_segments)
    return count


def _rollout(seed):
    """Three environments stepped 12 times by hand, trajectories closed where SEGMENTS says."""
    from carla_driving_rl_agent_amd.rl.agents.ppo import Rollout
    g = torch.Generator().manual_seed(seed)
    E = len(SEGMENTS)
    rollout = Rollout(E, STEPS, 'cpu')
    stops = [{seg[1]: seg[2] for seg in segs} for segs in SEGMENTS]
    for t in range(1, STEPS + 1):
        states = {k: torch.randn((E,) + shape, generator=g) for k, shape in STATE_SPEC.items()}
        value = torch.stack([torch.rand(E, generator=g) * 2 - 1, torch.randint(0, 4, (E,), generator=g).float()], dim=1)
        rollout.record(states, torch.rand((E, 2), generator=g), torch.randn((E, 2), generator=g), value, list(range(E)))
        for e in range(E):
            rollout.rewards[e].append(float(torch.rand((), generator=g)) * 10)
            rollout.env_steps[e] += 1
            if t in stops[e]:
                assert rollout.close_segment(e, terminal=stops[e][t]) == [s for s in SEGMENTS[e] if s[1] == t][0]
    return rollout


def _last_values(rollout, seed):
    g = torch.Generator().manual_seed(seed)
    estimate = torch.stack([torch.rand(rollout.envs, generator=g), torch.randint(0, 3, (rollout.envs,), generator=g).float()], dim=1)
    return torch.cat([torch.zeros((1, 2)) if seg[2] else estimate[e:e + 1] for e, seg, _ in rollout.trajectories()], dim=0)


def _memory():
    from carla_driving_rl_agent_amd.rl.agents.ppo import PPOMemory
    return PPOMemory(state_spec=STATE_SPEC, num_actions=2, device='cpu')


def _store_one_by_one(memory, rollout, last_values, keep_open):
    """The per-trajectory loop of PPOAgent.store with the memory calls of end_episode."""
    rows = [t for _, _, t in rollout.trajectories()]
    for s, trajectory in enumerate(rows):
        memory.extend(*trajectory)
        memory.end_trajectory(last_values[s:s + 1])
        memory.compute_returns(discount=GAMMA, append=True)
        memory.compute_advantages(GAMMA, LAMBDA, scale=SCALE, append=True)
        memory.update_index(append=True)
        if keep_open or s < len(rows) - 1:
            memory.drop_bootstrap()


def _store_together(memory, rollout, last_values, keep_open, append=True):
    closed = memory.extend_trajectories([t for _, _, t in rollout.trajectories()], last_values, GAMMA, LAMBDA, SCALE, append=append)
    if keep_open:
        memory.drop_bootstrap()
    return closed


def _assert_same_memory(a, b):
    assert len(a) == len(b) and a.index == b.index
    assert a._rewards == b._rewards and len(a._values) == len(b._values)
    for k in STATE_SPEC:
        assert torch.equal(a.states[k], b.states[k]), k
    for name in ('actions', 'log_probabilities', 'rewards', 'values', 'returns', 'advantages'):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and torch.equal(x, y), name


def test_rollout_hands_out_trajectories_in_memory_order():
    rollout = _rollout(1)
    assert rollout.segments == SEGMENTS and rollout.length == [STEPS] * 3 and rollout.terminal == [False, False, True]
    got = list(rollout.trajectories())
    assert [(e, seg) for e, seg, _ in got] == [(e, seg) for e in range(3) for seg in SEGMENTS[e]]
    for e, (start, stop, _, _), (states, actions, rewards, values, log_probs) in got:
        assert rewards == rollout.rewards[e][start:stop]
        for k in STATE_SPEC:
            assert torch.equal(states[k], rollout.blocks[k][start:stop, e])
        assert torch.equal(actions, rollout.blocks['/action'][start:stop, e])
        assert torch.equal(values, rollout.blocks['/value'][start:stop, e])
        assert torch.equal(log_probs, rollout.blocks['/log_prob'][start:stop, e])
        assert actions.is_contiguous() and actions.data_ptr() != rollout.blocks['/action'][start:stop, e].data_ptr()      # a copy
    # the whole-environment view keeps working
    states, actions, rewards, values, log_probs = rollout.trajectory(0)
    assert actions.shape[0] == STEPS and len(rewards) == STEPS


@pytest.mark.parametrize('keep_open', [False, True])
def test_extend_trajectories_leaves_the_memory_of_the_per_trajectory_loop(calls, keep_open):
    rollout = _rollout(2)
    lv = _last_values(rollout, 3)
    old, new = _memory(), _memory()
    _store_one_by_one(old, rollout, lv, keep_open)
    assert calls == dict(single=10, segments=0)
    returns, values, advantages = _store_together(new, rollout, lv, keep_open)
    assert calls == dict(single=10, segments=1)                 # ONE segmented call, none of the single-trajectory ones
    _assert_same_memory(old, new)
    assert len(new) == 36 and new.index == 36 and new.rewards.shape[0] == (36 if keep_open else 37)
    # per-trajectory views, in trajectory order: what end_episode logs
    lengths = [5, 5, 2, 12, 12]
    assert [int(r.shape[0]) for r in returns] == lengths and [int(a.shape[0]) for a in advantages] == lengths
    assert [int(v.shape[0]) for v in values] == [n + 1 for n in lengths]
    off = 0
    for s, n in enumerate(lengths):
        r = torch.cat([new.rewards[off:off + n], lv[s:s + 1, 0] * torch.pow(torch.tensor(10.0), lv[s:s + 1, 1])])
        ref = _one(r, torch.cat([new.values[off:off + n], lv[s:s + 1]]), GAMMA, LAMBDA, SCALE)
        assert torch.equal(returns[s], ref['returns']) and torch.equal(advantages[s], ref['advantages_raw']), s
        off += n


def test_a_second_rollout_is_appended_behind_a_kept_open_one(calls):
    """update_frequency = 2: store(keep_open=True), then store(keep_open=False) -- drop_bootstrap keeps working afterwards."""
    first, second = _rollout(4), _rollout(5)
    lv1, lv2 = _last_values(first, 6), _last_values(second, 7)
    old, new = _memory(), _memory()
    for rollout, lv, keep_open in ((first, lv1, True), (second, lv2, False)):
        _store_one_by_one(old, rollout, lv, keep_open)
        _store_together(new, rollout, lv, keep_open)
        _assert_same_memory(old, new)
    assert len(new) == 72 and new.returns.shape == (72, 2) and new.rewards.shape[0] == 73
    assert calls['segments'] == 2


def test_without_append_an_empty_memory_ends_up_the_same(calls):
    rollout = _rollout(8)
    lv = _last_values(rollout, 9)
    old, new = _memory(), _memory()
    _store_one_by_one(old, rollout, lv, keep_open=False)
    _store_together(new, rollout, lv, keep_open=False, append=False)
    _assert_same_memory(old, new)


def test_extend_trajectories_checks_its_arguments(calls):
    rollout = _rollout(10)
    rows = [t for _, _, t in rollout.trajectories()]
    with pytest.raises(ValueError):
        _memory().extend_trajectories(rows, torch.zeros((4, 2)), GAMMA, LAMBDA, SCALE, append=True)
    with pytest.raises(ValueError):
        _memory().extend_trajectories([], torch.zeros((0, 2)), GAMMA, LAMBDA, SCALE, append=True)
    assert calls['segments'] == 0


def test_lengths_are_validated_before_any_library_call(monkeypatch):
    from carla_driving_rl_agent_amd import _lib, engine

    def load():
        raise AssertionError('the library was reached')

    monkeypatch.setattr(_lib, 'load', load)
    r, v = torch.zeros(6), torch.zeros((6, 2))
    for lengths in ([2, 3], [0, 4], [4, 0], [], [2, 2, 2]):           # bad sum, zero lengths, no segment, sum + S != 6
        with pytest.raises(ValueError):
            engine.gae_returns_segments(r, v, lengths, GAMMA, LAMBDA, SCALE)
    with pytest.raises(AssertionError, match='the library was reached'):
        engine.gae_returns_segments(r, v, [2, 2], GAMMA, LAMBDA, SCALE)   # well-formed: goes on to the library
