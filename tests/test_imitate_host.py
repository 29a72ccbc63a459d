"""Host side of imitation learning (traces.py; PPOAgent.imitate / CARLAgent.imitation_learning): the windowing index, the action
conversion, the trace files, and every refusal that is decided before anything touches a GPU."""
import inspect
import os

import numpy as np
import pytest

from carla_driving_rl_agent_amd import traces
from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
from carla_driving_rl_agent_amd.rl.agents.ppo import PPOAgent


# ------------------------------------------------------------------------------------------------ window_index
def test_window_index_known_answers():
    idx = traces.window_index(8, 4).reshape(8, 4)
    assert idx.dtype == np.int32
    assert idx[0].tolist() == [0, 0, 0, 0]
    assert idx[1].tolist() == [0, 0, 0, 1]
    assert idx[5].tolist() == [2, 3, 4, 5]
    assert idx[7].tolist() == [4, 5, 6, 7]
    assert traces.window_index(6, 1).tolist() == list(range(6))
    assert traces.window_index(0, 3).shape == (0,)
    assert traces.window_index(2, 5).reshape(2, 5).tolist() == [[0] * 5, [0, 0, 0, 0, 1]]     # a trace shorter than the window
    assert int(traces.window_index(19, 4).max()) == 18                                       # never reaches past the trace
    with pytest.raises(ValueError):
        traces.window_index(3, 0)


# ------------------------------------------------------------------------------------------------ unit_actions
def test_unit_actions():
    a = np.array([[-1.0, 1.0], [0.0, 0.5], [-3.0, 7.0]], np.float32)
    u = traces.unit_actions(a, -1.0, 1.0)
    assert u.dtype == np.float32
    assert u.tolist() == [[0.0, 1.0], [0.5, 0.75], [0.0, 1.0]]           # at the bounds, inside, outside (clipped)
    low, high = np.array([0.0, -2.0], np.float32), np.array([10.0, 2.0], np.float32)
    u = traces.unit_actions(np.array([[2.5, -1.0], [10.0, 2.0], [11.0, -2.0]], np.float32), low, high)
    assert u.tolist() == [[0.25, 0.25], [1.0, 1.0], [1.0, 0.0]]           # per-action ranges
    with pytest.raises(ValueError):
        traces.unit_actions(a, 1.0, 1.0)


# ------------------------------------------------------------------------------------------------ files
def _write(tmp_path, episode, n=5, seed=0, info=True, T=None):
    rng = np.random.default_rng(seed)
    lead = (n,) if T is None else (n, T)
    states = dict(image=rng.uniform(-1, 1, lead + (4, 6, 3)).astype(np.float32), road=rng.uniform(0, 1, lead + (9,)).astype(np.float32))
    actions = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    rewards = rng.uniform(0, 1, n).astype(np.float32)
    done = np.zeros(n, np.float32)
    done[-1] = 1.0
    inf = dict(speed=rng.uniform(0, 30, n), similarity=rng.uniform(-1, 1, n)) if info else None
    path = traces.write_trace(str(tmp_path), episode, states, actions, rewards, done, inf)
    return path, states, actions, rewards, done, inf


def test_write_load_unpack_round_trip(tmp_path):
    path, states, actions, rewards, done, info = _write(tmp_path, 3, n=5, T=2)
    name = os.path.basename(path)
    assert name.startswith('trace-3-') and name.endswith('.npz')
    assert traces.trace_files(str(tmp_path), sort=True) == [name]
    (trace,) = list(traces.load_traces(str(tmp_path)))
    assert sorted(trace) == ['action', 'done', 'info_similarity', 'info_speed', 'reward', 'state_image', 'state_road']
    assert trace['action'].shape == (5, 2) and trace['reward'].shape == (6,) and trace['done'].shape == (5,)
    assert trace['info_speed'].shape == (5, 1) and trace['info_similarity'].shape == (5, 1)
    assert trace['reward'][-1] == 0.0 and np.array_equal(trace['reward'][:-1], rewards)
    assert np.array_equal(trace['info_speed'][:, 0], info['speed'].astype(np.float32))
    state, action, reward, d = traces.unpack_trace(trace)
    assert sorted(state) == ['state_image', 'state_road']
    assert np.array_equal(state['state_image'], states['image']) and np.array_equal(state['state_road'], states['road'])
    assert np.array_equal(action, actions) and reward.dtype == np.float32 and np.array_equal(d, done)
    packed = traces.unpack_trace(trace, unpack=False)
    assert sorted(packed) == ['action', 'done', 'info_similarity', 'info_speed', 'reward', 'state']
    # a second trace of the same episode within the same second keeps its own file
    other = _write(tmp_path, 3, seed=1)[0]
    assert other != path and len(traces.trace_files(str(tmp_path))) == 2
    # files that are not traces are not listed
    open(os.path.join(str(tmp_path), 'notes.npz'), 'w').close()
    open(os.path.join(str(tmp_path), 'trace-9.txt'), 'w').close()
    assert len(traces.trace_files(str(tmp_path))) == 2


def test_trace_without_done_or_info(tmp_path):
    np.savez_compressed(os.path.join(str(tmp_path), 'trace-1-x.npz'), state=np.zeros((3, 2), np.float32), action=np.zeros((3, 1), np.float32),
                        reward=np.zeros(4, np.float32))
    (trace,) = list(traces.load_traces(str(tmp_path)))
    state, action, reward, done = traces.unpack_trace(trace)
    assert state.shape == (3, 2) and action.shape == (3, 1) and done is None


def test_load_order_is_the_generator_s(tmp_path):
    for ep in range(6):
        _write(tmp_path, ep, n=2, seed=ep)
    names = traces.trace_files(str(tmp_path))
    first = lambda **kw: [float(t['action'][0, 0]) for t in traces.load_traces(str(tmp_path), **kw)]
    plain = first()
    assert len(plain) == 6
    a = first(shuffle=True, rng=np.random.default_rng(5))
    b = first(shuffle=True, rng=np.random.default_rng(5))
    c = first(shuffle=True, rng=np.random.default_rng(6))
    assert a == b and sorted(a) == sorted(plain) and a != plain and a != c
    want = [plain[i] for i in np.random.default_rng(5).permutation(len(names))]
    assert a == want
    assert first(max_amount=4, offset=1) == plain[1:4]
    with pytest.raises(ValueError):
        list(traces.load_traces(str(tmp_path), offset=-1))


# ------------------------------------------------------------------------------------------------ refusals, no GPU
def _stub(**kw):
    """A CARLAgent that was never constructed: exactly the attributes the host-side checks read."""
    env = FakeCARLAEnvironment(image_shape=(4, 6, 3), time_horizon=2, num_waypoints=5, vehicle_features=4, num_actions=2)
    agent = object.__new__(CARLAgent)
    agent.env, agent.num_actions, agent.data_parallel, agent.polyak_coeff = env, 2, False, 1.0
    agent.state_spec = dict(state_image=(4, 6, 3), state_road=(9,), state_vehicle=(4,), state_navigation=(5,))
    agent.__dict__.update(kw)
    return agent


def _trace(n=3, A=2, T=None, info=True, drop=()):
    lead = (n,) if T is None else (n, T)
    t = dict(state_image=np.zeros(lead + (4, 6, 3), np.float32), state_road=np.zeros(lead + (9,), np.float32),
             state_vehicle=np.zeros(lead + (4,), np.float32), state_navigation=np.zeros(lead + (5,), np.float32),
             action=np.zeros((n, A), np.float32), reward=np.zeros(n + 1, np.float32), done=np.zeros(n, np.float32))
    if info:
        t.update(info_speed=np.zeros((n, 1), np.float32), info_similarity=np.zeros((n, 1), np.float32))
    for k in drop:
        t.pop(k)
    return t


def test_imitate_without_a_traces_directory():
    with pytest.raises(ValueError, match='traces_dir'):
        _stub().imitate(close=False)
    with pytest.raises(ValueError, match='traces_dir'):
        _stub().collect_traces(1, 4)


def test_imitate_under_data_parallelism_is_refused(tmp_path):
    with pytest.raises(RuntimeError, match='one GPU'):
        _stub(data_parallel=True).imitate(traces_dir=str(tmp_path), close=False)


def test_traces_that_do_not_fit_the_agent():
    agent = _stub()
    assert agent._check_trace(_trace(), True, 0.5) == 3
    assert agent._check_trace(_trace(T=2), True, 0.5) == 3
    assert agent._check_trace(_trace(info=False), False, 0.0) == 3
    with pytest.raises(ValueError, match='width 3'):
        agent._check_trace(_trace(A=3), False, 0.0)
    with pytest.raises(ValueError, match='state_road'):
        agent._check_trace(_trace(drop=('state_road',)), False, 0.0)
    with pytest.raises(ValueError, match='time_horizon'):
        agent._check_trace(_trace(T=3), False, 0.0)
    for vw, aw in ((0.5, 0.0), (0.0, 1.0)):
        with pytest.raises(ValueError, match='value_weight=0 and aux_weight=0'):
            agent._check_trace(_trace(info=False), vw > 0 or aw > 0, vw)
    bad = _trace()
    bad['reward'] = bad['reward'][:-1]
    with pytest.raises(ValueError, match='reward'):
        agent._check_trace(bad, True, 0.5)


# ------------------------------------------------------------------------------------------------ signatures and the keyword mapping
def test_signatures():
    params = list(inspect.signature(PPOAgent.imitate).parameters.values())[1:]
    assert [(p.name, p.default) for p in params[:6]] == [('epochs', 1), ('batch_size', None), ('shuffle_batches', False),
                                                        ('shuffle_data', False), ('close', True), ('seed', None)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[6:])
    assert {p.name: p.default for p in params[6:]} == dict(traces_dir=None, policy_weight=1.0, value_weight=0.0, aux_weight=1.0, lr=None,
                                                          clip_norm=None, weights=None, max_traces=None)
    params = list(inspect.signature(CARLAgent.imitation_learning).parameters.values())[1:]
    assert [(p.name, p.default) for p in params[:-1]] == [('alpha', 0.5), ('beta', 0.5), ('clip_grad', 1.0), ('lr', 1e-3), ('polyak', None),
                                                         ('epochs', 1), ('shuffle_data', True), ('traces_dir', None)]
    assert params[-1].kind is inspect.Parameter.VAR_KEYWORD
    params = list(inspect.signature(PPOAgent.collect_traces).parameters.values())[1:]
    assert [(p.name, p.default) for p in params[2:]] == [('envs', None), ('record_threshold', 0.0), ('seeds', None), ('deterministic', False),
                                                        ('traces_dir', None), ('close', False)]


def test_imitation_learning_maps_its_keywords(monkeypatch):
    seen = {}
    monkeypatch.setattr(CARLAgent, 'imitate', lambda self, **kw: seen.update(kw) or 'done')
    agent = _stub()
    assert agent.imitation_learning(alpha=0.3, beta=0.2, clip_grad=0.7, lr=2e-3, epochs=4, shuffle_data=False, traces_dir='x',
                                    batch_size=16, close=False) == 'done'
    assert seen == dict(epochs=4, shuffle_data=False, traces_dir='x', policy_weight=0.3, value_weight=0.2, clip_norm=0.7, lr=2e-3,
                        batch_size=16, close=False)
    seen.clear()
    agent.imitation_learning(polyak=1.0)
    assert seen == dict(epochs=1, shuffle_data=True, traces_dir=None, policy_weight=0.5, value_weight=0.5, clip_norm=1.0, lr=1e-3)
    with pytest.raises(ValueError, match='polyak'):
        agent.imitation_learning(polyak=0.9)


def test_record_is_untouched():
    with pytest.raises(NotImplementedError):
        _stub().record(1)
