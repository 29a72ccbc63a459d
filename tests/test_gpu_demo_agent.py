"""Expert demonstrations inside the PPO update on the GPU, agent level (CARLAgent(demo_traces=...)):
FakeCARLAEnvironment at 48x64, time_horizon 4, two actions, minibatches of 8 rows; 48 demonstration rows in four traces written by
collect_traces.  Rollouts of 19 rows: with D = 2 the fresh rows go 6 + 6 + 6 + a remainder of 1, which trains as a minibatch of 3."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib, traces
from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
from carla_driving_rl_agent_amd.rl.parameters import ExponentialDecay

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T, A, BATCH, ROWS = 4, 2, 8, 19
KEYS = ('state_image', 'state_road', 'state_vehicle', 'state_navigation')
ARENAS = ('params', 'adam_m', 'adam_v')
LOG_KEYS = ('loss_demo', 'demo_log_prob', 'demo_mode_error', 'demo_rows_per_batch', 'demo_weight')


class EpisodeSeededEnv(FakeCARLAEnvironment):
    """Deterministic per episode: reset() re-seeds from an episode counter, whatever seed the agent hands over."""

    def __init__(self, episode=1):
        super().__init__(image_shape=(48, 64, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=A)
        self.episode = episode

    def seed(self, seed=None):
        pass

    def reset(self):
        self._rng = np.random.default_rng(1000 + self.episode)
        self.episode += 1
        return super().reset()


def _agent(tmp_path, env=None, **kw):
    cfg = dict(batch_size=BATCH, log_mode=None, seed=3, skip_data=0, drop_batch_remainder=False, shuffle=True, policy_lr=3e-4,
               value_lr=3e-4, dynamics_lr=3e-4, aug_intensity=0.0, weights_dir=str(tmp_path), name='t', optimization_steps=(1, 1),
               entropy_regularization=0.01)
    cfg.update(kw)
    return CARLAgent(env if env is not None else EpisodeSeededEnv(), **cfg)


@pytest.fixture(scope='module')
def demo_dir(tmp_path_factory):
    """Four traces of 12 rows, written by collect_traces from two environments over two episodes."""
    root = tmp_path_factory.mktemp('demo')
    out = str(root / 'traces')
    agent = _agent(root / 'w', name='collector')
    paths = agent.collect_traces(episodes=2, timesteps=12, envs=[EpisodeSeededEnv(21), EpisodeSeededEnv(41)], traces_dir=out)
    assert len(paths) == 4
    return out


def _snapshot(agent):
    torch.cuda.synchronize()
    eng = agent.network.engine
    steps = [int(x) for x in eng.named_buffer('hparams', dtype=torch.int32)[10:13].cpu()]
    return {n: getattr(eng, n).clone() for n in ARENAS}, (steps, agent._sample_offset, agent.network.action_index)


def _same(a, b):
    for n in ARENAS:
        assert torch.equal(a[0][n], b[0][n]), n
    assert a[1] == b[1]


@pytest.mark.parametrize('resample', [True, False])
def test_defaults_and_an_explicit_none_train_the_same_bits(tmp_path, resample):
    plain = _agent(tmp_path / 'a', resample_actions=resample)
    explicit = _agent(tmp_path / 'b', resample_actions=resample, demo_traces=None, demo_fraction=0.5, demo_weight=2.0, demo_rows=7,
                      demo_seed=1)
    for agent in (plain, explicit):
        agent.learn(episodes=2, timesteps=ROWS, close=False)
        assert getattr(agent.network.engine, '_demo_block', None) is None and agent._demo_active is False
    _same(_snapshot(plain), _snapshot(explicit))
    assert _snapshot(plain)[1][0][0] == 2 * 3          # two update()s of 8 + 8 + 3 rows


def _rollout(agent):
    agent.memory = agent.get_memory()
    agent.reset()
    rollout = agent.collect([agent.env], ROWS)
    agent.store(rollout, ROWS, keep_open=False)


def _store_by_hand(agent, demo_dir):
    parts = [agent._trace_tensors(t, None, True, 0.0) for t in traces.load_traces(demo_dir)]
    cat = lambda f: torch.cat([f(p) for p in parts], dim=0)
    return dict(states={k: cat(lambda p: p['states'][k]) for k in KEYS}, u=cat(lambda p: p['u']), speed=cat(lambda p: p['speed']),
                similarity=cat(lambda p: p['similarity']))


def _hand_update(twin, demo_dir, fraction, weight, demo_rng):
    """update() with demonstrations, written out on an agent that has none."""
    D = int(round(fraction * BATCH))
    store = _store_by_hand(twin, demo_dir)
    N = int(store['u'].shape[0])
    twin.network.set_hparams(**twin.hyper_parameters())
    value_batches = list(twin.get_value_batches())
    policy_batches = list(twin._batches(twin.policy_batch_tensors(), twin.shuffle, twin.shuffle_batches, BATCH - D))
    sizes = []
    for states, adv, actions, logp, speed, sim in policy_batches:
        n = int(adv.shape[0])
        idx = torch.as_tensor(demo_rng.choice(N, size=D, replace=False), device=DEV)
        z = lambda *s: torch.zeros(s, device=DEV)
        b = dict(states={k: torch.cat([states[k], store['states'][k][idx]]) for k in KEYS}, advantages=torch.cat([adv, z(D)]),
                 old_log_prob=torch.cat([logp, z(D, A)]), u=torch.cat([actions, store['u'][idx]]),
                 speed=torch.cat([speed, store['speed'][idx]]), similarity=torch.cat([sim, store['similarity'][idx]]),
                 demo_u=torch.cat([z(n, A), store['u'][idx]]), demo_w=torch.cat([z(n), torch.full((D,), weight, device=DEV)]))
        eng = twin.network.engine_for(n + D)
        b = eng.stage(b, 'demo')
        if twin.resample_actions:
            twin._sample_offset += 1
            eng.demo_forward_backward_resample(b, seed=twin.seed, offset=twin._sample_offset)
        else:
            eng.demo_forward_backward(b)
        eng.policy_apply()
        sizes.append(n + D)
    for batch in value_batches:
        twin.apply_value_gradients(twin.get_value_gradients(batch)[1])
    twin._reset_info()
    return sizes


@pytest.mark.parametrize('resample', [True, False])
def test_update_is_the_hand_written_loop(tmp_path, demo_dir, resample):
    kw = dict(resample_actions=resample)
    agent = _agent(tmp_path / 'a', demo_traces=demo_dir, demo_fraction=0.25, demo_weight=0.3, demo_seed=17, **kw)
    twin = _agent(tmp_path / 'b', **kw)
    assert (agent.demo_rows_per_batch, agent.demo_fresh_rows) == (2, 6)
    demo_rng = np.random.default_rng(17)
    for _ in range(2):
        for x in (agent, twin):
            _rollout(x)
        agent.update()
        assert _hand_update(twin, demo_dir, 0.25, 0.3, demo_rng) == [8, 8, 8, 3]
        for x in (agent, twin):
            x.memory.delete()
        _same(_snapshot(agent), _snapshot(twin))
    assert agent.demo_store.rows == 48 and agent.demo_store.left_out == 0
    assert _snapshot(agent)[1][0] == [8, 6, 14]        # per update() 4 policy steps and 3 value steps: the value loop saw the 19 fresh rows alone


def test_store_cap_and_a_store_that_is_too_small(tmp_path, demo_dir, capsys):
    agent = _agent(tmp_path / 'a', demo_traces=demo_dir, demo_rows=30)
    store = agent.load_demonstrations()
    assert (store.rows, store.left_out, store.traces) == (30, 18, 3)
    assert '18 rows left out' in capsys.readouterr().out
    first = next(iter(traces.load_traces(demo_dir)))
    want = traces.unit_actions(first['action'], agent.action_low, agent.action_high)
    assert np.array_equal(store.u[:12].cpu().numpy(), want), 'sorted file order'
    one = str(tmp_path / 'one')
    traces.write_trace(one, 1, {k: first[k][:1] for k in first if k.startswith('state_')}, first['action'][:1], first['reward'][:1],
                       first['done'][:1], dict(speed=first['info_speed'][:1], similarity=first['info_similarity'][:1]))
    small = _agent(tmp_path / 'b', demo_traces=one, demo_fraction=0.5)
    with pytest.raises(ValueError, match='holds 1 rows'):
        small.load_demonstrations()


def _store_log_prob(agent, demo_dir):
    """Mean log-probability of the store's expert actions under the agent's policy: train-mode forwards in chunks of the batch
    size, then cdrl_beta_clone_loss on the linear head outputs, forward quantities only (metrics[6])."""
    store = _store_by_hand(agent, demo_dir)
    eng = agent.network.engine
    total, chunks = 0.0, 0
    for lo in range(0, int(store['u'].shape[0]), BATCH):
        rows = slice(lo, lo + BATCH)
        eng.policy_forward({k: v[rows].contiguous() for k, v in store['states'].items()})
        lin = eng.buffer(_lib.BUF_LIN_P, (BATCH, 2 * A + 2))
        u = store['u'][rows].contiguous()
        dlin, metrics = torch.empty_like(lin), torch.zeros(16, device=DEV)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(eng.lib.cdrl_beta_clone_loss(_lib.ptr(lin), _lib.ptr(u), None, None, None, 0.0, 0.0, BATCH, A, 1.0, _lib.ptr(dlin),
                                                _lib.ptr(metrics), None, stream))
        total += float(metrics[6])
        chunks += 1
    return total / chunks


def test_demonstrations_raise_the_store_log_probability(tmp_path, demo_dir):
    """Both agents start from the same parameters and see the same kind of rollouts; only the first trains on the store.  Asserted:
    the ordering of the two final values, nothing about their size."""
    kw = dict(resample_actions=False, policy_lr=1e-3, dynamics_lr=1e-3)
    with_demo = _agent(tmp_path / 'a', demo_traces=demo_dir, demo_fraction=0.5, demo_weight=1.0, demo_seed=5, **kw)
    without = _agent(tmp_path / 'b', **kw)
    start = _store_log_prob(_agent(tmp_path / 'c', **kw), demo_dir)
    for agent in (with_demo, without):
        agent.learn(episodes=5, timesteps=ROWS, close=False)
    got, ref = _store_log_prob(with_demo, demo_dir), _store_log_prob(without, demo_dir)
    print(f'[demo agent] store log-probability: start {start:.4f}, with demonstrations {got:.4f}, without {ref:.4f}')
    assert np.isfinite([start, got, ref]).all()
    assert got > ref


def _lines(tmp_path, key):
    return [l for l in (json.loads(s) for s in open(tmp_path / 'logs' / 't' / 'summary.jsonl')) if l['key'] == key]


def test_log_keys_appear_once_per_update(tmp_path, monkeypatch, demo_dir):
    monkeypatch.chdir(tmp_path)                                          # Summary writes under ./logs/<name>
    agent = _agent(tmp_path, log_mode='summary', demo_traces=demo_dir, demo_weight=0.3)
    agent.learn(episodes=2, timesteps=ROWS, close=False)
    for key in LOG_KEYS:
        lines = _lines(tmp_path, key)
        assert len(lines) == 2 and all(l['n'] == 1 for l in lines), key
    assert all(l['mean'] == 2.0 for l in _lines(tmp_path, 'demo_rows_per_batch'))
    assert all(l['mean'] == pytest.approx(0.3) for l in _lines(tmp_path, 'demo_weight'))
    assert all(l['mean'] > 0.0 for l in _lines(tmp_path, 'demo_mode_error'))
    # a constant weight: the demonstration term of every pass is -weight times the rows' mean log-probability (either sign), and so
    # are the per-pass means of the two (each pass's two values are rounded to float32 once)
    for loss, logp in zip(_lines(tmp_path, 'loss_demo'), _lines(tmp_path, 'demo_log_prob')):
        assert np.isfinite(loss['mean']) and loss['mean'] == pytest.approx(-0.3 * logp['mean'], rel=1e-5, abs=1e-6)
    assert _lines(tmp_path, 'ratio')[0]['n'] == 4                        # the train-stats rows of the four mixed steps are logged as before


def test_save_state_in_the_middle_continues_bit_for_bit(tmp_path, demo_dir):
    make = lambda path, env, **kw: _agent(tmp_path / path, env=env, demo_traces=demo_dir, demo_weight=ExponentialDecay(0.8, 2, 0.5), **kw)
    p = make('p', EpisodeSeededEnv(1), demo_seed=4)
    p.learn(episodes=3, timesteps=ROWS, close=False)
    q = make('q', EpisodeSeededEnv(1), demo_seed=4)
    q.learn(episodes=2, timesteps=ROWS, close=False)
    q.save_state()
    meta = json.load(open(tmp_path / 'q' / 't' / 'learner_state.json'))
    assert meta['agent']['demo']['weight'] == dict(step=2)
    del q
    r = make('q', EpisodeSeededEnv(3), demo_seed=99, seed=11)
    r.load_state()
    assert r.demo_weight.step == 2 and r.demo_store is None              # the store is reloaded from the directory
    r.learn(episodes=1, timesteps=ROWS, close=False)
    _same(_snapshot(p), _snapshot(r))
    assert r.demo_rng.bit_generator.state == p.demo_rng.bit_generator.state
    # a state saved without the feature has no entry of it
    plain = _agent(tmp_path / 'plain')
    plain.save_state()
    assert 'demo' not in json.load(open(tmp_path / 'plain' / 't' / 'learner_state.json'))['agent']
