"""Full learner state on the GPU: an engine (and an agent) that imports a saved state continues bit for bit where the exporting one
went on (cdrl_learner_get / set_optimizer_state, LearnerEngine.export_state / import_state, CARLAgent(full_state=True)).  The engine
is deterministic, so every comparison is torch.equal / ==: any inequality is a bug."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib, synthetic
from carla_driving_rl_agent_amd.engine import LearnerEngine
from carla_driving_rl_agent_amd.init import init_engine_parameters

pytestmark = pytest.mark.gpu
B, T, H, W = 4, 2, 48, 64
ARENAS = ('params', 'adam_m', 'adam_v')
_CACHE = {}


def _batches(rows=B, count=4):
    """`count` fixed synthetic (policy, value) minibatches of `rows` rows, stored actions (no re-sampling)."""
    key = (rows, count)
    if key not in _CACHE:
        out = []
        for k in range(count):
            r = synthetic.make_rollout(rows, T=T, H=H, W=W, seed=70 + k)
            states = {n: torch.as_tensor(v).cuda() for n, v in r['states'].items()}
            speed = (torch.as_tensor(r['speed'][:, 0]) / 100.0).cuda().contiguous()
            sim = torch.as_tensor(r['similarity'][:, 0]).cuda().contiguous()
            adv = torch.as_tensor(np.random.default_rng(k).standard_normal(rows).astype(np.float32)).cuda()
            pol = dict(states=states, advantages=adv, old_log_prob=torch.as_tensor(r['old_log_prob']).cuda(), speed=speed,
                       similarity=sim, u=torch.as_tensor(r['action']).cuda(), du_da=None, du_db=None)
            val = dict(states=states, returns=torch.as_tensor(r['value']).cuda().contiguous(), speed=speed, similarity=sim)
            out.append((pol, val))
        _CACHE[key] = out
    return _CACHE[key]


def _engine(seed, rows=B, **kw):
    eng = LearnerEngine(rows, device='cuda:0', T=T, H=H, W=W, **kw)
    init_engine_parameters(eng, seed=seed)
    eng.reset_optimizer()
    return eng


def _steps(eng, batches):
    """One policy step and one value step per minibatch; the loss scalars of every pass."""
    losses = []
    for pol, val in batches:
        eng.policy_step(pol)
        losses.append(eng.metrics('policy')['loss'])
        eng.value_step(val)
        losses.append(eng.metrics('value')['loss'])
    return losses


def _snapshot(eng):
    opt = eng.get_optimizer_state()
    return {n: getattr(eng, n).clone() for n in ARENAS}, opt


def _assert_same(a, b):
    (arenas_a, opt_a), (arenas_b, opt_b) = a, b
    for n in ARENAS:
        assert torch.equal(arenas_a[n].view(torch.int32), arenas_b[n].view(torch.int32)), n
    assert opt_a == opt_b


@pytest.mark.parametrize('kw', [dict(optimizer='adam'), dict(optimizer='nadam'), dict(optimizer='adagrad'),
                                dict(optimizer='adam', polyak=0.9)], ids=['adam', 'nadam', 'adagrad', 'adam-polyak0.9'])
def test_engine_resumes_bit_for_bit(kw):
    batches = _batches()
    a = _engine(8, **kw)
    _steps(a, batches[:2])
    state = a.export_state()
    assert state['optimizer']['t_policy'] == 2 and state['optimizer']['t_value'] == 2 and state['optimizer']['t_dynamics'] == 4
    assert state['params'].dtype == np.float32 and state['params'].shape == (a.params_total,)
    assert state['adam_m'].shape == state['adam_v'].shape == (a.grads_total,)
    if kw['optimizer'] == 'nadam':
        assert all(0.0 < state['optimizer'][k] < 1.0 for k in ('m_cache_policy', 'm_cache_value', 'm_cache_dynamics'))
    else:
        assert all(state['optimizer'][k] == 1.0 for k in ('m_cache_policy', 'm_cache_value', 'm_cache_dynamics'))
    if kw['optimizer'] == 'adagrad':
        assert a.slot_init[1] == pytest.approx(0.1) and float(state['adam_v'].min()) >= np.float32(0.1)
    later_a = _steps(a, batches[2:])

    b = _engine(9, **kw)                             # other weights, fresh optimizer: everything comes from the state
    assert not torch.equal(a.params, b.params)
    b.import_state(json_round_trip(state))
    later_b = _steps(b, batches[2:])
    assert later_a == later_b
    _assert_same(_snapshot(a), _snapshot(b))
    assert b.get_optimizer_state()['t_policy'] == 4


def json_round_trip(state):
    """The state as it comes back from the container: arrays as they are, the rest through JSON."""
    out = {k: v for k, v in state.items() if k in ARENAS}
    out['manifest'] = json.loads(json.dumps(state['manifest']))
    # (the m_caches travel as float32 in the container: float32 -> Python float -> float32 is exact)
    out['optimizer'] = {k: (int(v) if k.startswith('t_') else float(np.float32(v))) for k, v in state['optimizer'].items()}
    return out


def test_the_step_counters_matter():
    """Negative control: arenas restored, counters reset -- what load() without the full state amounts to -- is another run."""
    batches = _batches()
    a = _engine(8)
    _steps(a, batches[:2])
    state = a.export_state()
    b = _engine(9)
    b.import_state(state)
    _assert_same(_snapshot(a), _snapshot(b))
    b.lib.cdrl_learner_reset_optimizer_steps(b.h, b._stream())
    for eng in (a, b):
        eng.policy_step(batches[2][0])
    opt_a, opt_b = a.get_optimizer_state(), b.get_optimizer_state()
    assert (opt_a['t_policy'], opt_b['t_policy']) == (3, 1)
    assert (opt_a['t_dynamics'], opt_b['t_dynamics']) == (5, 1)
    off, n = a.region('policy', True)
    assert not torch.equal(a.params[off:off + n], b.params[off:off + n])       # Adam's bias correction started over


def test_validation_writes_nothing():
    batches = _batches()
    eng = _engine(8, optimizer='nadam')
    _steps(eng, batches[:1])
    before = _snapshot(eng)
    good = eng.get_optimizer_state()
    for bad in (dict(t_policy=-1), dict(t_dynamics=-7), dict(m_cache_value=float('nan')), dict(m_cache_policy=0.0),
                dict(m_cache_dynamics=float('inf')), dict(m_cache_value=-0.5)):
        st = _lib.OptimizerState(**dict(good, **bad))
        assert eng.lib.cdrl_learner_set_optimizer_state(eng.h, C.byref(st), eng._stream()) == -1
        assert next(iter(bad)) in eng.lib.cdrl_last_error().decode()
        with pytest.raises(_lib.CdrlError):
            eng.set_optimizer_state(**dict(good, **bad))
        _assert_same(before, _snapshot(eng))
    # a state whose tables differ: refused before anything is written
    other = _engine(9, optimizer='nadam')
    _steps(other, batches[1:3])
    state = other.export_state()
    state['manifest'] = json.loads(json.dumps(state['manifest']))
    entry = state['manifest']['tables']['policy'][1]
    entry[1] = [d + 1 for d in entry[1]]
    with pytest.raises(_lib.CdrlError, match=entry[0].replace('.', r'\.')):
        eng.import_state(state)
    _assert_same(before, _snapshot(eng))
    state = other.export_state()
    state['manifest']['optimizer'] = 'adam'
    with pytest.raises(_lib.CdrlError, match='optimizer'):
        eng.import_state(state)
    state = other.export_state()
    state['adam_v'] = state['adam_v'][:-1]
    with pytest.raises(_lib.CdrlError, match='adam_v'):
        eng.import_state(state)
    state = other.export_state()
    state['optimizer']['t_value'] = -3            # (arenas fine, scalars not: the arenas must not have been written)
    with pytest.raises(_lib.CdrlError, match='t_value'):
        eng.import_state(state)
    _assert_same(before, _snapshot(eng))
    # set_optimizer_state leaves the hyper-parameter floats in front of the counters alone
    hp_before = eng.named_buffer('hparams', dtype=torch.int32)[:10].clone()
    eng.set_optimizer_state(**dict(good, t_policy=40, m_cache_policy=0.25))
    assert torch.equal(hp_before, eng.named_buffer('hparams', dtype=torch.int32)[:10])
    assert eng.get_optimizer_state() == dict(good, t_policy=40, m_cache_policy=0.25)


def test_state_moves_to_another_batch_size_and_through_a_shared_engine():
    batches = _batches()
    a = _engine(8)
    _steps(a, batches[:2])
    state = a.export_state()
    wide = _engine(9, rows=8)
    wide.import_state(state)
    _assert_same(_snapshot(a), _snapshot(wide))
    _steps(wide, _batches(rows=8, count=1))          # ... and it steps on from there
    assert wide.get_optimizer_state()['t_policy'] == 3
    # an engine over the owner's arenas (a ragged last minibatch) reads and writes the owner's block
    ragged = LearnerEngine(3, device='cuda:0', share_with=a, T=T, H=H, W=W)
    assert ragged.get_optimizer_state() == a.get_optimizer_state()
    ragged.set_optimizer_state(**dict(a.get_optimizer_state(), t_value=11, m_cache_value=0.5))
    assert a.get_optimizer_state()['t_value'] == 11 and a.get_optimizer_state()['m_cache_value'] == 0.5
    fresh = _engine(10)
    shared = LearnerEngine(3, device='cuda:0', share_with=fresh, T=T, H=H, W=W)
    shared.import_state(state)                       # delegated to the owner
    _assert_same(_snapshot(fresh), (dict(zip(ARENAS, (torch.as_tensor(state[n]).cuda() for n in ARENAS))), state['optimizer']))
    assert shared.export_state()['optimizer'] == state['optimizer']


def test_frozen_trunk_state():
    batches = _batches()
    frozen = _engine(8, freeze_trunk=True)
    _steps(frozen, batches[:2])
    state = frozen.export_state()
    assert (state['optimizer']['t_policy'], state['optimizer']['t_value'], state['optimizer']['t_dynamics']) == (2, 2, 0)
    off, n = frozen.region('trunk', True)

    def trunk_slots_untouched(eng):
        return all(bool((getattr(eng, name)[off:off + n] == init).all()) for name, init in zip(('adam_m', 'adam_v'), eng.slot_init))
    assert trunk_slots_untouched(frozen)
    assert bool((frozen.adam_v[:off] != 0).any())                        # (the policy head's slots did move)
    free = _engine(9)
    free.import_state(state)
    _assert_same(_snapshot(frozen), _snapshot(free))
    assert trunk_slots_untouched(free)
    back = _engine(10, freeze_trunk=True)
    back.import_state(free.export_state())
    _assert_same(_snapshot(frozen), _snapshot(back))
    assert _steps(frozen, batches[2:3]) == _steps(back, batches[2:3])
    _assert_same(_snapshot(frozen), _snapshot(back))
    assert trunk_slots_untouched(back) and back.get_optimizer_state()['t_dynamics'] == 0


# ------------------------------------------------------------------------------------------------ agent
def _env(episode):
    from carla_driving_rl_agent_amd.core import FakeCARLAEnvironment

    class EpisodeSeededEnv(FakeCARLAEnvironment):
        """Deterministic per episode: reset() re-seeds from an episode counter, whatever seed the agent hands over."""

        def __init__(self, episode):
            super().__init__(image_shape=(H, W, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=2,
                             image_range=(0.0, 1.0))
            self.episode = episode

        def seed(self, seed=None):
            pass

        def reset(self):
            self._rng = np.random.default_rng(1000 + self.episode)
            self.episode += 1
            return super().reset()

    return EpisodeSeededEnv(episode)


def _agent(env, path, **kw):
    from carla_driving_rl_agent_amd.core import CARLAgent
    return CARLAgent(env, batch_size=4, log_mode=None, aug_intensity=1.0, resample_actions=True, weights_dir=str(path), name='t', **kw)


def _agent_fingerprint(agent):
    net = agent.network
    torch.cuda.synchronize()
    obs = synthetic.make_rollout(1, T=T, H=H, W=W, seed=5)['states']
    counters = (net.action_index, agent._sample_offset, agent._aug_calls)
    pred = [t.clone() for t in net.predict({k: torch.as_tensor(v).cuda() for k, v in obs.items()})]
    return _snapshot(net.engine), counters, pred


def test_agent_resumes_bit_for_bit(tmp_path):
    p = _agent(_env(1), tmp_path / 'p', seed=3, full_state=True)
    p.learn(episodes=3, timesteps=8, close=False)
    want = _agent_fingerprint(p)

    q = _agent(_env(1), tmp_path / 'q', seed=3, full_state=True)
    q.learn(episodes=2, timesteps=8, save_every=2, close=False)
    saved = sorted(os.listdir(tmp_path / 'q' / 't'))
    assert 'learner_state.json' in saved and 'learner_state.index' in saved and not [f for f in saved if '.rank' in f or '.tmp' in f]
    del q

    resumed = _agent(_env(3), tmp_path / 'q', seed=11, full_state=True, load=True)
    assert resumed.seed == 3 and resumed._sample_offset == 4 and resumed.network.engine.get_optimizer_state()['t_policy'] == 4
    resumed.learn(episodes=1, timesteps=8, close=False)
    got = _agent_fingerprint(resumed)
    _assert_same(want[0], got[0])
    assert want[1] == got[1]
    assert len(want[2]) == 5
    for a, b in zip(want[2], got[2]):
        assert torch.equal(a, b)

    # the same continuation from the weight checkpoints alone is another run (the comparison above is not vacuous)
    plain = _agent(_env(3), tmp_path / 'q', seed=11, load=True)
    assert plain.full_state is False and plain.network.engine.get_optimizer_state()['t_policy'] == 0
    plain.learn(episodes=1, timesteps=8, close=False)
    assert not torch.equal(want[0][0]['params'], plain.network.engine.params)

    # explicit calls work whatever the keyword says
    plain.save_state()
    again = _agent(_env(3), tmp_path / 'q', seed=12)
    again.load_state()
    _assert_same(_snapshot(plain.network.engine), _snapshot(again.network.engine))
    assert again._sample_offset == plain._sample_offset and again.network.action_index == plain.network.action_index


def test_save_in_the_middle_of_an_update_period_says_what_it_leaves_out(tmp_path, capsys):
    agent = _agent(_env(1), tmp_path, seed=3, full_state=True, update_frequency=2)
    agent.learn(episodes=2, timesteps=8, save_every=1, close=False)
    lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith('[save_state]')]
    assert len(lines) == 1 and '8 rollout rows' in lines[0]          # the save behind episode 1; the one behind the update is silent
