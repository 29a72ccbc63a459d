"""Contrastive pre-training of the trunk, agent level (CARLAgent.learn_representation): FakeCARLAEnvironment at
48x64, time_horizon 4; a trace of 19 rows (written without the time_horizon axis, so it goes through the windowing gather) and one
of 3 rows; batch_size 8 = two views of 4 rows: 19 rows give floor(19 / 4) = 4 full minibatches, the 3-row trace gives none."""
import copy
import json

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import traces
from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T, A, BATCH = 4, 2, 8
ARENAS = ('params', 'adam_m', 'adam_v')
LOG_KEYS = ('representation_loss', 'representation_accuracy', 'representation_similarity_pos', 'representation_similarity_neg',
            'representation_embedding_norm')


def _env(seed=0):
    return FakeCARLAEnvironment(image_shape=(48, 64, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=A, seed=seed)


def _agent(tmp_path, **kw):
    cfg = dict(batch_size=BATCH, log_mode=None, seed=3, skip_data=0, drop_batch_remainder=False, shuffle=True, policy_lr=3e-4,
               value_lr=3e-4, dynamics_lr=3e-4, aug_intensity=0.0, weights_dir=str(tmp_path), name='t', optimization_steps=(1, 1),
               entropy_regularization=0.01)
    cfg.update(kw)
    return CARLAgent(_env(), **cfg)


def _record(path, episode, rows, seed):
    env = _env(seed)
    obs, frames, rewards = env.reset(), [], []
    for _ in range(rows):
        frames.append(obs)
        obs, reward, _, _ = env.step(np.zeros(A, np.float32))
        rewards.append(reward)
    newest = {k: np.stack([f[k] for f in frames])[:, -1] for k in frames[0]}          # (rows, ...): no time axis on disk
    return traces.write_trace(path, episode, newest, np.zeros((rows, A), np.float32), rewards, np.zeros(rows, np.float32), None)


@pytest.fixture(scope='module')
def traces_dir(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('traces'))
    _record(path, 1, 19, seed=11)
    _record(path, 2, 3, seed=12)
    return path


def _slice(eng, model, trainable=True):
    o, n = eng.region(model, trainable)
    return slice(o, o + n)


def _steps(eng):
    torch.cuda.synchronize()
    return [int(x) for x in eng.named_buffer('hparams', dtype=torch.int32)[10:13].cpu()]


def _host_equal(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_host_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_host_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def _lines(tmp_path, key):
    return [l for l in (json.loads(s) for s in open(tmp_path / 'logs' / 't' / 'summary.jsonl')) if l['key'] == key]


def test_one_epoch_trains_the_trunk_alone(tmp_path, monkeypatch, traces_dir, capsys):
    monkeypatch.chdir(tmp_path)                                          # Summary writes under ./logs/<name>
    agent = _agent(tmp_path, log_mode='summary', aug_intensity=1.0)
    eng = agent.network.engine
    before = {n: getattr(eng, n).clone() for n in ARENAS}
    steps0 = _steps(eng)
    host0 = copy.deepcopy(agent.host_state())
    agent.learn_representation(traces_dir=traces_dir)
    out = capsys.readouterr().out
    assert out.count('skipped') == 1 and '3 rows' in out
    assert _steps(eng) == [steps0[0], steps0[1], steps0[2] + 4]           # 19 rows -> 4 minibatches of 4 rows (x 2 views)
    for key in LOG_KEYS:
        (line,) = _lines(tmp_path, key)
        assert line['n'] == 4 and np.isfinite(line['mean']), key
    assert not torch.equal(before['params'][_slice(eng, 'trunk')], eng.params[_slice(eng, 'trunk')])
    for model in ('policy', 'value', 'old_policy'):
        for trainable in (True, False):
            sl = _slice(eng, model, trainable)
            assert torch.equal(before['params'][sl], eng.params[sl]), (model, trainable)
    for model in ('policy', 'value'):
        for name in ('adam_m', 'adam_v'):
            assert torch.equal(before[name][_slice(eng, model)], getattr(eng, name)[_slice(eng, model)]), (model, name)
    host1 = agent.host_state()
    differing = sorted(k for k in host0 if not _host_equal(host0[k], host1[k]))
    assert differing == ['rng'], differing
    assert torch.isfinite(eng.params).all()


def test_same_seed_same_result_and_vector_inputs_matter(tmp_path, traces_dir):
    a, b, keep = _agent(tmp_path), _agent(tmp_path, name='b'), _agent(tmp_path, name='keep')
    a.learn_representation(traces_dir=traces_dir, intensity=1.0)
    b.learn_representation(traces_dir=traces_dir, intensity=1.0)
    keep.learn_representation(traces_dir=traces_dir, intensity=1.0, vector_inputs='keep')
    torch.cuda.synchronize()
    for name in ARENAS:
        assert torch.equal(getattr(a.network.engine, name), getattr(b.network.engine, name)), name
    e, k = a.network.engine, keep.network.engine
    assert not torch.equal(e.params[_slice(e, 'trunk')], k.params[_slice(k, 'trunk')])
    with pytest.raises(ValueError, match='vector_inputs'):
        a.learn_representation(traces_dir=traces_dir, vector_inputs='drop')


def test_lr_comes_back_after_the_run_and_after_an_error(tmp_path, monkeypatch, traces_dir):
    agent = _agent(tmp_path)
    eng = agent.network.engine
    want = agent.hyper_parameters()
    seen = {}
    step = type(eng).repr_step

    def spy(self, states, temperature=0.1):
        seen.update(self.hp)
        return step(self, states, temperature)

    monkeypatch.setattr(type(eng), 'repr_step', spy)
    agent.learn_representation(traces_dir=traces_dir, lr=5e-3)
    assert seen['dynamics_lr'] == 5e-3 and seen['policy_lr'] == want['policy_lr']
    assert want['dynamics_lr'] == 3e-4 and {k: eng.hp[k] for k in want} == want

    def boom(self, states, temperature=0.1):
        raise RuntimeError('stop here')

    monkeypatch.setattr(type(eng), 'repr_step', boom)
    with pytest.raises(RuntimeError, match='stop here'):
        agent.learn_representation(traces_dir=traces_dir, lr=5e-3)
    assert {k: eng.hp[k] for k in want} == want


def test_learn_then_learn_representation_then_learn(tmp_path, traces_dir):
    agent = _agent(tmp_path)
    agent.learn(episodes=1, timesteps=19, close=False)
    agent.learn_representation(epochs=2, traces_dir=traces_dir, temperature=0.2)
    agent.learn(episodes=1, timesteps=19, close=False)
    assert torch.isfinite(agent.network.engine.params).all()
