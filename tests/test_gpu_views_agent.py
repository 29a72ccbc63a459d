"""CARLAgent(view_pipeline=...) through learn_representation, on the small traces of
tests/test_gpu_representation.py: FakeCARLAEnvironment at 48x64, time_horizon 4, a trace of 19 rows, batch_size 8 = two views of 4."""
import copy
import json

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import traces
from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment

pytestmark = pytest.mark.gpu
T, A, BATCH = 4, 2, 8
ARENAS = ('params', 'adam_m', 'adam_v')
IDENTITY = dict(crop_scale=(1.0, 1.0), jitter_prob=0, drop_prob=0, blur_prob=0)


def _env(seed=0):
    return FakeCARLAEnvironment(image_shape=(48, 64, 3), time_horizon=T, num_waypoints=5, vehicle_features=4, num_actions=A, seed=seed,
                                image_range=(0.0, 1.0))


def _agent(tmp_path, **kw):
    cfg = dict(batch_size=BATCH, log_mode=None, seed=3, skip_data=0, drop_batch_remainder=False, shuffle=True, policy_lr=3e-4,
               value_lr=3e-4, dynamics_lr=3e-4, aug_intensity=0.0, weights_dir=str(tmp_path), name='t', optimization_steps=(1, 1),
               entropy_regularization=0.01)
    cfg.update(kw)
    return CARLAgent(_env(), **cfg)


@pytest.fixture(scope='module')
def traces_dir(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('view_traces'))
    env = _env(11)
    obs, frames, rewards = env.reset(), [], []
    for _ in range(19):
        frames.append(obs)
        obs, reward, _, _ = env.step(np.zeros(A, np.float32))
        rewards.append(reward)
    newest = {k: np.stack([f[k] for f in frames])[:, -1] for k in frames[0]}
    traces.write_trace(path, 1, newest, np.zeros((19, A), np.float32), rewards, np.zeros(19, np.float32), None)
    return path


def _slice(eng, model, trainable=True):
    o, n = eng.region(model, trainable)
    return slice(o, o + n)


def _host_equal(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_host_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_host_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def _count_view_calls(monkeypatch, agent):
    """Counts the library's cdrl_views_batch calls made through the agent's augmenter (created here if need be)."""
    from carla_driving_rl_agent_amd.rl.augmentations import Augmenter
    if agent._augmenter is None:
        agent._augmenter = Augmenter(agent.device)
    calls = []
    real = agent._augmenter.lib.cdrl_views_batch

    class Lib:
        def __getattr__(self, name):
            return getattr(real_lib, name)

        def cdrl_views_batch(self, *a):
            calls.append(a[3])                  # V
            return real(*a)

    real_lib = agent._augmenter.lib
    monkeypatch.setattr(agent._augmenter, 'lib', Lib())
    return calls


def test_simclr_epoch_trains_the_trunk_alone(tmp_path, monkeypatch, traces_dir):
    agent = _agent(tmp_path, view_pipeline='simclr')
    assert agent.view_pipeline == 'simclr' and agent.view_options == {}
    assert 'view_pipeline' not in json.dumps(agent.config)
    calls = _count_view_calls(monkeypatch, agent)
    eng = agent.network.engine
    before = {n: getattr(eng, n).clone() for n in ARENAS}
    host0 = copy.deepcopy(agent.host_state())
    agent.learn_representation(traces_dir=traces_dir)
    torch.cuda.synchronize()
    assert calls == [BATCH] * 4, 'one library call per minibatch: 19 rows -> 4 minibatches of 4 rows x 2 views'
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
    assert differing == ['rng'], differing                  # sampler offset, augmentation generator and counter keep their bits
    assert torch.isfinite(eng.params).all()


def test_same_seed_same_trunk_and_not_the_agent_pipelines(tmp_path, monkeypatch, traces_dir):
    a, b = _agent(tmp_path, view_pipeline='simclr'), _agent(tmp_path, name='b', view_pipeline='simclr')
    old = _agent(tmp_path, name='old')
    assert old.view_pipeline == 'agent'
    calls = _count_view_calls(monkeypatch, old)
    for agent in (a, b, old):
        agent.learn_representation(traces_dir=traces_dir, intensity=1.0)
    torch.cuda.synchronize()
    assert calls == [], 'the default agent never reaches cdrl_views_batch'
    for name in ARENAS:
        assert torch.equal(getattr(a.network.engine, name), getattr(b.network.engine, name)), name
    e, o = a.network.engine, old.network.engine
    assert not torch.equal(e.params[_slice(e, 'trunk')], o.params[_slice(o, 'trunk')])


def test_identity_options_make_both_views_the_input(tmp_path, monkeypatch, traces_dir):
    monkeypatch.chdir(tmp_path)
    agent = _agent(tmp_path, log_mode='summary', view_pipeline=IDENTITY)
    assert agent.view_pipeline == 'simclr' and agent.view_options == IDENTITY
    seen = []
    views = CARLAgent.representation_views

    def spy(self, rows, plans, vector_inputs='zero'):
        out = views(self, rows, plans, vector_inputs)
        seen.append((isinstance(plans, np.ndarray), torch.equal(out['state_image'], torch.cat([rows['state_image']] * 2))))
        return out

    monkeypatch.setattr(CARLAgent, 'representation_views', spy)
    agent.learn_representation(traces_dir=traces_dir)
    assert seen == [(True, True)] * 4
    lines = [l for l in (json.loads(s) for s in open(tmp_path / 'logs' / 't' / 'summary.jsonl')) if l['key'] == 'representation_similarity_pos']
    (line,) = lines
    assert line['n'] == 4 and abs(line['mean'] - 1.0) <= 1e-5, line
