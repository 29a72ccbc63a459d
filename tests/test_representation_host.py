"""Host side of the representation stage (CARLAgent.learn_representation): the signature, every refusal that is
decided before anything touches a GPU, the view plans and the views without augmentation."""
import inspect

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
from carla_driving_rl_agent_amd.rl.agents.ppo import PPOAgent


def _stub(**kw):
    """A CARLAgent that was never constructed: exactly the attributes the host-side checks read."""
    env = FakeCARLAEnvironment(image_shape=(4, 6, 3), time_horizon=2, num_waypoints=5, vehicle_features=4, num_actions=2)
    agent = object.__new__(CARLAgent)
    agent.env, agent.num_actions, agent.data_parallel, agent.polyak_coeff = env, 2, False, 1.0
    agent.state_spec = dict(state_image=(4, 6, 3), state_road=(9,), state_vehicle=(4,), state_navigation=(5,))
    agent.should_update_dynamics, agent.clip_mode, agent.skip_nonfinite, agent.batch_size = True, 'tensor', False, 8
    agent.rng = np.random.default_rng(0)
    agent._augmenter, agent.device = None, 'cpu'
    agent.__dict__.update(kw)
    return agent


def test_signature():
    want = [('epochs', 1), ('batch_size', None), ('traces_dir', None), ('temperature', 0.1), ('intensity', 1.0), ('vector_inputs', 'zero'),
            ('lr', None), ('shuffle_data', True), ('max_traces', None), ('seed', None), ('close', False)]
    for cls in (CARLAgent, PPOAgent):
        params = list(inspect.signature(cls.learn_representation).parameters.values())[1:]
        assert [(p.name, p.default) for p in params] == want, cls
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params[:2])
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[2:])


def test_refusals_come_before_any_upload(tmp_path):
    d = str(tmp_path)
    with pytest.raises(RuntimeError, match='one GPU'):
        _stub(data_parallel=True).learn_representation(traces_dir=d)
    with pytest.raises(ValueError, match='update_dynamics=False'):
        _stub(should_update_dynamics=False).learn_representation(traces_dir=d)
    with pytest.raises(ValueError, match='gradient gate'):
        _stub(clip_mode='global').learn_representation(traces_dir=d)
    with pytest.raises(ValueError, match='gradient gate'):
        _stub(skip_nonfinite=True).learn_representation(traces_dir=d)
    with pytest.raises(ValueError, match='even'):
        _stub().learn_representation(batch_size=7, traces_dir=d)
    with pytest.raises(ValueError, match='even'):
        _stub(batch_size=5).learn_representation(traces_dir=d)
    with pytest.raises(ValueError, match='vector_inputs'):
        _stub().learn_representation(traces_dir=d, vector_inputs='drop')
    with pytest.raises(ValueError, match='temperature'):
        _stub().learn_representation(traces_dir=d, temperature=0.0)
    with pytest.raises(ValueError, match='traces_dir'):
        _stub().learn_representation()
    agent = _stub()
    state = agent.rng.bit_generator.state
    with pytest.raises(ValueError, match='traces_dir'):
        agent.learn_representation(batch_size=8)
    assert agent.rng.bit_generator.state == state, 'a refused call draws nothing'


def test_the_stage_style_call_reaches_the_hook(monkeypatch):
    """Stage.representation_learning does agent.learn_representation(**repr_args): the keywords bind and the method runs up to
    its first need of data (here: no traces directory anywhere); the base class's hook says who implements it."""
    with pytest.raises(ValueError, match='traces_dir'):
        _stub().learn_representation(**dict(epochs=1, traces_dir=None))
    with pytest.raises(NotImplementedError, match='CARLAgent'):
        PPOAgent.learn_representation(_stub(), **dict(epochs=1, traces_dir='x'))
    seen = {}

    def reached(self, d):
        seen.update(traces_dir=d)
        raise KeyError('reached')

    monkeypatch.setattr(CARLAgent, '_traces_dir', reached)
    with pytest.raises(KeyError, match='reached'):
        _stub().learn_representation(**dict(epochs=1, traces_dir='somewhere'))
    assert seen == dict(traces_dir='somewhere')


def _plan_key(plan):
    return tuple((k, tuple(v) if isinstance(v, list) else v) for k, v in sorted(plan.items()))


def test_view_plans_are_a_pure_function_of_the_seed():
    agent = _stub()
    draw = lambda seed: [_plan_key(p) for p in agent.representation_plans(1.0, np.random.default_rng(seed), 8, 1)]
    a, b, c = draw(5), draw(5), draw(6)
    assert a == b and a != c and len(a) == 8
    assert [dict(p)['offset'] for p in a] == list(range(1, 9))
    assert len(set(dict(p)['seed'] for p in a)) == 8, 'every view gets its own plan'
    assert agent.representation_plans(0.0, np.random.default_rng(5), 8, 1) == []


def test_without_plans_both_views_are_the_input():
    agent = _stub()
    rng = np.random.default_rng(1)
    rows = {k: torch.as_tensor(rng.random((4, 2) + shape, dtype=np.float32)) for k, shape in agent.state_spec.items()}
    keep = agent.representation_views(rows, [], 'keep')
    zero = agent.representation_views(rows, agent.representation_plans(0.0, rng, 8, 1), 'zero')
    for k, v in rows.items():
        assert keep[k].shape[0] == 8 and torch.equal(keep[k][:4], v) and torch.equal(keep[k][4:], v), k
    assert torch.equal(zero['state_image'], keep['state_image'])
    for k in ('state_road', 'state_vehicle', 'state_navigation'):
        assert zero[k].shape == keep[k].shape and not zero[k].any(), k
    with pytest.raises(ValueError, match='vector_inputs'):
        agent.representation_views(rows, [], 'drop')
