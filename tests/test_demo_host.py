"""Host side of the demonstration-augmented update (PPOAgent(demo_traces=...), rl/demonstrations.py): the split of a
policy minibatch, the draws, the constructor's refusals, the host state, and the float64 restatement's two limits.  No GPU."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd.rl import utils
from carla_driving_rl_agent_amd.rl.demonstrations import DemonstrationStore, demo_split, draw_rows
from carla_driving_rl_agent_amd.rl.parameters import ExponentialDecay
from tests import clone_ref, demo_ref
from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Two float64 compositions of one objective (scipy's special functions and a closed-form gradient here, torch's and autograd there):
# the special functions agree to a few 1e-14 relative, on terms -- log(eps) * (alpha - 1), (alpha - 1) / eps at a clipped action -- that
# reach 1e2 .. 1e4 times the result's scale.  1e-9 leaves room for that and stands four orders below the kernels' own 1e-5.
TOL64 = 1e-9


# ---------------------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize('rows,batch_size,fraction', [(10, 4, 0.25), (9, 4, 0.5), (256, 32, 0.25)])
def test_split_and_draws(rows, batch_size, fraction):
    D, fresh = demo_split(batch_size, fraction)
    assert (D, fresh) == demo_ref.split(batch_size, fraction) == {(4, 0.25): (1, 3), (4, 0.5): (2, 2), (32, 0.25): (8, 24)}[(batch_size, fraction)]
    store_rows = 3 * D + 1
    rng, demo_rng = np.random.default_rng(5), np.random.default_rng(6)
    for epoch in range(2):
        batches = utils.batch_indices(rows, fresh, shuffle=True, rng=rng)
        assert sorted(np.concatenate(batches).tolist()) == list(range(rows)), 'every fresh row exactly once per epoch'
        assert [len(b) for b in batches] == [fresh] * (rows // fresh) + ([rows % fresh] if rows % fresh else [])
        for b in batches:           # a remainder minibatch included
            idx = draw_rows(demo_rng, store_rows, D)
            assert idx.dtype == np.int32 and idx.shape == (D,) and len(set(idx.tolist())) == D
            assert idx.min() >= 0 and idx.max() < store_rows


@pytest.mark.parametrize('batch_size,fraction', [(4, 0.0), (4, 0.1), (4, 1.0), (4, 0.9), (2, 0.2), (8, -0.25), (8, float('nan'))])
def test_fractions_that_leave_no_row_of_a_kind_are_refused(batch_size, fraction):
    with pytest.raises(ValueError, match='demo_fraction'):
        demo_split(batch_size, fraction)
    with pytest.raises(ValueError):
        demo_ref.split(batch_size, fraction)


def _trace_tensors(n, A=2, first=0.0):
    val = torch.arange(n, dtype=torch.float32) + first
    return dict(states=dict(state_road=val[:, None].repeat(1, 3)), u=val[:, None].repeat(1, A), speed=val.clone(), similarity=-val)


def test_store_takes_traces_in_order_up_to_the_cap():
    store = DemonstrationStore([_trace_tensors(5), _trace_tensors(4, first=100.0), _trace_tensors(3, first=200.0)], cap=7, need=2)
    assert (store.rows, store.left_out, store.traces) == (7, 5, 2)
    assert store.speed.tolist() == [0, 1, 2, 3, 4, 100, 101]
    assert store.states['state_road'].shape == (7, 3) and store.u.shape == (7, 2)
    with pytest.raises(ValueError, match='holds 5 rows'):
        DemonstrationStore([_trace_tensors(5)], cap=64, need=6)


# ---------------------------------------------------------------------------------------------------------------- the agent
def _host_agent(monkeypatch, tmp_path, **kw):
    """A real CARLAgent whose learner engines are host-only (planned, never bound to a device)."""
    from carla_driving_rl_agent_amd.core import networks, CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    monkeypatch.setattr(networks, 'LearnerEngine',
                        lambda B, device=None, share_with=None, **cfg: LearnerEngine(B, device=None, share_with=share_with, **cfg))
    monkeypatch.setattr(networks, 'init_engine_parameters', lambda *a, **k: None)
    env = FakeCARLAEnvironment(image_shape=(48, 64, 3), time_horizon=4, num_waypoints=5, vehicle_features=4, num_actions=2)
    kw.setdefault('seed', 3)
    return CARLAgent(env, batch_size=8, log_mode=None, device='cpu', aug_intensity=0.0, weights_dir=str(tmp_path), **kw)


def test_defaults_leave_the_feature_off(monkeypatch, tmp_path):
    agent = _host_agent(monkeypatch, tmp_path)
    assert agent.demo_traces is None and not agent._demo_active
    assert 'demo' not in agent.host_state()
    explicit = _host_agent(monkeypatch, tmp_path, demo_traces=None, demo_fraction=0.5, demo_weight=3.0)
    assert explicit.demo_traces is None and not hasattr(explicit, 'demo_rng') and 'demo' not in explicit.host_state()
    assert json.dumps(agent.host_state(), sort_keys=True) == json.dumps(_host_agent(monkeypatch, tmp_path).host_state(), sort_keys=True)


def test_accepted_options(monkeypatch, tmp_path):
    agent = _host_agent(monkeypatch, tmp_path, demo_traces=str(tmp_path), demo_fraction=0.25, demo_weight=0.3, demo_rows=64, demo_seed=11)
    assert (agent.demo_rows_per_batch, agent.demo_fresh_rows, agent.demo_store_cap) == (2, 6, 64)
    assert agent.demo_weight() == 0.3 and agent.demo_store is None and not agent._demo_active
    agent.save_config()
    assert not any('demo' in k for k in agent.config)                   # not written to config.json
    sched = _host_agent(monkeypatch, tmp_path, demo_traces=str(tmp_path), demo_weight=ExponentialDecay(0.5, 10, 0.5))
    assert sched.demo_weight() == 0.5
    sched.on_episode_end()
    assert sched.demo_weight.step == 1 and sched.demo_weight() == pytest.approx(0.5 * 0.5 ** 0.1)


def test_constructor_refusals(monkeypatch, tmp_path):
    d = str(tmp_path)
    for kw, word in ((dict(joint_update=True), 'joint_update'), (dict(replay_rollouts=1, resample_actions=False), 'replay_rollouts'),
                     (dict(target_kl=0.01), 'target_kl'), (dict(kl_penalty=0.1), 'kl_penalty'), (dict(demo_fraction=0.01), 'demo_fraction'),
                     (dict(demo_fraction=1.0), 'demo_fraction'), (dict(demo_rows=1, demo_fraction=0.5), 'demo_rows'),
                     (dict(demo_weight=-0.1), 'demo_weight'), (dict(demo_weight=float('nan')), 'demo_weight')):
        with pytest.raises(ValueError, match=word):
            _host_agent(monkeypatch, tmp_path, demo_traces=d, **kw)
    with pytest.raises(ValueError, match='not a directory'):
        _host_agent(monkeypatch, tmp_path, demo_traces=os.path.join(d, 'missing'))
    # the same options without demo_traces stay accepted
    assert _host_agent(monkeypatch, tmp_path, joint_update=True).joint_update
    assert _host_agent(monkeypatch, tmp_path, target_kl=0.01).trust


def test_an_initialised_process_group_is_refused(monkeypatch, tmp_path):
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a: 1)
    monkeypatch.setattr(dist, 'get_rank', lambda *a: 0)
    with pytest.raises(ValueError, match='one process'):
        _host_agent(monkeypatch, tmp_path, demo_traces=str(tmp_path))


def _draw(agent):
    """One draw from every generator the agent's host state covers besides the demonstration generator, and the counters."""
    return (agent.seed, int(agent.rng.integers(2 ** 31)), float(agent._aug_rng.random()), int(np.random.randint(0, 2 ** 31 - 1)),
            random.random(), agent._sample_offset, agent._aug_calls, agent.network.action_index, agent.network.sample_seed)


def test_demonstration_draws_advance_no_other_generator(monkeypatch, tmp_path):
    agent = _host_agent(monkeypatch, tmp_path, demo_traces=str(tmp_path), demo_seed=4)
    before = json.dumps(agent.host_state(), sort_keys=True)
    torch_state = torch.get_rng_state()
    first = [draw_rows(agent.demo_rng, 40, agent.demo_rows_per_batch).tolist() for _ in range(5)]
    state = agent.host_state()
    assert state.pop('demo')['rng'] != json.loads(before)['demo']['rng']
    rest = json.loads(before)
    rest.pop('demo')
    assert json.dumps(state, sort_keys=True) == json.dumps(rest, sort_keys=True), 'every other generator and counter stands still'
    assert torch.equal(torch_state, torch.get_rng_state())
    twin = _host_agent(monkeypatch, tmp_path, demo_traces=str(tmp_path), demo_seed=4)
    assert [draw_rows(twin.demo_rng, 40, twin.demo_rows_per_batch).tolist() for _ in range(5)] == first, 'demo_seed fixes the draws'


def test_host_state_round_trip(monkeypatch, tmp_path):
    make = lambda **kw: _host_agent(monkeypatch, tmp_path, demo_traces=str(tmp_path), demo_weight=ExponentialDecay(0.5, 10, 0.5), **kw)
    agent = make(demo_seed=4)
    draw_rows(agent.demo_rng, 40, 2)
    agent.on_episode_end()
    agent.on_episode_end()
    state = json.loads(json.dumps(agent.host_state()))
    assert state['demo']['weight'] == dict(step=2)
    want = (draw_rows(agent.demo_rng, 40, 2).tolist(), agent.demo_weight(), _draw(agent))
    other = make(demo_seed=9, seed=8)
    other.set_host_state(state)
    assert (draw_rows(other.demo_rng, 40, 2).tolist(), other.demo_weight(), _draw(other)) == want
    # a state saved without the feature loads into an agent with it (one printed line), and the other way round
    plain = _host_agent(monkeypatch, tmp_path)
    make().set_host_state(json.loads(json.dumps(plain.host_state())))
    plain.set_host_state(state)


def test_base_class_has_no_mixed_pass(monkeypatch, tmp_path):
    from carla_driving_rl_agent_amd.rl.agents.ppo import PPOAgent
    agent = _host_agent(monkeypatch, tmp_path, demo_traces=str(tmp_path))
    with pytest.raises(NotImplementedError, match='CARLAgent'):
        PPOAgent.with_demonstrations(agent, ())


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _inputs(B=9, A=3, seed=0):
    rng = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)
    x = dict(lin=f(rng.standard_normal((B, 2 * A + 2)) * 1.5), adv=f(rng.standard_normal(B)), u=f(rng.beta(2, 2, (B, A))),
             du=f(rng.beta(2, 2, (B, A))), old=f(rng.standard_normal((B, A)) * 0.3), spd=f(rng.uniform(0, 0.3, B)),
             sim=f(rng.uniform(-1, 1, B)), ja=f(rng.uniform(-0.3, 0.3, (B, A))), jb=f(rng.uniform(-0.3, 0.3, (B, A))))
    x['u'][0, 0], x['u'][1, 1], x['du'][2, 0], x['du'][3, 1] = 0.0, 1.0, 0.0, 1.0
    return x


def _ref(x, w, jac, clip=0.2, ent=0.7):
    j = (x['ja'], x['jb']) if jac else (None, None)
    return demo_ref.mixed_loss(x['lin'], x['adv'], x['old'], x['spd'], x['sim'], x['u'], x['du'], w, clip, ent, *j)


@pytest.mark.parametrize('jac', [False, True])
def test_all_zero_weights_give_the_policy_objective(jac):
    """The existing float64 restatement of the policy loss (oracle.model, as tests/test_gpu_ops.py::test_policy_loss composes it)."""
    from oracle import model as OM
    x = _inputs()
    B, A = x['u'].shape
    ref = _ref(x, np.zeros(B), jac)
    tt = lambda a: torch.tensor(a, dtype=torch.float64)
    lt = torch.tensor(x['lin'], dtype=torch.float64, requires_grad=True)
    alpha, beta = OM.softplus101(lt[:, :A]), OM.softplus101(lt[:, A:2 * A])
    z = np.zeros((B, A), np.float32)
    us = OM._InjectedSample.apply(alpha, beta, tt(x['u']), tt(x['ja'] if jac else z), tt(x['jb'] if jac else z))
    logp = OM.beta_log_prob(torch.clamp(us, OM.EPSILON, 1.0 - OM.EPSILON), alpha, beta)
    ent = OM.beta_entropy(alpha, beta).mean()
    ratio = torch.exp(logp - tt(x['old'])).mean(dim=1)
    advt = tt(x['adv'])
    min_adv = torch.where(advt > 0, 1.2 * advt, 0.8 * advt)
    pl = -torch.minimum(ratio * advt, min_adv).mean()
    speed_loss = 0.5 * ((tt(x['spd']) - 2.0 * torch.sigmoid(lt[:, 2 * A + 1])) ** 2).mean()
    sim_loss = 0.5 * ((tt(x['sim']) - torch.tanh(lt[:, 2 * A])) ** 2).mean()
    total = pl - 0.7 * ent + speed_loss + sim_loss
    total.backward()
    want = [total.item(), pl.item(), ent.item(), speed_loss.item(), sim_loss.item(), ratio.mean().item(), logp.mean().item(), 0, 0, 0, 0]
    assert np.allclose(ref['metrics'], want, rtol=TOL64, atol=TOL64)
    assert rel_err(ref['dlin'], lt.grad.numpy()) < TOL64
    assert ref['passes'].any() and not ref['passes'].all()


def test_all_demonstration_rows_give_the_clone_objective():
    x = _inputs(seed=1)
    B, A = x['u'].shape
    w = np.random.default_rng(2).uniform(0.1, 2.0, B)
    nan = lambda a: np.full_like(a, np.nan)
    poisoned = dict(x, adv=nan(x['adv']), old=nan(x['old']), u=nan(x['u']), ja=nan(x['ja']), jb=nan(x['jb']))
    ref = _ref(poisoned, w, True)
    tt = lambda a: torch.tensor(a, dtype=torch.float64)
    lt = torch.tensor(x['lin'], dtype=torch.float64, requires_grad=True)
    total, out = clone_ref.clone_from_lin(lt, tt(x['du']), tt(w), tt(x['spd']), tt(x['sim']), entropy_coef=0.7, aux_weight=1.0)
    total.backward()
    slots = clone_ref.metric_slots(out)        # total, clone, entropy, speed, similarity, weight, logp, mode error
    want = [slots[0], 0.0, slots[2], slots[3], slots[4], 0.0, 0.0, slots[1], slots[6], slots[7], B]
    assert np.allclose(ref['metrics'], want, rtol=TOL64, atol=TOL64)
    assert rel_err(ref['dlin'], lt.grad.numpy()) < TOL64
    assert not ref['passes'].any() and ref['demo'].all()


@pytest.mark.parametrize('jac', [False, True])
def test_closed_form_gradient_matches_autograd_on_a_mixed_batch(jac):
    x = _inputs(B=11, seed=3)
    w = np.where(np.arange(11) % 3 == 0, 0.6, 0.0)
    ref = _ref(x, w, jac)
    lt = torch.tensor(x['lin'], dtype=torch.float64, requires_grad=True)
    j = (x['ja'], x['jb']) if jac else (None, None)
    total = demo_ref.mixed_total_torch(lt, x['adv'], x['old'], x['spd'], x['sim'], x['u'], x['du'], w, 0.2, 0.7, *j)
    total.backward()
    assert abs(float(total.detach()) - ref['total']) < TOL64 * max(1.0, abs(ref['total']))
    assert rel_err(ref['dlin'], lt.grad.numpy()) < TOL64
    assert ref['metrics'][10] == 4 and ref['metrics'][0] == ref['total']


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_library_exports_the_entries():
    from carla_driving_rl_agent_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cdrl.h')).read()
    lib = _lib.load()
    for name in ('cdrl_learner_demo_forward_backward', 'cdrl_learner_demo_forward_backward_resample', 'cdrl_learner_set_demo_block',
                 'cdrl_beta_mixed_policy_loss'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in _lib.PROTOTYPES and getattr(lib.raw, name) is not None
    assert 'cdrl_demo_stats' in header and C.sizeof(_lib.DemoStats) == 40
    from carla_driving_rl_agent_amd import engine as E
    assert E.DEMO_BLOCK_DOUBLES * 8 == C.sizeof(_lib.DemoStats) and len(E.DEMO_METRICS) == 11
