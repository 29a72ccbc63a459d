"""Optimizer choice and polyak averaging (cdrl_config.optimizer / polyak, PPOAgent(optimizer=..., polyak=...)) on the host: the
planner is optimizer-independent, bad values fail at create, shared engines and agents carry both settings to the engines, and the
numpy restatement of the optimizers (tests/optim_ref.py, which the GPU tests compare the kernels against) agrees with torch.optim
where the two are the same mathematics, and with hand-worked steps where torch has no twin.  No GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.optim_ref import OPTIMIZERS, SLOTS, F, OptState, clip_by_norm, polyak, slot_init, step  # noqa: E402


def _engine(B=8, **kw):
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    kw.setdefault('H', 48)
    kw.setdefault('W', 64)
    return LearnerEngine(B, device=None, **kw)


# ---------------------------------------------------------------------------------------------------------------- engine / C ABI
@pytest.mark.parametrize('B,kw', [(256, dict(H=90, W=120)), (16, dict(H=48, W=64, freeze_trunk=True)),
                                  (64, dict(H=36, W=108, A=3, compute='bf16'))])
def test_planner_identical_for_every_optimizer(B, kw):
    ref = _engine(B, **kw)
    assert ref.optimizer == 'adam' and ref.polyak == 1.0
    for name in OPTIMIZERS:
        for spelled in (name, name.upper()):
            e = _engine(B, optimizer=spelled, polyak=0.5, **kw)
            assert e.optimizer == name and e.polyak == 0.5
            for m in ('trunk', 'policy', 'value'):
                assert e.tables[m].entries == ref.tables[m].entries, (name, m)
            for m in ('trunk', 'policy', 'value', 'old_policy'):
                for tr in (True, False):
                    assert e.region(m, tr) == ref.region(m, tr), (name, m, tr)
            assert (e.params_total, e.grads_total, e.workspace_bytes) == (ref.params_total, ref.grads_total, ref.workspace_bytes)


@pytest.mark.parametrize('kw,match', [(dict(optimizer=8), 'unknown optimizer'), (dict(optimizer=-1), 'unknown optimizer'),
                                      (dict(optimizer='adamw'), 'unknown optimizer'), (dict(polyak=0.0), 'polyak'),
                                      (dict(polyak=1.0001), 'polyak'), (dict(polyak=-0.5), 'polyak'),
                                      (dict(polyak=float('nan')), 'polyak')])
def test_bad_optimizer_or_polyak_rejected_at_create(kw, match):
    from carla_driving_rl_agent_amd import _lib
    with pytest.raises(_lib.CdrlError, match=match):
        _engine(**kw)


def test_config_defaults():
    from carla_driving_rl_agent_amd import _lib
    cfg = _lib.Config()
    cfg.optimizer, cfg.polyak = 5, 0.25
    _lib.load().cdrl_config_default(C.byref(cfg))
    assert cfg.optimizer == 0 and cfg.polyak == 1.0


def test_slot_query_matches_the_table():
    from carla_driving_rl_agent_amd import _lib
    lib = _lib.load()
    assert _lib.OPTIMIZERS == OPTIMIZERS and _lib.OPTIMIZER_SLOTS == SLOTS
    for i, name in enumerate(OPTIMIZERS):
        used, init = (C.c_int32 * 2)(), (C.c_float * 2)()
        assert lib.cdrl_optimizer_slots(i, used, init) == 0
        assert [bool(u) for u in used] == [s is not None for s in SLOTS[name]], name
        assert tuple(init) == tuple(F(x) for x in slot_init(name)), name
        assert _engine(optimizer=name).slot_init == tuple(float(F(x)) for x in slot_init(name))
    used, init = (C.c_int32 * 2)(), (C.c_float * 2)()
    assert lib.cdrl_optimizer_slots(8, used, init) == -1


def test_shared_engines_inherit_optimizer_and_polyak():
    owner = _engine(32, optimizer='Nadam', polyak=0.9)
    shared = _engine(8, share_with=owner)
    assert shared.optimizer == 'nadam' and shared.polyak == owner.polyak == float(F(0.9))
    assert not shared.frozen
    other = _engine(8, share_with=owner, optimizer='sgd', polyak=1.0)
    assert other.optimizer == 'sgd' and other.polyak == 1.0


# ---------------------------------------------------------------------------------------------------------------- agents
def _host_agent(monkeypatch, cls='CARLAgent', **kw):
    """A real CARLAgent / CARLANetwork whose learner engines are host-only (device=None: planned, never bound)."""
    from carla_driving_rl_agent_amd.core import networks, CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    made = []

    def host_engine(B, device=None, share_with=None, **cfg):
        made.append(LearnerEngine(B, device=None, share_with=share_with, **cfg))
        return made[-1]

    monkeypatch.setattr(networks, 'LearnerEngine', host_engine)
    monkeypatch.setattr(networks, 'init_engine_parameters', lambda *a, **k: None)
    env = FakeCARLAEnvironment(image_shape=(36, 108, 3), time_horizon=4, num_waypoints=5, vehicle_features=4, num_actions=3)
    if cls == 'PPOAgent':
        from carla_driving_rl_agent_amd.rl.agents.ppo import PPOAgent
        agent = PPOAgent(env, batch_size=8, log_mode=None, seed=3, device='cpu',
                         network=dict(network=networks.CARLANetwork, control_policy=CARLAgent.DEFAULT_CONTROL,
                                      control_value=CARLAgent.DEFAULT_CONTROL_VALUE, dynamics=CARLAgent.DEFAULT_DYNAMICS), **kw)
    else:
        agent = CARLAgent(env, batch_size=8, log_mode=None, seed=3, device='cpu', aug_intensity=0.0, **kw)
    return agent, made


@pytest.mark.parametrize('cls', ['CARLAgent', 'PPOAgent'])
@pytest.mark.parametrize('name', OPTIMIZERS)
def test_agents_accept_every_optimizer(monkeypatch, cls, name):
    spelled = name.capitalize() if name != 'sgd' else 'SGD'
    agent, made = _host_agent(monkeypatch, cls, optimizer=spelled, polyak=0.99)
    assert agent.should_polyak_average and agent.polyak_coeff == 0.99
    assert made and all(e.optimizer == name and e.polyak == float(F(0.99)) for e in made)
    ragged = agent.network.engine_for(5)            # the ragged last minibatch shares the optimizer
    assert ragged.optimizer == name and ragged.polyak == float(F(0.99))


def test_agent_defaults_are_adam_without_averaging(monkeypatch):
    agent, made = _host_agent(monkeypatch)
    assert not agent.should_polyak_average
    assert all(e.optimizer == 'adam' and e.polyak == 1.0 for e in made)


@pytest.mark.parametrize('cls', ['CARLAgent', 'PPOAgent'])
def test_agents_reject_unknown_optimizer(monkeypatch, cls):
    with pytest.raises(ValueError, match='Select one of'):
        _host_agent(monkeypatch, cls, optimizer='lamb')


def test_frozen_agent_carries_optimizer(monkeypatch):
    agent, made = _host_agent(monkeypatch, optimizer='ftrl', update_dynamics=False)
    assert all(e.frozen and e.optimizer == 'ftrl' for e in made)


# ---------------------------------------------------------------------------------------------------------------- restatement
LRS = (2.0 ** -9, 3.0 * 2.0 ** -12, 2.0 ** -7, 2.0 ** -10)


def _torch_twin(name, p):
    o = torch.optim
    if name == 'sgd':
        return o.SGD([p], lr=LRS[0])
    if name == 'rmsprop':
        return o.RMSprop([p], lr=LRS[0], alpha=0.9, eps=1e-7)
    if name == 'adagrad':
        return o.Adagrad([p], lr=LRS[0], initial_accumulator_value=0.1, eps=1e-7)
    if name == 'adadelta':
        return o.Adadelta([p], lr=LRS[0], rho=0.95, eps=1e-7)
    if name == 'nadam':
        return o.NAdam([p], lr=LRS[0], betas=(0.9, 0.999), eps=1e-7, momentum_decay=0.004)
    raise KeyError(name)


# (no Adam: torch adds eps to the bias-corrected sqrt(v), Keras to sqrt(v) -- different mathematics at eps 1e-7)
@pytest.mark.parametrize('name', ['sgd', 'rmsprop', 'adagrad', 'adadelta', 'nadam'])
def test_restatement_matches_torch_optim(name):
    rng = np.random.default_rng(5)
    n = 4096
    p0 = rng.standard_normal(n) * 0.1
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = _torch_twin(name, p)
    st = OptState(name, n)
    mine = p0.copy()
    for k, lr in enumerate(LRS):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, -1, n)).astype(np.float32).astype(np.float64)
        p.grad = torch.tensor(g)
        for group in opt.param_groups:
            group['lr'] = lr
        opt.step()
        mine = step(st, mine, g, lr)
        ref = p.detach().numpy()
        err = np.abs(mine - ref).max() / np.abs(ref).max()
        # float32 scalar coefficients (TensorFlow) against torch's double ones: ~1e-8 of the parameters
        assert err < 1e-7, (name, k, err)
        upd, upd_ref = mine - p0, ref - p0
        assert np.abs(upd - upd_ref).max() / np.abs(upd_ref).max() < 1e-5, (name, k)


def test_adamax_two_steps_by_hand():
    st = OptState('adamax', 1)
    p = step(st, np.array([0.5]), np.array([0.2]), 0.125)
    # m = 0.2 * (1 - 0.9) = 0.02, v = max(0, |0.2|) = 0.2, p = 0.5 - 0.125 / (1 - 0.9) * 0.02 / (0.2 + 1e-7)
    b1 = float(F(0.9))
    m1 = 0.2 * float(F(1) - F(0.9))
    lr1 = float(F(F(0.125) / (F(1) - F(0.9))))
    p1 = 0.5 - lr1 * (m1 / (0.2 + float(F(1e-7))))
    assert abs(m1 - 0.02) < 1e-8 and abs(p1 - (0.5 - 1.25 * 0.1)) < 1e-6
    np.testing.assert_allclose(p, [p1], rtol=1e-15)
    np.testing.assert_allclose(st.m, [m1], rtol=1e-15)
    np.testing.assert_allclose(st.v, [0.2], rtol=1e-15)
    # step 2, g = -0.05 (|g| < beta2 v: v decays), lr 0.0625: m = m1 + (-0.05 - m1)(1 - 0.9), v = 0.999 * 0.2
    p = step(st, p, np.array([-0.05]), 0.0625)
    m2 = m1 + (-0.05 - m1) * float(F(1) - F(0.9))
    v2 = float(F(0.999)) * 0.2
    lr2 = float(F(F(0.0625) / (F(1) - F(np.power(F(b1), F(2))))))
    p2 = p1 - lr2 * (m2 / (v2 + float(F(1e-7))))
    assert abs(m2 - 0.013) < 1e-8 and abs(v2 - 0.1998) < 1e-8 and abs(lr2 - 0.0625 / 0.19) < 1e-6
    np.testing.assert_allclose(p, [p2], rtol=1e-15)
    np.testing.assert_allclose(st.m, [m2], rtol=1e-15)
    np.testing.assert_allclose(st.v, [v2], rtol=1e-15)
    # step 3, g = 0.5 > beta2 v: v = |g|
    step(st, p, np.array([0.5]), 0.0625)
    assert st.v[0] == 0.5


def test_ftrl_two_steps_by_hand():
    st = OptState('ftrl', 2)
    p0 = np.array([0.5, -0.25])
    # step 1, lr 0.125: n' = 0.1 + g^2; z = g - (sqrt(n') - sqrt(0.1)) / lr * p; p = -z / (sqrt(n') / lr)
    g1 = np.array([0.2, 0.0])
    p1 = step(st, p0, g1, 0.125)
    n0 = float(F(0.1))
    exp_n = [n0 + 0.04, n0]
    exp_z = [0.2 - (math.sqrt(n0 + 0.04) - math.sqrt(n0)) / 0.125 * 0.5, 0.0]       # a zero gradient leaves z at 0 ...
    exp_p = [-exp_z[0] / (math.sqrt(n0 + 0.04) / 0.125), 0.0]                        # ... and FTRL then sets the weight to 0
    np.testing.assert_allclose(st.v, exp_n, rtol=1e-15)
    np.testing.assert_allclose(st.m, exp_z, rtol=1e-14)
    np.testing.assert_allclose(p1, exp_p, rtol=1e-14)
    assert p1[1] == 0.0 and abs(exp_z[0] + 0.0317519) < 1e-7 and abs(exp_p[0] - 0.0106076) < 1e-7
    # step 2, lr 0.25
    g2 = np.array([-0.1, 0.3])
    p2 = step(st, p1, g2, 0.25)
    n2 = [exp_n[0] + 0.01, exp_n[1] + 0.09]
    z2 = [exp_z[i] + g2[i] - (math.sqrt(n2[i]) - math.sqrt(exp_n[i])) / 0.25 * exp_p[i] for i in range(2)]
    np.testing.assert_allclose(st.v, n2, rtol=1e-15)
    np.testing.assert_allclose(st.m, z2, rtol=1e-14)
    np.testing.assert_allclose(p2, [-z2[i] / (math.sqrt(n2[i]) / 0.25) for i in range(2)], rtol=1e-14)


def test_polyak_and_clip_conventions():
    a = 0.99
    new, old = np.array([1.0, -2.0], np.float32), np.array([0.5, 3.0], np.float32)
    # numpy's own evaluation in the reference (float32 arrays, Python float alpha): the float32 result of the GPU path
    ref = (F(a) * new + F(1.0 - float(F(a))) * old).astype(np.float32)
    np.testing.assert_array_equal(polyak(new, old, a, dt=np.float32), ref)
    np.testing.assert_allclose(polyak(new, old, a), a * new.astype(np.float64) + (1 - a) * old.astype(np.float64), rtol=1e-7)
    g = np.full(100, 0.5, np.float32)                        # norm 5 -> scaled to norm 1
    np.testing.assert_allclose(np.linalg.norm(clip_by_norm(g, 1.0)), 1.0, rtol=1e-7)
    np.testing.assert_array_equal(clip_by_norm(g, 10.0), g)
    np.testing.assert_array_equal(clip_by_norm(g, 0.0), g)


@pytest.mark.parametrize('name', OPTIMIZERS)
def test_float32_evaluation_stays_close(name):
    """The GPU test holds the kernels to the float32 evaluation of the restatement at 1e-6 and to the float64 one at the bounds
    below; this checks those bounds on the host for gradients of the engine's scale.  FTRL alone needs a loose one: its linear
    term subtracts two square roots of an accumulator that has barely moved (sqrt(0.1 + g^2) - sqrt(0.1) = 1.6e-6 for |g| = 1e-3,
    against a float32 spacing of 3e-8 at sqrt(0.1): 2 % of the difference) and divides it by the learning rate, so on a tensor
    whose gradient is that small the float32 result is only good to a few percent -- in TensorFlow as in the kernels."""
    rng = np.random.default_rng(9)
    n = 20000
    p = rng.standard_normal(n).astype(np.float32) * 0.05
    s64, s32 = OptState(name, n), OptState(name, n, dt=np.float32)
    p64, p32 = p.astype(np.float64), p.copy()
    for k, lr in enumerate((3e-4, 1e-3, 3e-4)):
        g = (rng.standard_normal(n) * 1e-3 * (50.0 if k == 2 else 1.0)).astype(np.float32)
        p64 = step(s64, p64, clip_by_norm(g, 1.0), lr)
        p32 = step(s32, p32, clip_by_norm(g, 1.0, dt=np.float32), lr).astype(np.float32)
        for a, b, what in ((p32, p64, 'params'), (s32.m, s64.m, 'm'), (s32.v, s64.v, 'v')):
            if not np.abs(b).max():
                continue
            err = np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()
            assert err < float64_bound(name, what), (name, k, what, err)


def float64_bound(name, what):
    """Relative bound (max |a - b| / max |b|) between the float32 kernels and the float64 restatement (see above)."""
    if name == 'ftrl':
        return 5e-2
    return 1e-6
