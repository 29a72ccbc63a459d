"""Optimizers other than Adam and polyak averaging on the GPU (cdrl_config.optimizer / polyak; include/cdrl.h table): the apply
kernels against the numpy restatement of tests/optim_ref.py on injected gradients (no forward runs), the slots each optimizer
leaves alone, the step counters and Nadam's m_cache, graph replay, and a few agent updates."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from carla_driving_rl_agent_amd import _lib
from carla_driving_rl_agent_amd.engine import LearnerEngine
from tests.optim_ref import OPTIMIZERS, SLOTS, F, OptState, clip_by_norm, polyak, slot_init, step
from tests.test_optimizers_host import float64_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W = 4, 48, 64
SENTINEL = 4321.0
SEQ = (('policy', 3e-4, 1e-3, 1.0), ('value', 1e-3, 5e-4, 1.0), ('policy', 5e-4, 2e-3, 50.0))     # (kind, head lr, trunk lr, grad scale)
_BASE = {}


def _base_params():
    if 'p' not in _BASE:
        from carla_driving_rl_agent_amd.init import init_engine_parameters
        eng = LearnerEngine(B, device='cuda:0', H=H, W=W)
        init_engine_parameters(eng, seed=8)
        _BASE['p'] = eng.params.clone()
    return _BASE['p']


def _engine(**kw):
    eng = LearnerEngine(B, device='cuda:0', H=H, W=W, **kw)
    eng.params.copy_(_base_params())
    eng.reset_optimizer()
    return eng


def _grads(eng, k, scale):
    g = torch.Generator().manual_seed(100 + k)
    x = torch.randn(eng.grads_total, generator=g) * 1e-3
    p_off, p_n = eng.region('policy', True)
    v_off, v_n = eng.region('value', True)
    x[p_off:p_off + p_n] *= scale          # scale 50: the per-tensor clip of the heads is active
    x[v_off:v_off + v_n] *= scale
    return x


def _hp(eng):
    torch.cuda.synchronize()
    raw = eng.named_buffer('hparams', dtype=torch.int32)[:16].cpu()
    return [int(x) for x in raw[10:13]], raw[13:16].view(torch.float32).tolist()


def _run(eng, seq=SEQ):
    """The apply sequence on the engine; returns the gradients it injected and the policy weights before each policy apply."""
    injected, before = [], []
    for k, (kind, lr, lr_t, scale) in enumerate(seq):
        eng.set_hparams(policy_lr=lr, value_lr=lr, dynamics_lr=lr_t)
        g = _grads(eng, k, scale)
        eng.grads.copy_(g.to(eng.grads.device))
        injected.append(g.numpy())
        if kind == 'policy':
            before.append(eng.params.clone())
            eng.policy_apply()
        else:
            eng.value_apply()
    torch.cuda.synchronize()
    return injected, before


def _segments(eng, model):
    off, _ = eng.region(model, True)
    return [(e['name'], off + e['offset'], e['numel']) for e in eng.tables[model].entries if e['trainable']]


def _restate(eng, p0, injected, opt, frozen, pk, dt):
    """Expected trainable parameters and optimizer states after SEQ (flat arrays over the arenas' trainable part)."""
    p = p0.astype(dt)
    st = {m: OptState(opt, eng.grads_total, dt) for m in ('trunk', 'policy', 'value')}
    for k, (kind, lr, lr_t, _) in enumerate(SEQ):
        g = injected[k]
        if not frozen:
            o, n = eng.region('trunk', True)
            sub = OptState(opt, n, dt)
            sub.m, sub.v, sub.t, sub.m_cache = st['trunk'].m[o:o + n], st['trunk'].v[o:o + n], st['trunk'].t, st['trunk'].m_cache
            p[o:o + n] = step(sub, p[o:o + n], g[o:o + n], lr_t)
            st['trunk'].t, st['trunk'].m_cache = sub.t, sub.m_cache
        o, n = eng.region(kind, True)
        gc = g[o:o + n].astype(dt)          # (tensors sit at aligned offsets: the padding between them is not compared)
        for _, s, c in _segments(eng, kind):
            gc[s - o:s - o + c] = clip_by_norm(g[s:s + c], 1.0, dt)
        sub = OptState(opt, n, dt)
        sub.m, sub.v, sub.t, sub.m_cache = st[kind].m[o:o + n], st[kind].v[o:o + n], st[kind].t, st[kind].m_cache
        new = step(sub, p[o:o + n], gc, lr)
        if pk < 1.0:
            new = polyak(new.astype(dt), p[o:o + n], pk, dt)
        p[o:o + n] = new
        st[kind].t, st[kind].m_cache = sub.t, sub.m_cache
    return p, st


def _check(eng, opt, frozen, pk, p0, injected, before):
    n_all = eng.grads_total
    params = eng.params.cpu().numpy()
    arenas = (eng.adam_m.cpu().numpy(), eng.adam_v.cpu().numpy())
    ref32 = _restate(eng, p0, injected, opt, frozen, pk, np.float32)
    ref64 = _restate(eng, p0, injected, opt, frozen, pk, np.float64)
    models = ('policy', 'value') if frozen else ('trunk', 'policy', 'value')
    for model in models:
        for name, s, c in _segments(eng, model):
            for ref, bound in ((ref32, 1e-6), (ref64, None)):
                p_ref, st = ref
                b = bound if bound is not None else float64_bound(opt, 'params')
                got, exp = params[s:s + c], p_ref[s:s + c]
                e = np.abs(got - exp).max() / (np.abs(exp).max() + 1e-30)
                assert e < b, (opt, frozen, pk, model, name, 'params', e)
                for arena, slot, flat in zip(arenas, SLOTS[opt], (st[model].m, st[model].v)):
                    if slot is None:
                        continue
                    b = bound if bound is not None else float64_bound(opt, slot)
                    got, exp = arena[s:s + c], flat[s:s + c]
                    e = np.abs(got - exp).max() / (np.abs(exp).max() + 1e-30)
                    assert e < b, (opt, frozen, pk, model, name, slot, e)
    for arena, slot in zip(arenas, SLOTS[opt]):
        if slot is None:
            assert (arena[:n_all] == SENTINEL).all(), (opt, 'unused slot written')
    if frozen:
        o, n = eng.region('trunk', True)
        assert np.array_equal(params[o:o + n], p0[o:o + n])
        for arena, init in zip(arenas, slot_init(opt)):
            sl = arena[o:o + n]
            assert (sl == SENTINEL).all() or (sl == F(init)).all()
    # step counters (policy 2, value 1, trunk 3 or untouched) and Nadam's m_cache = S_t of the last step
    steps, caches = _hp(eng)
    assert steps == [2, 1, 0 if frozen else 3], steps
    exp_cache = [ref32[1][m].m_cache if opt == 'nadam' else 1.0 for m in ('policy', 'value', 'trunk')]
    if frozen:
        exp_cache[2] = 1.0
    np.testing.assert_allclose(caches, exp_cache, rtol=1e-6)
    if opt != 'nadam':
        assert caches == [1.0, 1.0, 1.0]
    # the heads' non-trainable BatchNorm moving statistics are not averaged; old_policy is the pre-update policy
    for model in ('policy', 'value'):
        o, n = eng.region(model, False)
        assert np.array_equal(params[o:o + n], p0[o:o + n]), model
    po, pn = eng.region('policy', True)
    oo, on = eng.region('old_policy', True)
    assert on == pn and np.array_equal(params[oo:oo + on], before[-1].cpu().numpy()[po:po + pn])


@pytest.mark.parametrize('opt', OPTIMIZERS)
def test_apply_matches_restatement(opt):
    p0 = _base_params().cpu().numpy()
    for frozen in (False, True):
        for pk in (1.0, 0.9):
            eng = _engine(optimizer=opt, polyak=pk, freeze_trunk=frozen)
            for arena, slot in zip((eng.adam_m, eng.adam_v), SLOTS[opt]):
                if slot is None:
                    arena.fill_(SENTINEL)
            if frozen:          # a frozen trunk's slots keep whatever they hold
                o, n = eng.region('trunk', True)
                eng.adam_m[o:o + n] = SENTINEL
                eng.adam_v[o:o + n] = SENTINEL
            injected, before = _run(eng)
            _check(eng, opt, frozen, pk, p0, injected, before)
            # reset_optimizer: every slot at its initial value, counters 0, m_caches 1
            eng.reset_optimizer()
            m0, v0 = slot_init(opt)
            assert bool((eng.adam_m == F(m0)).all()) and bool((eng.adam_v == F(v0)).all())
            assert _hp(eng) == ([0, 0, 0], [1.0, 1.0, 1.0])
            slots = eng.optimizer_slots('policy')
            assert set(slots) == {s for s in SLOTS[opt] if s is not None}
            for views in slots.values():
                assert set(views) == {e['name'] for e in eng.tables['policy'].entries if e['trainable']}


def test_adam_polyak_one_is_the_default_path():
    a, b = _engine(), _engine(optimizer='ADAM', polyak=1.0)
    _run(a)
    _run(b)
    for name in ('params', 'adam_m', 'adam_v'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert _hp(a) == _hp(b)


def test_share_hparams_requires_the_same_optimizer():
    owner = _engine(optimizer='rmsprop', polyak=0.9)
    shared = LearnerEngine(2, device='cuda:0', share_with=owner, H=H, W=W)
    assert shared.optimizer == 'rmsprop' and shared.adam_v.data_ptr() == owner.adam_v.data_ptr()
    with pytest.raises(_lib.CdrlError, match='optimizer / polyak differ'):
        LearnerEngine(2, device='cuda:0', share_with=owner, H=H, W=W, optimizer='sgd')
    with pytest.raises(_lib.CdrlError, match='optimizer / polyak differ'):
        LearnerEngine(2, device='cuda:0', share_with=owner, H=H, W=W, polyak=1.0)


GRAPH_SEQ = tuple(SEQ[k % 2][:3] + (1.0 + 20.0 * (k == 4),) for k in range(7))     # policy / value alternating: 3 + 2 replays


def _graph_worker(rank, out, opt):
    sys.path.insert(0, ROOT)
    os.environ['CDRL_GRAPH'] = '1'
    torch.cuda.set_device(0)
    eng = _engine(optimizer=opt, polyak=0.9)
    assert eng.lib.cdrl_learner_tail_offset(eng.h) == eng.region('trunk', True)[1]     # graphs are on in this process
    _run(eng, GRAPH_SEQ)
    torch.save(dict(params=eng.params.cpu(), m=eng.adam_m.cpu(), v=eng.adam_v.cpu(), hp=_hp(eng)), os.path.join(out, f'{opt}.pt'))


@pytest.mark.parametrize('opt', ['nadam', 'adagrad'])
def test_graph_replay_is_bit_identical(tmp_path, opt):
    mp.spawn(_graph_worker, args=(str(tmp_path), opt), nprocs=1, join=True)
    g = torch.load(tmp_path / f'{opt}.pt')
    eng = _engine(optimizer=opt, polyak=0.9)
    _run(eng, GRAPH_SEQ)
    assert torch.equal(g['params'], eng.params.cpu())
    assert torch.equal(g['m'], eng.adam_m.cpu()) and torch.equal(g['v'], eng.adam_v.cpu())
    assert g['hp'] == _hp(eng)


@pytest.mark.parametrize('kw', [dict(optimizer='rmsprop', polyak=0.9), dict(optimizer='ftrl')])
def test_agent_learns_with_optimizer(tmp_path, kw):
    from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
    env = FakeCARLAEnvironment(image_shape=(36, 108, 3), time_horizon=4, num_waypoints=5, vehicle_features=4, num_actions=3)
    agent = CARLAgent(env, batch_size=8, log_mode=None, seed=3, skip_data=0, shuffle=True, policy_lr=3e-4, value_lr=3e-4,
                      dynamics_lr=3e-4, aug_intensity=0.0, weights_dir=str(tmp_path), name='t', optimization_steps=(1, 1), **kw)
    eng = agent.network.engine
    assert eng.optimizer == kw['optimizer'] and agent.should_polyak_average == ('polyak' in kw)
    p0 = eng.params.clone()
    agent.learn(episodes=2, timesteps=21, close=False)       # 21 timesteps, minibatch 8: a ragged last minibatch
    assert np.isfinite(eng.metrics('policy')['loss']) and np.isfinite(eng.metrics('value')['loss'])
    assert torch.isfinite(eng.params).all() and torch.isfinite(eng.adam_v).all()
    for m in ('trunk', 'policy', 'value'):
        o, n = eng.region(m, True)
        assert not torch.equal(p0[o:o + n], eng.params[o:o + n]), m
    assert agent.network._ragged, 'expected a ragged last minibatch'
    for r in agent.network._ragged.values():
        assert r.optimizer == eng.optimizer and r.polyak == eng.polyak
        assert r.adam_m.data_ptr() == eng.adam_m.data_ptr() and r.adam_v.data_ptr() == eng.adam_v.data_ptr()
    steps, _ = _hp(eng)
    assert steps[0] > 0 and steps[1] > 0 and steps[2] == steps[0] + steps[1]
