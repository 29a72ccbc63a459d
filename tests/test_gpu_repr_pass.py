"""Representation pass and trunk-only apply on the GPU (cdrl_learner_repr_forward_backward / cdrl_learner_trunk_apply,
include/cdrl.h): train-mode trunk forward, NT-Xent on the trunk's output, trunk backward, then the trunk's optimizer
step alone.  Gradients against the float64 restatement (tests/ntxent_ref.py) on the oracle model at the project's whole-pass
tolerance of 1e-4 (tests/util.check3, the engine's discrete decisions pinned); the apply against tests/optim_ref.py stepped with
the engine's own gradients; bit-level identities against the policy pass and between runs."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from carla_driving_rl_agent_amd import _lib
from carla_driving_rl_agent_amd.engine import LearnerEngine
from tests import ntxent_ref
from tests.optim_ref import SLOTS, OptState, step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
B, H, W, A = 32, 48, 64, 2
SENTINEL = 777.0
ARENAS = ('params', 'adam_m', 'adam_v')
TOL = 1e-4
TEMP = 0.2


def _host_states(batch=B, seed=21):
    """Two views of batch / 2 observations: the rows stacked twice, the second copy's images darkened and perturbed."""
    from tests.util import make_batches
    pol, _ = make_batches(batch // 2, H, W, seed=seed, A=A)
    rng = np.random.default_rng(seed + 3)
    out = {}
    for k, v in pol['states'].items():
        second = v.copy()
        if k == 'state_image':
            second = np.clip(0.8 * second + 0.1 * rng.random(second.shape, dtype=np.float32), 0.0, 1.0).astype(np.float32)
        out[k] = np.ascontiguousarray(np.concatenate([v, second], axis=0))
    return out


def _states(batch=B, seed=21):
    return {k: torch.as_tensor(v).to(DEV).contiguous() for k, v in _host_states(batch, seed).items()}


def _engines(n, batch=B, kinds=None, seed=4, **kw):
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    kinds = kinds or [{}] * n
    engs = [LearnerEngine(batch, device=DEV, H=H, W=W, **kw, **k) for k in kinds]
    init_engine_parameters(engs[0], seed=seed)
    for e in engs[1:]:
        for name in ARENAS:
            getattr(e, name).copy_(getattr(engs[0], name))
    return engs


def _slice(eng, model, trainable=True):
    o, n = eng.region(model, trainable)
    return slice(o, o + n)


def _hp(eng):
    torch.cuda.synchronize()
    raw = eng.named_buffer('hparams', dtype=torch.int32)[:16].cpu()
    return [int(x) for x in raw[10:13]], raw[13:16].view(torch.float32).tolist()      # (policy, value, dynamics)


def test_forward_is_the_policy_pass_forward_and_no_head_is_touched():
    r, h, p = _engines(3)
    st = _states()
    for e in (r, h):
        e.grads.zero_()
        for m in ('policy', 'value'):
            e.grads[_slice(e, m)] = SENTINEL
        for which in (_lib.BUF_METRICS_P, _lib.BUF_METRICS_V, _lib.BUF_LIN_P, _lib.BUF_LIN_V, _lib.BUF_AUX_P, _lib.BUF_AUX_V):
            e.buffer(which).fill_(SENTINEL)
    r.repr_forward_backward(st, TEMP)
    h.repr_forward_backward(st, TEMP, grad_scale=0.5)
    p.policy_forward(st)
    torch.cuda.synchronize()
    assert torch.equal(r.buffer(_lib.BUF_DYNAMICS), p.buffer(_lib.BUF_DYNAMICS))
    t = _slice(r, 'trunk', False)
    assert torch.equal(r.params[t], p.params[t]), 'trunk moving statistics'
    for m in ('policy', 'value'):
        assert bool((r.grads[_slice(r, m)] == SENTINEL).all()), m
    for which in (_lib.BUF_METRICS_P, _lib.BUF_METRICS_V, _lib.BUF_LIN_P, _lib.BUF_LIN_V, _lib.BUF_AUX_P, _lib.BUF_AUX_V):
        assert bool((r.buffer(which) == SENTINEL).all()), which
    one, half = r.grads[_slice(r, 'trunk')], h.grads[_slice(h, 'trunk')]
    assert float(one.abs().max()) > 0.0
    torch.testing.assert_close(half, 0.5 * one, rtol=1e-6, atol=0.0)
    assert torch.equal(r.buffer(_lib.BUF_METRICS_R), h.buffer(_lib.BUF_METRICS_R)), 'metrics stay unscaled'
    m = r.metrics('representation')
    assert m['temperature'] == np.float32(TEMP) and 0.0 <= m['accuracy'] <= 1.0 and m['loss'] > 0.0 and m['embedding_norm'] > 0.0
    # the head's moving statistics of both heads did not move either: the same bits as before the pass
    fresh, = _engines(1)
    for model in ('policy', 'value'):
        assert torch.equal(r.params[_slice(r, model, False)], fresh.params[_slice(fresh, model, False)]), model


def test_gradients_match_the_float64_restatement():
    """Trunk gradients of one representation pass against ntxent_ref on the float64 oracle model evaluated on the engine's own
    ReLU6 / max-pool decisions; per tensor, check3 at 1e-4 relative to the tensor's scale (floored at 1e-3 of the largest gradient,
    as tests/test_gpu_clone_pass.py does).  dyn.fc.b and dyn.bn.beta are compared too: no head BatchNorm follows the trunk's output
    in this pass, so their gradients are not analytically zero here (small, though: they are compared at the floor)."""
    from oracle import model as OM
    from tests.util import check3, engine_decisions, is_zero_gradient, make_pair
    oracle, eng = make_pair(B, H, W, seed=3, A=A, with64=True)
    hs = _host_states(seed=3)
    eng.repr_forward_backward({k: torch.as_tensor(v).to(DEV) for k, v in hs.items()}, TEMP)
    torch.cuda.synchronize()
    OM.DEC.items = engine_decisions(eng, oracle.cfg)
    try:
        OM.DEC.start('replay')
        _, g64, slots64, _ = ntxent_ref.repr_grads(oracle.o64, hs, TEMP)
        assert OM.DEC.cursor == len(OM.DEC.items)
        OM.DEC.start('replay')
        _, g32, _, _ = ntxent_ref.repr_grads(oracle, hs, TEMP)
    finally:
        OM.DEC.start('off')
    m = eng.buffer(_lib.BUF_METRICS_R).cpu().numpy()
    for k in (0, 2, 3, 4):
        print(f'[repr pass] metrics[{k}] {float(m[k]):.6f} (float64 {slots64[k]:.6f})')
        assert abs(float(m[k]) - slots64[k]) < TOL * max(1.0, abs(slots64[k])), (k, float(m[k]), slots64[k])
    views = eng.grad_views('trunk')
    gmax = max(float(g.abs().max()) for g in g64.values())
    assert gmax > 0.0
    worst, noise = (0.0, 0.0, ''), 0.0
    for name, g in g64.items():
        if is_zero_gradient(name) and name not in ('dyn.fc.b', 'dyn.bn.beta'):
            continue
        err, bound = check3(views[name].cpu().numpy(), g32[name].detach().numpy(), g.detach().numpy(), tol=TOL, floor=1e-3 * gmax)
        scale = max(float(g.abs().max()), 1e-3 * gmax)
        noise = max(noise, float((g32[name].detach().double() - g.detach()).abs().max()) / scale)
        if err >= worst[0]:
            worst = (err, bound, name)
        assert err <= bound, (name, err, bound)
    print(f'[repr pass] trunk: worst gradient error {worst[0]:.3e} on {worst[2]} (bound {worst[1]:.3e}); '
          f"the float32 oracle's own worst error {noise:.3e}")


def _segments(eng, model):
    off, _ = eng.region(model, True)
    return [(e['name'], off + e['offset'], e['numel']) for e in eng.tables[model].entries if e['trainable']]


@pytest.mark.parametrize('opt', ['adam', 'nadam', 'sgd'])
def test_trunk_apply_matches_restatement_and_leaves_the_heads(opt):
    from tests.test_optimizers_host import float64_bound
    eng, = _engines(1, optimizer=opt)
    eng.reset_optimizer()
    for arena, slot in zip((eng.adam_m, eng.adam_v), SLOTS[opt]):
        if slot is None:
            arena.fill_(SENTINEL)
    eng.set_hparams(dynamics_lr=1e-3)
    st = _states()
    p0 = eng.params.clone()
    m0, v0 = eng.adam_m.clone(), eng.adam_v.clone()
    steps0, caches0 = _hp(eng)
    o, n = eng.region('trunk', True)
    ref = {dt: (p0[o:o + n].cpu().numpy().astype(dt), OptState(opt, n, dt)) for dt in (np.float32, np.float64)}
    for _ in range(3):
        eng.repr_forward_backward(st, TEMP)
        g = eng.grads[o:o + n].cpu().numpy()
        eng.trunk_apply()
        for dt in ref:
            p, state = ref[dt]
            ref[dt] = (step(state, p, g, 1e-3), state)
    steps, caches = _hp(eng)
    assert steps == [steps0[0], steps0[1], steps0[2] + 3], steps
    assert caches[:2] == caches0[:2]
    if opt == 'nadam':
        np.testing.assert_allclose(caches[2], ref[np.float32][1].m_cache, rtol=1e-6)
    else:
        assert caches[2] == 1.0
    params, arenas = eng.params.cpu().numpy(), (eng.adam_m.cpu().numpy(), eng.adam_v.cpu().numpy())
    assert not np.array_equal(params[o:o + n], p0[o:o + n].cpu().numpy())
    worst = 0.0
    for name, s, c in _segments(eng, 'trunk'):
        for dt, bound in ((np.float32, 1e-6), (np.float64, None)):
            p_ref, state = ref[dt]
            b = bound if bound is not None else float64_bound(opt, 'params')
            got, exp = params[s:s + c], p_ref[s - o:s - o + c]
            e = np.abs(got - exp).max() / (np.abs(exp).max() + 1e-30)
            worst = max(worst, e)
            assert e < b, (opt, name, 'params', dt, e)
            for arena, slot, flat in zip(arenas, SLOTS[opt], (state.m, state.v)):
                if slot is None:
                    continue
                b = bound if bound is not None else float64_bound(opt, slot)
                got, exp = arena[s:s + c], flat[s - o:s - o + c]
                e = np.abs(got - exp).max() / (np.abs(exp).max() + 1e-30)
                assert e < b, (opt, name, slot, dt, e)
    print(f'[trunk apply {opt}] worst relative parameter error {worst:.2e}')
    # everything outside the trunk: the same bits as before
    for model in ('policy', 'value', 'old_policy'):
        for trainable in (True, False):
            sl = _slice(eng, model, trainable)
            assert torch.equal(eng.params[sl], p0[sl]), (model, trainable)
    for model in ('policy', 'value'):
        sl = _slice(eng, model)
        assert torch.equal(eng.adam_m[sl], m0[sl]) and torch.equal(eng.adam_v[sl], v0[sl]), model
    for arena, slot in zip(arenas, SLOTS[opt]):
        if slot is None:
            assert (arena == SENTINEL).all(), 'unused slot written'


def _three_steps(opt='adam', **kw):
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    eng = LearnerEngine(B, device=DEV, H=H, W=W, optimizer=opt, **kw)
    init_engine_parameters(eng, seed=2)
    eng.reset_optimizer()
    st = _states(seed=8)
    for _ in range(3):
        eng.repr_step(st, TEMP)
    torch.cuda.synchronize()
    eng._keep_states = st
    return eng


def test_repr_steps_are_deterministic_and_in_bounds(monkeypatch):
    x, y = _three_steps(), _three_steps()
    for name in ARENAS + ('grads',):
        assert torch.equal(getattr(x, name), getattr(y, name)), name
    assert torch.equal(x.buffer(_lib.BUF_METRICS_R), y.buffer(_lib.BUF_METRICS_R))
    monkeypatch.setenv('CDRL_GUARD', '1')
    g = _three_steps()
    assert g.check_guards() == (0, -1)
    assert torch.isfinite(g.params).all()
    for name in ARENAS:
        assert torch.equal(getattr(x, name), getattr(g, name)), name


def _graph_worker(rank, out):
    sys.path.insert(0, ROOT)
    os.environ['CDRL_GRAPH'] = '1'
    torch.cuda.set_device(0)
    eng = _three_steps('nadam')
    assert eng.lib.cdrl_learner_tail_offset(eng.h) == eng.region('trunk', True)[1]     # graphs are on in this process
    torch.save(dict(params=eng.params.cpu(), m=eng.adam_m.cpu(), v=eng.adam_v.cpu(), hp=_hp(eng),
                    metrics=eng.buffer(_lib.BUF_METRICS_R).cpu()), os.path.join(out, 'graph.pt'))


def test_graph_replay_is_bit_identical(tmp_path):
    """One capture and two replays of the pass and of the apply (same pointers) against three eager steps of a twin engine."""
    mp.spawn(_graph_worker, args=(str(tmp_path),), nprocs=1, join=True)
    g = torch.load(tmp_path / 'graph.pt')
    eng = _three_steps('nadam')
    assert torch.equal(g['params'], eng.params.cpu())
    assert torch.equal(g['m'], eng.adam_m.cpu()) and torch.equal(g['v'], eng.adam_v.cpu())
    assert g['hp'] == _hp(eng)
    assert torch.equal(g['metrics'], eng.buffer(_lib.BUF_METRICS_R).cpu())


def test_twenty_steps_on_one_pair_of_views_lower_the_loss():
    eng, = _engines(1)
    eng.reset_optimizer()
    eng.set_hparams(dynamics_lr=1e-3)
    st = _states(seed=5)
    losses = []
    for _ in range(20):
        eng.repr_step(st, TEMP)
        losses.append(eng.buffer(_lib.BUF_METRICS_R)[0].clone())
    losses = [float(x) for x in torch.stack(losses).cpu()]
    print('[repr pass] loss over 20 steps:', ' '.join(f'{x:.4f}' for x in losses))
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0]


def test_refusals():
    frozen, = _engines(1, freeze_trunk=True)
    st = _states()
    before = frozen.grads.clone()
    with pytest.raises(_lib.CdrlError, match='freeze_trunk'):
        frozen.repr_forward_backward(st, TEMP)
    with pytest.raises(_lib.CdrlError, match='freeze_trunk'):
        frozen.trunk_apply()
    assert torch.equal(before, frozen.grads)
    for kw, word in ((dict(clip_mode='global'), 'clip_mode'), (dict(skip_nonfinite=True), 'skip_nonfinite')):
        gated, = _engines(1, **kw)
        p0 = gated.params.clone()
        gated.repr_forward_backward(st, TEMP)           # the pass itself has nothing to do with the gate
        with pytest.raises(_lib.CdrlError, match=word):
            gated.trunk_apply()
        torch.cuda.synchronize()
        assert torch.equal(p0[_slice(gated, 'trunk')], gated.params[_slice(gated, 'trunk')])
    odd = LearnerEngine(7, device=DEV, H=H, W=W)
    z = lambda *s: torch.zeros(s, device=DEV)
    states = dict(state_image=z(7, 4, H, W, 3), state_road=z(7, 4, odd.cfg.road), state_vehicle=z(7, 4, odd.cfg.vehicle),
                  state_navigation=z(7, 4, odd.cfg.navigation))
    with pytest.raises(_lib.CdrlError, match='even'):
        odd.repr_forward_backward(states, TEMP)
    ok, = _engines(1)
    with pytest.raises(_lib.CdrlError, match='temperature'):
        ok.repr_forward_backward(st, 0.0)
    with pytest.raises(ValueError):
        ok.repr_forward_backward(dict(st, state_road=st['state_road'][:-1].contiguous()), TEMP)


def test_export_import_resumes_bit_for_bit():
    a = _three_steps('nadam')
    st = a._keep_states
    state = a.export_state()
    assert state['optimizer']['t_dynamics'] == 3 and state['optimizer']['t_policy'] == 0 and state['optimizer']['t_value'] == 0
    b = LearnerEngine(B, device=DEV, H=H, W=W, optimizer='nadam')
    b.import_state(state)
    for e in (a, b):
        e.repr_step(st, TEMP)
    torch.cuda.synchronize()
    for name in ARENAS:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.get_optimizer_state() == b.get_optimizer_state()
    assert a.get_optimizer_state()['t_dynamics'] == 4
