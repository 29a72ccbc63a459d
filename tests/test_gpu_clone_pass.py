"""Behaviour-cloning pass on the GPU (cdrl_learner_clone_forward_backward, include/cdrl.h): the clone loss in the
place of the policy loss on the stored-action policy pass, optionally with the value loss and the joint tail.  Gradients against
the float64 restatement (tests/clone_ref.py) on the oracle model at the project's whole-pass tolerance of 1e-4 (tests/util.check3,
the engine's discrete decisions pinned), and bit-level identities against the existing passes."""
import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from carla_driving_rl_agent_amd.engine import LearnerEngine
from tests import clone_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, H, W, A = 32, 48, 64, 2
SENTINEL = 777.0
ARENAS = ('params', 'adam_m', 'adam_v')
TOL = 1e-4


def _engines(n, batch=B, kinds=None, seed=4, **kw):
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    kinds = kinds or [{}] * n
    engs = [LearnerEngine(batch, device=DEV, H=H, W=W, **kw, **k) for k in kinds]
    init_engine_parameters(engs[0], seed=seed)
    for e in engs[1:]:
        for name in ARENAS:
            getattr(e, name).copy_(getattr(engs[0], name))
    for e in engs:
        e.set_hparams(entropy_coef=0.01)
    return engs


def _host_batches(batch=B, seed=21):
    from tests.util import make_batches
    pol, val = make_batches(batch, H, W, seed=seed, A=A)
    rng = np.random.default_rng(seed + 7)
    weight = rng.uniform(0.0, 2.0, batch).astype(np.float32)
    weight[::5] = 0.0
    clone = dict(states=pol['states'], u=pol['u'], weight=weight, speed=pol['speed'], similarity=pol['similarity'])
    return pol, val, clone


def _batches(batch=B, seed=21):
    """(stored-action policy batch, value batch, clone batch, clone batch with returns), on the device."""
    from tests.util import to_dev
    pol, val, clone = _host_batches(batch, seed)
    dpol, dval, dclone = to_dev(pol), to_dev(val), to_dev(clone)
    return dpol, dval, dclone, dict(dclone, returns=dval['returns'])


def _slice(eng, model, trainable=True):
    o, n = eng.region(model, trainable)
    return slice(o, o + n)


def _hp_steps(eng):
    torch.cuda.synchronize()
    return [int(x) for x in eng.named_buffer('hparams', dtype=torch.int32)[10:13].cpu()]


_FOUR = {}


def _four():
    """C (clone pass), H (clone pass at policy_weight 0.5), J (clone pass with returns), P (stored-action policy pass), V (value
    pass): one pass each on the same parameters; computed once."""
    if not _FOUR:
        c, h, j, p, v = _engines(5)
        dpol, dval, dclone, djoint = _batches()
        c.clone_forward_backward(dclone)
        h.clone_forward_backward(dclone, policy_weight=0.5)
        j.clone_forward_backward(djoint, value_weight=1.0)
        p.policy_forward_backward(dict(dpol, du_da=None, du_db=None))
        v.value_forward_backward(dval)
        torch.cuda.synchronize()
        _FOUR.update(c=c, h=h, j=j, p=p, v=v)
    return _FOUR


def test_forward_is_the_policy_pass_forward():
    f = _four()
    assert torch.equal(f['c'].buffer(_lib.BUF_LIN_P), f['p'].buffer(_lib.BUF_LIN_P))
    st = _slice(f['c'], 'trunk', False)
    assert torch.equal(f['c'].params[st], f['p'].params[st]), 'trunk moving statistics'
    assert not torch.equal(f['c'].grads[_slice(f['c'], 'policy')], f['p'].grads[_slice(f['p'], 'policy')])   # (another loss)


def test_policy_weight_scales_the_gradients_only():
    f = _four()
    for m in ('policy', 'trunk'):
        one, half = f['c'].grads[_slice(f['c'], m)], f['h'].grads[_slice(f['h'], m)]
        assert float(one.abs().max()) > 0.0
        torch.testing.assert_close(half, 0.5 * one, rtol=1e-6, atol=0.0)
    assert torch.equal(f['c'].buffer(_lib.BUF_METRICS_P), f['h'].buffer(_lib.BUF_METRICS_P)), 'metrics stay unscaled'


def test_with_returns_the_heads_are_those_of_the_separate_passes():
    f = _four()
    j, c, v = f['j'], f['c'], f['v']
    assert torch.equal(j.grads[_slice(j, 'value')], v.grads[_slice(v, 'value')])
    assert torch.equal(j.buffer(_lib.BUF_METRICS_V), v.buffer(_lib.BUF_METRICS_V))
    assert torch.equal(j.buffer(_lib.BUF_AUX_V), v.buffer(_lib.BUF_AUX_V))
    assert torch.equal(j.grads[_slice(j, 'policy')], c.grads[_slice(c, 'policy')])
    assert torch.equal(j.buffer(_lib.BUF_METRICS_P), c.buffer(_lib.BUF_METRICS_P))
    assert not torch.equal(j.grads[_slice(j, 'trunk')], c.grads[_slice(c, 'trunk')])      # (the value loss reached the trunk)


def test_value_weight_zero_leaves_no_value_gradient():
    (e,) = _engines(1)
    _, _, _, djoint = _batches()
    e.clone_forward_backward(djoint, value_weight=1.0)
    assert float(e.grads[_slice(e, 'value')].abs().max()) > 0.0
    e.clone_forward_backward(djoint, value_weight=0.0)
    torch.cuda.synchronize()
    assert not e.grads[_slice(e, 'value')].any()
    assert float(e.buffer(_lib.BUF_METRICS_V)[0]) > 0.0


def test_gradients_match_the_float64_restatement():
    """Policy-head and trunk gradients of one clone pass (weights with zeros, targets, aux_weight 0.6) against clone_ref on the
    float64 oracle model evaluated on the engine's own ReLU6 / max-pool decisions; per tensor, check3 at 1e-4 relative to the
    tensor's scale (floored at 1e-3 of the largest gradient, as tests/test_gpu_learner.py does), analytically zero gradients
    excluded."""
    from oracle import model as OM
    from tests.util import check3, engine_decisions, is_zero_gradient, make_pair, to_dev
    oracle, eng = make_pair(B, H, W, seed=3, A=A, with64=True)
    _, _, clone = _host_batches(seed=3)
    aw = 0.6
    eng.clone_forward_backward(to_dev(clone), aux_weight=aw)
    torch.cuda.synchronize()
    ob = dict(clone)
    OM.DEC.items = engine_decisions(eng, oracle.cfg)
    try:
        OM.DEC.start('replay')
        total64, gp64, gt64, out64 = clone_ref.clone_grads(oracle.o64, ob, aw)
        assert OM.DEC.cursor == len(OM.DEC.items)
        OM.DEC.start('replay')
        total32, gp32, gt32, _ = clone_ref.clone_grads(oracle, ob, aw)
    finally:
        OM.DEC.start('off')
    m = eng.buffer(_lib.BUF_METRICS_P).cpu().numpy()
    for k, ref in enumerate(clone_ref.metric_slots(out64)):
        assert abs(float(m[k]) - ref) < TOL * max(1.0, abs(ref)), (k, float(m[k]), ref)
    worst = {}
    for model, g64, g32 in (('policy', gp64, gp32), ('trunk', gt64, gt32)):
        views = eng.grad_views(model)
        gmax = max(float(g.abs().max()) for g in g64.values())
        assert gmax > 0.0
        for name, g in g64.items():
            if is_zero_gradient(name):
                continue
            err, bound = check3(views[name].cpu().numpy(), g32[name].detach().numpy(), g.detach().numpy(), tol=TOL, floor=1e-3 * gmax)
            if err >= worst.get(model, (0.0, 0.0, ''))[0]:
                worst[model] = (err, bound, name)
            assert err <= bound, (model, name, err, bound)
    for model, (err, bound, name) in worst.items():
        print(f'[clone pass] {model}: worst gradient error {err:.3e} on {name} (bound {bound:.3e})')


def test_frozen_trunk_writes_no_trunk_gradient():
    full, frozen = _engines(2, kinds=[{}, dict(freeze_trunk=True)])
    _, _, dclone, djoint = _batches()
    t = _slice(frozen, 'trunk')
    for batch, kw in ((dclone, {}), (djoint, dict(value_weight=1.0))):
        frozen.grads.zero_()
        frozen.grads[t] = SENTINEL
        for e in (full, frozen):
            e.clone_forward_backward(batch, **kw)
        torch.cuda.synchronize()
        assert bool((frozen.grads[t] == SENTINEL).all()), 'frozen clone pass wrote the trunk gradient slice'
        for m in ('policy', 'value') if 'returns' in batch else ('policy',):
            assert torch.equal(full.grads[_slice(full, m)], frozen.grads[_slice(frozen, m)]), m


def _three_steps(**kw):
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    eng = LearnerEngine(B, device=DEV, H=H, W=W, **kw)
    init_engine_parameters(eng, seed=2)
    _, _, dclone, djoint = _batches(seed=8)
    for k in range(3):
        eng.clone_step(djoint if k % 2 else dclone, value_weight=1.0 if k % 2 else 0.0)
    torch.cuda.synchronize()
    return eng


def test_clone_steps_are_deterministic_and_in_bounds(monkeypatch):
    x, y = _three_steps(), _three_steps()
    for name in ARENAS + ('grads',):
        assert torch.equal(getattr(x, name), getattr(y, name)), name
    monkeypatch.setenv('CDRL_GUARD', '1')
    g = _three_steps()
    assert g.check_guards() == (0, -1)
    assert torch.isfinite(g.params).all()
    for name in ARENAS:
        assert torch.equal(getattr(x, name), getattr(g, name)), name


def test_two_identical_passes_give_identical_gradients():
    (e,) = _engines(1)
    _, _, _, djoint = _batches()
    e.clone_forward_backward(djoint, value_weight=0.5)
    first = e.grads.clone()
    e.clone_forward_backward(djoint, value_weight=0.5)
    torch.cuda.synchronize()
    # (the moving statistics moved between the two; train-mode gradients do not read them)
    assert torch.equal(first, e.grads)


def test_clone_step_counters_and_what_it_touches():
    (e,) = _engines(1)
    e.reset_optimizer()
    _, _, dclone, djoint = _batches()
    before = {m: e.params[_slice(e, m)].clone() for m in ('trunk', 'policy', 'value')}
    e.clone_step(dclone)
    assert _hp_steps(e) == [1, 0, 1]
    for m in ('trunk', 'policy'):
        assert not torch.equal(before[m], e.params[_slice(e, m)]), m
    assert torch.equal(before['value'], e.params[_slice(e, 'value')])
    for name in ('adam_m', 'adam_v'):
        assert not getattr(e, name)[_slice(e, 'value')].any(), name
    e.clone_step(djoint, value_weight=0.5)
    assert _hp_steps(e) == [2, 1, 2]
    assert not torch.equal(before['value'], e.params[_slice(e, 'value')])
    assert torch.isfinite(e.params).all()
    # the applies copy old_policy <- policy BEFORE the step: it lags until update_old_policy
    assert not torch.equal(e.params[_slice(e, 'old_policy')], e.params[_slice(e, 'policy')])
    e.update_old_policy()
    torch.cuda.synchronize()
    for trainable in (True, False):
        assert torch.equal(e.params[_slice(e, 'old_policy', trainable)], e.params[_slice(e, 'policy', trainable)])


def test_malformed_batches_are_refused():
    (e,) = _engines(1)
    _, _, dclone, djoint = _batches()
    bad = [dict(dclone, u=dclone['u'][:, :1].contiguous()), dict(dclone, u=dclone['u'].double()), dict(dclone, u=dclone['u'].cpu()),
           dict(dclone, u=None), dict(dclone, weight=dclone['weight'][:-1].contiguous()), dict(dclone, speed=None),
           dict(dclone, similarity=dclone['similarity'][:-1].contiguous()), dict(djoint, returns=djoint['returns'][:, :1].contiguous()),
           dict(djoint, speed=None, similarity=None),
           dict(dclone, states=dict(dclone['states'], state_road=dclone['states']['state_road'][:-1].contiguous()))]
    before = e.grads.clone()
    for k, b in enumerate(bad):
        with pytest.raises(ValueError):
            e.clone_forward_backward(b)
        assert torch.equal(before, e.grads), k
    # the C entry on its own: what the Python checks let through as absent
    cb = _lib.CloneBatch(image=1, road=1, vehicle=1, navigation=1, u=None)
    import ctypes as C
    with pytest.raises(_lib.CdrlError, match='clone batch'):
        _lib.check(e.lib.cdrl_learner_clone_forward_backward(e.h, C.byref(cb), 1.0, 0.0, 1.0, 1.0, None), 'clone')
    without = dict(dclone, weight=None, speed=None, similarity=None)      # all optional parts absent: accepted
    e.clone_forward_backward(without, aux_weight=0.0)
    torch.cuda.synchronize()
    assert float(e.buffer(_lib.BUF_METRICS_P)[3]) == 0.0 and float(e.buffer(_lib.BUF_METRICS_P)[5]) == 1.0


def test_above_the_joint_limit_returns_are_refused():
    big = 2049
    e = LearnerEngine(big, device=DEV, H=H, W=W)
    z = lambda *s: torch.zeros(s, device=DEV)
    batch = dict(states=dict(state_image=z(big, 4, H, W, 3), state_road=z(big, 4, e.cfg.road), state_vehicle=z(big, 4, e.cfg.vehicle),
                             state_navigation=z(big, 4, e.cfg.navigation)),
                 u=z(big, A) + 0.5, speed=z(big), similarity=z(big), returns=z(big, 2))
    before = e.grads.clone()
    with pytest.raises(_lib.CdrlError, match='2048'):
        e.clone_forward_backward(batch, value_weight=1.0)
    torch.cuda.synchronize()
    assert torch.equal(before, e.grads)
