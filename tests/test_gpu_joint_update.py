"""Joint policy + value update on the GPU (cdrl_learner_joint_forward_backward / _resample / _joint_apply, include/cdrl.h): one
train-mode trunk forward and one trunk backward per minibatch for both losses, one trunk optimizer step.  The heads' gradients are
those of the separate passes bit for bit, the trunk's is their sum up to float32 rounding, and the apply is the separate applies'
arithmetic with the trunk stepped once."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from carla_driving_rl_agent_amd import _lib
from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
from carla_driving_rl_agent_amd.engine import LearnerEngine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
B, H, W = 32, 48, 64
SENTINEL = 777.0
ARENAS = ('params', 'adam_m', 'adam_v')


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------- 1. pair kernel, op level
GUARD = 64


def _guarded(n):
    """A float32 buffer of n elements with GUARD sentinel elements on either side: (whole buffer, the n-element view)."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


@pytest.mark.parametrize('Cc', [20, 320, 512])
@pytest.mark.parametrize('M', [1, 2, 16, 17, 129, 300, 2048])
def test_bn_small_bwd_pair(lib, M, Cc):
    """Two BatchNorms over the same input: dgamma / dbeta / coef of each bit-identical to cdrl_bn_small_bwd on it alone, dx the
    sum of the two input gradients within one ulp per term and the final add; nothing outside the outputs is written."""
    rng = np.random.default_rng(1000 * M + Cc)
    x = torch.as_tensor((rng.standard_normal((M, Cc)) * rng.uniform(0.5, 2.0, Cc) + rng.uniform(-1, 1, Cc)).astype(np.float32)).to(DEV)
    douts = [torch.as_tensor(rng.standard_normal((M, Cc)).astype(np.float32)).to(DEV) for _ in range(2)]
    stats, single = [], []
    for k in range(2):
        gam = torch.as_tensor(rng.uniform(0.5, 1.5, Cc).astype(np.float32)).to(DEV)
        bet = torch.as_tensor(rng.uniform(-1, 1, Cc).astype(np.float32)).to(DEV)
        mm, mv = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
        st, out = torch.zeros(4 * Cc, device=DEV), torch.zeros((M, Cc), device=DEV)
        _lib.check(lib.cdrl_bn_small_fwd(P(x), M, Cc, P(gam), P(bet), P(mm), P(mv), P(st), P(out), S()))
        dg, db, coef, dx = (torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV), torch.zeros(3 * Cc, device=DEV),
                            torch.zeros((M, Cc), device=DEV))
        _lib.check(lib.cdrl_bn_small_bwd(P(douts[k]), P(x), M, Cc, P(st), P(dg), P(db), P(coef), P(dx), S()))
        stats.append(st)
        single.append((dg, db, coef, dx))
    bufs = [_guarded(n) for n in (Cc, Cc, 3 * Cc, Cc, Cc, 3 * Cc, M * Cc)]
    (dgA, dbA, cfA, dgB, dbB, cfB, dx) = [v for _, v in bufs]
    _lib.check(lib.cdrl_bn_small_bwd_pair(P(douts[0]), P(douts[1]), P(x), M, Cc, P(stats[0]), P(stats[1]), P(dgA), P(dbA), P(cfA),
                                          P(dgB), P(dbB), P(cfB), P(dx), S()))
    torch.cuda.synchronize()
    for (whole, _), n in zip(bufs, (Cc, Cc, 3 * Cc, Cc, Cc, 3 * Cc, M * Cc)):
        assert _guards_intact(whole, n)
    for k, (dg, db, cf) in enumerate(((dgA, dbA, cfA), (dgB, dbB, cfB))):
        assert torch.equal(dg, single[k][0]), ('dgamma', k)
        assert torch.equal(db, single[k][1]), ('dbeta', k)
        assert torch.equal(cf, single[k][2]), ('coef', k)
    a, b = single[0][3].double(), single[1][3].double()
    err = (dx.view(M, Cc).double() - (a + b)).abs()
    bound = 4.0 * 2.0 ** -24 * (a.abs() + b.abs())
    worst = float((err - bound).max())
    print(f'[pair M={M} C={Cc}] max |dx - (dxA + dxB)| = {float(err.max()):.3e}, worst excess over the bound {worst:.3e}')
    assert bool((err <= bound).all())


# ---------------------------------------------------------------------------------------------- engines
def _engines(n, batch=B, compute='f32', kinds=None, **kw):
    """n engines over identical arenas (the first one initialised, the others copies); kinds: per-engine extra keywords."""
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    kinds = kinds or [{}] * n
    engs = [LearnerEngine(batch, device=DEV, H=H, W=W, compute=compute, **kw, **k) for k in kinds]
    init_engine_parameters(engs[0], seed=4)
    for e in engs[1:]:
        for name in ARENAS:
            getattr(e, name).copy_(getattr(engs[0], name))
    return engs


def _batches(batch=B, seed=21):
    from tests.util import make_batches, to_dev
    pol, val = make_batches(batch, H, W, seed=seed)
    dpol, dval = to_dev(pol), to_dev(val)
    joint = dict(dpol)
    joint['returns'] = dval['returns']
    return dpol, dval, joint


def _slice(eng, model, trainable=True):
    o, n = eng.region(model, trainable)
    return slice(o, o + n)


def _hp_steps(eng):
    torch.cuda.synchronize()
    return [int(x) for x in eng.named_buffer('hparams', dtype=torch.int32)[10:13].cpu()]


_THREE = {}


def _three(batch, compute, stored=False):
    """A (joint pass), P (policy pass), V (value pass) after one pass each on the same parameters and batch; computed once."""
    key = (batch, compute, stored)
    if key not in _THREE:
        a, p, v = _engines(3, batch, compute)
        dpol, dval, joint = _batches(batch)
        if stored:
            a.joint_forward_backward(joint)
            p.policy_forward_backward(dpol)
        else:
            a.joint_forward_backward_resample(joint, seed=9, offset=3)
            p.policy_forward_backward_resample(dpol, seed=9, offset=3)
        v.value_forward_backward(dval)
        torch.cuda.synchronize()
        _THREE[key] = (a, p, v)
    return _THREE[key]


# ---------------------------------------------------------------------------------------------- 2. heads are exact
@pytest.mark.parametrize('compute,stored', [('f32', False), ('bf16s', False), ('f32', True)])
def test_joint_heads_match_separate_passes(compute, stored):
    a, p, v = _three(B, compute, stored)
    assert torch.equal(a.grads[_slice(a, 'policy')], p.grads[_slice(p, 'policy')])
    assert torch.equal(a.grads[_slice(a, 'value')], v.grads[_slice(v, 'value')])
    for which in (_lib.BUF_METRICS_P, _lib.BUF_AUX_P) + (() if stored else (_lib.BUF_SAMPLE,)):
        assert torch.equal(a.buffer(which), p.buffer(which)), which
    for which in (_lib.BUF_METRICS_V, _lib.BUF_AUX_V):
        assert torch.equal(a.buffer(which), v.buffer(which)), which
    st = _slice(a, 'trunk', False)
    assert torch.equal(a.params[st], p.params[st]), 'trunk moving statistics: one update per joint pass'
    assert torch.equal(a.params[st], v.params[st])


def test_policy_split_form_matches_the_one_call_pass():
    """policy_forward then policy_backward (the split form of the C ABI) against policy_forward_backward on the stored-action batch:
    the same ops in the same order, so gradients, metrics and moving statistics are equal bit for bit."""
    x, y = _engines(2, batch=4)
    dpol, _, _ = _batches(batch=4)
    batch = dict(dpol, du_da=None, du_db=None)
    x.policy_forward_backward(batch)
    y.policy_forward(batch['states'])
    y.policy_backward(batch)
    torch.cuda.synchronize()
    for model in ('policy', 'trunk'):
        assert torch.equal(x.grads[_slice(x, model)], y.grads[_slice(y, model)]), model
        assert torch.equal(x.params[_slice(x, model, False)], y.params[_slice(y, model, False)]), f'{model} moving statistics'
    assert torch.equal(x.buffer(_lib.BUF_METRICS_P), y.buffer(_lib.BUF_METRICS_P))
    assert float(x.grads[_slice(x, 'trunk')].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------- 3. trunk gradient is the sum
def test_joint_trunk_gradient_is_the_sum():
    """Per trainable trunk tensor max|g_A - (g_P + g_V)| / (max|g_P| + max|g_V|), the sum formed in float64.  Bound: twice the
    per-group bound tests/test_gpu_learner.py holds an engine gradient to at this minibatch (each of the three gradients is within
    that bound of its exact value; triangle inequality).  A wiring mistake -- one head not reaching the trunk, dyn.g overwritten
    instead of summed -- is an O(1) error."""
    from tests.test_gpu_learner import _pinned_group, _pinned_tol
    from tests.util import is_degenerate_bias, is_zero_gradient
    batch = 64
    a, p, v = _three(batch, 'f32')
    bounds = {g: 2.0 * t for g, t in _pinned_tol(batch).items()}
    ga, gp, gv = (e.grad_views('trunk') for e in (a, p, v))
    worst = {}
    for name in ga:
        if is_zero_gradient(name) or is_degenerate_bias(name):
            continue
        x, y = gp[name].double(), gv[name].double()
        denom = float(x.abs().max()) + float(y.abs().max())
        assert denom > 0.0, name
        e = float((ga[name].double() - (x + y)).abs().max()) / denom
        grp = _pinned_group(name)
        if e > worst.get(grp, (0.0, ''))[0]:
            worst[grp] = (e, name)
    for grp, (e, name) in sorted(worst.items()):
        print(f'[joint trunk gradient] {grp}: worst {e:.3e} on {name} (bound {bounds[grp]:.1e})')
    assert set(worst) == set(bounds)
    for grp, (e, name) in worst.items():
        assert e <= bounds[grp], (grp, name, e, bounds[grp])


# ---------------------------------------------------------------------------------------------- 4. apply is exact
GATES = {'plain': dict(), 'gated': dict(clip_mode='global', skip_nonfinite=True)}


def _inject(engs, seed=5, scale=1e-2):
    g = torch.randn(engs[0].grads_total, generator=torch.Generator().manual_seed(seed)).mul_(scale).to(DEV)
    for e in engs:
        e.grads.copy_(g)
    return g


@pytest.mark.parametrize('gate', sorted(GATES))
@pytest.mark.parametrize('optimizer', ['adam', 'nadam'])
def test_joint_apply_matches_separate_applies(optimizer, gate):
    kw = dict(optimizer=optimizer, **GATES[gate])
    a, c, f, s = _engines(4, 4, kinds=[{}, {}, dict(freeze_trunk=True), {}], **kw)
    for e in (a, c, f, s):
        e.reset_optimizer()
        if gate == 'gated':     # thresholds on either side of the lists' norms: the policy's and the trunk's lists are clipped
            e.set_hparams(clip_norm_policy=0.05, clip_norm_value=100.0, clip_norm_dynamics=0.5)
    _inject((a, c, f, s))
    k = 2
    for _ in range(k):
        a.joint_apply()
        c.policy_apply()
        f.policy_apply()
        f.value_apply()
        s.policy_apply()
        s.value_apply()
    torch.cuda.synchronize()
    t = _slice(a, 'trunk')
    for name in ARENAS:
        assert torch.equal(getattr(a, name)[t], getattr(c, name)[t]), ('trunk', name)
        for m in ('policy', 'value'):
            assert torch.equal(getattr(a, name)[_slice(a, m)], getattr(f, name)[_slice(f, m)]), (m, name)
    for trainable in (True, False):
        o = _slice(a, 'old_policy', trainable)
        assert torch.equal(a.params[o], f.params[o])
    assert not torch.equal(a.params[t], f.params[t])        # (the joint apply did step the trunk)
    assert _hp_steps(a) == [k, k, k]
    assert _hp_steps(s) == [k, k, 2 * k]
    if optimizer == 'nadam':        # m_caches: the trunk's as after k policy applies, the heads' as on the frozen engine
        mc = lambda e: e.named_buffer('hparams')[13:16].cpu()
        assert torch.equal(mc(a)[2], mc(c)[2]) and torch.equal(mc(a)[:2], mc(f)[:2])


# ---------------------------------------------------------------------------------------------- 5. gate with a NaN
def _first_trainable(eng, model):
    e = next(e for e in eng.tables[model].entries if e['trainable'])
    return eng.region(model, True)[0] + e['offset']


def _state(eng, models):
    torch.cuda.synchronize()
    out = {(m, name): getattr(eng, name)[_slice(eng, m)].clone() for m in models for name in ARENAS}
    if 'policy' in models:
        for trainable in (True, False):
            out[('old_policy', trainable)] = eng.params[_slice(eng, 'old_policy', trainable)].clone()
    return out


def _same_state(before, after):
    return all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize('clip_mode', ['tensor', 'global'])
def test_joint_apply_gate_with_a_nan(clip_mode):
    (a,) = _engines(1, 4, clip_mode=clip_mode, skip_nonfinite=True)
    a.reset_optimizer()
    # one NaN in the trunk's list: trunk and policy head skipped together, the value head applied
    _inject((a,))
    a.grads[_first_trainable(a, 'trunk')] = float('nan')
    tp, v0 = _state(a, ('trunk', 'policy')), _state(a, ('value',))
    a.joint_apply()
    assert _same_state(tp, _state(a, ('trunk', 'policy')))
    assert not torch.equal(v0[('value', 'params')], a.params[_slice(a, 'value')])
    assert _hp_steps(a) == [0, 1, 0]
    st = a.gate_stats()
    assert (st['policy']['skipped'], st['policy']['applied']) == (1, 0)
    assert (st['value']['skipped'], st['value']['applied']) == (0, 1)
    # one NaN in the value head's list only: the value head skipped, trunk and policy head applied
    _inject((a,))
    a.grads[_first_trainable(a, 'value')] = float('nan')
    tp, v0 = _state(a, ('trunk', 'policy')), _state(a, ('value',))
    a.joint_apply()
    now = _state(a, ('trunk', 'policy'))
    assert _same_state(v0, _state(a, ('value',)))
    for m in ('trunk', 'policy'):
        assert not torch.equal(tp[(m, 'params')], now[(m, 'params')]), m
    assert _hp_steps(a) == [1, 1, 1]
    st = a.gate_stats()
    assert (st['policy']['skipped'], st['policy']['applied']) == (1, 1)
    assert (st['value']['skipped'], st['value']['applied']) == (1, 1)
    assert torch.isfinite(a.params).all()


# ---------------------------------------------------------------------------------------------- 6. frozen trunk
def test_joint_on_a_frozen_trunk():
    full, frozen = _engines(2, kinds=[{}, dict(freeze_trunk=True)])
    _, _, joint = _batches()
    t = _slice(frozen, 'trunk')
    frozen.grads.zero_()
    frozen.grads[t] = SENTINEL
    for e in (full, frozen):
        e.joint_forward_backward_resample(joint, seed=9, offset=3)
    torch.cuda.synchronize()
    assert bool((frozen.grads[t] == SENTINEL).all()), 'frozen joint pass wrote the trunk gradient slice'
    for m in ('policy', 'value'):
        assert torch.equal(full.grads[_slice(full, m)], frozen.grads[_slice(frozen, m)]), m
    before = [getattr(frozen, name)[t].clone() for name in ARENAS]
    heads = frozen.params[_slice(frozen, 'value')].clone()
    k = 2
    for _ in range(k):
        frozen.joint_apply()
    torch.cuda.synchronize()
    for was, name in zip(before, ARENAS):
        assert torch.equal(was, getattr(frozen, name)[t]), name
    assert not torch.equal(heads, frozen.params[_slice(frozen, 'value')])
    assert _hp_steps(frozen) == [k, k, 0]


# ---------------------------------------------------------------------------------------------- 7. determinism and bounds
def _three_steps(**kw):
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    eng = LearnerEngine(B, device=DEV, H=H, W=W, **kw)
    init_engine_parameters(eng, seed=2)
    _, _, joint = _batches(seed=8)
    for k in range(3):
        eng.joint_forward_backward_resample(joint, seed=5, offset=k)
        eng.joint_apply()
    torch.cuda.synchronize()
    return eng


def test_joint_steps_are_deterministic_and_in_bounds(monkeypatch):
    x, y = _three_steps(), _three_steps()
    for name in ARENAS + ('grads',):
        assert torch.equal(getattr(x, name), getattr(y, name)), name
    monkeypatch.setenv('CDRL_GUARD', '1')
    g = _three_steps()
    assert g.check_guards() == (0, -1)
    assert torch.isfinite(g.params).all()
    for name in ARENAS:
        assert torch.equal(getattr(x, name), getattr(g, name)), name


# ---------------------------------------------------------------------------------------------- 8. train stats
def test_joint_train_stats_rows():
    eng = _three_steps(train_stats=8)
    eng.train_stats_reset()
    _, _, joint = _batches(seed=8)
    for k in range(2):
        eng.joint_forward_backward_resample(joint, seed=6, offset=k)
        eng.joint_apply()
    rows = eng.train_stats()['rows']
    assert [r['kind'] for r in rows] == ['policy', 'value', 'policy', 'value']
    for pr, vr in (rows[0:2], rows[2:4]):
        assert pr['trunk_norms'] and pr['trunk_norms'] == vr['trunk_norms']
        assert pr['t_dynamics'] == vr['t_dynamics'] == pr['t_head'] == vr['t_head']
    assert rows[0]['trunk_norms'] != rows[2]['trunk_norms']
    assert rows[2]['t_dynamics'] == rows[0]['t_dynamics'] + 1


# ---------------------------------------------------------------------------------------------- 9. agent
def _agent(tmp_path, **kw):
    cfg = dict(batch_size=8, log_mode=None, seed=3, skip_data=1, drop_batch_remainder=True, shuffle=True, policy_lr=3e-4,
               value_lr=3e-4, dynamics_lr=3e-4, aug_intensity=0.0, weights_dir=str(tmp_path), name='t', optimization_steps=(1, 1))
    cfg.update(kw)
    env = FakeCARLAEnvironment(image_shape=(36, 108, 3), time_horizon=4, num_waypoints=5, vehicle_features=4, num_actions=3)
    return CARLAgent(env, **cfg)


def test_agent_joint_update(tmp_path):
    agent = _agent(tmp_path, joint_update=True)
    eng = agent.network.engine
    before = {m: eng.params[_slice(eng, m)].clone() for m in ('trunk', 'policy', 'value')}
    agent.learn(episodes=1, timesteps=17, save_every='end', close=False)
    assert torch.isfinite(eng.params).all()
    for m, was in before.items():
        assert not torch.equal(was, eng.params[_slice(eng, m)]), m
    tp, tv, tt = _hp_steps(eng)
    assert tp == tv == tt > 0
    twin = _agent(tmp_path, name='twin', joint_update=False)
    twin.learn(episodes=1, timesteps=17, save_every='end', close=False)
    sp, sv, st = _hp_steps(twin.network.engine)
    assert sp == sv > 0 and st == 2 * sp
    with pytest.raises(ValueError):
        _agent(tmp_path, name='bad', joint_update=True, optimization_steps=(1, 2))


# ---------------------------------------------------------------------------------------------- 10. data parallel
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out, frozen):
    """world 1: three joint steps plain and with the collectives forced over a one-rank NCCL group (twice); world 2: one rank per
    GPU on rank-dependent batches."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    dev = torch.device(f'cuda:{rank}')
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    from carla_driving_rl_agent_amd.parallel import DataParallelLearner
    from tests.util import make_batches, to_dev
    runs = (('plain', False), ('forced', True), ('forced2', True)) if world == 1 else (('ranks', True),)
    res = {}
    for tag, force in runs:
        eng = LearnerEngine(B, device=str(dev), H=H, W=W, freeze_trunk=frozen)
        init_engine_parameters(eng, seed=5)
        eng.grads.zero_()
        if frozen:      # (never written: the sentinel must survive, and the arenas compare as a whole)
            t0, tn = eng.region('trunk', True)
            eng.grads[t0:t0 + tn] = SENTINEL
        dp = DataParallelLearner(eng, force_collectives=force)
        dp.broadcast_parameters()
        pol, val = make_batches(B, H, W, seed=61 + rank)
        joint = to_dev(pol, str(dev))
        joint['returns'] = to_dev(val, str(dev))['returns']
        for k in range(3):
            dp.joint_step(joint, resample=(11, 2 * k + rank))
        torch.cuda.synchronize()
        if frozen:
            assert bool((eng.grads[t0:t0 + tn] == SENTINEL).all())
        res[tag] = dict(grads=eng.grads.cpu(), params=eng.params.cpu(), m=eng.adam_m.cpu(), v=eng.adam_v.cpu())
    torch.save(res, os.path.join(out, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('frozen', [False, True])
def test_joint_world1_nccl_is_bit_identical(tmp_path, frozen):
    mp.spawn(_worker, args=(1, _free_port(), str(tmp_path), frozen), nprocs=1, join=True)
    res = torch.load(tmp_path / 'r0.pt')
    for k in ('grads', 'params', 'm', 'v'):
        assert torch.equal(res['plain'][k], res['forced'][k]), k
        assert torch.equal(res['forced'][k], res['forced2'][k]), k


def test_joint_two_rank_rccl(tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs')
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), False), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f'r{r}.pt')['ranks'] for r in range(2))
    for k in ('params', 'm', 'v'):
        assert torch.equal(r0[k], r1[k]), k
