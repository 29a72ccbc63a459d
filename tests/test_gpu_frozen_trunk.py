"""Frozen trunk on the GPU (cdrl_config.freeze_trunk = 1, CARLAgent(update_dynamics=False); reference core/carla_agent.py:77-80,
351-373,430-463): the trunk forward runs in training mode and updates its BatchNorm moving statistics, the heads train exactly as in a
full pass, and the trunk's parameters, gradient slice and Adam state are never written."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
from carla_driving_rl_agent_amd.engine import LearnerEngine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W = 32, 48, 64
SENTINEL = 777.0


def _env(**kw):
    cfg = dict(image_shape=(36, 108, 3), time_horizon=4, num_waypoints=5, vehicle_features=4, num_actions=3)
    cfg.update(kw)
    return FakeCARLAEnvironment(**cfg)


def _agent(tmp_path, **kw):
    cfg = dict(batch_size=8, log_mode=None, seed=3, skip_data=1, drop_batch_remainder=True, shuffle=True, policy_lr=3e-4,
               value_lr=3e-4, dynamics_lr=3e-4, aug_intensity=0.0, weights_dir=str(tmp_path), name='t', optimization_steps=(1, 1))
    cfg.update(kw)
    return CARLAgent(_env(), **cfg)


def _hp_steps(eng):
    """Adam step counters (policy, value, trunk) of the engine's device hyper-parameter block."""
    torch.cuda.synchronize()
    return [int(x) for x in eng.named_buffer('hparams', dtype=torch.int32)[10:13].cpu()]


def _trunk(eng):
    t0, tn = eng.region('trunk', True)
    s0, sn = eng.region('trunk', False)
    return (eng.params[t0:t0 + tn].clone(), eng.adam_m[t0:t0 + tn].clone(), eng.adam_v[t0:t0 + tn].clone(),
            eng.params[s0:s0 + sn].clone())


def test_agent_frozen_learn_trains_heads_only(tmp_path):
    agent = _agent(tmp_path, update_dynamics=False)
    eng = agent.network.engine
    assert eng.frozen and agent.network.rollout.frozen
    assert set(agent.network.trainable_variables()) == {'policy', 'value'}
    p0, m0, v0, st0 = _trunk(eng)
    heads0 = {m: eng.params[eng.region(m, True)[0]:sum(eng.region(m, True))].clone() for m in ('policy', 'value')}
    agent.learn(episodes=1, timesteps=17, save_every='end', close=False)
    p1, m1, v1, st1 = _trunk(eng)
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    assert not torch.equal(st0, st1), 'trunk moving statistics must follow the training-mode forward'
    for m, before in heads0.items():
        o, n = eng.region(m, True)
        assert not torch.equal(before, eng.params[o:o + n]), m
    assert torch.isfinite(eng.params).all()
    tp, tv, tt = _hp_steps(eng)
    assert tp > 0 and tv > 0 and tt == 0


def _pair(compute):
    """A full and a frozen engine over identical arenas (same seeds, same layout)."""
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    full = LearnerEngine(B, device='cuda:0', H=H, W=W, compute=compute)
    frozen = LearnerEngine(B, device='cuda:0', H=H, W=W, compute=compute, freeze_trunk=True)
    assert frozen.workspace_bytes < full.workspace_bytes
    init_engine_parameters(full, seed=4)
    for name in ('params', 'adam_m', 'adam_v'):
        getattr(frozen, name).copy_(getattr(full, name))
    t0, tn = frozen.region('trunk', True)
    frozen.grads.zero_()
    frozen.grads[t0:t0 + tn] = SENTINEL
    return full, frozen


def _head_grads(eng, m):
    o, n = eng.region(m, True)
    return eng.grads[o:o + n]


@pytest.mark.parametrize('compute', ['f32', 'bf16', 'bf16s'])
def test_frozen_pass_matches_full_pass(compute):
    from tests.util import make_batches, to_dev
    from carla_driving_rl_agent_amd import _lib
    full, frozen = _pair(compute)
    pol, val = make_batches(B, H, W, seed=21)
    dpol, dval = to_dev(pol), to_dev(val)
    t0, tn = frozen.region('trunk', True)
    s0, sn = frozen.region('trunk', False)
    for e in (full, frozen):
        e.policy_forward_backward_resample(dpol, seed=9, offset=3)
    torch.cuda.synchronize()
    assert torch.equal(_head_grads(full, 'policy'), _head_grads(frozen, 'policy'))
    for which in (_lib.BUF_METRICS_P, _lib.BUF_AUX_P, _lib.BUF_SAMPLE):
        assert torch.equal(full.buffer(which), frozen.buffer(which)), which
    assert torch.equal(full.params[s0:s0 + sn], frozen.params[s0:s0 + sn])
    assert bool((frozen.grads[t0:t0 + tn] == SENTINEL).all()), 'frozen pass wrote the trunk gradient slice'
    for e in (full, frozen):
        e.value_forward_backward(dval)
    torch.cuda.synchronize()
    assert torch.equal(_head_grads(full, 'value'), _head_grads(frozen, 'value'))
    for which in (_lib.BUF_METRICS_V, _lib.BUF_AUX_V):
        assert torch.equal(full.buffer(which), frozen.buffer(which)), which
    assert torch.equal(full.params[s0:s0 + sn], frozen.params[s0:s0 + sn])
    assert bool((frozen.grads[t0:t0 + tn] == SENTINEL).all())


def test_frozen_apply_matches_full_heads_and_leaves_trunk():
    full, frozen = _pair('f32')
    g = torch.randn(full.grads_total, generator=torch.Generator().manual_seed(5)).mul_(1e-2).to('cuda:0')
    full.grads.copy_(g)
    frozen.grads.copy_(g)
    t0, tn = frozen.region('trunk', True)
    trunk_before = [x[t0:t0 + tn].clone() for x in (frozen.params, frozen.adam_m, frozen.adam_v)]
    for _ in range(2):
        for e in (full, frozen):
            e.policy_apply()
            e.value_apply()
    torch.cuda.synchronize()
    for m in ('policy', 'value'):
        o, n = full.region(m, True)
        for name in ('params', 'adam_m', 'adam_v'):
            assert torch.equal(getattr(full, name)[o:o + n], getattr(frozen, name)[o:o + n]), (m, name)
    o, n = full.region('old_policy', True)
    assert torch.equal(full.params[o:o + n], frozen.params[o:o + n])
    for before, now in zip(trunk_before, (frozen.params, frozen.adam_m, frozen.adam_v)):
        assert torch.equal(before, now[t0:t0 + tn])
    assert not torch.equal(trunk_before[0], full.params[t0:t0 + tn])      # (the full engine did step its trunk)
    assert _hp_steps(frozen) == [2, 2, 0] and _hp_steps(full) == [2, 2, 4]


def test_transfer_full_checkpoint_into_frozen_agent(tmp_path):
    src = _agent(tmp_path, name='src')
    src.learn(episodes=1, timesteps=17, save_every='end', close=False)
    saved = src.network.get_weights()
    dst = _agent(tmp_path, name='src', update_dynamics=False, load_full=False, load=True, seed=11)
    eng = dst.network.engine
    assert eng.frozen
    for k, v in eng.export_params('trunk').items():
        assert np.array_equal(v, saved['trunk'][k]), k
    heads0 = eng.export_params('policy')
    dst.learn(episodes=1, timesteps=17, close=False)
    trunk = eng.export_params('trunk')
    tr = {e['name'] for e in eng.tables['trunk'].entries if e['trainable']}
    for k in tr:
        assert np.array_equal(trunk[k], saved['trunk'][k]), k
    assert any(not np.array_equal(heads0[k], v) for k, v in eng.export_params('policy').items())


def test_guard_bands_intact_on_frozen_learner(monkeypatch):
    from tests.util import make_batches, to_dev
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    from carla_driving_rl_agent_amd.parallel import DataParallelLearner
    monkeypatch.setenv('CDRL_GUARD', '1')
    eng = LearnerEngine(B, device='cuda:0', H=H, W=W, freeze_trunk=True)
    init_engine_parameters(eng, seed=2)
    dp = DataParallelLearner(eng)
    pol, val = make_batches(B, H, W, seed=8)
    dpol, dval = to_dev(pol), to_dev(val)
    for k in range(3):
        dp.update_step(dpol, dval, resample=(5, k))
    torch.cuda.synchronize()
    bad, first = eng.check_guards()
    assert bad == 0, f'{bad} guard bands overwritten, first at workspace byte {first}'
    assert torch.isfinite(eng.params).all()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    """world 1: the frozen update-step plain and with the collectives forced over a one-rank NCCL group, twice each;
    world 2: one rank per GPU, the frozen update-step on rank-dependent batches."""
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
        eng = LearnerEngine(B, device=str(dev), H=H, W=W, freeze_trunk=True)
        init_engine_parameters(eng, seed=5)
        t0, tn = eng.region('trunk', True)
        eng.grads[t0:t0 + tn] = SENTINEL
        dp = DataParallelLearner(eng, force_collectives=force)
        assert dp._comm is None
        dp.broadcast_parameters()
        pol, val = make_batches(B, H, W, seed=61 + rank)
        dpol, dval = to_dev(pol, str(dev)), to_dev(val, str(dev))
        for k in range(3):
            dp.update_step(dpol, dval, resample=(11, 2 * k + rank))
        torch.cuda.synchronize()
        assert bool((eng.grads[t0:t0 + tn] == SENTINEL).all())
        res[tag] = dict(grads=eng.grads.cpu(), params=eng.params.cpu(), m=eng.adam_m.cpu(), v=eng.adam_v.cpu())
    torch.save(res, os.path.join(out, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def test_frozen_world1_nccl_is_bit_identical(tmp_path):
    mp.spawn(_worker, args=(1, _free_port(), str(tmp_path)), nprocs=1, join=True)
    res = torch.load(tmp_path / 'r0.pt')
    for k in ('grads', 'params', 'm', 'v'):
        assert torch.equal(res['plain'][k], res['forced'][k]), k
        assert torch.equal(res['forced'][k], res['forced2'][k]), k


def test_frozen_two_rank_rccl(tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs')
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f'r{r}.pt')['ranks'] for r in range(2))
    for k in ('params', 'm', 'v'):
        assert torch.equal(r0[k], r1[k]), k
