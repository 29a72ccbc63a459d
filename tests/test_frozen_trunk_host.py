"""Frozen trunk (cdrl_config.freeze_trunk, CARLAgent(update_dynamics=False)) on the host: the planner's layout and workspace, the
create-time check of the flag, and what DataParallelLearner reduces over gloo for a frozen engine.  No GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SENTINEL = 12345.0


def _engine(B, **kw):
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    return LearnerEngine(B, device=None, **kw)


@pytest.mark.parametrize('B,kw', [(256, dict(H=90, W=120)), (1024, dict(H=90, W=120, compute='bf16s')),
                                  (64, dict(H=36, W=108, A=3, compute='bf16'))])
def test_frozen_planner_same_layout_smaller_workspace(B, kw):
    full, frozen = _engine(B, **kw), _engine(B, freeze_trunk=True, **kw)
    assert not full.frozen and frozen.frozen
    for m in ('trunk', 'policy', 'value'):
        assert frozen.tables[m].entries == full.tables[m].entries, m
    for m in ('trunk', 'policy', 'value', 'old_policy'):
        for tr in (True, False):
            assert frozen.region(m, tr) == full.region(m, tr), (m, tr)
    assert frozen.params_total == full.params_total and frozen.grads_total == full.grads_total
    assert frozen.workspace_bytes < full.workspace_bytes, (frozen.workspace_bytes, full.workspace_bytes)
    # no trunk gradient becomes final mid-pass on a frozen learner
    assert frozen.tail_offset() == frozen.region('trunk', True)[1]


def test_shared_engines_inherit_the_flag():
    owner = _engine(32, H=48, W=64, freeze_trunk=True)
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    assert LearnerEngine(8, device=None, share_with=owner, H=48, W=64).frozen
    assert not LearnerEngine(8, device=None, share_with=owner, H=48, W=64, freeze_trunk=False).frozen


@pytest.mark.parametrize('value', [2, -1])
def test_invalid_freeze_trunk_rejected_at_create(value):
    from carla_driving_rl_agent_amd import _lib
    with pytest.raises(_lib.CdrlError, match='freeze_trunk'):
        _engine(8, H=48, W=64, freeze_trunk=value)


def test_config_default_is_not_frozen():
    import ctypes as C
    from carla_driving_rl_agent_amd import _lib
    cfg = _lib.Config()
    cfg.freeze_trunk = 7
    _lib.load().cdrl_config_default(C.byref(cfg))
    assert cfg.freeze_trunk == 0


class FrozenStandIn:
    """The engine surface DataParallelLearner touches, over the real (frozen) arena layout: a pass writes rank-dependent head
    gradients (scaled by grad_scale, as the loss kernels do) and rank-dependent moving statistics -- and, like the frozen engine,
    never the trunk's gradient slice.  Every access to the arenas goes through plain tensors, so a reduction of the trunk slice
    would show up as a changed sentinel."""

    def __init__(self, rank):
        self.layout = _engine(16, H=48, W=64, freeze_trunk=True)
        self.frozen = True
        self.rank = rank
        self.params = torch.zeros(self.layout.params_total)
        self.grads = torch.zeros(self.layout.grads_total)
        self.adam_m = torch.zeros(self.layout.grads_total)
        self.adam_v = torch.zeros(self.layout.grads_total)
        t0, tn = self.region('trunk', True)
        self.grads[t0:t0 + tn] = SENTINEL
        self.applied = []

    def region(self, model, trainable):
        return self.layout.region(model, trainable)

    def tail_offset(self):
        return self.layout.tail_offset()

    def _pass(self, model, scale):
        off, n = self.region(model, True)
        self.grads[off:off + n] = (torch.arange(n, dtype=torch.float32) % 97 + 1.0) * (self.rank + 1) * scale
        for m in ('policy', 'trunk', 'value', 'old_policy'):
            s0, sn = self.region(m, False)
            self.params[s0:s0 + sn] = torch.arange(sn, dtype=torch.float32) % 13 + 10.0 * self.rank

    def policy_forward_backward(self, batch, grad_scale=1.0):
        self._pass('policy', grad_scale)

    def value_forward_backward(self, batch, grad_scale=1.0):
        self._pass('value', grad_scale)

    def policy_apply(self):
        self.applied.append('policy')

    def value_apply(self):
        self.applied.append('value')


def _worker(rank, world, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from carla_driving_rl_agent_amd.parallel import DataParallelLearner
        eng = FrozenStandIn(rank)
        dp = DataParallelLearner(eng)
        assert dp.frozen and dp._comm is None
        dp.update_step({}, {})
        np.save(os.path.join(out, f'grads{rank}.npy'), eng.grads.numpy())
        np.save(os.path.join(out, f'params{rank}.npy'), eng.params.numpy())
        assert eng.applied == ['policy', 'value']
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_data_parallel_frozen_reduces_heads_only(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    layout = _engine(16, H=48, W=64, freeze_trunk=True)
    g = [np.load(tmp_path / f'grads{r}.npy') for r in range(world)]
    p = [np.load(tmp_path / f'params{r}.npy') for r in range(world)]
    np.testing.assert_array_equal(g[0], g[1])
    np.testing.assert_array_equal(p[0], p[1])
    for m in ('policy', 'value'):
        off, n = layout.region(m, True)
        base = np.arange(n, dtype=np.float32) % 97 + 1.0
        # each rank wrote base * (rank + 1) / world: the SUM is the average of the two ranks' gradients
        np.testing.assert_allclose(g[0][off:off + n], base * (1 + 2) / world, rtol=1e-6)
    t0, tn = layout.region('trunk', True)
    assert np.all(g[0][t0:t0 + tn] == SENTINEL), 'the trunk gradient slice was touched'
    for m in ('policy', 'trunk', 'value', 'old_policy'):
        s0, sn = layout.region(m, False)
        base = np.arange(sn, dtype=np.float32) % 13
        np.testing.assert_allclose(p[0][s0:s0 + sn], base + 10.0 * (0 + 1) / world, rtol=1e-6)
