"""Behaviour-cloning loss kernel on the GPU (cdrl_beta_clone_loss, include/cdrl.h) against its float64 restatement
(tests/clone_ref.py), at the project's loss-kernel tolerance of 1e-5 (tests/test_gpu_ops.py::test_policy_loss).

Shapes: one row; a row count that is a multiple of nothing; exactly one trip of the 256-thread row loop; one trip plus one row at
the largest supported action count; the joint pass's row limit."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from tests import clone_ref
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-5
SENTINEL = 777.0
GUARD_ROWS = 4
SHAPES = [(1, 1), (7, 3), (256, 2), (257, 8), (2048, 2)]


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(a):
    return torch.as_tensor(a).to(DEV).contiguous() if a is not None else None


def _inputs(B, A):
    rng = np.random.default_rng(100 * B + A)
    lin = (rng.standard_normal((B, 2 * A + 2)) * 1.5).astype(np.float32)
    u = np.clip(rng.beta(2, 2, (B, A)), 1e-4, 1 - 1e-4).astype(np.float32)
    flat = u.reshape(-1)
    for i, v in enumerate((0.0, 1.0, 0.5)):         # exact 0 and 1 (clipped by _clip_actions) and 0.5, wherever the shape has room
        flat[(i * 5) % flat.size] = v
    if flat.size == 1:
        flat[0] = 0.0
    w = rng.uniform(0.0, 2.0, B).astype(np.float32)
    w[rng.integers(0, B, max(1, B // 4))] = 0.0
    spd = rng.uniform(0, 0.3, B).astype(np.float32)
    sim = rng.uniform(-1, 1, B).astype(np.float32)
    return lin, u, w, spd, sim


def _reference(lin, u, w, spd, sim, ec, aw):
    tt = lambda x: torch.tensor(x, dtype=torch.float64) if x is not None else None
    lt = torch.tensor(lin, dtype=torch.float64, requires_grad=True)
    total, out = clone_ref.clone_from_lin(lt, tt(u), tt(w), tt(spd), tt(sim), ec, aw)
    total.backward()
    return lt.grad.numpy(), out


def _launch(lib, lin, u, w, spd, sim, ec, aw, gs, with_aux=True):
    B, A = u.shape
    L = 2 * A + 2
    dlin = torch.full((B + GUARD_ROWS, L), SENTINEL, device=DEV)
    aux = torch.full((B + GUARD_ROWS, 4 * A), SENTINEL, device=DEV)
    metrics = torch.full((16,), SENTINEL, device=DEV)
    keep = [dev(lin), dev(u), dev(w), dev(spd), dev(sim)]
    _lib.check(lib.cdrl_beta_clone_loss(*[P(k) for k in keep], ec, aw, B, A, gs, P(dlin), P(metrics), P(aux) if with_aux else None, S()))
    torch.cuda.synchronize()
    assert bool((dlin[B:] == SENTINEL).all()), 'rows behind dlin were written'
    assert bool((aux[B:] == SENTINEL).all()), 'rows behind aux were written'
    assert bool((metrics[8:] == SENTINEL).all()), 'metric slots behind [7] were written'
    return dlin[:B].cpu().numpy(), metrics[:8].cpu().numpy(), aux[:B].cpu().numpy()


@pytest.mark.parametrize('B,A', SHAPES)
def test_clone_loss_matches_float64(lib, B, A):
    lin, u, w, spd, sim = _inputs(B, A)
    assert {0.0} <= set(u.reshape(-1).tolist())
    aw = 0.6
    worst = dict(metrics=0.0, dlin=0.0, aux=0.0)
    for weighted, targets, ec in itertools.product((False, True), (False, True), (0.0, 0.7)):
        args = (lin, u, w if weighted else None, spd if targets else None, sim if targets else None)
        g64, out = _reference(*args, ec, aw)
        slots = clone_ref.metric_slots(out)
        for gs in (1.0, 0.25):
            dlin, metrics, aux = _launch(lib, *args, ec, aw, gs)
            for k, ref in enumerate(slots):
                e = abs(float(metrics[k]) - ref) / max(1.0, abs(ref))
                worst['metrics'] = max(worst['metrics'], e)
                assert e < TOL, (k, float(metrics[k]), ref, weighted, targets, ec, gs)
            e = rel_err(dlin, gs * g64) if np.abs(g64).max() > 0 else float(np.abs(dlin).max())
            worst['dlin'] = max(worst['dlin'], e)
            assert e < TOL, ('dlin', e, weighted, targets, ec, gs)
            if not targets:
                assert not dlin[:, 2 * A:].any(), 'no targets: the similarity / speed columns are exactly 0'
            for i, k in enumerate(('alpha', 'beta', 'log_prob', 'entropy_elems')):
                e = rel_err(aux[:, i * A:(i + 1) * A], out[k].detach().numpy())
                worst['aux'] = max(worst['aux'], e)
                assert e < TOL, (k, e)
    print(f'[clone loss B={B} A={A}] worst relative error: metrics {worst["metrics"]:.2e}, dlin {worst["dlin"]:.2e}, aux {worst["aux"]:.2e}')


@pytest.mark.parametrize('B,A', SHAPES)
def test_zero_weights_leave_entropy_and_auxiliary_gradients(lib, B, A):
    lin, u, _, spd, sim = _inputs(B, A)
    zeros = np.zeros(B, np.float32)
    dlin, metrics, _ = _launch(lib, lin, u, zeros, spd, sim, 0.0, 1.0, 1.0)
    assert not dlin[:, :2 * A].any(), 'zero weights and no entropy bonus: no gradient reaches alpha / beta'
    assert metrics[1] == 0.0 and metrics[5] == 0.0
    assert np.abs(dlin[:, 2 * A:]).max() > 0.0
    g64, out = _reference(lin, u, zeros, spd, sim, 0.7, 1.0)
    dlin, metrics, _ = _launch(lib, lin, u, zeros, spd, sim, 0.7, 1.0, 1.0, with_aux=False)
    assert rel_err(dlin, g64) < TOL
    total = float(out['total'].detach())
    assert abs(float(metrics[0]) - total) < TOL * max(1.0, abs(total))
    # the entropy part alone: what is left of the alpha / beta columns equals the run without targets
    only, _, _ = _launch(lib, lin, u, zeros, None, None, 0.7, 1.0, 1.0)
    assert np.array_equal(only[:, :2 * A], dlin[:, :2 * A])


def test_more_than_eight_actions_are_refused(lib):
    B, A = 4, 9
    lin, u, _, _, _ = _inputs(B, A)
    dlin, metrics = torch.zeros((B, 2 * A + 2), device=DEV), torch.zeros(16, device=DEV)
    keep = [dev(lin), dev(u)]
    with pytest.raises(_lib.CdrlError, match='num_actions'):
        _lib.check(lib.cdrl_beta_clone_loss(P(keep[0]), P(keep[1]), None, None, None, 0.0, 1.0, B, A, 1.0, P(dlin), P(metrics), None, S()))
    torch.cuda.synchronize()
    assert not dlin.any()


def test_one_target_without_the_other_is_refused(lib):
    B, A = 4, 2
    lin, u, _, spd, _ = _inputs(B, A)
    dlin, metrics = torch.zeros((B, 2 * A + 2), device=DEV), torch.zeros(16, device=DEV)
    keep = [dev(lin), dev(u), dev(spd)]
    with pytest.raises(_lib.CdrlError, match='together'):
        _lib.check(lib.cdrl_beta_clone_loss(P(keep[0]), P(keep[1]), None, P(keep[2]), None, 0.0, 1.0, B, A, 1.0, P(dlin), P(metrics), None,
                                            S()))


@pytest.mark.parametrize('B,A', [(7, 3), (257, 8)])
def test_surrogate_at_ratio_one_is_the_likelihood_gradient(lib, B, A):
    """cdrl_beta_ppo_loss with advantage 1, old log-probabilities equal to the ones the clone call wrote, no entropy bonus and no
    Jacobians: its ratio is 1, inside the clip range, so its alpha / beta gradient is that of the unit-weight clone loss."""
    lin, u, _, spd, sim = _inputs(B, A)
    dclone, _, aux = _launch(lib, lin, u, None, spd, sim, 0.0, 1.0, 1.0)
    old = dev(np.ascontiguousarray(aux[:, 2 * A:3 * A]))
    adv = torch.ones(B, device=DEV)
    dlin = torch.zeros((B, 2 * A + 2), device=DEV)
    metrics, hp, paux = torch.zeros(16, device=DEV), torch.zeros(16, device=DEV), torch.zeros((B, 4 * A), device=DEV)
    keep = [dev(lin), adv, old, dev(spd), dev(sim), dev(u)]
    _lib.check(lib.cdrl_beta_ppo_loss(*[P(k) for k in keep], None, None, 0.2, 0.0, B, A, 1.0, P(dlin), P(metrics), P(paux), P(hp), S()))
    torch.cuda.synchronize()
    got = dlin.cpu().numpy()
    assert abs(float(metrics[5]) - 1.0) < 1e-6, 'ratio'
    assert rel_err(got[:, :2 * A], dclone[:, :2 * A]) < TOL
    assert rel_err(got[:, 2 * A:], dclone[:, 2 * A:]) < TOL          # (aux_weight 1: the auxiliary columns agree as well)
