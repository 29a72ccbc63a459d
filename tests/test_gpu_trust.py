"""Trust-region guard of the policy steps on the GPU (cdrl_config.trust, cdrl_beta_kl; include/cdrl.h).

1. The KL kernel as an op (engine.beta_kl) against its float64 restatement (tests/trust_ref.py) at the project's loss-kernel
   tolerance of 1e-5, applied as tests/test_gpu_clone_loss.py applies it.  Shapes: the row-loop boundaries of the 256-thread workgroup
   (1, 3, 255, 256, 257, 700 rows) times the action bounds (1, 2, 8).
2. The learner: a guard that never fires leaves the bits of a learner without it; the latch skips policy_apply as skip_nonfinite
   skips, and nothing else; the penalty's gradient; the re-sampled pass; the refusals; graph replay of the guarded forms.
3. The agent: target_kl that never fires trains the default agent's bits; one below the BatchNorm-mode floor stops the policy steps."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from carla_driving_rl_agent_amd import _lib
from carla_driving_rl_agent_amd.engine import LearnerEngine, beta_kl
from tests import trust_ref
from tests.test_gpu_grad_gate import _agent, _summary
from tests.test_gpu_optimizers import B, H, W, _engine, _hp
from tests.util import make_batches, rel_err, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
TOL = 1e-5
EPS32 = float(np.finfo(np.float32).eps)
SENTINEL = 777.0
GUARD_ROWS = 4
ROWS = (1, 3, 255, 256, 257, 700)
ACTIONS = (1, 2, 8)


# ---------------------------------------------------------------------------------------------------------------- 1. the op
def _inputs(rows, A):
    rng = np.random.default_rng(1000 * rows + A)
    lin = (rng.standard_normal((rows, 2 * A + 2)) * 1.5).astype(np.float32)
    anchor = np.exp(rng.uniform(np.log(1.01), np.log(60.0), (rows, 2, A))).astype(np.float32)
    anchor.reshape(-1)[0] = 1.01                                          # the head's lower bound
    return lin, anchor


def _launch(lin, anchor, kl_coef, gs=1.0, base=None):
    """-> (dlin rows as the kernel left them, metrics[:3]); guard rows behind dlin and the slots behind metrics[2] stay intact."""
    rows, L = lin.shape
    dlin = torch.full((rows + GUARD_ROWS, L), SENTINEL, device=DEV)
    if base is not None:
        dlin[:rows] = torch.as_tensor(base).to(DEV)
    metrics = torch.full((16,), SENTINEL, device=DEV)
    beta_kl(torch.as_tensor(lin).to(DEV), torch.as_tensor(anchor).to(DEV), kl_coef, gs, dlin[:rows], metrics[:3])
    torch.cuda.synchronize()
    assert bool((dlin[rows:] == SENTINEL).all()), 'rows behind dlin were written'
    assert bool((metrics[3:] == SENTINEL).all()), 'metric slots behind [2] were written'
    return dlin[:rows].cpu().numpy(), metrics[:3].cpu().numpy()


@pytest.mark.parametrize('A', ACTIONS)
@pytest.mark.parametrize('rows', ROWS)
def test_kl_matches_float64(rows, A):
    lin, anchor = _inputs(rows, A)
    ref = trust_ref.kl_from_lin(lin, anchor)
    assert ref['kl'] > 0.0
    # kl_coef = 0: the metrics, and a sentinel-filled dlin that keeps its bits
    dlin, metrics = _launch(lin, anchor, 0.0)
    assert bool((dlin == SENTINEL).all()), 'kl_coef = 0 touched dlin'
    worst = 0.0
    for k in range(3):
        e = abs(float(metrics[k]) - ref['metrics'][k]) / max(1.0, abs(ref['metrics'][k]))
        worst = max(worst, e)
        assert e < TOL, (k, float(metrics[k]), ref['metrics'][k])
    m_none = beta_kl(torch.as_tensor(lin).to(DEV), torch.as_tensor(anchor).to(DEV))         # (no dlin at all)
    assert np.array_equal(m_none.cpu().numpy(), metrics)
    # kl_coef > 0 onto zeros: the gradient itself, one rounding per element
    zeros = np.zeros_like(lin)
    grads = {}
    for c, gs in ((1.0, 1.0), (0.37, 1.0), (1.0, 0.25)):
        got, m = _launch(lin, anchor, c, gs, base=zeros)
        assert np.array_equal(m, metrics), 'the coefficient changed the metrics'
        e = rel_err(got, c * gs * ref['dlin'])
        assert e < TOL, ('dlin', c, gs, e)
        assert not got[:, 2 * A:].any(), 'the similarity / speed columns carry no KL'
        grads[(c, gs)] = got
    # c times what kl_coef = 1 adds, to float rounding (the product c * gradient is rounded once in either order)
    d1, dc = grads[(1.0, 1.0)].astype(np.float64), grads[(0.37, 1.0)].astype(np.float64)
    assert (np.abs(dc - 0.37 * d1) <= 2.0 * EPS32 * np.abs(0.37 * d1) + 1e-45).all()
    # accumulation onto what a loss left there: float32(base + term)
    base = (np.random.default_rng(rows + A).standard_normal(lin.shape) * 0.1).astype(np.float32)
    got, _ = _launch(lin, anchor, 0.37, 1.0, base=base)
    exact = base.astype(np.float64) + 0.37 * ref['dlin']
    assert (np.abs(got - exact) <= TOL * np.abs(0.37 * ref['dlin']).max() + EPS32 * np.abs(exact)).all()
    assert np.array_equal(got[:, 2 * A:], base[:, 2 * A:])
    print(f'[beta kl rows={rows} A={A}] kl {ref["kl"]:.4g}, worst metric error {worst:.2e}, dlin {rel_err(grads[(1.0, 1.0)], ref["dlin"]):.2e}')


@pytest.mark.parametrize('rows,A', [(3, 1), (257, 2), (700, 8)])
def test_anchor_equal_to_the_policy_gives_zero(rows, A):
    lin, _ = _inputs(rows, A)
    a, b = trust_ref.head_alpha_beta(lin)
    anchor = np.stack([a, b], axis=1).astype(np.float32)          # the float32 (alpha, beta) an inference forward would hand over
    _, metrics = _launch(lin, anchor, 0.0)
    assert 0.0 <= float(metrics[0]) < 1e-6 and float(metrics[2]) <= float(metrics[0])
    assert abs(float(metrics[1])) < 1e-6


@pytest.mark.parametrize('rows,A', [(1, 1), (257, 2)])
def test_nan_anchor_gives_nan(rows, A):
    lin, anchor = _inputs(rows, A)
    anchor[rows // 2, 1, A - 1] = np.nan
    _, metrics = _launch(lin, anchor, 0.0)
    assert np.isnan(metrics).all(), metrics


def test_more_than_eight_actions_are_refused():
    lin, anchor = _inputs(4, 9)
    dlin = torch.zeros((4, 20), device=DEV)
    with pytest.raises(_lib.CdrlError, match='num_actions'):
        beta_kl(torch.as_tensor(lin).to(DEV), torch.as_tensor(anchor).to(DEV), 1.0, 1.0, dlin)
    with pytest.raises(_lib.CdrlError, match='kl_coef'):
        beta_kl(torch.as_tensor(lin[:, :6]).contiguous().to(DEV), torch.as_tensor(anchor[:, :, :2]).contiguous().to(DEV), -1.0, 1.0,
                dlin[:, :6].contiguous())
    torch.cuda.synchronize()
    assert not dlin.any()


# ---------------------------------------------------------------------------------------------------------------- 2. the learner
_BATCH = {}


def _batches():
    if not _BATCH:
        pol, val = make_batches(B, H, W, seed=21, faithful=False)
        _BATCH['pol'], _BATCH['val'] = to_dev(pol), to_dev(val)
    return _BATCH['pol'], _BATCH['val']


def _anchor(value):
    return torch.full((B, 2, 2), float(value), device=DEV)


def _state(eng):
    torch.cuda.synchronize()
    return dict(params=eng.params.clone(), m=eng.adam_m.clone(), v=eng.adam_v.clone(), hp=_hp(eng))


def _same(a, b, what):
    for k in ('params', 'm', 'v'):
        assert torch.equal(a[k], b[k]), (what, k)
    assert a['hp'] == b['hp'], (what, a['hp'], b['hp'])


def _sequence(eng, anchor):
    """Passes and applies of both heads, stored-action and re-sampled; anchor None: the batches of a learner without the guard."""
    pol, val = _batches()
    if anchor is not None:
        pol = dict(pol, anchor=anchor)
    for k in range(2):
        # (set_hparams stages its block in ONE pinned buffer per learner: the upload in front must have run before the next is staged)
        torch.cuda.synchronize()
        eng.set_hparams(policy_lr=3e-4 * (k + 1), value_lr=1e-3, dynamics_lr=5e-4)
        eng.policy_forward_backward(pol)
        eng.policy_apply()
        eng.value_forward_backward(val)
        eng.value_apply()
    eng.policy_forward_backward_resample(pol, seed=5, offset=2)
    eng.policy_apply()


@pytest.mark.parametrize('kw', [dict(), dict(optimizer='nadam', polyak=0.9)], ids=['adam', 'nadam-polyak'])
def test_a_guard_that_never_fires_leaves_the_bits(kw):
    plain, guarded = _engine(**kw), _engine(trust=True, **kw)
    guarded.set_hparams(target_kl=1e30, kl_coef=0.0)
    _sequence(plain, None)
    _sequence(guarded, _anchor(3.0))
    _same(_state(guarded), _state(plain), 'never firing')
    assert _hp(plain)[0] == [3, 2, 5]
    st = guarded.trust_stats()
    assert (st['passes'], st['stop'], st['stop_pass'], st['skipped'], st['armed']) == (3, 0, -1, 0, 1)
    assert st['kl_last'] > 0.0 and st['kl_max'] >= st['kl_last'] and abs(st['kl_sum'] - 3 * st['kl_last']) < st['kl_sum']
    assert st['target_kl'] == np.float32(1e30) and st['kl_stop_factor'] == 1.5 and st['kl_coef'] == 0.0


def test_latch_skips_the_policy_apply_and_nothing_else():
    eng = _engine(trust=True)
    eng.set_hparams(target_kl=1e-3)
    pol, val = _batches()
    eng.policy_forward_backward(dict(pol, anchor=_anchor(50.0)))
    st = eng.trust_stats()
    assert (st['stop'], st['stop_pass'], st['armed'], st['passes'], st['skipped']) == (1, 0, 1, 1, 0)
    assert st['kl_last'] > 1.5e-3 and st['kl_last'] == st['kl_max'] and abs(st['kl_sum'] - st['kl_last']) <= 1e-6 * st['kl_last']
    snap = _state(eng)                  # behind the pass: its forward moved the BatchNorm moving statistics, the apply may move nothing
    eng.policy_apply()
    _same(_state(eng), snap, 'latched policy_apply')         # policy, old_policy, trunk, every slot, counters, m_caches
    assert eng.trust_stats()['skipped'] == 1
    # the value step is not the latch's business
    eng.value_forward_backward(val)
    eng.value_apply()
    after = _state(eng)
    for model in ('value', 'trunk'):
        o, n = eng.region(model, True)
        assert not torch.equal(after['params'][o:o + n], snap['params'][o:o + n]), model
    assert after['hp'][0] == [0, 1, 1]
    o, n = eng.region('policy', True)
    assert torch.equal(after['params'][o:o + n], snap['params'][o:o + n])
    # a pass without an anchor is not gated by the old latch
    eng.policy_forward_backward(pol)
    eng.policy_apply()
    st = eng.trust_stats()
    assert (st['stop'], st['armed'], st['skipped'], st['passes']) == (1, 0, 1, 1)
    assert _hp(eng)[0] == [1, 1, 2]
    assert not torch.equal(eng.params[o:o + n], snap['params'][o:o + n])
    # ... and a second measured pass is gated again, without moving stop_pass
    eng.policy_forward_backward(dict(pol, anchor=_anchor(50.0)))
    eng.policy_apply()
    st = eng.trust_stats()
    assert (st['stop'], st['stop_pass'], st['armed'], st['skipped'], st['passes']) == (1, 0, 1, 2, 2) and _hp(eng)[0] == [1, 1, 2]
    # one block for the engines that share the optimizer
    shared = LearnerEngine(2, device=DEV, share_with=eng, H=H, W=W)
    assert shared.trust and shared.trust_stats() == st
    shared.trust_reset()
    st = eng.trust_stats()
    assert (st['stop'], st['stop_pass'], st['armed'], st['skipped'], st['passes'], st['kl_sum'], st['kl_max']) == (0, -1, 0, 0, 0, 0.0, 0.0)
    assert st['target_kl'] == np.float32(1e-3)                # the host's head stays
    eng.policy_forward_backward(dict(pol, anchor=_anchor(50.0)))
    assert eng.trust_stats()['stop_pass'] == 0


def test_nan_anchor_latches():
    eng = _engine(trust=True)
    eng.set_hparams(target_kl=1e30)
    pol, _ = _batches()
    anchor = _anchor(3.0)
    anchor[1, 0, 0] = float('nan')
    eng.policy_forward_backward(dict(pol, anchor=anchor))
    snap = _state(eng)
    eng.policy_apply()
    _same(_state(eng), snap, 'NaN KL')
    st = eng.trust_stats()
    assert np.isnan(st['kl_last']) and st['stop'] == 1 and st['skipped'] == 1


def test_penalty_adds_its_gradient_behind_the_policy_loss():
    eng = _engine(trust=True)
    pol, _ = _batches()
    batch = dict(pol, anchor=_anchor(50.0))
    L = 2 * 2 + 2
    o, n = eng.region('policy', True)

    def run(c):
        eng.set_hparams(kl_coef=c)
        eng.policy_forward_backward(batch)          # (no apply in between: the same weights, the same train-mode forward)
        torch.cuda.synchronize()
        return (eng.named_buffer('policy.lin.g', shape=(B, L)).cpu().numpy().astype(np.float64),
                eng.grads[o:o + n].cpu().numpy().astype(np.float64), eng.buffer(_lib.BUF_LIN_P, (B, L)).cpu().numpy())

    c = 0.5
    g0, h0, lin0 = run(0.0)
    g1, h1, lin1 = run(c)
    g2, h2, _ = run(2 * c)
    assert np.array_equal(lin0, lin1)
    ref = c * trust_ref.kl_from_lin(lin0, batch['anchor'].cpu().numpy())['dlin']
    assert np.abs(ref).max() > 0.0
    # g1 = float32(g0 + term): the difference is the term up to half an ulp of the sum
    assert (np.abs((g1 - g0) - ref) <= TOL * np.abs(ref).max() + EPS32 * np.abs(g1)).all()
    assert np.array_equal(g1[:, 4:], g0[:, 4:])
    # pushed through the head: its backward is linear in dlin, so twice the coefficient adds twice as much to every head gradient
    d1, d2 = h1 - h0, h2 - h0
    assert np.abs(d1).max() > 0.0 and rel_err(d2, 2.0 * d1) < 1e-4, rel_err(d2, 2.0 * d1)


def test_resampled_pass_measures_the_same_kl():
    eng = _engine(trust=True)
    pol, _ = _batches()
    batch = dict(pol, anchor=_anchor(2.5))
    eng.policy_forward_backward(batch)
    stored = eng.trust_stats()
    eng.policy_forward_backward_resample(batch, seed=9, offset=4)
    again = eng.trust_stats()
    assert again['passes'] == 2 and again['kl_last'] == stored['kl_last'] > 0.0 and again['stop'] == 0
    lin = eng.buffer(_lib.BUF_LIN_P, (B, 6)).cpu().numpy()
    ref = trust_ref.kl_from_lin(lin, batch['anchor'].cpu().numpy())['kl']
    assert abs(stored['kl_last'] - ref) < TOL * max(1.0, ref)


def test_refusals():
    pol, val = _batches()
    plain, guarded = _engine(), _engine(trust=True)
    snap = _state(plain)
    with pytest.raises(_lib.CdrlError, match='trust'):
        plain.policy_forward_backward(dict(pol, anchor=_anchor(2.0)))
    with pytest.raises(_lib.CdrlError, match='trust'):
        plain.policy_forward_backward_resample(dict(pol, anchor=_anchor(2.0)), seed=1, offset=1)
    _same(_state(plain), snap, 'refused pass')
    for call in (plain.trust_stats, plain.trust_reset):
        with pytest.raises(_lib.CdrlError, match='trust'):
            call()
    with pytest.raises(_lib.CdrlError, match='trust'):
        plain.set_hparams(target_kl=0.01)
    snap = _state(guarded)
    joint = dict(pol, returns=val['returns'])
    with pytest.raises(_lib.CdrlError, match='trust'):
        guarded.joint_forward_backward(joint)
    with pytest.raises(_lib.CdrlError, match='trust'):
        guarded.joint_forward_backward_resample(joint, seed=1, offset=1)
    with pytest.raises(_lib.CdrlError, match='trust'):
        guarded.joint_apply()
    _same(_state(guarded), snap, 'refused joint')
    with pytest.raises(_lib.CdrlError, match='trust differs'):
        LearnerEngine(2, device=DEV, share_with=guarded, H=H, W=W, trust=False)
    with pytest.raises(_lib.CdrlError, match='trust differs'):
        LearnerEngine(2, device=DEV, share_with=plain, H=H, W=W, trust=True)
    with pytest.raises(_lib.CdrlError, match='kl_stop_factor'):
        guarded.set_hparams(kl_stop_factor=0.0)
    guarded.hp['kl_stop_factor'] = 1.5
    with pytest.raises(ValueError, match='anchor'):
        guarded.policy_forward_backward(dict(pol, anchor=torch.ones((B, 2, 3), device=DEV)))


def _graph_run(eng):
    """Measured passes that stay inside the region, one that leaves it, the value step, one more measured pass: the second
    stored-action pass and every apply behind the first of its kind replay a captured graph when graphs are on."""
    eng.set_hparams(target_kl=0.6)          # the stop at 0.9: above the KL to the near anchor (about 0.4), below the far one's (above 2)
    pol, val = _batches()
    near, far = dict(pol, anchor=_anchor(3.0)), dict(pol, anchor=_anchor(50.0))
    for batch in (near, near, far):
        eng.policy_forward_backward(batch)
        eng.policy_apply()
    eng.value_forward_backward(val)
    eng.value_apply()
    eng.policy_forward_backward(near)
    eng.policy_apply()
    st = _state(eng)
    return dict(params=st['params'].cpu(), m=st['m'].cpu(), v=st['v'].cpu(), hp=st['hp'], trust=eng.trust_stats())


def _graph_worker(rank, out):
    sys.path.insert(0, ROOT)
    os.environ['CDRL_GRAPH'] = '1'
    torch.cuda.set_device(0)
    eng = _engine(trust=True)
    assert eng.lib.cdrl_learner_tail_offset(eng.h) == eng.region('trunk', True)[1]     # graphs are on in this process
    torch.save(_graph_run(eng), os.path.join(out, 'trust.pt'))


def test_guarded_passes_and_applies_replay_from_a_graph(tmp_path):
    mp.spawn(_graph_worker, args=(str(tmp_path),), nprocs=1, join=True)
    g = torch.load(tmp_path / 'trust.pt')
    e = _graph_run(_engine(trust=True))
    assert (e['trust']['stop'], e['trust']['stop_pass'], e['trust']['skipped'], e['trust']['passes']) == (1, 2, 2, 4)
    assert e['hp'][0] == [2, 1, 3]
    assert g['trust'] == e['trust'] and g['hp'] == e['hp']
    assert torch.equal(g['params'], e['params']) and torch.equal(g['m'], e['m']) and torch.equal(g['v'], e['v'])


def test_guard_bands_stay_intact(monkeypatch):
    monkeypatch.setenv('CDRL_GUARD', '1')
    eng = _engine(trust=True)
    eng.set_hparams(target_kl=1e30, kl_coef=0.3)
    _sequence(eng, _anchor(4.0))
    eng.trust_reset()
    assert eng.trust_stats()['passes'] == 0
    assert eng.check_guards() == (0, -1)


# ---------------------------------------------------------------------------------------------------------------- 3. the agent
@pytest.mark.parametrize('resample', [True, False])
def test_agent_with_a_guard_that_never_fires_trains_the_same_bits(tmp_path, monkeypatch, resample):
    monkeypatch.chdir(tmp_path)
    out = []
    for name, kw in (('plain', {}), ('guarded', dict(target_kl=1e30))):
        agent = _agent(tmp_path / name, resample_actions=resample, log_mode=None, **kw)
        agent.learn(episodes=1, timesteps=17, close=False)
        eng = agent.network.engine
        assert eng.trust == bool(kw)
        out.append((_state(eng), agent._sample_offset, agent.network.action_index, agent))
    _same(out[1][0], out[0][0], 'agent')
    assert out[1][1:3] == out[0][1:3]
    assert out[0][0]['hp'][0][0] == 4
    st = out[1][3].network.engine.trust_stats()
    assert (st['passes'], st['stop'], st['skipped']) == (4, 0, 0) and st['kl_last'] > 0.0


def test_agent_stops_the_policy_steps_below_the_floor(tmp_path, monkeypatch):
    from carla_driving_rl_agent_amd.core import CARLAgent
    monkeypatch.chdir(tmp_path)

    class Counting(CARLAgent):
        passes = 0

        def get_policy_gradients(self, batch):
            self.passes += 1
            return super().get_policy_gradients(batch)

    # below the floor that the BatchNorm modes put between the acting and the training forward: the first minibatch latches
    agent = _agent(tmp_path, cls=Counting, target_kl=1e-12, optimization_steps=(3, 1))
    eng = agent.network.engine
    before = _state(eng)
    agent.learn(episodes=1, timesteps=17, close=False)
    after = _state(eng)
    o, n = eng.region('policy', True)
    assert torch.equal(after['params'][o:o + n], before['params'][o:o + n])
    assert after['hp'][0] == [0, 2, 2]                       # no policy step, two value steps, the trunk stepped with the value head
    o, n = eng.region('value', True)
    assert not torch.equal(after['params'][o:o + n], before['params'][o:o + n])
    assert agent.passes == 2                                  # the two minibatches of the first epoch; epochs two and three were not run
    got = _summary(tmp_path)
    assert got['kl_divergence']['mean'] > 0.0 and got['kl_divergence_max']['mean'] >= got['kl_divergence']['mean']
    assert got['kl_stop_pass']['mean'] == 0 and got['kl_stopped_steps']['mean'] == 2
    st = eng.trust_stats()
    assert (st['stop'], st['stop_pass'], st['skipped'], st['passes']) == (1, 0, 2, 2)
    print(f'[trust] step-0 KL between the acting and the training forward at B = 8: {st["kl_sum"] / st["passes"]:.4g}')


def test_anchors_cover_the_kept_rows(tmp_path, monkeypatch):
    from carla_driving_rl_agent_amd.core import CARLAgent
    monkeypatch.chdir(tmp_path)

    class Watching(CARLAgent):
        seen = []

        def begin_trust_region(self):
            super().begin_trust_region()
            rows = self.with_replay(self.memory.advantages, 'advantages').shape[0]
            self.seen.append((tuple(self._trust_anchor.shape), rows, sum(p.rows for p in self._replay_active)))

    agent = _agent(tmp_path, cls=Watching, replay_rollouts=1, resample_actions=False, target_kl=1e30, log_mode=None)
    agent.learn(episodes=1, timesteps=17, close=False)
    agent.learn(episodes=1, timesteps=17, close=False)
    (shape0, rows0, kept0), (shape1, rows1, kept1) = agent.seen
    assert shape0 == (rows0, 2, 2) and kept0 == 0
    assert shape1 == (rows1, 2, 2) and kept1 > 0 and rows1 == rows0 + kept1
    assert torch.isfinite(agent.network.engine.params).all()
    st = agent.network.engine.trust_stats()
    assert st['stop'] == 0 and st['passes'] > 0 and agent._trust_anchor is None


def test_joint_update_is_refused(tmp_path):
    with pytest.raises(ValueError, match='joint_update'):
        _agent(tmp_path, target_kl=0.01, joint_update=True, optimization_steps=(1, 1))
