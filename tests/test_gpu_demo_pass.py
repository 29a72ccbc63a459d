"""Demonstration-augmented policy pass on the GPU (cdrl_learner_demo_forward_backward(_resample), include/cdrl.h):
the mixed loss in the place of the policy loss on the policy pass.  Bit-level identities against the policy pass, whole-pass
gradients against the float64 oracle model driven by the restatement's d(loss)/d(lin) (tests/demo_ref.py) at the project's
whole-pass tolerance of 1e-4 (tests/util.check3, the engine's discrete decisions pinned)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from carla_driving_rl_agent_amd import _lib
from carla_driving_rl_agent_amd import engine as E
from carla_driving_rl_agent_amd.engine import LearnerEngine
from tests import demo_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
B, H, W, A = 32, 48, 64, 2
DEMO_ROWS = 8
SENTINEL = 777.0
ARENAS = ('params', 'adam_m', 'adam_v')
TOL = 1e-4


def _engines(n, kinds=None, seed=4, **kw):
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    kinds = kinds or [{}] * n
    engs = [LearnerEngine(B, device=DEV, H=H, W=W, **kw, **k) for k in kinds]
    init_engine_parameters(engs[0], seed=seed)
    for e in engs[1:]:
        for name in ARENAS:
            getattr(e, name).copy_(getattr(engs[0], name))
    for e in engs:
        e.set_hparams(entropy_coef=0.01)
    return engs


def _host_batch(seed=21):
    """A faithful policy batch (stored u with injected Jacobians) whose rows 3, 7, ... 31 are demonstration rows."""
    from tests.util import make_batches
    pol, _ = make_batches(B, H, W, seed=seed, A=A)
    rng = np.random.default_rng(seed + 11)
    demo_w = np.zeros(B, np.float32)
    demo_w[3::4] = rng.uniform(0.2, 1.5, DEMO_ROWS).astype(np.float32)
    demo_u = np.clip(rng.beta(2, 2, (B, A)), 1e-3, 1 - 1e-3).astype(np.float32)
    demo_u[3, 0], demo_u[7, 1] = 0.0, 1.0
    return dict(pol, demo_u=demo_u, demo_w=demo_w)


def _batch(seed=21):
    from tests.util import to_dev
    return to_dev(_host_batch(seed))


def _slice(eng, model, trainable=True):
    o, n = eng.region(model, trainable)
    return slice(o, o + n)


_PASSES = {}


def _passes():
    """D (demo pass), Z (demo pass with demo_w = 0), P (policy pass), ZR / PR (the re-sampled pair at one seed and offset): one pass
    each on the same parameters; computed once."""
    if not _PASSES:
        d, z, p, zr, pr = _engines(5)
        b = _batch()
        zero = dict(b, demo_w=torch.zeros_like(b['demo_w']))
        d.demo_forward_backward(b)
        z.demo_forward_backward(zero)
        p.policy_forward_backward(b)
        zr.demo_forward_backward_resample(zero, seed=9, offset=5)
        pr.policy_forward_backward_resample(b, seed=9, offset=5)
        torch.cuda.synchronize()
        _PASSES.update(d=d, z=z, p=p, zr=zr, pr=pr)
    return _PASSES


def test_forward_is_the_policy_pass_forward():
    f = _passes()
    assert torch.equal(f['d'].buffer(_lib.BUF_LIN_P), f['p'].buffer(_lib.BUF_LIN_P))
    st = _slice(f['d'], 'trunk', False)
    assert torch.equal(f['d'].params[st], f['p'].params[st]), 'trunk moving statistics'
    assert not torch.equal(f['d'].grads[_slice(f['d'], 'policy')], f['p'].grads[_slice(f['p'], 'policy')])   # (another loss)
    m = f['d'].metrics('demo')
    assert m['demo_rows'] == DEMO_ROWS and m['demo_loss'] != 0.0


@pytest.mark.parametrize('pair', [('z', 'p'), ('zr', 'pr')], ids=['stored', 'resampled'])
def test_zero_weights_give_the_policy_pass_bits(pair):
    f = _passes()
    z, p = f[pair[0]], f[pair[1]]
    for m in ('policy', 'trunk'):
        assert float(p.grads[_slice(p, m)].abs().max()) > 0.0
        assert torch.equal(z.grads[_slice(z, m)], p.grads[_slice(p, m)]), m
    assert torch.equal(z.buffer(_lib.BUF_METRICS_P)[:7], p.buffer(_lib.BUF_METRICS_P)[:7])
    assert torch.equal(z.buffer(_lib.BUF_AUX_P), p.buffer(_lib.BUF_AUX_P))
    if pair[0] == 'zr':
        assert torch.equal(z.named_buffer('sample.u'), p.named_buffer('sample.u')), 'same Philox offsets'


def _oracle_grads(learner, batch, decisions):
    """The demonstration pass on an OracleLearner: its own linear head outputs, the restatement's d(loss)/d(lin) on them (float64
    numpy), pulled back through the model by autograd."""
    from oracle import model as OM
    OM.DEC.items = decisions
    OM.DEC.start('replay')
    try:
        b = learner._cast({k: v for k, v in batch.items() if k == 'states'})
        d = OM.dynamics_forward(b['states'], learner.trunk, learner.cfg, training=True)
        p = learner.policy
        h = OM.control_branch(d, p, 'pi', True)
        lin = torch.cat([h @ p[f'pi.{k}.w'] + p[f'pi.{k}.b'] for k in ('alpha', 'beta', 'similarity', 'speed')], dim=1)
        assert OM.DEC.cursor == len(OM.DEC.items)
    finally:
        OM.DEC.start('off')
    ref = demo_ref.mixed_loss(lin.detach().double().numpy(), batch['advantages'], batch['old_log_prob'], batch['speed'],
                              batch['similarity'], batch['u'], batch['demo_u'], batch['demo_w'], learner.hp['clip_ratio'],
                              learner.hp['entropy_coef'], batch['du_da'], batch['du_db'])
    pulled = (lin * torch.as_tensor(ref['dlin']).to(lin.dtype)).sum()
    return ref, learner._grads(pulled, learner.policy, learner.pspec), learner._grads(pulled, learner.trunk, learner.tspec)


def test_gradients_match_the_float64_restatement():
    from tests.util import check3, engine_decisions, is_zero_gradient, make_pair, to_dev
    oracle, eng = make_pair(B, H, W, seed=3, A=A, with64=True)
    batch = _host_batch(seed=3)
    demo = batch['demo_w'] > 0
    poisoned = dict(batch)
    for k in ('advantages', 'old_log_prob', 'u', 'du_da', 'du_db'):       # a demonstration row's PPO inputs are never read
        poisoned[k] = batch[k].copy()
        poisoned[k][demo] = np.nan
    eng.demo_forward_backward(to_dev(poisoned))
    torch.cuda.synchronize()
    decisions = engine_decisions(eng, oracle.cfg)
    ref64, gp64, gt64 = _oracle_grads(oracle.o64, batch, decisions)
    _, gp32, gt32 = _oracle_grads(oracle, batch, decisions)
    ppo = ref64['passes'][~demo]
    assert ppo.any() and not ppo.all(), 'the minimum is routed both ways among the PPO rows'
    m = eng.buffer(_lib.BUF_METRICS_P).cpu().numpy()
    for k, r in enumerate(ref64['metrics']):
        assert abs(float(m[k]) - r) < TOL * max(1.0, abs(r)), (k, float(m[k]), r)
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
        print(f'[demo pass] {model}: worst gradient error {err:.3e} on {name} (bound {bound:.3e})')


def test_frozen_trunk_writes_no_trunk_gradient():
    full, frozen = _engines(2, kinds=[{}, dict(freeze_trunk=True)])
    b = _batch()
    t = _slice(frozen, 'trunk')
    frozen.grads.zero_()
    frozen.grads[t] = SENTINEL
    for e in (full, frozen):
        e.demo_forward_backward(b)
    torch.cuda.synchronize()
    assert bool((frozen.grads[t] == SENTINEL).all()), 'frozen demonstration pass wrote the trunk gradient slice'
    assert torch.equal(full.grads[_slice(full, 'policy')], frozen.grads[_slice(frozen, 'policy')])


def _three_steps(**kw):
    """Three demonstration steps (pass + policy_apply) on one engine with a demonstration block; the gradients of the first pass
    and of a repeated pass on the final parameters ride along."""
    from carla_driving_rl_agent_amd.init import init_engine_parameters
    eng = LearnerEngine(B, device=DEV, H=H, W=W, **kw)
    init_engine_parameters(eng, seed=2)
    eng.set_hparams(entropy_coef=0.01)
    block = E.demo_block(DEV)
    eng.set_demo_block(block)
    b = eng.stage(_batch(seed=8), 'demo')
    eng.demo_forward_backward(b)
    first = eng.grads.clone()
    eng.demo_forward_backward(b)
    second = eng.grads.clone()
    for _ in range(3):
        eng.demo_step(b)
    torch.cuda.synchronize()
    return eng, dict(first=first.cpu(), second=second.cpu(), params=eng.params.cpu(), m=eng.adam_m.cpu(), v=eng.adam_v.cpu(),
                     block=E.read_demo_block(block), metrics=eng.buffer(_lib.BUF_METRICS_P).cpu())


def _graph_worker(rank, out):
    sys.path.insert(0, ROOT)
    os.environ['CDRL_GRAPH'] = '1'
    torch.cuda.set_device(0)
    eng, res = _three_steps()
    assert eng.lib.cdrl_learner_tail_offset(eng.h) == eng.region('trunk', True)[1]     # graphs are on in this process
    torch.save(res, os.path.join(out, 'demo.pt'))


def test_replayed_graph_passes_equal_the_first_pass(tmp_path):
    mp.spawn(_graph_worker, args=(str(tmp_path),), nprocs=1, join=True)
    g = torch.load(tmp_path / 'demo.pt')
    _, e = _three_steps()
    # (the moving statistics moved between the two passes; train-mode gradients do not read them)
    assert torch.equal(g['first'], g['second']), 'the replayed pass repeats the captured one'
    assert g['block'] == e['block'] and g['block']['passes'] == 5 and g['block']['rows_sum'] == 5 * DEMO_ROWS
    for k in ('first', 'params', 'm', 'v', 'metrics'):
        assert torch.equal(g[k], e[k]), k


def test_guard_bands_stay_intact(monkeypatch):
    _, plain = _three_steps()
    monkeypatch.setenv('CDRL_GUARD', '1')
    eng, guarded = _three_steps()
    assert eng.check_guards() == (0, -1)
    assert torch.isfinite(eng.params).all()
    for k in ('params', 'm', 'v'):
        assert torch.equal(plain[k], guarded[k]), k


def test_malformed_batches_are_refused():
    (e,) = _engines(1)
    b = _batch()
    bad = [dict(b, demo_u=None), dict(b, demo_w=None), dict(b, demo_u=b['demo_u'][:, :1].contiguous()), dict(b, demo_u=b['demo_u'].double()),
           dict(b, demo_w=b['demo_w'].cpu()), dict(b, demo_w=b['demo_w'][:-1].contiguous()),
           dict(b, anchor=torch.ones((B, 2, A), device=DEV)), dict(b, advantages=b['advantages'][:-1].contiguous()),
           dict(b, states=dict(b['states'], state_road=b['states']['state_road'][:-1].contiguous()))]
    before = e.grads.clone()
    for k, x in enumerate(bad):
        for call in (e.demo_forward_backward, lambda y: e.demo_forward_backward_resample(y, seed=1, offset=0)):
            with pytest.raises(ValueError):
                call(x)
        assert torch.equal(before, e.grads), k
    with pytest.raises(ValueError, match='float64'):
        e.set_demo_block(torch.zeros(5, device=DEV))
    # the C entries on their own: what the Python checks let through as absent
    pb = e._policy_batch(b)
    for args, word in (((None, _lib.ptr(b['demo_w'])), 'demo_u'), ((_lib.ptr(b['demo_u']), None), 'demo_w')):
        with pytest.raises(_lib.CdrlError, match=word):
            _lib.check(e.lib.cdrl_learner_demo_forward_backward(e.h, C.byref(pb), *args, 1.0, None), 'demo')
        with pytest.raises(_lib.CdrlError, match=word):
            _lib.check(e.lib.cdrl_learner_demo_forward_backward_resample(e.h, C.byref(pb), *args, 1, 0, 1.0, None), 'demo')
    anchored = e._policy_batch(dict(b, anchor=torch.ones((B, 2, A), device=DEV)))
    with pytest.raises(_lib.CdrlError, match='anchor'):
        _lib.check(e.lib.cdrl_learner_demo_forward_backward(e.h, C.byref(anchored), _lib.ptr(b['demo_u']), _lib.ptr(b['demo_w']), 1.0, None))
    with pytest.raises(_lib.CdrlError, match='null'):
        _lib.check(e.lib.cdrl_learner_demo_forward_backward(e.h, None, _lib.ptr(b['demo_u']), _lib.ptr(b['demo_w']), 1.0, None))
    torch.cuda.synchronize()
    assert torch.equal(before, e.grads)


def test_pass_without_an_anchor_clears_the_trust_latch():
    (e,) = _engines(1, trust=True)
    b = _batch()
    e.policy_forward_backward(dict(b, anchor=torch.full((B, 2, A), 2.0, device=DEV)))
    assert e.trust_stats()['armed'] == 1
    e.demo_forward_backward(b)
    assert e.trust_stats()['armed'] == 0
