"""Mixed policy loss kernel on the GPU (cdrl_beta_mixed_policy_loss, include/cdrl.h) against its float64
restatement (tests/demo_ref.py) at the project's loss-kernel tolerance of 1e-5, and bit for bit against cdrl_beta_ppo_loss when no
row is a demonstration row.

Shapes: two small odd row counts, and 300 rows, which send the 256-thread row loop on a second trip."""
import ctypes as C

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from carla_driving_rl_agent_amd import engine as E
from tests import demo_ref
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-5
SENTINEL = 777.0
GUARD_ROWS = 4
SHAPES = [(5, 2), (7, 3), (300, 2)]
POSITIONS = ('none', 'all', 'first', 'last', 'alternating')
CLIP, ENT = 0.2, 0.7
F32_EPS = np.float32(np.finfo(np.float32).eps)
PPO_KEYS = ('lin', 'adv', 'old', 'spd', 'sim', 'u', 'ja', 'jb')


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(a):
    return torch.as_tensor(a).to(DEV).contiguous() if a is not None else None


def demo_weights(B, position):
    w = np.zeros(B, np.float32)
    rng = np.random.default_rng(B)
    if position == 'all':
        w[:] = rng.uniform(0.1, 2.0, B)
    elif position == 'first':
        w[0] = 0.3
    elif position == 'last':
        w[-1] = 1.7
    elif position == 'alternating':
        w[::2] = rng.uniform(0.1, 2.0, (B + 1) // 2)
    return w


def inputs(B, A, position, jac):
    """Actions with 0, 1 and the float32 epsilon exactly; per PPO row (index mod 4) advantage sign and the side of the clip band
    the ratio lies on cycle through the four combinations, so the surrogate's minimum takes both branches."""
    rng = np.random.default_rng(1000 * B + A)
    lin = (rng.standard_normal((B, 2 * A + 2)) * 1.5).astype(np.float32)
    u = np.clip(rng.beta(2, 2, (B, A)), 1e-4, 1 - 1e-4).astype(np.float32)
    du = np.clip(rng.beta(2, 2, (B, A)), 1e-4, 1 - 1e-4).astype(np.float32)
    for t in (u, du):
        for r in range(min(B, 6)):          # rows 0..5: 0, 1, eps, 0, 1, eps -- any four rows of one kind among them meet all three
            t[r, r % A] = (0.0, 1.0, F32_EPS)[r % 3]
    w = demo_weights(B, position)
    sign = np.where(np.arange(B) % 4 < 2, 1.0, -1.0)
    adv = (sign * rng.uniform(0.5, 1.5, B)).astype(np.float32)
    delta = np.where(np.arange(B) % 2 == 0, 0.5, -0.5)       # ratio e^0.5 above, e^-0.5 below the band [0.8, 1.2]
    spd = rng.uniform(0, 0.3, B).astype(np.float32)
    sim = rng.uniform(-1, 1, B).astype(np.float32)
    ja = rng.uniform(-0.3, 0.3, (B, A)).astype(np.float32) if jac else None
    jb = rng.uniform(-0.3, 0.3, (B, A)).astype(np.float32) if jac else None
    zeros = np.zeros(B, np.float32)
    logp = demo_ref.mixed_loss(lin, adv, np.zeros((B, A)), spd, sim, u, du, zeros, CLIP, ENT)['log_prob']
    old = (logp - delta[:, None]).astype(np.float32)
    return dict(lin=lin, adv=adv, old=old, spd=spd, sim=sim, u=u, ja=ja, jb=jb, du=du, w=w)


def reference(x):
    return demo_ref.mixed_loss(x['lin'], x['adv'], x['old'], x['spd'], x['sim'], x['u'], x['du'], x['w'], CLIP, ENT, x['ja'], x['jb'])


def launch(lib, x, gs=1.0, block=None, entry='mixed'):
    B, A = x['u'].shape
    dlin = torch.full((B + GUARD_ROWS, 2 * A + 2), SENTINEL, device=DEV)
    aux = torch.full((B + GUARD_ROWS, 4 * A), SENTINEL, device=DEV)
    metrics = torch.full((16,), SENTINEL, device=DEV)
    hp = torch.zeros(16, device=DEV)
    keep = [dev(x[k]) for k in PPO_KEYS]
    if entry == 'mixed':
        extra = [dev(x['du']), dev(x['w'])]
        _lib.check(lib.cdrl_beta_mixed_policy_loss(*[P(k) for k in keep + extra], CLIP, ENT, B, A, gs, P(dlin), P(metrics), P(aux), P(hp),
                                                   P(block), S()))
    else:
        _lib.check(lib.cdrl_beta_ppo_loss(*[P(k) for k in keep], CLIP, ENT, B, A, gs, P(dlin), P(metrics), P(aux), P(hp), S()))
    torch.cuda.synchronize()
    assert bool((dlin[B:] == SENTINEL).all()), 'rows behind dlin were written'
    assert bool((aux[B:] == SENTINEL).all()), 'rows behind aux were written'
    assert bool((metrics[11 if entry == 'mixed' else 7:] == SENTINEL).all()), 'metric slots behind the last one were written'
    return dlin[:B].cpu().numpy(), metrics.cpu().numpy(), aux[:B].cpu().numpy()


@pytest.mark.parametrize('jac', [False, True], ids=['stored', 'jacobians'])
@pytest.mark.parametrize('B,A', SHAPES)
def test_without_demonstration_rows_the_bits_are_the_policy_loss(lib, B, A, jac):
    x = inputs(B, A, 'none', jac)
    for gs in (1.0, 0.25):
        dm, mm, am = launch(lib, x, gs)
        dp, mp, ap = launch(lib, x, gs, entry='ppo')
        assert np.array_equal(dm.view(np.uint32), dp.view(np.uint32)), 'dlin'
        assert np.array_equal(mm[:7].view(np.uint32), mp[:7].view(np.uint32)), 'metrics 0..6'
        assert np.array_equal(am.view(np.uint32), ap.view(np.uint32)), 'aux'
        assert not mm[7:11].any(), 'no demonstration row: slots 7..10 are 0'


@pytest.mark.parametrize('jac', [False, True], ids=['stored', 'jacobians'])
@pytest.mark.parametrize('position', POSITIONS)
@pytest.mark.parametrize('B,A', SHAPES)
def test_matches_float64(lib, B, A, position, jac):
    x = inputs(B, A, position, jac)
    ref = reference(x)
    acts = np.where(ref['demo'][:, None], x['du'], x['u'])
    for kind in (ref['demo'], ~ref['demo']):
        if kind.sum() >= 4:
            assert {0.0, 1.0, float(F32_EPS)} <= set(acts[kind].reshape(-1).tolist()), 'the clip values are among the rows of this kind'
    if (~ref['demo']).sum() >= 4:
        ppo = ref['passes'][~ref['demo']]
        assert ppo.any() and not ppo.all(), 'the reference routes the minimum both ways among the PPO rows'
    for gs in (1.0, 0.25):
        dlin, metrics, aux = launch(lib, x, gs)
        e = rel_err(dlin, gs * ref['dlin'])
        print(f'[mixed loss B={B} A={A} {position} jac={jac} gs={gs}] dlin {e:.2e}')
        assert e < TOL, ('dlin', e)
        for k, r in enumerate(ref['metrics']):
            e = abs(float(metrics[k]) - r) / max(1.0, abs(r))
            assert e < TOL, (k, float(metrics[k]), r)
        assert metrics[10] == ref['demo'].sum()
        for i, k in enumerate(('alpha', 'beta', 'log_prob', 'entropy')):
            assert rel_err(aux[:, i * A:(i + 1) * A], ref[k]) < TOL, k


@pytest.mark.parametrize('B,A', SHAPES)
def test_demonstration_rows_ignore_their_ppo_inputs(lib, B, A):
    x = inputs(B, A, 'alternating', True)
    clean, mclean, _ = launch(lib, x)
    demo = x['w'] > 0
    y = {k: (v.copy() if v is not None else None) for k, v in x.items()}
    for k in ('adv', 'old', 'u', 'ja', 'jb'):
        y[k][demo] = np.nan
    got, mgot, _ = launch(lib, y)
    assert np.isfinite(got).all() and np.isfinite(mgot[:11]).all()
    assert np.array_equal(got.view(np.uint32), clean.view(np.uint32))
    assert np.array_equal(mgot[:11].view(np.uint32), mclean[:11].view(np.uint32))


def test_block_holds_the_sums_of_three_launches(lib):
    block = E.demo_block(DEV)
    want = np.zeros(4)
    for n, (shape, position) in enumerate((((5, 2), 'first'), ((300, 2), 'alternating'), ((7, 3), 'all'))):
        _, metrics, _ = launch(lib, inputs(*shape, position, False), block=block)
        want += metrics[7:11].astype(np.float64)
        st = E.read_demo_block(block)
        assert st['passes'] == n + 1
    got = [st[k] for k in ('loss_sum', 'log_prob_sum', 'mode_error_sum', 'rows_sum')]
    assert got == want.tolist(), (got, want)
    assert st['rows_sum'] == 1 + 150 + 7


def test_two_launches_give_the_same_bits(lib):
    x = inputs(300, 2, 'alternating', True)
    a, b = launch(lib, x), launch(lib, x)
    for s, t in zip(a, b):
        assert np.array_equal(s.view(np.uint32), t.view(np.uint32))


def test_refusals(lib):
    x = inputs(5, 2, 'first', False)
    B, A = 5, 2
    dlin, metrics, hp = torch.zeros((B, 2 * A + 2), device=DEV), torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)
    keep = [dev(x[k]) for k in PPO_KEYS] + [dev(x['du']), dev(x['w'])]

    def call(args=None, B=B, A=A, dlin=dlin, metrics=metrics):
        args = keep if args is None else args
        return lib.cdrl_beta_mixed_policy_loss(*[P(k) for k in args], CLIP, ENT, B, A, 1.0, P(dlin), P(metrics), None, P(hp), None, S())

    for kw, word in ((dict(A=0), 'num_actions'), (dict(A=9), 'num_actions'), (dict(B=0), 'B = 0'), (dict(dlin=None), 'null'),
                     (dict(metrics=None), 'null')):
        with pytest.raises(_lib.CdrlError, match=word):
            _lib.check(call(**kw))
    for i in (0, 5, 8, 9):          # lin, u, demo_u, demo_w
        args = list(keep)
        args[i] = None
        with pytest.raises(_lib.CdrlError, match='null'):
            _lib.check(call(args))
    torch.cuda.synchronize()
    assert not dlin.any() and not metrics.any(), 'a refused call writes nothing'
    _lib.check(call())
    torch.cuda.synchronize()
    assert dlin.any()
