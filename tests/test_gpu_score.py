"""cdrl_beta_score on the device (csrc/score.hip) through the C ABI against its numpy / float64 restatement
(tests/score_ref.py, scipy's betainc): every sum within 1e-9 of max(1, |reference|), every PIT entry within 1e-9 absolute, every
count exact -- on inputs whose reference PIT keeps 1e-6 away from every bin edge and coverage bound --, accumulation, the ignored
tail of a padded chunk, the iteration cap, non-finite parameters and the argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from carla_driving_rl_agent_amd.engine import SCORE_BINS, SCORE_LAYOUT, beta_score, score_block, score_block_size
from tests import score_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BOUND = 1e-9                # sums: of max(1, |reference|); PIT entries: absolute
EPS = score_ref.EPS
SENTINEL = -7.0             # no PIT is negative
HEAD, ACTION = SCORE_LAYOUT['head'], SCORE_LAYOUT['action']


def _dev(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dtype)


def _launch(dist, value, u, returns, speed, similarity, rows, count, A, block, pit):
    lib = _lib.load()
    torch.cuda.synchronize()
    return lib.cdrl_beta_score(_lib.ptr(dist), _lib.ptr(value), _lib.ptr(u), _lib.ptr(returns), _lib.ptr(speed), _lib.ptr(similarity),
                               rows, count, A, _lib.ptr(block), _lib.ptr(pit), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _draw(rows, A, hi, seed):
    """`rows` rows of inputs whose reference PIT is at least 1e-6 away from every edge: alpha, beta in [1.01, hi]; per element u
    drawn from the Beta itself (three in eight), uniformly (two), or exactly 0 / 1, eps, 1 - eps (one each).  More rows than needed
    are drawn and the ones with an element near an edge dropped; at most 1 % may go (expected: 13 edges x 2e-6 ~ 3e-5)."""
    rng = np.random.default_rng(seed)
    n = rows + 8
    alpha = rng.uniform(1.01, hi, (n, A)).astype(np.float32)
    beta = rng.uniform(1.01, hi, (n, A)).astype(np.float32)
    kind = (np.arange(n * A).reshape(n, A) + seed) % 8
    u = rng.beta(alpha.astype(np.float64), beta.astype(np.float64)).astype(np.float32)
    u = np.where((kind == 3) | (kind == 4), rng.uniform(0.0, 1.0, (n, A)).astype(np.float32), u)
    u = np.where(kind == 5, (np.arange(n)[:, None] % 2).astype(np.float32), u)          # exactly 0 and exactly 1
    u = np.where(kind == 6, EPS, u)
    u = np.where(kind == 7, np.float32(1.0) - EPS, u).astype(np.float32)
    near = score_ref.edge_distance(score_ref.pit(alpha, beta, u)) < 1e-6
    assert near.sum() <= 0.01 * near.size, f'{near.sum()} of {near.size} drawn elements lie within 1e-6 of an edge'
    index = np.flatnonzero(~near.any(axis=1))[:rows]
    assert index.shape[0] == rows
    value = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(0.0, 3.0, n), rng.uniform(0.0, 2.0, n), rng.uniform(-1.0, 1.0, n)],
                     axis=1).astype(np.float32)
    returns = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(0.0, 3.0, n)], axis=1).astype(np.float32)
    speed, similarity = rng.uniform(0.0, 2.0, n).astype(np.float32), rng.uniform(-1.0, 1.0, n).astype(np.float32)
    return tuple(x[index] for x in (alpha, beta, u, value, returns, speed, similarity))


def _dist(alpha, beta):
    """(rows, 4, A) as cdrl_learner_predict writes it; the mean and std columns hold a value no sum may pick up."""
    d = np.full((alpha.shape[0], 4, alpha.shape[1]), 1e30, np.float32)
    d[:, 0], d[:, 1] = alpha, beta
    return d


@pytest.fixture(scope='module')
def cases():
    """The drawn inputs and their reference blocks, computed once and shared."""
    out = {}
    for rows in (1, 7, 300):
        for A in (1, 2, 3):
            for hi in (5.0, 500.0):
                alpha, beta, u, value, returns, speed, similarity = _draw(rows, A, hi, seed=1000 * rows + 10 * A + int(hi))
                out[rows, A, hi] = dict(alpha=alpha, beta=beta, u=u, value=value, returns=returns, speed=speed, similarity=similarity,
                                        block=score_ref.block(alpha, beta, value, u, returns, speed, similarity),
                                        pit=score_ref.pit(alpha, beta, u))
    return out


def _run(c, lo=0, hi=None, block=None, pit=None, returns=True, aux=True, pad=0):
    """One launch over rows [lo, hi) of a case, `pad` more rows behind them in dist / value (copies of the last row)."""
    hi = c['alpha'].shape[0] if hi is None else hi
    A = c['alpha'].shape[1]
    index = np.minimum(np.arange(lo, hi + pad), hi - 1)
    dist, value = _dev(_dist(c['alpha'][index], c['beta'][index])), _dev(c['value'][index])
    block = score_block(A, DEV) if block is None else block
    beta_score(dist, value, _dev(c['u'][lo:hi]), _dev(c['returns'][lo:hi]) if returns else None, _dev(c['speed'][lo:hi]) if aux else None,
               _dev(c['similarity'][lo:hi]) if aux else None, count=hi - lo, block=block, pit=pit)
    return block


@pytest.mark.parametrize('hi', [5.0, 500.0])
@pytest.mark.parametrize('A', [1, 2, 3])
@pytest.mark.parametrize('rows', [1, 7, 300])
def test_block_and_pit_against_the_restatement(cases, rows, A, hi):
    c = cases[rows, A, hi]
    pit = torch.full((rows, A), SENTINEL, dtype=torch.float64, device=DEV)
    got = _run(c, pit=pit).cpu().numpy()
    exact, err = score_ref.compare(got, c['block'], A)
    e_pit = float(np.abs(pit.cpu().numpy() - c['pit']).max())
    print(f'score rows={rows} A={A} alpha, beta <= {hi:g}: worst sum error / max(1, |ref|) {err:.3e}, worst PIT error {e_pit:.3e}')
    assert exact, (got[score_ref.count_slots(A)], c['block'][score_ref.count_slots(A)])
    assert err < BOUND and e_pit < BOUND
    assert got[HEAD['rows']] == rows and got[HEAD['nonfinite']] == 0 and got[HEAD['pit_unconverged']] == 0
    again = _run(c).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))                   # the same rows: the same bits


@pytest.mark.parametrize('A', [1, 2, 3])
def test_count_below_rows_adds_to_a_filled_block(cases, A):
    """count < rows into a block that holds known values: prior + reference, and the rows behind `count` do not enter; the pit
    buffer is written in [0, count) and left alone behind."""
    c = cases[300, A, 500.0]
    prior = np.arange(score_block_size(A), dtype=np.float64) * 0.5 + 3.0
    block = _dev(prior, torch.float64)
    pit = torch.full((300 + 5, A), SENTINEL, dtype=torch.float64, device=DEV)
    lib_pit = pit[:290]                                                                 # (count, A): a view of the larger buffer
    got = _run(c, 0, 290, block=block, pit=lib_pit, pad=10).cpu().numpy()
    cut = {k: c[k][:290] for k in ('alpha', 'beta', 'value', 'u', 'returns', 'speed', 'similarity')}
    want = score_ref.block(cut['alpha'], cut['beta'], cut['value'], cut['u'], cut['returns'], cut['speed'], cut['similarity'], prior=prior)
    exact, err = score_ref.compare(got, want, A)
    print(f'score count=290 of 300 rows, A={A}, into a filled block: worst error {err:.3e}')
    assert exact and err < BOUND
    host = pit.cpu().numpy()
    assert not (host[:290] == SENTINEL).any() and (host[290:] == SENTINEL).all()
    assert np.abs(host[:290] - c['pit'][:290]).max() < BOUND


@pytest.mark.parametrize('rows,A,split', [(7, 2, 3), (300, 3, 256), (300, 1, 44)])
def test_two_launches_over_a_split_equal_one(cases, rows, A, split):
    c = cases[rows, A, 5.0]
    one = _run(c).cpu().numpy()
    block = _run(c, 0, split)
    two = _run(c, split, rows, block=block, pad=2).cpu().numpy()
    exact, err = score_ref.compare(two, one, A)
    print(f'score rows={rows} A={A} split at {split}: worst difference {err:.3e}')
    assert exact and err < BOUND


def test_null_returns_aux_and_pit_leave_their_slots(cases):
    c = cases[7, 2, 5.0]
    prior = np.full(score_block_size(2), 2.5)
    value_slots = [HEAD[k] for k in ('rows_returns', 'value_error', 'value_error2', 'returns', 'returns2')]
    aux_slots = [HEAD[k] for k in ('rows_aux', 'speed_error2', 'similarity_error2')]
    full = score_ref.block(c['alpha'], c['beta'], c['value'], c['u'], c['returns'], c['speed'], c['similarity'], prior=prior)
    for returns, aux in ((False, False), (True, False), (False, True)):
        got = _run(c, block=_dev(prior, torch.float64), returns=returns, aux=aux).cpu().numpy()         # (a null pit as well)
        want = full.copy()
        if not returns:
            want[value_slots] = 2.5
        if not aux:
            want[aux_slots] = 2.5
        assert (got[value_slots] == 2.5).all() == (not returns) and (got[aux_slots] == 2.5).all() == (not aux)
        exact, err = score_ref.compare(got, want, 2)
        assert exact and err < BOUND, (returns, aux, err)
    unused = [5, 6, 7, 14, 15]
    assert (got[unused] == 2.5).all()


def test_the_iteration_cap_counts_and_returns(cases):
    """alpha = beta = 1e6 at u = 0.5 needs 526 steps: the launch returns, the element is counted once, its pit entry is NaN and the
    histogram holds one element less; its log-likelihood still enters the sums."""
    c = {k: v.copy() for k, v in cases[7, 2, 5.0].items()}
    c['alpha'][3, 1] = c['beta'][3, 1] = 1e6
    c['u'][3, 1] = 0.5
    no_pit = np.zeros((7, 2), bool)
    no_pit[3, 1] = True
    pit = torch.full((7, 2), SENTINEL, dtype=torch.float64, device=DEV)
    got = _run(c, pit=pit).cpu().numpy()
    torch.cuda.synchronize()
    want = score_ref.block(c['alpha'], c['beta'], c['value'], c['u'], c['returns'], c['speed'], c['similarity'], no_pit=no_pit)
    exact, err = score_ref.compare(got, want, 2)
    # (no bound on the sums here: ln B(1e6, 1e6) is a difference of lgamma values near 2.7e7, whose own ulp is 4e-9 on either side)
    print(f'score with one capped element: worst error {err:.3e}')
    assert exact and np.isfinite(got).all()
    first = slice(SCORE_LAYOUT['head_size'], SCORE_LAYOUT['head_size'] + SCORE_LAYOUT['action_size'])      # action 0 is as it was
    assert (np.abs(got[first] - want[first]) < BOUND * np.maximum(1.0, np.abs(want[first]))).all()
    assert got[HEAD['pit_unconverged']] == 1 and got[HEAD['nonfinite']] == 0
    host = pit.cpu().numpy()
    assert np.isnan(host[3, 1]) and np.isfinite(np.delete(host.reshape(-1), 7)).all()
    groups = got[SCORE_LAYOUT['head_size']:].reshape(2, SCORE_LAYOUT['action_size'])
    assert groups[:, ACTION['histogram']:].sum() == 7 * 2 - 1 and groups[:, ACTION['count']].sum() == 14


@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_non_finite_parameters_are_counted_and_left_out(cases, bad):
    c = {k: v.copy() for k, v in cases[7, 2, 500.0].items()}
    c['alpha'][2, 0] = bad
    c['beta'][5, 1] = bad
    pit = torch.full((7, 2), SENTINEL, dtype=torch.float64, device=DEV)
    got = _run(c, pit=pit).cpu().numpy()
    assert got[HEAD['nonfinite']] == 2 and np.isfinite(got).all()
    want = score_ref.block(c['alpha'], c['beta'], c['value'], c['u'], c['returns'], c['speed'], c['similarity'])
    exact, err = score_ref.compare(got, want, 2)
    assert exact and err < BOUND
    host = pit.cpu().numpy()
    assert np.isnan(host[2, 0]) and np.isnan(host[5, 1]) and np.isfinite(host).sum() == 12


def test_argument_errors_write_nothing(cases):
    c = cases[7, 2, 5.0]
    dist, value, u = _dev(_dist(c['alpha'], c['beta'])), _dev(c['value']), _dev(c['u'])
    returns, speed, similarity = _dev(c['returns']), _dev(c['speed']), _dev(c['similarity'])
    block = torch.full((score_block_size(2),), 4.0, dtype=torch.float64, device=DEV)
    pit = torch.full((7, 2), SENTINEL, dtype=torch.float64, device=DEV)
    good = dict(dist=dist, value=value, u=u, returns=returns, speed=speed, similarity=similarity, rows=7, count=7, A=2, block=block, pit=pit)
    lib = _lib.load()
    for change, message in ((dict(dist=None), 'null'), (dict(value=None), 'null'), (dict(u=None), 'null'), (dict(block=None), 'null'),
                            (dict(rows=0, count=0), 'count'), (dict(count=0), 'count'), (dict(count=8), 'count'),
                            (dict(A=0), 'num_actions'), (dict(A=9), 'num_actions'),
                            (dict(speed=None), 'both or neither'), (dict(similarity=None), 'both or neither')):
        assert _launch(**{**good, **change}) == -1, change
        assert message in lib.cdrl_last_error().decode(), (change, lib.cdrl_last_error())
    torch.cuda.synchronize()
    assert bool((block == 4.0).all()) and bool((pit == SENTINEL).all())
    assert _launch(**good) == 0
    torch.cuda.synchronize()
    assert block[HEAD['rows']].item() == 4.0 + 7
    # the Python entry refuses the same, and a wrong shape, dtype or device, before the library is called
    for kw in (dict(count=8), dict(count=0), dict(speed=speed), dict(returns=returns[:, :1]), dict(block=block.float()),
               dict(pit=pit[:3]), dict(block=block.cpu())):
        with pytest.raises(ValueError, match='beta_score'):
            beta_score(dist, value, u, **kw)
    with pytest.raises(ValueError, match='beta_score'):
        beta_score(dist.double(), value, u)
    assert SCORE_BINS == 10
