"""cdrl_vtrace_segments against the float64 restatement of tests/vtrace_ref.py: lengths on every boundary of the kernel (256-thread
stride, unroll-by-8 scans, the LDS chunk of engine.VTRACE_CHUNK rows), A in {1, 2, 3}, five (gamma, lambda, rho_bar, c_bar) points,
ratios on both sides of the clips, actions exactly 0 and 1, one ratio beyond float32 and one beyond float64.  Bounds (the project's
loss-kernel bound): adv_raw, returns and base * 10^exp of returns_be within 1e-5 * max(1, max|returns|), rho within 1e-5 relative,
adv within 1e-5 * scale.  The inputs and the reference are built once per A / per case and never written to."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import vtrace_ref as VR

pytestmark = pytest.mark.gpu

from carla_driving_rl_agent_amd.engine import VTRACE_CHUNK as CH      # noqa: E402

LENGTHS = [1, 2, 255, 256, 257, 8, CH - 1, CH, CH + 1, 2 * CH + 1]
POINTS = [(0.9999, 0.999, 1.0, 1.0), (0.99, 0.95, 2.0, 1.5), (1.0, 1.0, 1.0, 1.0), (0.99, 0.0, 1.0, 1.0), (0.99, 0.95, 1.0, 0.0)]
SCALE = 2.0
GUARD = 64
NAMES = ('returns', 'returns_be', 'adv_raw', 'adv', 'rho')


@functools.lru_cache(maxsize=None)
def _inputs(A, lengths=tuple(LENGTHS), seed=0):
    """Host arrays in the kernel's layout.  rewards' bootstrap entries hold the bootstrap VALUE, as end_trajectory leaves them (the
    V-trace kernel does not read them; the GAE kernel of the on-policy identity does).  log_prob_old = log pi / A - delta / A per
    action with delta ~ N(0, 1.2): ratio = exp(delta)."""
    rng = np.random.default_rng(100 * A + seed)
    S, N = len(lengths), sum(lengths)
    values_be = np.stack([rng.uniform(-1, 1, N + S), rng.uniform(0, 2, N + S)], 1).astype(np.float32)
    rewards = rng.uniform(0, 10, N + S).astype(np.float32)
    ends = np.cumsum(lengths) + np.arange(S)                # padded index of every bootstrap entry
    values_be[ends[::2]] = 0.0                              # every second trajectory ends at a terminal state
    rewards[ends] = VR.values(values_be)[ends]
    alpha = rng.uniform(0.5, 6.0, (N, A)).astype(np.float32)
    beta = rng.uniform(0.5, 6.0, (N, A)).astype(np.float32)
    actions = rng.uniform(0.0, 1.0, (N, A)).astype(np.float32)
    actions[3 % N], actions[N // 2], actions[N - 1, 0] = 0.0, 1.0, 1.0        # exactly 0 and exactly 1
    delta = rng.normal(0.0, 1.2, N)
    delta[N // 3], delta[N // 3 + 1] = 120.0, 800.0         # beyond float32 (finite in float64) / beyond float64
    log_pi = VR.log_pi(alpha, beta, actions)
    log_prob_old = np.repeat(((log_pi - delta) / A)[:, None], A, axis=1).astype(np.float32)
    return dict(rewards=rewards, values_be=values_be, alpha=alpha, beta=beta, actions=actions, log_prob_old=log_prob_old)


ORDER = ('rewards', 'values_be', 'alpha', 'beta', 'actions', 'log_prob_old')


@functools.lru_cache(maxsize=None)
def _device(A):
    return {k: torch.tensor(v).cuda() for k, v in _inputs(A).items()}


def _launch(A, lengths, point, inputs=None):
    from carla_driving_rl_agent_amd.engine import vtrace_segments
    d = inputs if inputs is not None else _device(A)
    gamma, lam, rho_bar, c_bar = point
    out = vtrace_segments(*(d[k] for k in ORDER), list(lengths), gamma, lam, rho_bar, c_bar, SCALE)
    torch.cuda.synchronize()
    return dict(zip(NAMES, out))


def _check_bounds(got, ref, tag=''):
    """The bounds of the module docstring; prints every figure before it asserts.  -> the figures."""
    g = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}
    span = max(1.0, float(np.abs(ref['returns']).max()))
    fig = dict(adv_raw=np.abs(g['adv_raw'] - ref['adv_raw']).max() / span, returns=np.abs(g['returns'] - ref['returns']).max() / span,
               returns_be=np.abs(g['returns_be'][:, 0] * 10.0 ** g['returns_be'][:, 1] - ref['returns']).max() / span,
               adv=np.abs(g['adv'] - ref['adv']).max() / SCALE)
    with np.errstate(over='ignore'):
        ref_rho = ref['rho'].astype(np.float32).astype(np.float64)      # the output is float32: inf where the ratio exceeds it
    finite = np.isfinite(ref_rho)
    assert np.array_equal(np.isinf(g['rho']), ~finite), 'rho: overflow rows'
    fig['rho'] = (np.abs(g['rho'][finite] - ref['rho'][finite]) / ref['rho'][finite]).max()
    print(f'vtrace bounds {tag}: ' + ' '.join(f'{k}={v:.3e}' for k, v in fig.items()) + f' span={span:.4g}')
    for k in ('returns', 'returns_be', 'adv_raw', 'adv'):
        assert np.isfinite(g[k]).all(), k
    assert np.abs(g['returns_be'][:, 0]).max() <= 1.0
    for k, v in fig.items():
        assert v <= 1e-5, (k, v)
    return fig


@pytest.mark.parametrize('A', [1, 2, 3])
def test_inputs_put_ratios_on_both_sides_of_the_clips(A):
    """CPU side: the reference alone sees >= 20 % of the rows below 1 and >= 20 % above the largest rho_bar, and the overflow rows."""
    h = _inputs(A)
    ratio = VR.ratios(h['alpha'], h['beta'], h['actions'], h['log_prob_old'])
    assert (ratio < 1.0).mean() >= 0.2
    for _, _, rho_bar, _ in POINTS:
        assert (ratio > rho_bar).mean() >= 0.2
    log_ratio = VR.log_pi(h['alpha'], h['beta'], h['actions']) - h['log_prob_old'].astype(np.float64).sum(1)
    assert (log_ratio > 100).sum() >= 2 and np.isinf(ratio).sum() == 1
    assert (h['actions'] == 0.0).any() and (h['actions'] == 1.0).any()


@pytest.mark.parametrize('point', POINTS, ids=[f'g{g}_l{l}_r{r}_c{c}' for g, l, r, c in POINTS])
@pytest.mark.parametrize('A', [1, 2, 3])
def test_segments_match_the_float64_reference(A, point):
    h = _inputs(A)
    ref = VR.segments(*(h[k] for k in ORDER), LENGTHS, *point, SCALE)
    _check_bounds(_launch(A, LENGTHS, point), ref, tag=f'A={A} {point}')


def test_on_policy_rows_match_the_gae_kernel():
    """rho_bar = c_bar = 1 and log_prob_old one nat below log pi: every ratio clips to exactly 1, and adv_raw / returns are those of
    cdrl_gae_returns_segments up to the float32 rounding of its deltas (same bound)."""
    from carla_driving_rl_agent_amd.engine import gae_returns_segments
    A, point = 2, (0.9999, 0.999, 1.0, 1.0)
    h = dict(_inputs(A))
    log_pi = VR.log_pi(h['alpha'], h['beta'], h['actions'])
    h['log_prob_old'] = np.repeat(((log_pi - 1.0) / A)[:, None], A, axis=1).astype(np.float32)
    assert (VR.ratios(h['alpha'], h['beta'], h['actions'], h['log_prob_old']) > 1.0).all()
    d = {k: torch.tensor(v).cuda() for k, v in h.items()}
    got = _launch(A, LENGTHS, point, inputs=d)
    ret, _, adv_raw, adv = gae_returns_segments(d['rewards'], d['values_be'], LENGTHS, point[0], point[1], SCALE)
    span = max(1.0, float(ret.abs().max()))
    err = dict(returns=float((got['returns'] - ret).abs().max()) / span, adv_raw=float((got['adv_raw'] - adv_raw).abs().max()) / span,
               adv=float((got['adv'] - adv).abs().max()) / SCALE)
    print('vtrace on-policy vs gae:', err)
    assert max(err.values()) <= 1e-5, err


def test_each_segment_alone_gives_the_same_bits():
    A, point = 3, (0.99, 0.95, 2.0, 1.5)
    d = _device(A)
    many = _launch(A, LENGTHS, point)
    row = 0
    for s, n in enumerate(LENGTHS):
        one = {k: (d[k][row + s:row + s + n + 1] if k in ('rewards', 'values_be') else d[k][row:row + n]).contiguous() for k in ORDER}
        alone = _launch(A, [n], point, inputs=one)
        for k in NAMES:
            assert torch.equal(alone[k], many[k][row:row + n]), (s, n, k)
        row += n


def _raw_call(lib, d, seg_off, S, N, A, point, bufs, **override):
    from carla_driving_rl_agent_amd import _lib
    args = dict(d, seg_off=seg_off, **bufs)
    args.update(override)                                   # (a None entry: the null-pointer cases)
    p = lambda k: _lib.ptr(args[k])
    gamma, lam, rho_bar, c_bar = point
    return lib.cdrl_vtrace_segments(p('rewards'), p('values_be'), p('alpha'), p('beta'), p('actions'), p('log_prob_old'), p('seg_off'),
                                    S, N, A, gamma, lam, rho_bar, c_bar, SCALE, p('returns'), p('returns_be'), p('adv_raw'), p('adv'),
                                    p('rho'), p('scratch'), C.c_void_p(torch.cuda.current_stream().cuda_stream))


SENTINEL = -12345.0


def _sentinel_bufs(N, scratch):
    f = lambda n: torch.full((n,), SENTINEL, dtype=torch.float32, device='cuda')
    return dict(returns=f(N), returns_be=f(2 * N), adv_raw=f(N), adv=f(N), rho=f(N),
                scratch=torch.zeros(scratch, dtype=torch.float64, device='cuda'))


@pytest.mark.parametrize('offsets,written', [([0, 5, 99, 21], [(0, 5, 0)]), ([0, 5, 5, 14], [(0, 5, 0), (5, 14, 2)])],
                         ids=['middle_beyond_N', 'middle_empty'])
def test_a_malformed_middle_segment_writes_nothing(offsets, written):
    """Three segments over N = 21 rows; the middle one is malformed (and, in the first case, so is the last one, whose start is the
    middle one's end): the rows no well-formed segment owns keep their sentinel, the others are correct.
    written: (first row, end row, segment index) of the well-formed ones."""
    from carla_driving_rl_agent_amd import _lib
    lib = _lib.load()
    A, point, S, N = 2, (0.99, 0.95, 2.0, 1.5), 3, 21
    h = {k: v[:(N + S if k in ('rewards', 'values_be') else N)] for k, v in _inputs(A).items()}
    d = {k: torch.tensor(v).cuda() for k, v in h.items()}
    bufs = _sentinel_bufs(N, int(lib.cdrl_vtrace_segments_scratch_doubles(N, S)))
    seg_off = torch.tensor(offsets, dtype=torch.int32, device='cuda')
    _lib.check(_raw_call(lib, d, seg_off, S, N, A, point, bufs), 'cdrl_vtrace_segments')
    torch.cuda.synchronize()
    owned = np.zeros(N, bool)
    for lo, hi, s in written:
        owned[lo:hi] = True
        pad = slice(lo + s, hi + s + 1)
        ref = VR.trajectory(h['rewards'][pad], h['values_be'][pad], *(h[k][lo:hi] for k in ORDER[2:]), *point, SCALE)
        got = {k: (bufs[k].view(N, 2) if k == 'returns_be' else bufs[k])[lo:hi] for k in NAMES}
        _check_bounds(got, ref, tag=f'rows {lo}:{hi}')
    assert not owned.all()
    for k in NAMES:
        rows = (bufs[k].view(N, 2) if k == 'returns_be' else bufs[k]).cpu().numpy()
        assert (rows[~owned] == SENTINEL).all(), k


def test_guard_bands_around_outputs_and_scratch_stay_intact():
    from carla_driving_rl_agent_amd import _lib
    lib = _lib.load()
    A, point = 3, (0.9999, 0.999, 1.0, 1.0)
    S, N = len(LENGTHS), sum(LENGTHS)
    need = int(lib.cdrl_vtrace_segments_scratch_doubles(N, S))
    assert need == 4 * N
    pattern32 = torch.tensor([0x5A5AA5A5], dtype=torch.int32).view(torch.float32).item()
    pattern64 = torch.tensor([0x5A5AA5A55A5AA5A5], dtype=torch.int64).view(torch.float64).item()

    def banded(n, dtype, pattern):
        return torch.full((GUARD + n + GUARD,), pattern, dtype=dtype, device='cuda')

    full = dict(returns=banded(N, torch.float32, pattern32), returns_be=banded(2 * N, torch.float32, pattern32),
                adv_raw=banded(N, torch.float32, pattern32), adv=banded(N, torch.float32, pattern32),
                rho=banded(N, torch.float32, pattern32), scratch=banded(need, torch.float64, pattern64))
    before = {k: b.clone() for k, b in full.items()}
    inner = {k: b[GUARD:b.numel() - GUARD] for k, b in full.items()}
    seg_off = torch.tensor(np.concatenate([[0], np.cumsum(LENGTHS)]), dtype=torch.int32).cuda()
    _lib.check(_raw_call(lib, _device(A), seg_off, S, N, A, point, inner), 'cdrl_vtrace_segments')
    torch.cuda.synchronize()
    for k, b in full.items():
        as_int = torch.int32 if b.dtype == torch.float32 else torch.int64      # bit patterns, not float comparisons
        assert torch.equal(b[:GUARD].view(as_int), before[k][:GUARD].view(as_int)), f'{k}: front band'
        assert torch.equal(b[-GUARD:].view(as_int), before[k][-GUARD:].view(as_int)), f'{k}: back band'
    ref = _launch(A, LENGTHS, point)
    for k in NAMES:
        assert torch.equal(inner[k].view(ref[k].shape), ref[k]), k


def test_argument_errors_are_reported_without_a_launch():
    from carla_driving_rl_agent_amd import _lib
    lib = _lib.load()
    A, point, S, N = 2, (0.99, 0.95, 1.0, 1.0), 2, 4
    h = {k: v[:(N + S if k in ('rewards', 'values_be') else N)] for k, v in _inputs(A).items()}
    d = {k: torch.tensor(v).cuda() for k, v in h.items()}
    bufs = _sentinel_bufs(N, 4 * N)
    seg_off = torch.tensor([0, 2, 4], dtype=torch.int32, device='cuda')
    call = lambda S_=S, N_=N, A_=A, point_=point, **kw: _raw_call(lib, d, kw.pop('seg_off', seg_off), S_, N_, A_, point_, bufs, **kw)
    cases = [(dict(S_=0), 'S ='), (dict(N_=1), 'N ='), (dict(A_=0), 'A ='), (dict(A_=9), 'A ='), (dict(S_=1, N_=2 ** 31 - 1), '32-bit'),
             (dict(point_=(0.99, 0.95, -0.5, 1.0)), 'rho_bar'), (dict(point_=(0.99, 0.95, 1.0, -1.0)), 'c_bar')]
    cases += [({k: None}, 'null') for k in ORDER + NAMES + ('scratch', 'seg_off')]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in lib.cdrl_last_error().decode(), kw
    torch.cuda.synchronize()
    for k in NAMES:
        assert (bufs[k] == SENTINEL).all(), k               # nothing was launched
    assert call() == 0                                      # the well-formed call of the same buffers goes through
    torch.cuda.synchronize()
    assert (bufs['returns'] != SENTINEL).all()
    assert int(lib.cdrl_vtrace_segments_scratch_doubles(4, 2)) == 16 and int(lib.cdrl_vtrace_segments_scratch_doubles(1, 2)) == 0
