"""Occlusion saliency on the device (csrc/explain.hip, CARLAgent.explain) against its numpy / float64 restatement
(tests/explain_ref.py): the occluded rows bit for bit, the baseline, the scores, the maps, the agent-level call against the same
engine on numpy-built rows, and that a call between two learn() calls leaves training bit for bit where it was."""
import os

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
from carla_driving_rl_agent_amd.engine import occlusion_baseline, occlusion_maps, occlusion_rows, occlusion_scores
from carla_driving_rl_agent_amd.explain import MODALITIES, occlusion_row_count
from tests import explain_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
KEYS = ('state_image', 'state_road', 'state_vehicle', 'state_navigation')
SENTINEL = -12345.0             # no input holds it: images and vectors are drawn from [0, 1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _observation(T, H, W, seed):
    rng = np.random.default_rng(seed)
    return dict(state_image=rng.random((T, H, W, 3), dtype=np.float32), state_road=rng.random((T, 9), dtype=np.float32),
                state_vehicle=rng.random((T, 4), dtype=np.float32), state_navigation=rng.random((T, 5), dtype=np.float32))


def _dev(obs):
    return {k: torch.as_tensor(v).to(DEV) for k, v in obs.items()}


def _rows_in_chunks(d, base, grid, per_frame, modalities, count, N):
    """All N rows through launches of `count` rows into one sentinel-filled buffer of ceil(N / count) * count rows."""
    total = -(-N // count) * count
    bufs = {k: torch.full((total,) + tuple(v.shape), SENTINEL, dtype=torch.float32, device=DEV) for k, v in d.items()}
    for first in range(0, N, count):
        occlusion_rows(d['state_image'], base, d['state_road'], d['state_vehicle'], d['state_navigation'], grid, per_frame,
                       modalities, first, {k: v[first:first + count] for k, v in bufs.items()})
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _check_rows(obs, grids, counts, baselines=('zero', 'mean', 'given')):
    d = _dev(obs)
    T, H, W, _ = obs['state_image'].shape
    given = torch.as_tensor(np.random.default_rng(99).random((T, H, W, 3), dtype=np.float32)).to(DEV)
    for name in baselines:
        base = given if name == 'given' else occlusion_baseline(d['state_image'], name)
        base_np = base.cpu().numpy()
        for grid in grids:
            for per_frame in (False, True):
                for modalities in (False, True):
                    N = occlusion_row_count(T, grid[0], grid[1], per_frame, modalities)
                    want = explain_ref.rows(obs['state_image'], base_np, obs['state_road'], obs['state_vehicle'],
                                            obs['state_navigation'], grid, per_frame, modalities)
                    for count in counts(N):
                        got = _rows_in_chunks(d, base, grid, per_frame, modalities, count, N)
                        what = (name, grid, per_frame, modalities, count)
                        for k in KEYS:
                            assert not (got[k] == SENTINEL).any(), what + (k, 'stale data left in a chunk')
                            assert np.array_equal(_bits(got[k][:N]), _bits(want[k])), what + (k,)
                            assert np.array_equal(_bits(got[k][0]), _bits(obs[k])), what + (k, 'row 0')
                            for r in range(N, got[k].shape[0]):                 # beyond N: copies of row 0
                                assert np.array_equal(_bits(got[k][r]), _bits(obs[k])), what + (k, r)


# (1, 5, 7): a row of 105 floats, so every row but the first starts off 16-byte alignment; (2, 10, 14) with (3, 4): uneven cells
@pytest.mark.parametrize('T,H,W', [(1, 5, 7), (2, 10, 14), (4, 12, 16)])
def test_rows_bit_exact(T, H, W):
    _check_rows(_observation(T, H, W, seed=T), [(1, 1), (3, 4), (H, W)], lambda N: (1, 5, N, N + 3))


# more than one workgroup per row (4096 floats each), the last one partial: 18432 floats take the 16-byte path, 13959 (not a
# multiple of 4) the 4-byte one; spans that the rectangle does not reach are plain copies
@pytest.mark.parametrize('T,H,W', [(2, 48, 64), (3, 33, 47)])
def test_rows_bit_exact_over_several_workgroups(T, H, W):
    _check_rows(_observation(T, H, W, seed=7), [(1, 1), (3, 4), (5, 7)], lambda N: (5, N + 3), baselines=('mean', 'given'))


def test_rows_from_a_misaligned_stack_take_the_narrow_path():
    """A row length that allows 16-byte accesses, the image 4 bytes off alignment."""
    obs = _observation(2, 10, 14, seed=3)
    d = _dev(obs)
    n = obs['state_image'].size
    store = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    store[1:n + 1].copy_(d['state_image'].reshape(-1))
    d['state_image'] = store[1:n + 1].view(2, 10, 14, 3)
    assert d['state_image'].data_ptr() % 16 == 4 and n % 4 == 0
    base = occlusion_baseline(d['state_image'], 'mean')
    got = _rows_in_chunks(d, base, (3, 4), True, True, 7, occlusion_row_count(2, 3, 4, True, True))
    want = explain_ref.rows(obs['state_image'], base.cpu().numpy(), obs['state_road'], obs['state_vehicle'], obs['state_navigation'],
                            (3, 4), True, True)
    for k in KEYS:
        assert np.array_equal(_bits(got[k][:want[k].shape[0]]), _bits(want[k])), k


def test_rows_refuse_misuse():
    d = _dev(_observation(2, 10, 14, seed=1))
    base = occlusion_baseline(d['state_image'], 'zero')
    out = {k: torch.empty((4,) + tuple(v.shape), device=DEV) for k, v in d.items()}
    args = lambda **kw: {**dict(image=d['state_image'], baseline=base, road=d['state_road'], vehicle=d['state_vehicle'],
                                navigation=d['state_navigation'], grid=(3, 4), per_frame=False, modalities=True, first=0, out=out), **kw}
    occlusion_rows(**args())
    for bad in (dict(grid=(11, 4)), dict(grid=(3, 0)), dict(first=-1), dict(baseline=base[:1]), dict(image=d['state_image'].double()),
                dict(out={k: v[:, :1] for k, v in out.items()}), dict(out=dict(state_image=out['state_image'])),
                dict(road=d['state_road'][:1])):
        with pytest.raises(ValueError):
            occlusion_rows(**args(**bad))
    with pytest.raises(ValueError):
        occlusion_baseline(d['state_image'], 'median')


@pytest.mark.parametrize('T,H,W', [(1, 5, 7), (2, 48, 64), (4, 90, 120)])
def test_baseline_mean(T, H, W):
    image = np.random.default_rng(T).random((T, H, W, 3), dtype=np.float32)
    x = torch.as_tensor(image).to(DEV)
    got = occlusion_baseline(x, 'mean')
    assert torch.equal(got, occlusion_baseline(x, 'mean'))                      # the same input, the same bytes
    g = got.cpu().numpy()
    assert (g == g[:, :1, :1]).all()                                            # one value per frame and channel
    m64 = image.astype(np.float64).mean(axis=(1, 2))
    # one rounding of a double mean whose own error is ~1e-16 relative: half a float32 ulp
    half_ulp = 0.5 * np.spacing(np.abs(m64).astype(np.float32)).astype(np.float64)
    err = np.abs(g[:, 0, 0].astype(np.float64) - m64)
    print(f'baseline mean {T}x{H}x{W}: worst error {err.max():.3e}, half ulp {half_ulp.min():.3e}')
    assert (err <= half_ulp * (1.0 + 1e-6)).all()
    # a constant image: P equal 24-bit values sum exactly in double, so the mean is the constant
    c = torch.full((T, H, W, 3), 0.5, dtype=torch.float32, device=DEV)
    assert bool((occlusion_baseline(c, 'mean') == 0.5).all())
    assert bool((occlusion_baseline(x, 'zero') == 0.0).all())


@pytest.mark.parametrize('N', [2, 7, 200])
@pytest.mark.parametrize('A', [1, 2, 3])
def test_scores_against_the_restatement(N, A):
    rng = np.random.default_rng(100 * N + A)
    alpha = rng.uniform(1.01, 50.0, (N, A)).astype(np.float32)
    beta = rng.uniform(1.01, 50.0, (N, A)).astype(np.float32)
    value = np.stack([rng.uniform(-1.0, 1.0, N), rng.uniform(0.0, 6.0, N)], axis=1).astype(np.float32)
    same = N - 1                                                               # a row equal to row 0
    alpha[same], beta[same], value[same] = alpha[0], beta[0], value[0]
    got = occlusion_scores(*(torch.as_tensor(x).to(DEV) for x in (alpha, beta, value))).cpu().numpy()
    want = explain_ref.scores(alpha, beta, value)
    assert got.shape == (N - 1, 2 + A) and got.dtype == np.float64
    v = value[:, 0].astype(np.float64) * 10.0 ** value[:, 1].astype(np.float64)
    scale = np.maximum(1.0, np.maximum(np.abs(v[0]), np.abs(v[1:])))
    e_kl = np.abs(got[:, 0] - want[:, 0]).max()
    e_mean = np.abs(got[:, 2:] - want[:, 2:]).max()
    e_value = (np.abs(got[:, 1] - want[:, 1]) / scale).max()
    print(f'scores N={N} A={A}: kl {e_kl:.3e}, mean {e_mean:.3e}, value / max(1, |V|) {e_value:.3e}')
    assert e_kl < 1e-5 and e_mean < 1e-5 and e_value < 1e-5
    assert (got[same - 1] == 0.0).all()


MAP_CASES = [(1, 5, 7, 2, 3), (2, 10, 14, 3, 4), (4, 12, 16, 12, 16), (2, 48, 64, 3, 4), (1, 48, 64, 1, 1)]


@pytest.mark.parametrize('F,H,W,gh,gw', MAP_CASES)
def test_maps(F, H, W, gh, gw):
    rng = np.random.default_rng(F * H + gw)
    K, cells = 4, F * gh * gw
    s = rng.normal(size=(cells + 4, K)) * np.array([1e-3, 50.0, 0.2, 1.0])      # the four rows behind the cells are ignored
    s[:, 3] = 0.0                                                               # an all-zero column
    s[cells:, 3] = 9.0                                                          # ... whose modality rows must not count
    sd = torch.as_tensor(s).to(DEV)
    for normalize in (True, False):
        near = occlusion_maps(sd, F, (gh, gw), (H, W), 'nearest', normalize).cpu().numpy()
        want = explain_ref.maps(s, F, (gh, gw), (H, W), 'nearest', normalize)
        assert near.shape == (K, F, H, W) and near.dtype == np.float32
        assert np.array_equal(_bits(near), _bits(want.astype(np.float32))), normalize       # the one rounding of s / max|s|
        assert not np.isnan(near).any() and (near[3] == 0.0).all()
    lin = occlusion_maps(sd, F, (gh, gw), (H, W), 'bilinear', True).cpu().numpy()
    want = explain_ref.maps(s, F, (gh, gw), (H, W), 'bilinear', True)
    err = np.abs(lin.astype(np.float64) - want).max()
    print(f'bilinear maps {F}x{H}x{W} grid {gh}x{gw}: worst error on scores in [-1, 1] {err:.3e}')
    assert err < 1e-5
    assert not np.isnan(lin).any() and (lin[3] == 0.0).all()
    assert np.abs(lin).max() <= 1.0 and np.abs(near).max() > 1.0


def test_bilinear_on_a_full_grid_returns_the_scores():
    F, H, W, K = 2, 10, 14, 3
    s = np.random.default_rng(5).normal(size=(F * H * W, K))
    sd = torch.as_tensor(s).to(DEV)
    for normalize in (False, True):
        got = occlusion_maps(sd, F, (H, W), (H, W), 'bilinear', normalize).cpu().numpy()
        ref = s / np.abs(s).max(axis=0) if normalize else s
        want = np.moveaxis(ref.reshape(F, H, W, K), -1, 0).astype(np.float32)
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(got), _bits(occlusion_maps(sd, F, (H, W), (H, W), 'nearest', normalize).cpu().numpy()))


# ---------------------------------------------------------------- agent level
def _env(**kw):
    cfg = dict(image_shape=(48, 64, 3), time_horizon=2, num_waypoints=5, vehicle_features=4, num_actions=2)
    cfg.update(kw)
    return FakeCARLAEnvironment(**cfg)


def _agent(env, root, **kw):
    cfg = dict(batch_size=8, log_mode=None, seed=5, skip_data=0, shuffle=True, policy_lr=3e-4, value_lr=3e-4, dynamics_lr=3e-4,
               aug_intensity=0.0, weights_dir=os.path.join(str(root), 'weights'), evaluation_dir=os.path.join(str(root), 'evaluation'),
               name='explain')
    cfg.update(kw)
    return CARLAgent(env, **cfg)


def _batch(agent, E, seed):
    envs = [_env(seed=seed + e) for e in range(E)]
    return agent.observe([env.reset() for env in envs], agent.preprocess())


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """An agent after a few learn() steps: the moving statistics are no longer at their initial values."""
    agent = _agent(_env(seed=1, episode_length=None), tmp_path_factory.mktemp('explain'))
    agent.learn(episodes=1, timesteps=12, close=False)
    return agent


def _score_bounds(got, want, value0, values):
    v0 = float(value0[0]) * 10.0 ** float(value0[1])
    v = values[:, 0].astype(np.float64) * 10.0 ** values[:, 1].astype(np.float64)
    scale = np.maximum(1.0, np.maximum(abs(v0), np.abs(v)))
    return (np.abs(got[:, 0] - want[:, 0]).max(), (np.abs(got[:, 1] - want[:, 1]) / scale).max(), np.abs(got[:, 2:] - want[:, 2:]).max())


@pytest.mark.parametrize('chunk', [4, 32])
def test_explain_against_the_same_engine_on_numpy_rows(trained, chunk):
    agent = trained
    state = _batch(agent, 2, seed=60)
    index = agent.network.action_index
    out = agent.explain(state, grid=(3, 4), chunk=chunk, row=1)
    assert agent.network.action_index == index
    one = {k: state[k][1].cpu().numpy() for k in KEYS}
    base = occlusion_baseline(state['state_image'][1].contiguous(), 'mean').cpu().numpy()
    rows = explain_ref.rows(one['state_image'], base, one['state_road'], one['state_vehicle'], one['state_navigation'], (3, 4), False, True)
    N = occlusion_row_count(2, 3, 4, False, True)
    assert rows['state_image'].shape[0] == N == 17
    alpha, beta, value = (x.cpu().numpy() for x in agent.network.distribution_and_value({k: torch.as_tensor(v) for k, v in rows.items()},
                                                                                      chunk=chunk))
    want = explain_ref.scores(alpha, beta, value)
    got = np.concatenate([out['scores'].cpu().numpy().reshape(12, 4),
                          np.array([[out['modalities'][m][n] for n in out['names']] for m in MODALITIES])])
    e_kl, e_value, e_mean = _score_bounds(got, want, value[0], value[1:])
    print(f'explain chunk={chunk}: kl {e_kl:.3e}, value {e_value:.3e}, mean {e_mean:.3e} (expected: identical)')
    assert e_kl < 1e-5 and e_value < 1e-5 and e_mean < 1e-5
    assert out['names'] == ['kl', 'value', 'mean_0', 'mean_1'] and out['frames'] == 1 and out['grid'] == (3, 4)
    assert tuple(out['scores'].shape) == (1, 3, 4, 4) and out['scores'].dtype == torch.float64 and out['scores'].is_cuda
    assert set(out['maps']) == set(out['names'])
    assert all(tuple(m.shape) == (1, 48, 64) and m.dtype == torch.float32 and m.is_cuda for m in out['maps'].values())
    # the decision of row 0 is the one predict() reports, and the occlusions move it
    assert np.array_equal(out['alpha'].cpu().numpy(), alpha[0]) and np.array_equal(out['beta'].cpu().numpy(), beta[0])
    assert np.array_equal(out['value'].cpu().numpy(), value[0])
    assert torch.equal(out['mean'], out['alpha'] / (out['alpha'] + out['beta']))
    assert (got[:, 0] > 0.0).any()
    # nearest, normalised: every pixel of a cell holds float32(score / max |score|)
    maps = explain_ref.maps(got[:12], 1, (3, 4), (48, 64), 'nearest', True).astype(np.float32)
    for k, name in enumerate(out['names']):
        assert np.array_equal(_bits(out['maps'][name].cpu().numpy()), _bits(maps[k])), name


def test_one_cell_over_all_frames_is_the_image_modality(trained):
    out = trained.explain(_batch(trained, 1, seed=61), grid=(1, 1), per_frame=False, baseline='zero')
    cell = out['scores'].cpu().numpy().reshape(4)
    assert np.array_equal(cell, np.array([out['modalities']['image'][n] for n in out['names']]))        # the same input: the same bits
    assert cell[0] > 0.0


def test_constant_image_and_zero_vectors_score_exactly_zero(trained):
    state = _batch(trained, 1, seed=62)
    state['state_image'] = torch.full_like(state['state_image'], 0.5)
    state['state_road'] = torch.zeros_like(state['state_road'])
    out = trained.explain(state, grid=(3, 4), baseline='mean', per_frame=True, upsample='bilinear')
    assert bool((out['scores'] == 0.0).all())                                   # the mean of a constant image is the image
    assert all(bool((m == 0.0).all()) for m in out['maps'].values())            # ... and 0 / 0 is not formed
    assert all(v == 0.0 for v in out['modalities']['image'].values())
    assert all(v == 0.0 for v in out['modalities']['road'].values())            # zeroing what is zero already
    assert out['modalities']['vehicle']['kl'] > 0.0


def test_per_frame_gives_a_map_per_frame(trained):
    state = _batch(trained, 1, seed=63)
    given = torch.rand((2, 48, 64, 3), device=DEV)
    out = trained.explain(state, grid=(2, 3), per_frame=True, baseline=given, modalities=False, normalize=False, chunk=5)
    assert out['frames'] == 2 and tuple(out['scores'].shape) == (2, 2, 3, 4) and 'modalities' not in out
    assert all(tuple(m.shape) == (2, 48, 64) for m in out['maps'].values())
    s = out['scores'].cpu().numpy()
    kl = out['maps']['kl'].cpu().numpy()
    assert kl[1, 47, 63] == np.float32(s[1, 1, 2, 0]) and kl[0, 0, 0] == np.float32(s[0, 0, 0, 0])
    assert not np.array_equal(s[0], s[1])


def _learner_state(agent):
    s = agent.network.engine.export_state()
    return s['params'], s['adam_m'], s['adam_v'], s['optimizer']


def test_explain_between_two_learn_calls_changes_nothing(tmp_path):
    def run(with_explain):
        agent = _agent(_env(seed=2, episode_length=None), tmp_path / f'run{int(with_explain)}')
        agent.learn(episodes=1, timesteps=12, close=False)
        if with_explain:
            state = _batch(agent, 2, seed=70)
            agent.explain(state, grid=(3, 4), chunk=8)
            agent.explain(state, grid=(1, 1), per_frame=True, baseline='zero', row=1, chunk=3)
            agent.explain(state, grid=(2, 5), modalities=False, upsample='bilinear', baseline=state['state_image'][1])
        agent.learn(episodes=1, timesteps=12, close=False)
        sample = agent.predict(_batch(agent, 1, seed=71))
        return _learner_state(agent), agent.network.action_index, sample

    (p0, m0, v0, o0), i0, s0 = run(False)
    (p1, m1, v1, o1), i1, s1 = run(True)
    assert i0 == i1 and o0 == o1
    assert np.array_equal(p0, p1) and np.array_equal(m0, m1) and np.array_equal(v0, v1)     # parameters, moving statistics, slots
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))                                     # the next sampled predict
    assert np.isfinite(p0).all()
