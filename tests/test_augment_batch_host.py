"""Host side of the batched shard augmentation: the packed plan array has AugPlan's bytes, a blur size the kernels do not have is
refused before the upload, and the shard path draws its plans exactly as the per-environment loop does."""
import numpy as np
import pytest


def _kernel(k, seed=3):
    w = np.random.default_rng(seed).normal(1.0, 0.25, (k, k, 3)).astype(np.float32).reshape(-1)
    return list(w) + [0.0] * (75 - w.size)


# the eleven plans of tests/test_gpu_augment.py::CASES
CASES = [
    ('identity', {}),
    ('jitter', dict(jitter=1, brightness=0.13, contrast=1.4, saturation=0.6, hue=-0.11)),
    ('jitter2', dict(jitter=1, brightness=-0.2, contrast=0.3, saturation=1.7, hue=0.2)),
    ('blur3', dict(blur_size=3, blur_kernel=_kernel(3))),
    ('blur5', dict(blur_size=5, blur_kernel=_kernel(5), normalize=1)),
    ('salt_pepper', dict(salt_pepper=1, sp_amount=0.1, sp_prob=0.5)),
    ('gauss', dict(gauss_noise=1, gn_amount=0.1, gn_std=0.075)),
    ('normalize', dict(normalize=1)),
    ('cutout', dict(cutout_size=6, cutout_cell=21)),
    ('dropout', dict(dropout_size=81, dropout_amount=0.04)),
    ('all', dict(jitter=1, brightness=0.05, contrast=1.2, saturation=1.3, hue=0.07, blur_size=3, blur_kernel=_kernel(3, 9),
                 salt_pepper=1, gauss_noise=1, normalize=1, cutout_size=6, cutout_cell=3, dropout_size=81)),
]


def eleven_plans():
    """One plan per case, each with its own seed and offset."""
    from carla_driving_rl_agent_amd.rl.augmentations import empty_plan
    plans = []
    for i, (_, kw) in enumerate(CASES):
        p = empty_plan(seed=0x1234567890abcdef + 7919 * i, offset=17 + 3 * i)
        p.update(kw)
        plans.append(p)
    return plans


def _bytes(plans):
    from carla_driving_rl_agent_amd.rl.augmentations import to_struct
    return b''.join(bytes(to_struct(p)) for p in plans)


def test_pack_plans_has_the_struct_layout():
    import ctypes as C
    from carla_driving_rl_agent_amd.rl.augmentations import AugPlan, pack_plans, empty_plan
    one = pack_plans([empty_plan()])
    assert one.nbytes == C.sizeof(AugPlan)
    assert one.tobytes() == _bytes([empty_plan()])
    assert pack_plans([empty_plan(seed=2 ** 63 - 2, offset=2 ** 40 + 5)]).tobytes() == _bytes([empty_plan(seed=2 ** 63 - 2, offset=2 ** 40 + 5)])


def test_pack_plans_matches_to_struct_for_the_eleven_cases():
    from carla_driving_rl_agent_amd.rl.augmentations import pack_plans
    plans = eleven_plans()
    packed = pack_plans(plans)
    assert packed.shape == (11,)
    assert packed.tobytes() == _bytes(plans)
    for i, p in enumerate(plans):                       # and one at a time: no field leaks into a neighbouring record
        assert pack_plans([p]).tobytes() == _bytes([p]), CASES[i][0]


def test_pack_plans_matches_to_struct_for_drawn_plans():
    from carla_driving_rl_agent_amd.rl.augmentations import pack_plans, draw_plan
    rng = np.random.default_rng(11)
    plans = [draw_plan(1.0, rng, offset=i + 1) for i in range(50)]
    assert len({(p['jitter'], p['blur_size'], p['salt_pepper'], p['gauss_noise'], p['cutout_size'], p['dropout_size'])
                for p in plans}) > 5                   # the draw covers many op combinations
    assert pack_plans(plans).tobytes() == _bytes(plans)


def test_pack_plans_refuses_a_blur_size_the_kernels_do_not_have():
    from carla_driving_rl_agent_amd.rl.augmentations import pack_plans, empty_plan
    bad = empty_plan()
    bad.update(blur_size=4)
    with pytest.raises(ValueError, match='blur_size'):
        pack_plans([empty_plan(), bad])


def test_shard_helper_draws_as_successive_draw_plan_calls():
    from carla_driving_rl_agent_amd.rl.augmentations import draw_plans, draw_plan
    E, n = 9, 21
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    got = draw_plans(1.0, a, E, first_offset=n + 1)
    ref = [draw_plan(1.0, b, offset=n + 1 + e) for e in range(E)]
    assert [p['offset'] for p in got] == list(range(n + 1, n + E + 1))
    assert _bytes(got) == _bytes(ref)
    # the generator is left where E single draws leave it
    assert a.bit_generator.state == b.bit_generator.state
    assert _bytes([draw_plan(1.0, a, offset=99)]) == _bytes([draw_plan(1.0, b, offset=99)])


class _RecordingAugmenter:
    """Stands in for the device augmenter: returns the images unchanged and records the plans it was given."""
    log = []

    def __init__(self, device='cpu'):
        self.device = device

    def __call__(self, images, plan):
        import torch
        self.log.append(('single', [plan]))
        return torch.as_tensor(images, dtype=torch.float32)

    def batch(self, images, plans):
        import torch
        self.log.append(('batch', list(plans)))
        return torch.as_tensor(np.stack(images, axis=0) if isinstance(images, list) else images, dtype=torch.float32)


def _host_agent(monkeypatch, **kw):
    """A real CARLAgent whose learner engines are host-only (planned, never bound to a device)."""
    from carla_driving_rl_agent_amd.core import networks, CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    monkeypatch.setattr(networks, 'LearnerEngine', lambda B, device=None, share_with=None, **cfg: LearnerEngine(B, device=None, share_with=share_with, **cfg))
    monkeypatch.setattr(networks, 'init_engine_parameters', lambda *a, **k: None)
    envs = [FakeCARLAEnvironment(image_shape=(36, 108, 3), time_horizon=4, num_waypoints=5, vehicle_features=4, num_actions=2,
                                 image_range=(0.0, 1.0), seed=s) for s in (1, 2, 3)]
    return CARLAgent(envs[0], batch_size=8, log_mode=None, seed=7, device='cpu', aug_intensity=1.0, **kw), envs


def test_observe_takes_the_shard_path_with_the_plans_of_the_loop(monkeypatch):
    """PPOAgent.observe with a preprocess function that carries `shard`: one call for the three environments, the same keys,
    shapes and values as the per-environment loop, the same plans with the same offsets, the same number of draws."""
    from carla_driving_rl_agent_amd.rl import augmentations
    monkeypatch.setattr(augmentations, 'Augmenter', _RecordingAugmenter)
    results = {}
    for flag in (True, False):
        agent, envs = _host_agent(monkeypatch, batch_augment=flag)
        fn = agent.preprocess()
        assert hasattr(fn, 'shard') == flag
        _RecordingAugmenter.log = []
        first = agent.observe([env.reset() for env in envs], fn)
        second = agent.observe([env.step(np.zeros(2))[0] for env in envs], fn)
        assert agent._aug_calls == 6
        results[flag] = (first, second, list(_RecordingAugmenter.log))
    batched, looped = results[True], results[False]
    assert [kind for kind, _ in batched[2]] == ['batch'] * 2 and [kind for kind, _ in looped[2]] == ['single'] * 6
    plans = lambda log: [p for _, ps in log for p in ps]
    assert [p['offset'] for p in plans(batched[2])] == [1, 2, 3, 4, 5, 6]
    assert _bytes(plans(batched[2])) == _bytes(plans(looped[2]))
    for a, b in zip(batched[:2], looped[:2]):
        assert list(a) == list(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and bool((a[k] == b[k]).all()), k
    assert batched[0]['state_image'].shape == (3, 4, 36, 108, 3)


def test_one_observation_and_intensity_zero_keep_the_loop(monkeypatch):
    from carla_driving_rl_agent_amd.rl import augmentations
    monkeypatch.setattr(augmentations, 'Augmenter', _RecordingAugmenter)
    agent, envs = _host_agent(monkeypatch, batch_augment=True)
    _RecordingAugmenter.log = []
    agent.observe([envs[0].reset()], agent.preprocess())
    assert [kind for kind, _ in _RecordingAugmenter.log] == ['single'] and agent._aug_calls == 1
    agent.aug_intensity = 0.0
    assert not hasattr(agent.preprocess(), 'shard')
