"""Host side of the contrastive view pipeline: the plan layout, draw_view_plans, every refusal that is decided
before anything touches a GPU, CARLAgent(view_pipeline=...), and the float64 restatement (tests/views_ref.py) against its own
float32 run on the cases the device is compared with it on."""
import ctypes as C

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd.core import CARLAgent, FakeCARLAEnvironment
from carla_driving_rl_agent_amd.rl import augmentations as aug
from tests import views_ref

SHAPES = [(23, 31), (90, 120), (90, 360)]


def _stub(**kw):
    """A CARLAgent that was never constructed (as tests/test_representation_host.py builds it)."""
    env = FakeCARLAEnvironment(image_shape=(4, 6, 3), time_horizon=2, num_waypoints=5, vehicle_features=4, num_actions=2)
    agent = object.__new__(CARLAgent)
    agent.env, agent.num_actions, agent.data_parallel, agent.polyak_coeff = env, 2, False, 1.0
    agent.state_spec = dict(state_image=(4, 6, 3), state_road=(9,), state_vehicle=(4,), state_navigation=(5,))
    agent.should_update_dynamics, agent.clip_mode, agent.skip_nonfinite, agent.batch_size = True, 'tensor', False, 8
    agent.rng = np.random.default_rng(0)
    agent._augmenter, agent.device = None, 'cpu'
    agent.__dict__.update(kw)
    return agent


def _rows(agent, seed=1):
    rng = np.random.default_rng(seed)
    return {k: torch.as_tensor(rng.random((4, 2) + shape, dtype=np.float32)) for k, shape in agent.state_spec.items()}


def test_plan_layouts_agree():
    assert aug.VIEW_PLAN_DTYPE.itemsize == C.sizeof(aug.ViewPlan) == 112
    assert aug.VIEW_PLAN_DTYPE.names == tuple(n for n, _ in aug.ViewPlan._fields_)
    for name, _ in aug.ViewPlan._fields_:
        assert aug.VIEW_PLAN_DTYPE.fields[name][1] == getattr(aug.ViewPlan, name).offset, name
    assert aug.VIEW_PLAN_DTYPE['blur_w'].shape == (16,)


def test_plans_are_a_pure_function_of_the_seed():
    draw = lambda seed: aug.draw_view_plans(1.0, np.random.default_rng(seed), 64, 90, 120)
    a, b, c = draw(5), draw(5), draw(6)
    assert a.dtype == aug.VIEW_PLAN_DTYPE and a.shape == (64,)
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert len(set(p.tobytes() for p in a)) == 64, 'every view gets its own plan'


@pytest.mark.parametrize('shape,taps', list(zip(SHAPES, (3, 9, 9))))
def test_every_drawn_plan_is_valid(shape, taps):
    H, W = shape
    plans = aug.draw_view_plans(1.0, np.random.default_rng(H + W), 512, H, W, flip_prob=0.5)
    assert aug.pack_view_plans(plans, H, W) is plans or aug.pack_view_plans(plans, H, W).tobytes() == plans.tobytes()
    assert aug.view_blur_taps(H, W) == taps
    assert set(plans['blur_taps'].tolist()) == {0, taps}
    fired = plans['blur_taps'] > 0
    total = plans['blur_w'].astype(np.float64).sum(axis=1)
    assert np.abs(total[fired] - 1.0).max() <= 1e-6 and not plans['blur_w'][~fired].any()
    assert (plans['blur_w'][:, taps:] == 0).all()
    assert plans['crop_h'].min() >= 2 and plans['crop_w'].min() >= 2
    assert (plans['crop_y'] + plans['crop_h']).max() <= H and (plans['crop_x'] + plans['crop_w']).max() <= W
    assert plans['crop_y'].min() >= 0 and plans['crop_x'].min() >= 0
    assert plans['crop_h'].min() < H and plans['crop_y'].max() > 0, 'crops and offsets do vary'
    assert 0 < plans['flip'].sum() < 512
    # the aspect ratio is kept: both sides come from the one fraction
    assert np.abs(plans['crop_h'] / H - plans['crop_w'] / W).max() <= 0.5 / H + 0.5 / W + 1e-12
    # jitter scalars inside draw_plan's ranges at alpha = 1, identity where the jitter does not fire
    j = plans['jitter'] == 1
    assert np.abs(plans['brightness']).max() <= 0.2 and np.abs(plans['hue']).max() <= 0.2
    assert np.abs(plans['contrast'] - 1).max() <= 0.8 + 1e-6 and np.abs(plans['saturation'] - 1).max() <= 0.8 + 1e-6
    assert not plans['brightness'][~j].any() and (plans['contrast'][~j] == 1).all()


def test_firing_rates():
    """4096 plans: 4 binomial sigmas at p = 0.8 are 0.025."""
    plans = aug.draw_view_plans(1.0, np.random.default_rng(18), 4096, 90, 120)
    assert abs((plans['jitter'] == 1).mean() - 0.8) <= 0.025
    assert abs((plans['drop'] == 1).mean() - 0.2) <= 0.025
    assert abs((plans['blur_taps'] > 0).mean() - 0.5) <= 0.025
    assert not plans['flip'].any(), 'flip_prob defaults to 0'
    assert aug.draw_view_plans(1.0, np.random.default_rng(18), 4096, 90, 120, flip_prob=1.0)['flip'].all()


def test_strength_scales_the_jitter_and_no_python_loop_over_plans():
    weak = aug.draw_view_plans(0.25, np.random.default_rng(3), 256, 23, 31, jitter_prob=1.0)
    assert np.abs(weak['brightness']).max() <= 0.05 + 1e-7 and np.abs(weak['contrast'] - 1).max() <= 0.2 + 1e-6

    class Counting:
        """Forwards to a Generator and counts the calls: one per field, whatever the number of plans."""
        def __init__(self):
            self.rng, self.calls = np.random.default_rng(0), 0

        def __getattr__(self, name):
            self.calls += 1
            return getattr(self.rng, name)

    few, many = Counting(), Counting()
    aug.draw_view_plans(1.0, few, 2, 90, 120)
    aug.draw_view_plans(1.0, many, 2048, 90, 120)
    assert few.calls == many.calls <= 16


def test_option_refusals():
    draw = lambda **kw: aug.draw_view_plans(1.0, np.random.default_rng(0), 4, 23, 31, **kw)
    for bad in ((0.0, 1.0), (0.5, 1.2), (0.9, 0.5), (-0.1, 0.5), 0.5):
        with pytest.raises(ValueError, match='crop_scale'):
            draw(crop_scale=bad)
    for name in ('flip_prob', 'jitter_prob', 'drop_prob', 'blur_prob'):
        for bad in (-0.01, 1.01):
            with pytest.raises(ValueError, match=name):
                draw(**{name: bad})
    with pytest.raises(ValueError, match='blur_sigma'):
        draw(blur_sigma=(0.0, 1.0))
    with pytest.raises(ValueError, match='unknown view option'):
        aug.check_view_options(crop=(0.5, 1.0))
    with pytest.raises(ValueError, match='2 x 2'):
        aug.draw_view_plans(1.0, np.random.default_rng(0), 4, 1, 31)
    assert len(draw(crop_scale=(1.0, 1.0))) == 4 and len(aug.draw_view_plans(1.0, np.random.default_rng(0), 0, 23, 31)) == 0


def test_plan_refusals_name_the_plans():
    H, W = 23, 31
    good = views_ref.plan(H, W)
    w3 = list(views_ref.gaussian(3, 1.0))

    def refused(match, indices, *bad):
        plans = [good, *bad, good]
        with pytest.raises(ValueError, match=match) as e:
            aug.pack_view_plans(plans, H, W)
        assert str(indices) in str(e.value), str(e.value)

    refused('outside', [1], dict(good, crop_y=1))                                    # full height at offset 1
    refused('outside', [1, 2], dict(good, crop_x=-1, crop_w=4), dict(good, crop_x=W - 3, crop_w=4))
    refused('smaller than 2', [1, 2], dict(good, crop_h=1), dict(good, crop_w=0))
    refused('blur_taps', [1, 2, 3, 4], dict(good, blur_taps=4, blur_w=[0.25] * 4), dict(good, blur_taps=17, blur_w=[1 / 16] * 16),
            dict(good, blur_taps=1, blur_w=[1.0]), dict(good, blur_taps=-3))
    refused('sum to 1', [1, 2], dict(good, blur_taps=3, blur_w=[0.3, 0.3, 0.3]), dict(good, blur_taps=3, blur_w=[0.5, 0.5, 2e-5]))
    refused('sum to 1', [2], dict(good, blur_taps=3, blur_w=w3), dict(good, blur_taps=3, blur_w=[np.nan, 0.5, 0.5]))
    with pytest.raises(ValueError, match='VIEW_PLAN_DTYPE'):
        aug.pack_view_plans(np.zeros(3, np.float32), H, W)
    ok = aug.pack_view_plans([good, dict(good, blur_taps=3, blur_w=w3, crop_y=H - 2, crop_h=2)], H, W)
    assert ok.dtype == aug.VIEW_PLAN_DTYPE and ok['blur_taps'].tolist() == [0, 3] and ok['crop_h'].tolist() == [H, 2]
    assert ok.tobytes()[:112] == aug.empty_view_plans(1, H, W).tobytes()
    # plans drawn for one frame size are refused at a smaller one
    with pytest.raises(ValueError, match='outside'):
        aug.pack_view_plans(aug.draw_view_plans(1.0, np.random.default_rng(0), 8, 90, 120), 23, 31)


def test_view_pipeline_keyword():
    assert CARLAgent.view_pipeline == 'agent' and CARLAgent.view_options == {}
    assert _stub().view_pipeline == 'agent'
    env = FakeCARLAEnvironment(image_shape=(4, 6, 3), time_horizon=2, num_waypoints=5, vehicle_features=4, num_actions=2)
    for bad in ('SimCLR', 'crop', None, 3):
        with pytest.raises(ValueError, match='view_pipeline'):
            CARLAgent(env, view_pipeline=bad)
    with pytest.raises(ValueError, match='unknown view option'):
        CARLAgent(env, view_pipeline=dict(crop=(0.5, 1.0)))
    with pytest.raises(ValueError, match='drop_prob'):
        CARLAgent(env, view_pipeline=dict(drop_prob=2.0))
    assert CARLAgent.parse_view_pipeline('agent') == ('agent', {})
    assert CARLAgent.parse_view_pipeline('simclr') == ('simclr', {})
    assert CARLAgent.parse_view_pipeline(dict(flip_prob=0.5)) == ('simclr', dict(flip_prob=0.5))


def test_agent_pipeline_is_untouched(monkeypatch):
    """view_pipeline='agent': the plans are draw_plans' dicts and the views never reach Augmenter.views."""
    def boom(*a, **k):
        raise AssertionError('Augmenter.views reached')

    monkeypatch.setattr(aug.Augmenter, 'views', boom)
    monkeypatch.setattr(aug, 'draw_view_plans', boom)
    agent = _stub()
    plans = agent.representation_plans(1.0, np.random.default_rng(5), 8, 1)
    want = aug.draw_plans(1.0, np.random.default_rng(5), 8, first_offset=1)
    assert isinstance(plans, list) and len(plans) == 8 and [p['offset'] for p in plans] == list(range(1, 9))
    assert [(p['seed'], p['jitter'], p['blur_size'], tuple(p['blur_kernel'])) for p in plans] == \
        [(p['seed'], p['jitter'], p['blur_size'], tuple(p['blur_kernel'])) for p in want]
    rows = _rows(agent)
    out = agent.representation_views(rows, [], 'keep')
    for k, v in rows.items():
        assert torch.equal(out[k][:4], v) and torch.equal(out[k][4:], v), k


def test_simclr_plans_and_the_intensity_zero_views():
    agent = _stub(view_pipeline='simclr', view_options=dict(flip_prob=1.0))
    plans = agent.representation_plans(0.5, np.random.default_rng(5), 8, 1)
    want = aug.draw_view_plans(0.5, np.random.default_rng(5), 8, 4, 6, flip_prob=1.0)
    assert isinstance(plans, np.ndarray) and plans.tobytes() == want.tobytes() and plans['flip'].all()
    none = agent.representation_plans(0.0, np.random.default_rng(5), 8, 1)
    assert isinstance(none, list) and none == []
    rows = _rows(agent)
    zero = agent.representation_views(rows, none, 'zero')
    assert torch.equal(zero['state_image'][:4], rows['state_image']) and torch.equal(zero['state_image'][4:], rows['state_image'])
    for k in ('state_road', 'state_vehicle', 'state_navigation'):
        assert zero[k].shape[0] == 8 and not zero[k].any(), k


def test_record_plans_go_to_augmenter_views_without_a_doubled_copy(monkeypatch):
    seen = {}

    class Fake:
        def views(self, rows, plans, copies=2):
            seen.update(rows=rows, plans=plans, copies=copies)
            return torch.cat([rows, rows]) + 1.0

    agent = _stub(view_pipeline='simclr', _augmenter=Fake())
    rows = _rows(agent)
    plans = agent.representation_plans(1.0, np.random.default_rng(2), 8, 1)
    out = agent.representation_views(rows, plans, 'keep')
    assert seen['rows'] is rows['state_image'] and seen['plans'] is plans and seen['copies'] == 2
    assert torch.equal(out['state_image'], torch.cat([rows['state_image']] * 2) + 1.0)
    assert torch.equal(out['state_road'], torch.cat([rows['state_road']] * 2))
    assert set(out) == set(CARLAgent.STATE_KEYS)


@pytest.mark.parametrize('name', list(views_ref.cases()))
def test_the_reference_holds_alone(name):
    """float32 run against float64 run on the device test's inputs, at the device test's bounds."""
    shape, plans, jitter = views_ref.cases()[name]
    N, T, H, W = shape
    plans = views_ref.as_dicts(aug.pack_view_plans(plans, H, W))
    rows = views_ref.rows_of(shape)
    r64, r32 = views_ref.views(rows, plans), views_ref.views(rows, plans, np.float32)
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and r64.shape == (2 * N, T, H, W, 3)
    figures = views_ref.check(r32, r64, jitter)
    print(name, figures)


def test_the_reference_identity_and_flip_are_exact():
    rows = views_ref.rows_of(views_ref.SMALL)
    N, T, H, W = views_ref.SMALL
    for dtype in (np.float32, np.float64):
        same = views_ref.views(rows, [views_ref.plan(H, W)] * 6, dtype)
        assert np.array_equal(same, np.concatenate([rows, rows]).astype(dtype))
        flipped = views_ref.views(rows, [views_ref.plan(H, W, flip=1)] * 6, dtype)
        assert np.array_equal(flipped, np.concatenate([rows, rows])[:, :, :, ::-1].astype(dtype))
