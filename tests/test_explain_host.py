"""Host side of CARLAgent.explain (explain.py): the cell geometry, the row count, the argument checks of explain()
itself (raised before anything touches a device) and the declarations of the new entry points."""
import os
import re
import types

import numpy as np
import pytest

from carla_driving_rl_agent_amd import _lib, explain
from carla_driving_rl_agent_amd.core import CARLAgent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('cdrl_occlusion_baseline', 'cdrl_occlusion_rows', 'cdrl_occlusion_scores', 'cdrl_occlusion_maps')


@pytest.mark.parametrize('H,W,gh,gw', [(5, 7, 2, 3), (5, 7, 5, 7), (5, 7, 1, 1), (90, 120, 6, 8), (90, 360, 4, 9)])
def test_cells_partition_the_frame(H, W, gh, gw):
    cells = explain.occlusion_cells(H, W, gh, gw)
    assert len(cells) == gh * gw
    cover = np.zeros((H, W), np.int64)
    for (y0, y1, x0, x1) in cells:
        assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W            # inside the frame and not empty
        cover[y0:y1, x0:x1] += 1
    assert (cover == 1).all()                                     # every pixel in exactly one cell
    # row-major: cell (cy, cx) sits at cy * gw + cx and follows the stated integer rule
    for cy in range(gh):
        for cx in range(gw):
            assert cells[cy * gw + cx] == ((cy * H) // gh, ((cy + 1) * H) // gh, (cx * W) // gw, ((cx + 1) * W) // gw)


def test_cells_refuse_a_grid_outside_the_frame():
    for gh, gw in ((0, 1), (1, 0), (6, 7), (5, 8), (-1, 3)):
        with pytest.raises(ValueError):
            explain.occlusion_cells(5, 7, gh, gw)


def test_row_count():
    for T in (1, 2, 4):
        for gh, gw in ((1, 1), (3, 4), (6, 8)):
            for per_frame in (False, True):
                for modalities in (False, True):
                    F = T if per_frame else 1
                    assert explain.occlusion_frames(T, per_frame) == F
                    assert explain.occlusion_row_count(T, gh, gw, per_frame, modalities) == 1 + F * gh * gw + (4 if modalities else 0)
    assert explain.occlusion_row_count(4, 6, 8, False, True) == 53 and explain.occlusion_row_count(4, 9, 12, True, True) == 437
    assert explain.score_names(2) == ['kl', 'value', 'mean_0', 'mean_1']


def _state(E=2, T=2, H=6, W=8):
    return dict(state_image=np.zeros((E, T, H, W, 3), np.float32), state_road=np.zeros((E, T, 9), np.float32),
                state_vehicle=np.zeros((E, T, 4), np.float32), state_navigation=np.zeros((E, T, 5), np.float32))


GIVEN = np.zeros((2, 6, 8, 3), np.float32)          # a baseline stack of the right shape: no device call in front of the network
MISUSE = [(dict(grid=(0, 4)), r'^explain: grid \(0, 4\) outside 1\.\.6 x 1\.\.8$'),
          (dict(grid=(3, 0)), r'^explain: grid \(3, 0\) outside 1\.\.6 x 1\.\.8$'),
          (dict(grid=(7, 4)), r'^explain: grid \(7, 4\) outside 1\.\.6 x 1\.\.8$'),
          (dict(grid=(3, 9)), r'^explain: grid \(3, 9\) outside 1\.\.6 x 1\.\.8$'),
          (dict(grid=5), r'^explain: grid must be a pair \(gh, gw\), got 5$'),
          (dict(baseline='median'), r"^explain: baseline 'median': one of \('zero', 'mean'\) or a \(2, 6, 8, 3\) tensor$"),
          (dict(baseline=np.zeros((2, 6, 8), np.float32)), r'^explain: a baseline stack must be \(2, 6, 8, 3\), got \(2, 6, 8\)$'),
          (dict(baseline=np.zeros((1, 6, 8, 3), np.float32)), r'^explain: a baseline stack must be \(2, 6, 8, 3\), got \(1, 6, 8, 3\)$'),
          (dict(upsample='cubic'), r"^explain: upsample 'cubic': one of \('nearest', 'bilinear'\)$"),
          (dict(chunk=0), r'^explain: chunk = 0: 1 to 65535 rows per forward$'),
          (dict(chunk=-3), r'^explain: chunk = -3: 1 to 65535 rows per forward$'),
          (dict(chunk=65536), r'^explain: chunk = 65536: 1 to 65535 rows per forward$'),
          (dict(row=2), r'^explain: row 2 outside 0\.\.1$'),
          (dict(row=-1), r'^explain: row -1 outside 0\.\.1$')]


def _stub():
    return types.SimpleNamespace(device='cpu', num_actions=2)        # (no `network`: reaching it is an AttributeError)


@pytest.mark.parametrize('kw,message', MISUSE, ids=[repr(sorted(kw.items())[0]) for kw, _ in MISUSE])
def test_explain_refuses_misuse_before_it_touches_the_network(kw, message):
    """CARLAgent.explain on a stand-in without a network: every listed misuse raises the ValueError of explain's own check, with
    its own text.  Every other argument is valid (a given baseline of the right shape), so nothing else can raise in its place."""
    args = dict(baseline=GIVEN)
    args.update(kw)
    with pytest.raises(ValueError, match=message):
        CARLAgent.explain(_stub(), _state(), **args)
    # the pure check raises the same
    with pytest.raises(ValueError, match=message):
        explain.check_arguments((2, 2, 6, 8, 3), 2, args.get('grid', (6, 8)), args['baseline'], args.get('upsample', 'nearest'),
                                args.get('chunk', 32), args.get('row', 0))


@pytest.mark.parametrize('kw', [dict(), dict(grid=(1, 1)), dict(grid=(6, 8), upsample='bilinear', chunk=1, row=1),
                                dict(chunk=65535, per_frame=True, modalities=False, normalize=False)])
def test_a_valid_call_gets_past_the_checks(kw):
    """The same stand-in with nothing wrong: the call passes every check and fails only where it reaches for the network."""
    with pytest.raises(AttributeError, match='network'):
        CARLAgent.explain(_stub(), _state(), baseline=GIVEN, **kw)


def test_check_arguments_accepts_what_is_allowed():
    shape = (2, 2, 6, 8, 3)
    assert explain.check_arguments(shape, 2, (3, 4), 'mean', 'nearest', 32, 0) == (3, 4, 1, 0)
    assert explain.check_arguments(shape, 2, (6, 8), 'zero', 'bilinear', 1, 1) == (6, 8, 0, 1)
    assert explain.check_arguments(shape, 2, [1, 1], np.zeros((2, 6, 8, 3), np.float32), 'nearest', 64, 1) == (1, 1, None, 0)


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, 'include', 'cdrl.h')) as f:
        header = f.read()
    for name in ENTRIES:
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in _lib.PROTOTYPES
    assert 'explain' in _build_sources()


def _build_sources():
    import importlib.util
    spec = importlib.util.spec_from_file_location('cdrl_build_for_test', os.path.join(ROOT, 'carla-driving-rl-agent_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SOURCES
