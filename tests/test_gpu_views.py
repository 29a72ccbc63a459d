"""The contrastive view pipeline on the device (cdrl_views_batch) against its float64 restatement
(tests/views_ref.py): the exact cases, every stage alone and all together, the per-view and per-frame wiring, the guards."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import views_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, T, H, W = views_ref.SMALL
_REF = {}


def _aug():
    from carla_driving_rl_agent_amd.rl.augmentations import Augmenter
    return Augmenter(DEV)


def _small():
    if 'rows' not in _REF:
        _REF['rows'] = views_ref.rows_of(views_ref.SMALL)
        _REF['dev'] = torch.as_tensor(_REF['rows']).to(DEV)
    return _REF['rows'], _REF['dev']


def _packed(plans, h=H, w=W):
    from carla_driving_rl_agent_amd.rl.augmentations import pack_view_plans
    return pack_view_plans(plans, h, w)


def test_exact_cases(lib):
    rows, dev = _small()
    twice = torch.cat([dev, dev])
    aug = _aug()
    assert torch.equal(aug.views(dev, [views_ref.plan(H, W)] * 6), twice), 'empty plan'
    full = views_ref.plan(H, W, crop_y=0, crop_x=0, crop_h=H, crop_w=W)
    assert torch.equal(aug.views(dev, [full] * 6), twice), 'full-size crop'
    assert torch.equal(aug.views(dev, [views_ref.plan(H, W, flip=1)] * 6), twice.flip(3)), 'flip'
    assert torch.equal(aug.views(dev, [views_ref.plan(H, W)] * 9, copies=3), torch.cat([dev, dev, dev])), 'three copies'
    _, plans, _ = views_ref.cases()['mixed']
    a, b = aug.views(dev, plans), aug.views(dev, plans)
    assert torch.equal(a, b) and not torch.equal(a, twice), 'same call twice'
    assert torch.equal(dev, torch.as_tensor(rows).to(DEV)), 'the rows are only read'


@pytest.mark.parametrize('name', list(views_ref.cases()))
def test_matches_the_reference(lib, name):
    shape, plans, jitter = views_ref.cases()[name]
    rows = views_ref.rows_of(shape)
    packed = _packed(plans, shape[2], shape[3])
    got = _aug().views(torch.as_tensor(rows).to(DEV), packed).cpu().numpy()
    ref = views_ref.views(rows, views_ref.as_dicts(packed))
    assert got.shape == ref.shape == (2 * shape[0], shape[1], shape[2], shape[3], 3)
    print(name, views_ref.check(got, ref, jitter))


def test_views_are_wired_per_view(lib):
    """Six different plans in one call = six one-view calls, bit for bit."""
    _, dev = _small()
    packed = _packed(views_ref.cases()['mixed'][1])
    aug = _aug()
    together = aug.views(dev, packed)
    for v in range(6):
        alone = aug.views(dev[v % N:v % N + 1], packed[v:v + 1], copies=1)
        assert torch.equal(together[v:v + 1], alone), v
    assert not torch.equal(together[0], together[3]), 'views 0 and 3 share a row, not a plan'


def test_frames_share_the_geometry_not_the_mean(lib):
    packed = _packed(views_ref.cases()['mixed'][1])
    same = torch.as_tensor(views_ref.rows_of(views_ref.SMALL, equal_frames=True)).to(DEV)
    out = _aug().views(same, packed)
    assert torch.equal(out[:, 0], out[:, 1]), 'equal frames stay equal under every plan'
    # two different frames under one contrast-heavy plan: each is shifted about ITS OWN mean
    rows = views_ref.rows_of(views_ref.SMALL)
    rows[:, 1] *= 0.25
    one = _packed([views_ref.plan(H, W, **views_ref.JITTER)] * 6)
    got = _aug().views(torch.as_tensor(rows).to(DEV), one).cpu().numpy()
    print(views_ref.check(got, views_ref.views(rows, views_ref.as_dicts(one)), True))


def _call(lib, rows, n, out, v, t, h, w, plans, ws):
    ptr = lambda x: C.c_void_p(x.data_ptr() if x is not None else None)
    rc = lib.cdrl_views_batch(ptr(rows), n, ptr(out), v, t, h, w, ptr(plans), ptr(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_guards_and_refusals(lib):
    rows, dev = _small()
    packed = _packed(views_ref.cases()['mixed'][1])
    plans = torch.from_numpy(packed.view(np.uint8)).to(DEV)
    V, n = 6, T * H * W * 3
    need = int(lib.cdrl_views_workspace_floats(V, T, H, W))
    assert need == V * (2 * n + 3 * T) and lib.cdrl_views_workspace_floats(0, T, H, W) == 0
    pad, canary = 4096, -7.5
    out_buf = torch.full((V * n + 2 * pad,), canary, device=DEV)
    ws_buf = torch.full((need + 2 * pad,), canary, device=DEV)
    out, ws = out_buf[pad:pad + V * n], ws_buf[pad:pad + need]
    assert _call(lib, dev, N, out, V, T, H, W, plans, ws) == 0
    want = _aug().views(dev, packed)
    assert torch.equal(out.view_as(want), want)
    for buf, m in ((out_buf, V * n), (ws_buf, need)):
        assert (buf[:pad] == canary).all() and (buf[pad + m:] == canary).all()

    def refused(what, *args):
        out.fill_(canary)
        rc = _call(lib, *args)
        msg = lib.cdrl_last_error()
        assert rc < 0 and msg, what
        assert (out == canary).all(), f'{what}: something was launched'
        return msg.decode()

    for i, what in ((0, 'rows'), (2, 'out'), (7, 'plans'), (8, 'workspace')):
        args = [dev, N, out, V, T, H, W, plans, ws]
        args[i] = None
        assert 'null' in refused(f'null {what}', *args)
    assert 'shape' in refused('H < 2', dev, N, out, V, T, 1, W, plans, ws)
    assert 'shape' in refused('W < 2', dev, N, out, V, T, H, 1, plans, ws)
    assert 'shape' in refused('T < 1', dev, N, out, V, 0, H, W, plans, ws)
    for v, n_rows in ((0, 1), (-1, 1), (V, 0), (V, V + 1)):
        assert 'V' in refused(f'V {v}, N {n_rows}', dev, n_rows, out, v, T, H, W, plans, ws)
    assert 'overlaps' in refused('workspace = rows', dev, N, out, V, T, H, W, plans, dev)
    assert 'overlaps' in refused('workspace = out', dev, N, out, V, T, H, W, plans, out)
    assert 'overlaps' in refused('workspace ends inside out', dev, N, out, V, T, H, W, plans, out_buf[:need])
    assert 'overlaps' in refused('workspace starts inside rows', dev, N, out, V, T, H, W, plans, dev.view(-1)[-8:])
