"""cdrl_bn_plan against an independent restatement of vcol_geom and of the three dispatch predicates of csrc/bn.hip (bn_apply_t,
bn_bwd_reduce, bn_bwd_apply), for every case of tests/test_gpu_bn_variants.py (the same buffer layouts, built on the CPU -- the query
launches nothing and only looks at the views' numbers) and for a sweep of (Mg, C).  Also, on the CPU: the coverage the GPU module
asserts, its size limit, and the float32-numpy evaluation of dy behind its per-channel bound.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from carla_driving_rl_agent_amd import _lib
from tests import bn_ref
from tests import test_gpu_bn_variants as V

NB_STATS, NB_APPLY = 128, 2048


def cdiv(a, b):
    return -(-a // b)


def vcol_geom(Mg, Cc, max_blocks):
    """vec channels per thread; C / vec lanes, at most 256 per pass; the rest of the 256 threads are row lanes; a block takes at
    least two rows per row lane and a whole number of row-lane steps"""
    vec = 4 if Cc % 4 == 0 else 2 if Cc % 2 == 0 else 1
    lanes = Cc // vec
    cx = min(lanes, 256)
    cy = max(256 // cx, 1)
    rb = cdiv(max(cdiv(Mg, max_blocks), 2 * cy), cy) * cy
    return dict(vec=vec, cx=cx, cy=cy, nloop=cdiv(lanes, cx), rb=rb, nb=cdiv(Mg, rb))


def aligned(view, vec):
    """view: (address, ld, coff) or None"""
    return int(view is not None and view[1] % vec == 0 and view[2] % vec == 0 and view[0] % (4 * vec) == 0)


def expected_plan(y, out, dout, shuffle_ctot, Mg, Cc, has_stats, relu6, pass_src, pass_gdst, dy_addr, bcast):
    a = vcol_geom(Mg, Cc, NB_APPLY)
    v = a['vec']
    a.update(al0=aligned(y, v), al1=aligned(out, v), al2=aligned(pass_src, v))
    a['form'] = int(bool(has_stats and shuffle_ctot and a['nloop'] == 1 and v >= 2 and a['al0'] and (pass_src is None or a['al2'])))
    r = vcol_geom(Mg, Cc, NB_STATS)
    r.update(al0=aligned(dout, v), al1=aligned(y, v), al2=aligned(pass_gdst, v))
    dense = y[1] == Cc and y[2] == 0 and r['al1']
    r['form'] = int(bool(not bcast and shuffle_ctot and relu6 and r['nloop'] == 1 and dense and v >= 2 and (pass_gdst is None or r['al2'])))
    b = vcol_geom(Mg, Cc, NB_STATS)
    b.update(al0=aligned(dout, v), al1=aligned(y, v), al2=int(dy_addr % (4 * v) == 0))
    b['form'] = int(bool(b['nloop'] == 1 and v >= 2 and dense and b['al2']))
    return dict(apply=a, reduce=r, bapply=b)


def tup(v):
    return None if v is None else (v.p, v.ld, v.coff)


@pytest.mark.parametrize('c,dt', V.PARAMS)
def test_plan_of_every_gpu_case(lib, c, dt):
    b = V.setup(c, dt, 'cpu')
    assert c.G in (1, 3, 4) and c.G * c.Mg * c.C < 1_000_000
    got = V.plan(lib, c, b)
    v = [tup(x) for x in V.views(c, b)]
    want = expected_plan(v[0], v[1], v[2], b.ctot, c.Mg, c.C, not c.nostats, c.relu6, v[3], v[6], b.dy.t.data_ptr(), c.bcast)
    assert got == want, (got, want)
    for k in got:
        assert got[k]['nb'] * got[k]['rb'] >= c.Mg > (got[k]['nb'] - 1) * got[k]['rb']
    forms = [got[k]['form'] for k, on in (('apply', c.fwd and not c.bcast), ('reduce', c.bwd), ('bapply', c.bwd)) if on]
    assert tuple(forms) == tuple(c.expect), (got, c.expect)


def test_plan_sweep(lib):
    """C in 1..1100, Mg in {1, 7, 100, 4097}, dense aligned views with shuffle + ReLU6 + pass-through (everything the fast forms ask of
    the arguments, so the form depends on the geometry alone) and the plain form."""
    base = 1 << 20
    out = (C.c_int32 * 30)()
    for Cc in range(1, 1101):
        for Mg in (1, 7, 100, 4097):
            for sh in (0, 1):
                ctot = 2 * Cc if sh else 0
                y, wide, wide0 = _lib.View(base, Cc, 0), _lib.View(base, 2 * Cc, Cc), _lib.View(base, 2 * Cc, 0)
                ps = C.byref(wide0) if sh else None
                n = lib.cdrl_bn_plan(C.byref(y), C.byref(wide), C.byref(wide), ctot, 3, Mg, Cc, 1, 1, ps, ps, ps, ps, C.c_void_p(base), 0, 0, out, 30)
                assert n == 30
                got = {k: dict(zip(V.PLAN_FIELDS, out[10 * i:10 * i + 10])) for i, k in enumerate(('apply', 'reduce', 'bapply'))}
                p0 = (base, 2 * Cc, 0) if sh else None
                want = expected_plan((base, Cc, 0), (base, 2 * Cc, Cc), (base, 2 * Cc, Cc), ctot, Mg, Cc, 1, 1, p0, p0, base, 0)
                assert got == want, (Cc, Mg, sh, got, want)
                for k in got:
                    assert got[k]['nb'] * got[k]['rb'] >= Mg > (got[k]['nb'] - 1) * got[k]['rb'], (Cc, Mg, k, got[k])


def test_plan_refuses_bad_arguments(lib):
    y = _lib.View(1 << 20, 8, 0)
    out = (C.c_int32 * 30)()
    r = C.byref(y)
    assert lib.cdrl_bn_plan(r, r, r, 0, 1, 0, 8, 1, 1, None, None, None, None, None, 0, 0, out, 30) < 0           # Mg = 0
    assert lib.cdrl_bn_plan(r, r, r, 0, 1, 10, 8, 1, 1, None, None, None, None, None, 3, 0, out, 30) < 0          # Mg % bcast_rows
    assert lib.cdrl_bn_plan(r, r, r, 0, 1, 10, 8, 1, 1, r, None, None, None, None, 0, 0, out, 30) < 0             # half a pair
    assert lib.cdrl_bn_plan(r, r, r, 0, 1, 10, 8, 1, 1, None, None, None, None, None, 0, 2, out, 30) < 0          # tensor type
    assert lib.cdrl_bn_plan(r, r, r, 0, 1, 10, 8, 1, 1, None, None, None, None, None, 0, 0, out, 30) == 30


def test_coverage_on_the_host(lib):
    """What tests/test_gpu_bn_variants.py::test_coverage asserts on the GPU, from the same buffers built on the CPU."""
    missing = V.coverage_gaps(lib, 'cpu')
    assert not missing, missing


def test_float32_numpy_meets_the_per_channel_bound():
    """The per-channel 2e-5 bound of dy: the same formula evaluated in float32 numpy against the float64 reference, on every case's
    inputs, stays below a quarter of it.  Worst value over the cases: 1.4e-6."""
    worst = 0.0
    for c in V.CASES:
        if not c.bwd:
            continue
        for dt in c.types:
            inp = V.setup(c, dt, 'cpu').inp
            stats = bn_ref.train_stats(inp.y, *bn_ref.draw_affine(c.C), c.G, c.Mg) if c.real else inp.stats
            ref = bn_ref.backward(inp.y, inp.d, stats, c.G, c.Mg, c.relu6, c.bcast)
            e = V.f32_numpy_noise(c, inp, stats, ref)
            assert e * V.F32_NUMPY_MARGIN < V.TOL, (V.case_id(c, dt), e)
            worst = max(worst, e)
    print(f'worst float32-numpy dy error per channel: {worst:.3e}')


def test_reference_pieces():
    """the reference's own building blocks against hand-computed values"""
    assert bn_ref.shuffle_map(np.arange(8), 8).tolist() == [0, 4, 1, 5, 2, 6, 3, 7]
    assert bn_ref.view_cols(4, 4, 8).tolist() == [2, 6, 3, 7] and bn_ref.view_cols(3, 2, 0).tolist() == [3, 4]
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e38], np.float32)             # ties to even: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert bn_ref.to_bf16(x).tolist()[:3] == [1.0, 1.0, 1.015625]
    st = np.array([[[1.0]], [[2.0]], [[3.0]], [[-1.0]]], np.float32)
    y = np.array([[0.0], [1.0], [2.0], [3.0]], np.float32)                       # z = -1, 2, 5, 8: closed, open, open, closed
    r = bn_ref.backward(y, np.ones((4, 1), np.float32), st, 1, 4, 1)
    assert r.s1.item() == 2.0 and r.s2.item() == 0.0 + 2.0 and r.dbeta.item() == 2.0                                    # xhat = -2, 0, 2, 4
    assert np.allclose(r.dy[:, 0], 3.0 * (np.array([0, 1, 1, 0]) - 0.5 - np.array([-2, 0, 2, 4]) * 0.5))
    assert bn_ref.apply(y, st, 1, 4, 1)[:, 0].tolist() == [0.0, 2.0, 5.0, 6.0]
    assert bn_ref.gap(np.arange(8.0).reshape(4, 2), 2).tolist() == [[1.0, 2.0], [5.0, 6.0]]
