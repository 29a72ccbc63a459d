"""cdrl_gemm_nn_plan against an independent restatement of the dispatch ladder of gemm_nn (csrc/gemm.hip) as the commit before the plan
struct had it (tests/nn_ref.py::expected_plan), over a sweep of shapes, B orders and view alignments, with the invariants the kernels rely
on.  The sweep producing no (NT, WR) outside REQUIRED is the proof that the removed launch_nn<2, 4> / launch_nn<4, 4> branches were dead.
Also, on the CPU: the coverage the GPU module asserts, its cases' plans, the engine products, the exactness condition of its exact inputs,
and tests/nn_ref.py against hand-computed values.  The query launches nothing and reads no memory.  No GPU."""
import ctypes as C

import numpy as np

from carla_driving_rl_agent_amd import _lib
from tests import nn_ref
from tests import test_gpu_nn_variants as V
from tests.nn_ref import RT, SPLITK, TILE, cdiv

BASE = 1 << 20
SWEEP_M = (1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 12288)
SWEEP = (1, 2, 3, 4, 5, 9, 16, 24, 31, 32, 33, 58, 64, 65, 92, 96, 97, 116, 128, 129, 130, 132, 232, 255, 256, 257, 300, 320, 352, 464, 512, 768, 2048)


def views(K):
    """(name, a address, ld, coff, B address): dense, padded with an even offset, odd ld, odd offset, pointers = 4 mod 8 and = 8 mod 16"""
    even = K + K % 2
    return (('dense', BASE, K, 0, BASE), ('pad', BASE, even + 6, 2, BASE), ('pad4', BASE, cdiv(K, 4) * 4 + 8, 4, BASE), ('oddld', BASE, even + 5, 0, BASE),
            ('oddoff', BASE, even + 6, 1, BASE), ('p4', BASE + 4, K, 0, BASE + 4), ('p8', BASE + 8, K, 0, BASE + 8), ('b8', BASE, K, 0, BASE + 8))


def invariants(lib, p, M, N, K, a_addr, ld, coff):
    assert p['gz'] * p['kchunk'] >= K > (p['gz'] - 1) * p['kchunk'] or (p['gz'] == 1 and K < 1)
    assert p['kchunk'] % 32 == 0
    assert p['ws_elems'] <= lib.cdrl_gemm_nn_workspace_elems(M, N, K)
    if p['kernel'] == SPLITK:
        assert p['NT'] % 2 == 0 and p['WR'] == 2 and p['gz'] >= 2 and M <= 2048 and K >= 256
        assert p['ws_elems'] == p['gz'] * M * N and p['act_fused'] == 1 and 1 <= p['reduce_grid'] <= 2048
        assert (p['gz'] - 1) * p['kchunk'] < K                  # no empty slab: every slab writes its piece of the workspace
    else:
        assert p['gz'] == 1 and p['ws_elems'] == 0 and p['act_fused'] == 0 and p['reduce_grid'] == 0
    if p['kernel'] == RT:
        assert p['a16'] and p['b16'] and p['NT'] == 3 and M >= 2048 and N >= 129 and K >= 64
        assert (p['gx'], p['gy']) == (cdiv(M, 96), cdiv(N, 128))
        assert K % 4 == 0 and ld % 4 == 0 and coff % 4 == 0 and a_addr % 16 == 0       # every float4 address of a is 16-byte aligned
    else:
        assert (p['NT'], p['WR']) in ((1, 4), (3, 4), (2, 2), (4, 2))
        assert p['gx'] == cdiv(M, 32 * p['WR']) and p['gy'] * 32 * p['NT'] >= N > (p['gy'] - 1) * 32 * p['NT']
        if p['VEC']:
            assert nn_ref.vec_addresses_aligned(M, K, a_addr, ld, coff, p['kchunk'], p['gz'])
    if p['a16']:
        assert all((a_addr + 4 * (m * ld + coff + k)) % 16 == 0 for m in range(min(M, 3)) for k in range(0, K, 4))


def test_plan_sweep(lib):
    """M, K, N over the sweep, both B orders, with and without workspace, the view alignments in rotation (all of them for a subset)"""
    seen, i = set(), 0
    for M in SWEEP_M:
        for K in SWEEP:
            for N in SWEEP:
                i += 1
                vs = views(K)
                for name, a_addr, ld, coff, b_addr in (vs if (K in (64, 65, 232, 256) or N in (132, 232)) else (vs[0], vs[1 + i % 7])):
                    for order in ('w', 'wt'):
                        sbk, sbn = nn_ref.b_strides(order, K, N)
                        for ws in (0, 1):
                            got = V.plan_of(lib, M, N, K, a_addr, ld, coff, b_addr, sbk, sbn, ws)
                            want = nn_ref.expected_plan(M, N, K, a_addr, ld, coff, b_addr, sbk, sbn, ws)
                            assert got == want, (M, K, N, name, order, ws, got, want)
                            invariants(lib, got, M, N, K, a_addr, ld, coff)
                            seen.add(nn_ref.signature(got))
    assert seen == V.REQUIRED, (sorted(seen - V.REQUIRED), sorted(V.REQUIRED - seen))


def test_named_decisions(lib):
    q = lambda M, K, N, ws=1, order='w', a=None: V.plan_of(lib, M, N, K, BASE, *(a or (K, 0)), BASE, *nn_ref.b_strides(order, K, N), ws)      # noqa: E731
    # 2048 x 256 x 2048: 32 x 16 = 512 workgroups collapse to one split and fall through: to the row-stacked kernel with 16-byte rows, else to the tile kernel
    p = q(2048, 256, 2048)
    assert (p['kernel'], p['gz'], p['ws_elems'], p['NT'], p['WR']) == (RT, 1, 0, 3, 0)
    p = q(2048, 256, 2048, a=(258, 2))
    assert (p['kernel'], p['gz'], p['ws_elems'], p['NT'], p['WR']) == (TILE, 1, 0, 4, 2)
    assert q(2048, 256, 64)['kernel'] == SPLITK and q(2049, 256, 64)['kernel'] == TILE and q(64, 255, 64)['kernel'] == TILE
    assert q(64, 256, 96)['kernel'] == TILE and q(64, 256, 64, ws=0)['kernel'] == TILE
    p = q(1, 256, 33)
    assert (p['gz'], p['kchunk'], p['ws_elems'], p['reduce_grid']) == (8, 32, 8 * 33, 1)
    p = q(65, 257, 128)
    assert (p['gz'], p['kchunk'], 257 - (p['gz'] - 1) * p['kchunk'], p['VEC']) == (5, 64, 1, 0)
    p = q(64, 300, 64)
    assert (p['gz'], p['kchunk'], 300 - (p['gz'] - 1) * p['kchunk']) == (5, 64, 44)
    for order in ('w', 'wt'):
        p = q(1024, 768, 768, order=order)
        assert (p['kernel'], p['NT'], p['gx'], p['gy'], p['gz'], p['kchunk'], p['reduce_grid']) == (SPLITK, 4, 16, 6, 6, 128, 2048)
    assert [q(64, 32, N, ws=0)['NT'] for N in (129, 232, 320)] == [3, 4, 4] and [q(64, 32, N, ws=0)['gy'] for N in (129, 232, 320)] == [2, 2, 3]
    # the row-stacked kernel needs 16-byte rows on both operands; N = 129 only through W^T
    assert q(12288, 232, 232, ws=0)['kernel'] == RT and q(12288, 232, 232, ws=0, a=(238, 2))['kernel'] == TILE
    assert q(2048, 64, 129, ws=0)['kernel'] == TILE and q(2048, 64, 129, ws=0, order='wt')['kernel'] == RT
    # empty products launch nothing
    for M, N in ((0, 64), (64, 0), (-1, 64)):
        p = q(M, 64, N)
        assert p['kernel'] == -1 and p['ws_elems'] == 0, p


def test_query_arguments(lib):
    v = _lib.View(None, 64, 0)
    out = (C.c_int32 * 14)()
    assert lib.cdrl_gemm_nn_plan(C.byref(v), 0, 64, 1, 64, 64, 64, 0, out, 14) == 14 and out[0] == TILE       # null pointers are fine
    assert lib.cdrl_gemm_nn_plan(C.byref(v), 0, 64, 1, 64, 64, 64, 0, out, 3) == 14
    assert lib.cdrl_gemm_nn_plan(C.byref(v), 0, 64, 1, 64, 64, 64, 0, None, 14) == -1 and lib.cdrl_last_error()
    assert lib.cdrl_gemm_nn_plan(None, 0, 64, 1, 64, 64, 64, 0, out, 14) == -1
    assert lib.cdrl_gemm_nn_plan(C.byref(_lib.View(None, 64, 1)), 0, 64, 1, 64, 64, 64, 0, out, 14) == -1 and b'fit' in lib.cdrl_last_error()
    assert lib.cdrl_gemm_nn_workspace_elems(2048, 64, 256) == 8 * 2048 * 64 and lib.cdrl_gemm_nn_workspace_elems(2049, 64, 256) == 0
    assert lib.cdrl_gemm_nn_workspace_elems(64, 64, 255) == 0 and lib.cdrl_gemm_nn_workspace_elems(0, 64, 256) == 0
    # the entry refuses before anything is launched (host pointers would fault otherwise)
    w, done = _lib.View(BASE, 64, 0), C.c_int(5)
    ex = lambda a, c, ws, ao, act, B=BASE: lib.cdrl_gemm_nn_ex(C.byref(a), C.c_void_p(B) if B else None, 64, 1, None, C.byref(c), 64, 64, 64, 0,      # noqa: E731
                                                               C.c_void_p(ws) if ws else None, C.c_void_p(ao) if ao else None, act, C.byref(done), None)
    assert ex(_lib.View(BASE, 64, 1), w, 0, 0, 0) == -1 and b'fit' in lib.cdrl_last_error() and done.value == 0
    assert ex(w, _lib.View(BASE, 63, 0), 0, 0, 0) == -1 and b'fit' in lib.cdrl_last_error()
    assert ex(w, _lib.View(BASE, 64, -1), 0, 0, 0) == -1
    assert ex(v, w, 0, 0, 0) == -1 and ex(w, v, 0, 0, 0) == -1 and ex(w, w, 0, 0, 0, B=0) == -1 and b'null' in lib.cdrl_last_error()
    assert ex(w, w, 0, BASE, 1) == -1 and b'workspace' in lib.cdrl_last_error()
    assert ex(w, w, 0, 0, 5) == -1 and ex(w, w, 0, 0, -1) == -1 and b'activation' in lib.cdrl_last_error()
    for fn, args in (('cdrl_act_fwd', (None, None, 4, 0, None)), ('cdrl_act_bwd', (None, None, None, 4, 0, None)), ('cdrl_permute_bt', (None, None, 1, 1, 1, None)),
                     ('cdrl_colsum', (C.byref(w), 4, 4, None, None)), ('cdrl_reduce_partials', (None, 1, 1, 0, 1, None, None, 0, None))):
        assert getattr(lib, fn)(*args) == -1 and lib.cdrl_last_error(), fn
    assert lib.cdrl_act_fwd(C.c_void_p(BASE), C.c_void_p(BASE), 4, 7, None) == -1 and lib.cdrl_act_fwd(C.c_void_p(BASE), C.c_void_p(BASE), 0, 1, None) == -1
    assert lib.cdrl_reduce_partials(C.c_void_p(BASE), 4, 4, 2, 5, C.c_void_p(BASE), C.c_void_p(BASE), 0, None) == -1        # rows shorter than n1 + n2
    assert lib.cdrl_reduce_partials(C.c_void_p(BASE), 4, 4, 2, 6, C.c_void_p(BASE), None, 0, None) == -1                    # n2 without out2


def test_bias_gradient_queries(lib):
    for rows in (1, 2, 255, 256, 257, 1024, 5000):
        for Cn in (1, 2, 5, 16, 96, 320, 512, 768, 1028):
            assert lib.cdrl_colsum_partial_rows(rows, Cn) == nn_ref.vcol_geom(rows, Cn)[5]
    assert nn_ref.vcol_geom(1024, 1028)[:4] == (4, 256, 1, 2) and nn_ref.vcol_geom(1024, 116)[:3] == (4, 29, 8) and nn_ref.vcol_geom(256, 5)[:3] == (1, 5, 51)
    for nparts in (1, 63, 64, 65, 511, 512, 513, 1025):
        for n in (1, 4, 37, 2032, 2033, 2048, 2053):
            assert lib.cdrl_reduce_partials_cx(nparts, n, 0) == lib.cdrl_reduce_partials_cx(nparts, n - n // 2, n // 2) == nn_ref.reduce_cx(nparts, n)
    assert [nn_ref.reduce_cx(p, n) for p, n in ((64, 37), (65, 37), (65, 2032), (65, 2033), (1025, 2053))] == [16, 4, 4, 16, 16]
    assert lib.cdrl_colsum_partial_rows(0, 4) == 0 and lib.cdrl_reduce_partials_cx(0, 4, 0) == 0


def test_plan_of_every_gpu_case(lib):
    """the GPU module's cases, their expectations and the restatement agree (the same check_plan the GPU run starts every case with)"""
    for c in V.CASES:
        p = V.plan_query(lib, c)
        V.check_plan(lib, p, c)
        L, cnt = V.chain(p, c)
        assert 2 <= cnt <= 3 and 1 <= L <= max(c.K, 32 + 8)
        if p['kernel'] == SPLITK:
            assert L == p['kchunk'] + p['gz'] < c.K


def test_coverage_on_the_host(lib):
    """What tests/test_gpu_nn_variants.py::test_coverage and ::test_engine_products assert on the GPU (the plan queries need none)."""
    V.test_coverage(lib)
    V.test_engine_products(lib)
    have = {nn_ref.signature(V.plan_query(lib, c)) for c in V.CASES}
    assert have == V.REQUIRED


def test_engine_products_table():
    """the products of the default network at minibatch 256, written out by hand: (M, K, N, order, workspace, fused activation)"""
    got = {(p['M'], p['K'], p['N'], p['order'], p['ws'], p['act']) for p in V.engine_products() if p['M'] in (256, 1024)}
    R6, S6 = nn_ref.RELU6, nn_ref.SWISH6
    want = {(1024, 9, 16, 'w', False, None), (1024, 4, 16, 'w', False, None), (1024, 5, 16, 'w', False, None), (1024, 16, 16, 'w', False, None),
            (1024, 16, 16, 'wt', False, None), (1024, 768, 768, 'w', True, None), (1024, 768, 768, 'wt', True, None), (1024, 16, 96, 'w', False, None),
            (1024, 96, 16, 'wt', False, None), (256, 352, 512, 'w', True, None), (256, 512, 352, 'wt', True, None), (256, 512, 320, 'w', True, S6),
            (256, 320, 512, 'wt', True, None), (256, 320, 320, 'w', True, S6), (256, 320, 320, 'wt', True, None)}
    assert got == want, (sorted(got - want, key=str), sorted(want - got, key=str))
    assert R6 == 1 and all(p['dense_out'] and not p['acc'] for p in V.engine_products())


def test_exact_cases_satisfy_their_condition():
    """the integer inputs of every case: integers within their ranges, S < 2^24 for every output element"""
    for c in V.CASES:
        inp = nn_ref.draw([11, c.M, c.K, c.N, len(c.a), len(c.order), c.acc, 1], c.M, c.K, c.N, c.bias, c.acc, True)
        assert nn_ref.exact_condition(inp), V.case_id(c)
        assert (np.abs(inp.A).max() > 512 or inp.A.size < 64) and (inp.bias is None) == (not c.bias) and (inp.base is None) == (not c.acc)


def test_reference_pieces():
    """the reference's own building blocks against hand-computed values"""
    A, Bm = np.array([[1, 2], [3, -4]], np.float32), np.array([[1, 0, 2], [-1, 1, 0]], np.float32)
    c, s = nn_ref.product(A, Bm, np.array([10, 20, 30]), np.array([[1, 1, 1], [-2, -2, -2]]))
    assert c.tolist() == [[-1 + 11, 2 + 21, 2 + 31], [7 + 8, -4 + 18, 6 + 28]] and s.tolist() == [[3 + 11, 2 + 21, 2 + 31], [7 + 12, 4 + 22, 6 + 32]]
    for order in ('w', 'wt'):
        sbk, sbn = nn_ref.b_strides(order, 2, 3)
        assert np.array_equal(nn_ref.b_logical(nn_ref.b_flat(Bm, order), 2, 3, sbk, sbn), Bm)
    assert nn_ref.b_strides('w', 2, 3) == (3, 1) and nn_ref.b_strides('wt', 2, 3) == (1, 2) and nn_ref.b_flat(Bm, 'wt').tolist() == [1, -1, 0, 1, 2, 0]
    whole = np.arange(20.0)
    assert nn_ref.a_logical(whole, 2, 7, 3, 2).tolist() == [[3, 4], [10, 11]]
    x = np.array([-1.0, -0.0, 0.0, 1e-45, 3.0, 6.0, 7.0])
    assert nn_ref.act_fwd(x, nn_ref.RELU6).tolist() == [0, 0, 0, 1e-45, 3, 6, 6] and nn_ref.act_deriv(x, nn_ref.RELU6).tolist() == [0, 0, 0, 1, 1, 0, 0]
    assert np.allclose(nn_ref.act_fwd(np.array([0.0, 1.0, -1.0]), nn_ref.SWISH6), [0.0, 0.7310585786300049, -0.2689414213699951], rtol=1e-15)
    assert np.allclose(nn_ref.act_deriv(np.array([0.0, 1.0]), nn_ref.SWISH6), [0.5, 0.9276705118714867], rtol=1e-14)
    assert np.allclose(nn_ref.act_deriv(np.array([0.0, 1.0]), nn_ref.TANH), [1.0, 0.41997434161402614], rtol=1e-14)
    assert np.allclose(nn_ref.act_deriv(np.array([0.0, 2.0, -2.0]), nn_ref.SIGMOID), [0.25, 0.10499358540350652, 0.10499358540350652], rtol=1e-14)
    assert nn_ref.act_fwd(np.array([-1000.0, 1000.0]), nn_ref.SIGMOID).tolist() == [0.0, 1.0] and np.isfinite(nn_ref.act_deriv(np.array([-1000.0, 1000.0]), nn_ref.TANH)).all()
    xs, below, above = nn_ref.swish6_clamp()
    assert abs(xs - 6.01466) < 1e-5 and abs(float(nn_ref.swish(xs)) - 6.0) < 1e-12 and np.nextafter(below, np.float32(7)) == above
    assert nn_ref.act_fwd(np.array([float(below), float(above), 20.0]), nn_ref.SWISH6).tolist()[1:] == [6.0, 6.0]
    assert nn_ref.act_deriv(np.array([float(below), float(above), 20.0]), nn_ref.SWISH6).tolist()[1:] == [0.0, 0.0]
    assert nn_ref.act_deriv(np.array([float(below)]), nn_ref.SWISH6)[0] > 1.0
    xi = nn_ref.act_inputs(300)
    for v in (0.0, 6.0, below, above, 20.0, -88.0, 100.0, np.nextafter(np.float32(6), np.float32(0)), np.nextafter(np.float32(0), np.float32(1))):
        assert (xi == np.float32(v)).any(), v
    assert np.signbit(xi[xi == 0]).any() and not np.signbit(xi[xi == 0]).all() and nn_ref.act_inputs(1).shape == (1,)
    assert nn_ref.units(np.array([1.0 + 2.0 ** -23]), np.array([1.0]))[0] == 2.0
    assert nn_ref.f32_sum(np.array([[2.0 ** 24, 1.0], [1.0, 1.0]])).tolist() == [2.0 ** 24, 2.0]
    assert nn_ref.f32_sum(np.array([[3.0], [4.0]]), np.array([0.5], np.float32)).tolist() == [7.5]
    assert nn_ref.permute_bt(np.arange(6), 3, 2, 1).tolist() == [0, 2, 4, 1, 3, 5]
    # the restated ladder at hand-computed points
    e = nn_ref.expected_plan(128, 232, 32, BASE, 32, 0, BASE, 232, 1, 0)
    assert (e['kernel'], e['NT'], e['WR'], e['gx'], e['gy'], e['VEC'], e['a16'], e['b16']) == (TILE, 4, 2, 2, 2, 1, 1, 1)
    e = nn_ref.expected_plan(128, 92, 33, BASE, 33, 0, BASE, 1, 33, 0)
    assert (e['kernel'], e['NT'], e['WR'], e['gx'], e['gy'], e['BT'], e['VEC'], e['b16']) == (TILE, 3, 4, 1, 1, 1, 0, 0)
    assert nn_ref.vec_addresses_aligned(4, 64, BASE, 64, 0, nn_ref.NO_CHUNK, 1) and not nn_ref.vec_addresses_aligned(4, 64, BASE, 65, 0, nn_ref.NO_CHUNK, 1)
    assert not nn_ref.vec_addresses_aligned(4, 64, BASE + 4, 64, 0, nn_ref.NO_CHUNK, 1) and not nn_ref.vec_addresses_aligned(4, 64, BASE, 64, 1, nn_ref.NO_CHUNK, 1)
