"""cdrl_pwconv_plan, cdrl_pwconv_x3_plan and cdrl_pwconv_x3_wide_bwd_plan against an independent restatement of the dispatch of pw_nn, pw_x3
and pw_x3_wide_bwd as the commit before the plan structs had it (tests/pwf_ref.py), over a sweep of groups, rows, channel counts, prologue /
epilogue / accumulate / mode combinations and view alignments, with the invariants the kernels rely on.  The sweep reaching exactly the
REQUIRED sets of tests/test_gpu_pw_variants.py shows that the ladders hold nothing the plans cannot select and select nothing the ladders
lack.  Also, on the CPU: the GPU module's coverage, its cases' exactness condition, the restatement against hand-computed plans, and the
signatures the engine's own dry build reaches in the three compute modes.  The queries launch nothing and read no
memory.  No GPU."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np

from carla_driving_rl_agent_amd import _lib
from tests import pwf_ref as R
from tests import test_gpu_pw_variants as V
from tests.test_gemm_nn_plan_host import BASE, views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS = (1, 3, 4, 8, 128)
MGS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 389, 3072, 20000)
CH = (2, 4, 24, 26, 32, 34, 58, 64, 66, 92, 96, 97, 116, 128, 129, 130, 232, 256, 258)
LDS_LIMIT = 160 * 1024


def q_nn(lib, a_addr, ld, coff, G, Mg, N, K, pro, epi, acc, packed, pbf, at, part, y_addr=BASE):
    out = (C.c_int32 * len(R.NN_FIELDS))()
    rc = lib.cdrl_pwconv_plan(C.byref(_lib.View(a_addr, ld, coff)), C.byref(_lib.View(BASE, N, 0)), y_addr, G, Mg, N, K, pro, epi, acc, packed, pbf, at,
                              part, out, len(R.NN_FIELDS))
    return dict(zip(R.NN_FIELDS, out)), rc


def q_x3(lib, a_addr, ld, coff, G, Mg, N, K, pro, epi, packed=1, nbpg=0):
    out = (C.c_int32 * len(R.X3_FIELDS))()
    rc = lib.cdrl_pwconv_x3_plan(C.byref(_lib.View(a_addr, ld, coff)), C.byref(_lib.View(BASE, N, 0)), G, Mg, N, K, pro, epi, packed, nbpg, out,
                                 len(R.X3_FIELDS))
    return dict(zip(R.X3_FIELDS, out)), rc


def q_x3b(lib, a_addr, ld, coff, G, Mg, N, K, ctot, epi, acc, operands=1, c_ld=None):
    out = (C.c_int32 * len(R.X3B_FIELDS))()
    rc = lib.cdrl_pwconv_x3_wide_bwd_plan(C.byref(_lib.View(a_addr, ld, coff)), C.byref(_lib.View(BASE, c_ld or N, 0)), G, Mg, N, K, ctot, epi, acc,
                                          operands, out, len(R.X3B_FIELDS))
    return dict(zip(R.X3B_FIELDS, out)), rc


def nn_invariants(lib, p, G, Mg, N, K):
    assert p['nbpg'] * p['tpb'] >= p['tiles_g'] >= p['nbpg'] >= 1             # no workgroup is without a tile
    assert p['tpb'] == R.cdiv(p['tiles_g'], p['nbpg']) and (p['gx'], p['gy']) == (G * p['nbpg'], R.cdiv(N, 128))
    assert p['tiles_g'] * p['bm'] >= Mg > (p['tiles_g'] - 1) * p['bm'] and p['wc'] * p['wr'] == 4 and p['bm'] == 32 * p['wr']
    assert p['lds_bytes'] == R.nn_lds_bytes(p['ksm'], p['nt'], p['pro']) <= LDS_LIMIT
    assert p['gy'] * 32 * p['nt'] >= N and 2 * p['ksm'] >= K and p['nbpg'] == lib.cdrl_pwconv_fused_partial_rows(G, Mg, N, K)
    assert p['packed_elems'] == lib.cdrl_pwconv_pack_elems(N, K)


def test_pw_nn_plan_sweep(lib):
    """G, Mg, K, N over the sweep with the view alignments in rotation; at a rotating (G, Mg) every prologue / epilogue / accumulate / mode /
    packing combination, the partial buffer and every alignment"""
    seen, refused, i = set(), set(), 0
    combos = [(pro, epi, acc, packed, pbf, at, part) for pro in range(3) for epi in range(3) for acc in (0, 1) for packed, pbf in ((0, 0), (1, 0), (1, 1))
              for at in (0, 1) for part in (0, 1)]
    for K in CH + (0, 1, 3):
        for N in CH + (0, 1):
            vs = views(max(K, 2))
            for gi, G in enumerate(GS + (0,)):
                for mi, Mg in enumerate(MGS + (0,)):
                    i += 1
                    full = (gi + mi + i) % 23 == 0
                    for ci, cb in enumerate(combos if full else (combos[i % len(combos)], combos[(7 * i + 3) % len(combos)])):
                        for name, a_addr, ld, coff, y_addr in (vs if full and ci % 9 == 0 else (vs[0], vs[1 + (i + ci) % 7])):
                            got, rc = q_nn(lib, a_addr, ld, coff, G, Mg, N, K, *cb, y_addr=y_addr)
                            want, why = R.nn_expected(G, Mg, N, K, *cb, a_addr, ld, coff, y_addr)
                            assert got == want and rc == (0 if want['ok'] else -1), (G, Mg, N, K, cb, name, got, want, why)
                            refused.update(why[:1])
                            if rc != 0:
                                assert lib.cdrl_last_error().startswith(b'pw_nn: ')
                            if G >= 1 and Mg >= 1 and N >= 1 and K <= 256 and N <= 256:
                                if got['ok']:
                                    nn_invariants(lib, got, G, Mg, N, K)
                                    seen.add(R.nn_signature(got))
    # a 2 GB operand: 20000 x 128 rows of 232 floats
    got, rc = q_nn(lib, BASE, 232, 0, 128, 140000, 116, 116, 0, 0, 0, 0, 0, 0, 0)
    want, why = R.nn_expected(128, 140000, 116, 116, 0, 0, 0, 0, 0, 0, 0, BASE, 232, 0)
    assert got == want and rc == -1 and why == ['big']
    refused.add('big')
    assert seen == V.REQUIRED, (sorted(seen - V.REQUIRED)[:5], sorted(V.REQUIRED - seen)[:5])
    assert refused == set(R.NN_REFUSALS), refused


def test_pw_x3_plan_sweep(lib):
    seen, refused, i = set(), set(), 0
    for K in CH + (0, 3, 5):
        for N in CH + (0, 1):
            for G in GS + (0,):
                for Mg in MGS + (0,):
                    i += 1
                    vs = views(max(K, 2))
                    for name, a_addr, ld, coff, _ in (vs if i % 11 == 0 else (vs[0], vs[1 + i % 7])):
                        for pro, epi in (((0, 0), (0, 1), (1, 0), (1, 1)) if i % 3 == 0 else ((i % 2, (i // 2) % 2),)):
                            for packed, nbpg in ((1, 0), (1, 1 + i % 5), (i % 2, R.cdiv(max(Mg, 1), 32)), (1, 700)):
                                got, rc = q_x3(lib, a_addr, ld, coff, G, Mg, N, K, pro, epi, packed, nbpg)
                                want, why = R.x3_expected(G, Mg, N, K, pro, epi, packed, nbpg, a_addr, ld, coff)
                                assert got == want and rc == (0 if want['ok'] else -1), (G, Mg, N, K, pro, epi, packed, nbpg, name, got, want, why)
                                refused.update(why[:1])
                                if got['ok']:
                                    assert 1 <= got['nbpg'] <= got['tiles_g'] and got['tiles_g'] * got['bm'] >= Mg > (got['tiles_g'] - 1) * got['bm']
                                    assert got['gx'] == G * got['nbpg'] and got['gy'] * 128 >= N and got['kp'] >= K
                                    assert got['packed_bytes'] == lib.cdrl_pwconv_x3_packed_bytes_n(K, N)
                                    if nbpg == 0:
                                        assert got['nbpg'] == lib.cdrl_pwconv_x3_partial_rows(G, Mg, N, K)
                                    # every 16-byte chunk a thread loads starts at a multiple of what the form's loads need (dword; 16 bytes)
                                    assert (a_addr + 4 * coff) % (16 if got['form'] else 8) == 0 and (4 * ld) % (16 if got['form'] else 8) == 0
                                    seen.add(R.x3_signature(got))
    got, rc = q_x3(lib, BASE, 232, 0, 128, 140000, 116, 116, 0, 0)
    assert rc == -1 and got == R.x3_expected(128, 140000, 116, 116, 0, 0, 1, 0, BASE, 232, 0)[0] and got['refusal'] == R.X3_REFUSALS['big']
    refused.add('big')
    assert seen == V.REQUIRED_X3, (sorted(seen - V.REQUIRED_X3), sorted(V.REQUIRED_X3 - seen))
    assert refused == set(R.X3_REFUSALS), refused


def test_pw_x3_wide_bwd_plan_sweep(lib):
    seen, refused, i = set(), set(), 0
    for K in CH:
        for N in CH + (1,):
            for G in (1, 4, 128, 0):
                for Mg in (1, 31, 32, 33, 65, 3072, 0):
                    i += 1
                    vs = views(K)
                    for name, a_addr, ld, coff, _ in (vs if i % 5 == 0 else (vs[0], vs[1 + i % 7])):
                        for ctot, vld, vcoff in ((0, ld, coff), (2 * K, 2 * K, (0, K, 1)[i % 3]), (2 * K + 2, 2 * K + 2, 0)):
                            for epi, acc, operands in ((0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1), (i % 2, 0, 0)):
                                got, rc = q_x3b(lib, a_addr, vld, vcoff, G, Mg, N, K, ctot, epi, acc, operands)
                                want, why = R.x3b_expected(G, Mg, N, K, ctot, epi, acc, operands, a_addr, vld, vcoff, N)
                                assert got == want and rc == (0 if want['ok'] else -1), (G, Mg, N, K, ctot, vld, vcoff, epi, acc, name, got, want, why)
                                refused.update(why[:1])
                                assert got['rows'] == lib.cdrl_pwconv_x3_wide_bwd_rows(Mg)
                                if got['ok']:
                                    assert got['rows'] * 32 >= Mg > (got['rows'] - 1) * 32 and (got['gx'], got['gy']) == (G * got['rows'], R.cdiv(N, 128))
                                    seen.add(R.x3b_signature(got))
    got, rc = q_x3b(lib, BASE, 232, 0, 128, 20000, 232, 232, 0, 0, 0)
    assert rc == -1 and got['refusal'] == R.X3B_REFUSALS['big'] and got == R.x3b_expected(128, 20000, 232, 232, 0, 0, 0, 1, BASE, 232, 0, 232)[0]
    refused.add('big')
    assert b'not instantiated together' in (q_x3b(lib, BASE, 232, 0, 4, 64, 232, 232, 0, 1, 1)[1] == -1 and lib.cdrl_last_error())
    assert seen == V.REQUIRED_X3B and refused == set(R.X3B_REFUSALS), (seen, refused)


def test_restatement_against_hand_computed_plans():
    """tests/pwf_ref.py at points worked out by hand from the kernels' tile shapes"""
    # 116 -> 116 channels, 4 groups of 3072 rows: K pairs pad to 64, four column tiles of one wave each -> 32-row tiles, 96 per group;
    # 64 / 4 runs two workgroups per CU: 512 / 4 = 128 per group would be more than 96 tiles -> one tile each
    p, why = R.nn_expected(4, 3072, 116, 116, 0, 1, 0, 1, 0, 0, 1, BASE, 116, 0)
    assert not why and (p['ksm'], p['nt'], p['wc'], p['wr'], p['bm'], p['tiles_g'], p['occ'], p['nbpg'], p['tpb'], p['gx'], p['gy']) == (64, 4, 4, 1, 32, 96, 2, 96, 1, 384, 1)
    assert p['lds_bytes'] == 32 * 130 * 4 and p['packed_elems'] == 4 * 2 * 32 * 64
    # 232 -> 232, 4 x 3072: K pairs pad to 128, one workgroup per CU, two column blocks: 256 / 8 = 32 workgroups per group walk 3 tiles each
    p, why = R.nn_expected(4, 3072, 232, 232, 2, 2, 0, 1, 0, 0, 1, BASE, 232, 0, BASE)
    assert not why and (p['ksm'], p['nt'], p['bm'], p['tiles_g'], p['occ'], p['nbpg'], p['tpb'], p['gx'], p['gy']) == (128, 4, 32, 96, 1, 32, 3, 128, 2)
    assert p['lds_bytes'] == (32 * 258 + 14 * 128) * 4
    # 24 -> 58 at 128 groups of 389 rows: 16 pairs, two column tiles -> 64-row tiles, 7 per group; three workgroups per CU: 768 / 128 = 6 per group
    p, why = R.nn_expected(128, 389, 58, 24, 1, 1, 0, 0, 0, 0, 1, BASE, 24, 0)
    assert not why and (p['ksm'], p['nt'], p['bm'], p['tiles_g'], p['occ'], p['nbpg'], p['tpb']) == (16, 2, 64, 7, 3, 6, 2)
    assert p['lds_bytes'] == 64 * 34 * 4                # 8704 bytes: above the 2 x 2 x 64 doubles of the epilogue and the 4096 of the scratch
    # three column tiles need K <= 64; K > 128 needs N > 96; an odd offset; an epilogue without its buffer; accumulate with an epilogue stays a run-time add
    assert R.nn_expected(4, 64, 96, 66, 0, 0, 0, 0, 0, 0, 0, BASE, 66, 0)[1] == ['tile'] and R.nn_expected(4, 64, 96, 130, 0, 0, 0, 0, 0, 0, 0, BASE, 130, 0)[1] == ['tile']
    assert R.nn_expected(4, 64, 64, 64, 0, 0, 0, 0, 0, 0, 0, BASE, 66, 1)[1] == ['align'] and R.nn_expected(4, 64, 64, 64, 2, 0, 0, 0, 0, 0, 0, BASE, 67, 1, BASE)[1] == []
    assert R.nn_expected(4, 64, 64, 64, 2, 0, 0, 0, 0, 0, 0, BASE, 64, 0, BASE + 4)[1] == ['align'] and R.nn_expected(4, 64, 64, 64, 0, 1, 0, 0, 0, 0, 0, BASE, 64, 0)[1] == ['part']
    assert R.nn_expected(4, 64, 64, 64, 0, 1, 1, 0, 0, 0, 1, BASE, 64, 0)[0]['acc'] == 0 and R.nn_expected(4, 64, 64, 64, 1, 2, 0, 0, 0, 0, 1, BASE, 64, 0)[1] == ['pro_epi']
    assert R.nn_expected(4, 64, 64, 64, 0, 0, 0, 1, 0, 1, 0, BASE, 64, 0)[1] == ['storage'] and R.nn_expected(4, 64, 64, 64, 0, 0, 0, 1, 1, 1, 0, BASE, 64, 0)[0]['mode'] == 2
    # x3: 58 channels at a 232-byte pitch and offset 58 run the persistent form; 232 needs multiples of 4; 128 groups of 5 tiles get 4 workgroups
    p, why = R.x3_expected(4, 3072, 58, 58, 1, 1, 1, 0, BASE, 116, 58)
    assert not why and (p['form'], p['kp'], p['nt'], p['bm'], p['tiles_g'], p['nbpg']) == (0, 64, 2, 64, 48, 48)
    p, why = R.x3_expected(4, 3072, 232, 232, 1, 1, 1, 0, BASE, 232, 0)
    assert not why and (p['form'], p['kp'], p['nt'], p['bm'], p['nbpg'], p['gx'], p['gy'], p['packed_bytes']) == (1, 256, 4, 32, 96, 384, 2, 2 * 3 * 16 * 2 * 128 * 8 * 2)
    assert R.x3_expected(4, 3072, 232, 232, 1, 1, 1, 0, BASE, 234, 2)[1] == ['align'] and R.x3_expected(4, 3072, 232, 230, 1, 1, 1, 0, BASE, 230, 0)[1] == ['shape']
    assert R.x3_expected(128, 131, 97, 64, 0, 1, 1, 0, BASE, 64, 0)[0]['nbpg'] == 4 and R.x3_expected(128, 131, 97, 64, 0, 1, 1, 5, BASE, 64, 0)[0]['nbpg'] == 5
    assert R.x3_expected(128, 131, 97, 64, 0, 1, 1, 6, BASE, 64, 0)[1] == ['nbpg'] and R.x3_expected(4, 65, 232, 232, 0, 1, 1, 2, BASE, 232, 0)[1] == ['nbpg']
    # wide backward: dense dz in multiples of 4, shuffled dz with an even half width
    assert R.x3b_expected(4, 65, 232, 232, 0, 1, 0, 1, BASE, 232, 0, 232)[0]['rows'] == 3 and R.x3b_expected(4, 65, 232, 232, 0, 0, 0, 1, BASE, 234, 2, 232)[1] == ['align']
    assert R.x3b_expected(4, 65, 232, 232, 464, 0, 0, 1, BASE, 464, 2, 232)[1] == [] and R.x3b_expected(4, 65, 232, 232, 466, 0, 0, 1, BASE, 466, 0, 232)[1] == ['align']
    assert R.x3b_expected(4, 65, 116, 116, 0, 0, 0, 1, BASE, 116, 0, 116)[1] == ['shape'] and R.x3b_expected(4, 65, 232, 232, 0, 1, 1, 1, BASE, 232, 0, 232)[1] == ['epi_acc']
    # the op's pieces
    assert R.fma32(np.float32(3), np.float32(0.5), np.float32(0.25)) == np.float32(1.75)
    assert R.relu6_mask(np.array([0, 1, 12, 13], np.float32), np.float32(0.5), np.float32(0)).tolist() == [False, True, False, False]
    ap = R.prologue(2, np.array([[4.0, 4.0]]), 1, 1, stats=np.array([[[1, 1]], [[2, 2]], [[1, 1]], [[0, 7]]], np.float32),
                    coef=np.array([[[0.5, 0.5]], [[1, 1]], [[2, 2]]], np.float32), y=np.array([[3.0, 3.0]]), relu6=True)
    assert ap.tolist() == [[0.5 * ((4 - 1) - 4 * 2), 0.5 * ((0 - 1) - 4 * 2)]]              # second column: z = 3 + 7 is beyond 6 -> masked
    c, s = R.product(np.array([[1, -2]], np.float32), np.array([[3], [4]], np.float32), np.array([10.0]), np.array([[-1.0]]))
    assert c.tolist() == [[3 - 8 + 10 - 1]] and s.tolist() == [[3 + 8 + 10 + 1]]
    assert R.stats_partials(np.array([[1.0], [2.0], [3.0], [4.0]]), 2, 2).tolist() == [[[3.0], [5.0]], [[7.0], [25.0]]]
    assert R.bound(64, 1.0) == 67 * 2.0 ** -24 and R.bound(64, 1.0, x3=True) == (384 + 8) * 2.0 ** -24


def test_query_arguments(lib):
    v, out = _lib.View(None, 64, 0), (C.c_int32 * 19)()
    args = (0, 4, 64, 64, 64, 0, 0, 0, 0, 0, 0, 0)
    assert lib.cdrl_pwconv_plan(C.byref(v), C.byref(v), *args, out, 19) == 0 and out[0] == 1        # null pointers are fine
    assert lib.cdrl_pwconv_plan(C.byref(v), C.byref(v), *args, out, 18) == -1 and b'exactly 19' in lib.cdrl_last_error()
    assert lib.cdrl_pwconv_plan(None, C.byref(v), *args, out, 19) == -1 and lib.cdrl_pwconv_plan(C.byref(v), C.byref(v), *args, None, 19) == -1
    o13, o8 = (C.c_int32 * 13)(), (C.c_int32 * 8)()
    assert lib.cdrl_pwconv_x3_plan(C.byref(v), C.byref(v), 4, 64, 64, 64, 0, 0, 1, 0, o13, 13) == 0 and lib.cdrl_pwconv_x3_plan(C.byref(v), None, 4, 64, 64, 64, 0, 0, 1, 0, o13, 13) == -1
    assert lib.cdrl_pwconv_x3_wide_bwd_plan(C.byref(v), C.byref(v), 4, 64, 232, 232, 0, 0, 0, 1, o8, 7) == -1
    # the entry refuses before anything is launched (host pointers would fault otherwise)
    w = _lib.View(BASE, 64, 0)
    ex = lambda **kw: lib.cdrl_pwconv_ex(C.byref(kw.get('a', w)), kw.get('st'), kw.get('y'), kw.get('coef'), 0, 0, None, C.c_void_p(BASE), 64, 1, None, C.byref(w), 0,      # noqa: E731
                                         kw.get('G', 4), 64, 64, kw.get('K', 64), kw.get('epi', 0), None, None, kw.get('part'), None, 0, kw.get('at', 0), None)
    assert ex(a=v) == -1 and b'null' in lib.cdrl_last_error() and ex(y=C.c_void_p(BASE)) == -1 and ex(epi=2) == -1
    assert ex(G=0) == -1 and b'nothing to launch' in lib.cdrl_last_error() and ex(K=0) == -1 and b'column pair' in lib.cdrl_last_error()
    assert ex(epi=1) == -1 and b'partial buffer' in lib.cdrl_last_error() and ex(at=1) == -1 and b'bf16' in lib.cdrl_last_error()
    assert ex(a=_lib.View(BASE, 65, 0)) == -1 and b'alignment' in lib.cdrl_last_error() and ex(at=7) == -1


def test_coverage_on_the_host(lib):
    """what tests/test_gpu_pw_variants.py::test_coverage asserts on the GPU (the plan queries need none), and the exactness condition of
    every case's integer inputs"""
    V.test_coverage(lib)
    for c in V.CASES:
        if c.G * c.Mg <= 2048:
            r = R.draw(V.rng_of(c, True), c.G, c.Mg, c.K, c.N, c.pro, c.epi, c.acc, True, bf16=c.mode == 2, relu6=bool(c.relu6))
            assert R.exact_condition(r, bf16=c.mode > 0), V.case_id(c)
            assert (np.abs(r.a).max() >= 2 or r.a.size < 64) and (r.base is None) == (not c.acc) and (r.y is None) == (c.pro != 2)
            c64, s, _ = V.reference(c, r, c.mode)
            assert np.array_equal(c64, np.round(c64 * 16) / 16) and float(s.max()) * 16 < 2 ** 24


DUMP = r'''
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from carla_driving_rl_agent_amd.engine import LearnerEngine
out = {}
for compute in ('f32', 'bf16', 'bf16s'):
    e = LearnerEngine(256, device=None, H=90, W=120, compute=compute)
    n = e.lib.cdrl_learner_pw_signatures(e.h, None, 0)
    buf = C.create_string_buffer(n)
    assert e.lib.cdrl_learner_pw_signatures(e.h, buf, n) == n
    out[compute] = buf.value.decode().split('\n')[:-1]
print(json.dumps(out))
'''

# what the default network's learner launches of this family at minibatch 256, 90 x 120 (DESIGN.md 3.9 has the same table): float32 runs
# its unit convs' forward on the split-precision kernels and their backward in the fused form (csrc/gemm_pw_bwd.hip), which leaves pw_nn
# the backward-data of the one conv neither takes; the bf16 modes run forward and backward-data on pw_nn
ENGINE_NN_BF = ((128, 4, 0, 1, 0), (128, 4, 2, 0, 0), (128, 4, 2, 0, 1), (128, 4, 2, 2, 0), (16, 1, 0, 1, 0), (16, 1, 2, 2, 0), (16, 2, 0, 1, 0), (32, 1, 2, 0, 1),
                (32, 2, 0, 1, 0), (32, 2, 2, 0, 0), (32, 2, 2, 2, 0), (32, 3, 0, 1, 0), (64, 2, 2, 2, 0), (64, 4, 0, 1, 0), (64, 4, 2, 0, 0), (64, 4, 2, 0, 1),
                (64, 4, 2, 2, 0))
ENGINE_REACHED = {
    'f32': {('nn', 128, 4, 2, 0, 0, 1), ('x3', 0, 128, 4, 0, 1), ('x3', 0, 32, 1, 0, 1), ('x3', 0, 32, 2, 0, 1), ('x3', 0, 64, 2, 0, 1), ('x3', 0, 64, 4, 0, 1),
            ('x3', 1, 256, 4, 0, 1), ('x3b', 0, 0, 0), ('x3b', 1, 1, 0)},
    'bf16': {('nn', ksm, nt, pro, epi, 1, acc) for ksm, nt, pro, epi, acc in ENGINE_NN_BF},
    'bf16s': {('nn', ksm, nt, pro, epi, 2, acc) for ksm, nt, pro, epi, acc in ENGINE_NN_BF},
}


@functools.lru_cache(maxsize=None)
def _engine_signatures():
    r = subprocess.run([sys.executable, '-c', DUMP, ROOT], capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if not k.startswith('CDRL_')})
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


def test_engine_reached_signatures():
    """the learner's dry build in the three compute modes: every plan it notes is accepted, is a REQUIRED signature, and the set is the
    written-out one (a change in the planner that reaches another instantiation shows up here)"""
    got = _engine_signatures()
    req = {'nn': V.REQUIRED, 'x3': V.REQUIRED_X3, 'x3b': V.REQUIRED_X3B}
    for compute, lines in got.items():
        recs = [(ln.split()[0],) + tuple(int(x) for x in ln.split()[1:]) for ln in lines]
        assert recs and all(r[1] == 1 for r in recs), (compute, recs)               # ok
        sigs = {(r[0],) + r[2:] for r in recs}
        assert all(s[1:] in req[s[0]] for s in sigs), compute
        assert sigs == ENGINE_REACHED[compute], (compute, sorted(sigs - ENGINE_REACHED[compute]), sorted(ENGINE_REACHED[compute] - sigs))
