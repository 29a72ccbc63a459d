"""cdrl_gemm_tn_plan and cdrl_reduce_partials_plan against an independent restatement of the host decisions of csrc/gemm_tn_direct.hip
(tnd_plan), csrc/gemm_tn_lds.hip (tnl_plan, gemm_tn_lds_supported) and csrc/gemm.hip (the reduce ladder), over a sweep of shapes, with
the invariants the kernels rely on, and every refusal with its code.  Also, on the CPU: the coverage the GPU module asserts, its cases'
plans, the share of flagged operand pairs of its bf16 cases, and tests/tn_ref.py against hand-computed values.  The queries launch
nothing and read no memory.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from carla_driving_rl_agent_amd import _lib
from tests import test_gpu_tn_variants as V
from tests import tn_ref

BASE = 1 << 20
GROUPS, STORAGE, TWO_GB, VIEW = 1, 2, 3, 4
WORDS = {GROUPS: 'multiple of G', STORAGE: 'bf16 activation storage', TWO_GB: '2 GB', VIEW: 'fit'}
SWEEP = (8, 16, 24, 32, 33, 58, 64, 65, 80, 92, 96, 98, 116, 128, 130, 232, 464, 768)


def cdiv(a, b):
    return -(-a // b)


def reduce_form(aligned, nparts, n, stride):
    """0 few partials; 1 / 2 / 3 float4 loads with 16 / 4 / 1 column lanes per block; 4 / 5 scalar with 16 / 4 column lanes"""
    v4 = aligned and n % 4 == 0 and stride % 4 == 0
    if v4 and nparts < 16 and n >= 4096:
        return 0, cdiv(n, 1024)
    if v4 and nparts >= 16:
        if cdiv(n, 64) >= 160:              # enough 64-output blocks to fill the chip
            return 1, cdiv(n, 64)
        if cdiv(n, 16) >= 128 or nparts < 128:
            return 2, cdiv(n, 16)
        return 3, cdiv(n, 4)
    if cdiv(n, 16) >= 128 or nparts <= 64:
        return 4, cdiv(n, 16)
    return 5, cdiv(n, 4)


def lds_ok(a, d, N, K, shuf):
    """pairs of adjacent columns: everything even, and both halves of a shuffled tensor even"""
    return not any(x % 2 for x in (a[0], a[1], d[0], d[1], K, N)) and not (shuf and (shuf // 2) % 2)


def expected(M, N, K, G, apro, dpro, shuf, bf, at, a=None, d=None):
    """the plan of an accepted call for views (ld, coff), dense when not given -- or the refusal code"""
    a, d = a or (K, 0), d or ((shuf or N), 0)
    if G < 1 or M % G:
        return GROUPS
    e = dict(ok=1, refusal=0, kernel=-1, mode=0, apro=apro, dpro=dpro, NJW=0, WK=0, NSPL=0, RS=0, RS2=0, U=0, gy=0, gz=0, nspg=0, nsplit=0,
             rows_per=0, part_slots=0, part_elems=0, reduce_form=0, dhalf=0)
    if M <= 0 or N <= 0 or K <= 0:
        return e
    if at and not bf:
        return STORAGE
    if max(M * a[0], M * d[0], M * N) * 4 >= 1 << 31:
        return TWO_GB
    Mg = M // G
    shuf = shuf if dpro else 0
    e.update(gy=cdiv(K, 128), gz=cdiv(N, 128))
    if K >= 96 and N >= 96 and lds_ok(a, d, N, K, shuf):
        # ~384 workgroups over all column blocks and groups, at least 128 rows each, whole chunks of 32 rows
        ns = max(1, min(Mg // 128, max(1, 384 // (e['gy'] * e['gz'] * G))))
        rows_per = cdiv(cdiv(Mg, ns), 32) * 32
        nspg = cdiv(Mg, rows_per)
        e.update(kernel=2, mode=2 if at else 1 if bf else (0 if V.LDS_F32 else 3), rows_per=rows_per, nspg=nspg, nsplit=G * nspg, part_slots=G * nspg,
                 dhalf=int(bool(shuf) and N % 4 == 2))
    else:
        # the 4 waves go to the tiles of the first 128-block: along k first (n with the D prologue), then along the other side, the rest
        # splits the rows; a wave takes 1, 2 or 4 tiles
        t1, t2 = min(4, cdiv(K, 32)), min(4, cdiv(N, 32))
        if dpro:
            t1, t2 = t2, t1
        wk = 4 if t1 >= 3 else t1
        left = 4 // wk
        nspl = min(left, t2)
        njw = cdiv(t2, nspl)
        njw = 4 if njw == 3 else njw
        rs = left // nspl
        rs2 = 2 if Mg >= 256 else 1
        ns = max(1, min(Mg // (128 * rs2), max(1, 1024 // (e['gy'] * e['gz'] * G * rs))))
        rows_per = cdiv(cdiv(Mg, ns), 2) * 2
        nspg = cdiv(Mg, rows_per)
        e.update(kernel=int(dpro), mode=2 if at else 1 if bf else 0, NJW=njw, WK=wk, NSPL=nspl, RS=rs, RS2=rs2, U=8 if (bf or dpro) else 4,
                 rows_per=rows_per, nspg=nspg, nsplit=G * nspg, part_slots=G * nspg * rs)
    e['part_elems'] = e['part_slots'] * K * N
    e['reduce_form'] = reduce_form(True, e['part_slots'], K * N, K * N)[0]
    return e


def query(lib, M, N, K, G, apro=0, dpro=0, shuf=0, relu=0, bf=0, at=0, a=None, d=None):
    va, vd = _lib.View(BASE, *(a or (K, 0))), _lib.View(BASE, *(d or ((shuf or N), 0)))
    out = (C.c_int32 * len(V.PLAN_FIELDS))()
    n = lib.cdrl_gemm_tn_plan(C.byref(va), C.byref(vd), M, N, K, G, apro, dpro, shuf, relu, bf, at, out, len(out))
    assert n == len(V.PLAN_FIELDS), n
    return dict(zip(V.PLAN_FIELDS, out))


def check(lib, got, want, what):
    if isinstance(want, int):
        assert got['ok'] == 0 and got['refusal'] == want and got['kernel'] == -1, (what, got, want)
        msg = lib.cdrl_last_error().decode()
        assert WORDS[want] in msg or (want == VIEW and 'D prologue' in msg), (what, msg)
    else:
        assert got == want, (what, got, want)


def invariants(lib, p, M, N, K, G):
    """what the kernels rely on, from the plan alone"""
    Mg = M // G
    assert p['NJW'] in ((0,) if p['kernel'] == 2 else (1, 2, 4)) and (p['kernel'] == 1) == (p['dpro'] == 1 and p['kernel'] != 2)
    assert p['part_elems'] <= lib.cdrl_gemm_tn_ex_workspace_elems(M, N, K, G)
    assert p['nspg'] * p['rows_per'] >= Mg > (p['nspg'] - 1) * p['rows_per'] and p['nsplit'] == G * p['nspg']
    if p['kernel'] == 2:
        assert p['rows_per'] % 32 == 0 and p['part_slots'] == p['nsplit']
        return
    assert p['WK'] * p['NSPL'] * p['RS'] <= 4 and p['part_slots'] == p['nsplit'] * p['RS'] and p['rows_per'] % 2 == 0
    # every row of a workgroup belongs to exactly one share; shares are even-sized except possibly the last non-empty one
    TS = p['RS'] * p['RS2']
    for length in {p['rows_per'], Mg - (p['nspg'] - 1) * p['rows_per']}:
        per = (cdiv(length, TS) + 1) // 2 * 2
        covered = 0
        for s in range(TS):
            beg = s * per
            end = min(beg + per, length)
            n = max(0, end - beg)
            assert beg >= covered
            if n:
                assert beg == covered and (n % 2 == 0 or end == length)
                covered = end
        assert covered == length, (length, TS, per)


def mg_set():
    return sorted({m + e for m in (128, 256, 512) for e in (-1, 0, 1)} | {1, 7, 100, 3000})


def test_plan_sweep(lib):
    """K, N over SWEEP, G in 1..4, Mg around 128 / 256 / 512, every prologue combination and operand type along the way"""
    i = 0
    mgs = mg_set()
    for K in SWEEP:
        for N in SWEEP:
            for G in (1, 2, 3, 4):
                for Mg in mgs:
                    i += 1
                    apro, dpro, bf = i & 1, i >> 1 & 1, i % 3
                    shuf = 2 * N if dpro and i % 5 < 2 else 0
                    d = (shuf, N * (i % 2), shuf) if shuf else None
                    got = query(lib, G * Mg, N, K, G, apro, dpro, shuf, dpro * (i % 2), int(bf > 0), int(bf == 2), d=d[:2] if d else None)
                    want = expected(G * Mg, N, K, G, apro, dpro, shuf, int(bf > 0), int(bf == 2), d=d[:2] if d else None)
                    check(lib, got, want, (K, N, G, Mg, apro, dpro, shuf, bf))
                    invariants(lib, got, G * Mg, N, K, G)
                    assert (got['kernel'] == 2) == (K >= 96 and N >= 96 and K % 2 == 0 and N % 2 == 0 and not (shuf and N % 2)), (K, N, shuf)


def test_lds_kernel_exactly_for_supported_wide_views(lib):
    ok = query(lib, 300, 116, 116, 2)
    assert ok['kernel'] == 2
    for kw in (dict(a=(117, 0)), dict(a=(118, 1)), dict(d=(117, 0)), dict(d=(118, 1))):
        p = query(lib, 300, 116, 116, 2, **kw)
        check(lib, p, expected(300, 116, 116, 2, 0, 0, 0, 0, 0, **kw), kw)
        assert p['kernel'] == 0 and p['NJW'] == 4, (kw, p)
    assert query(lib, 300, 116, 116, 2, dpro=1, shuf=234, d=(234, 118))['kernel'] == 1          # an odd half of the shuffled tensor
    assert query(lib, 300, 116, 116, 2, dpro=1, shuf=232, d=(232, 116))['kernel'] == 2
    assert query(lib, 300, 96, 94, 2)['kernel'] == 0 and query(lib, 300, 94, 96, 2)['kernel'] == 0 and query(lib, 300, 96, 96, 2)['kernel'] == 2
    for N, dh in ((98, 1), (100, 0), (102, 1), (130, 1)):
        assert query(lib, 300, N, 116, 2, dpro=1, shuf=2 * N, d=(2 * N, 0))['dhalf'] == dh
        assert query(lib, 300, N, 116, 2, dpro=1)['dhalf'] == 0


def test_every_refusal_has_its_code_and_words(lib):
    q = lambda *a, **k: query(lib, *a, **k)         # noqa: E731
    assert q(200, 58, 58, 2)['ok'] == 1
    check(lib, q(200, 58, 58, 0), GROUPS, 'G 0')
    check(lib, q(200, 58, 58, 3), GROUPS, 'M % G')
    check(lib, q(200, 58, 58, 2, bf=0, at=1), STORAGE, 'bf16 tensors without bf16 operands')
    assert q(200, 58, 58, 2, bf=1, at=1)['mode'] == 2 and q(200, 58, 58, 2, bf=1, at=0)['mode'] == 1
    rows = (1 << 29) // 116
    assert q(rows - rows % 4 - 4, 116, 116, 4)['ok'] == 1
    check(lib, q(rows - rows % 4 + 4, 116, 116, 4), TWO_GB, 'operands of 2 GB')
    check(lib, q(rows - rows % 4 + 4, 58, 58, 4, a=(116, 58)), TWO_GB, 'a view of 2 GB')
    check(lib, q(rows - rows % 4 + 4, 58, 58, 4, d=(116, 58)), TWO_GB, 'd view of 2 GB')
    for kw in (dict(a=(58, 1)), dict(a=(57, 0)), dict(a=(58, -1)), dict(d=(58, 1)), dict(d=(57, 0)), dict(dpro=1, shuf=116, d=(116, 59)),
               dict(dpro=1, shuf=116, d=(115, 0)), dict(dpro=1, shuf=117, d=(118, 0)), dict(shuf=116, d=(116, 0)), dict(relu=1),
               dict(dpro=1, shuf=-2)):
        check(lib, q(200, 58, 58, 2, **kw), VIEW, kw)
    # an empty product is accepted and launches nothing
    for M, N, K in ((0, 58, 58), (200, 0, 58), (200, 58, 0)):
        p = q(M, N, K, 2)
        assert p['ok'] == 1 and p['kernel'] == -1 and p['part_slots'] == 0, p
    # the query's own arguments
    v = _lib.View(None, 58, 0)
    out = (C.c_int32 * 21)()
    assert lib.cdrl_gemm_tn_plan(C.byref(v), C.byref(v), 200, 58, 58, 2, 0, 0, 0, 0, 0, 0, out, 21) == 21 and out[0] == 1     # null pointers are fine
    assert lib.cdrl_gemm_tn_plan(C.byref(v), C.byref(v), 200, 58, 58, 2, 0, 0, 0, 0, 0, 2, out, 21) == -1 and lib.cdrl_last_error()
    assert lib.cdrl_gemm_tn_plan(C.byref(v), C.byref(v), 200, 58, 58, 2, 0, 0, 0, 0, 0, 0, None, 21) == -1
    assert lib.cdrl_gemm_tn_plan(None, C.byref(v), 200, 58, 58, 2, 0, 0, 0, 0, 0, 0, out, 21) == 21 and (out[0], out[1]) == (0, VIEW)
    assert lib.cdrl_gemm_tn_plan(C.byref(v), C.byref(v), 200, 58, 58, 2, 0, 0, 0, 0, 0, 0, out, 3) == 21
    # the entry refuses what the plan refuses, and null tensors, before anything is launched (host pointers would fault otherwise)
    ex = lambda va, vd, M, G, bf, at, y=None, shuf=0, out_=BASE, ws=BASE: lib.cdrl_gemm_tn_ex(      # noqa: E731
        C.byref(va), None, C.byref(vd), y, y, y, shuf, 0, C.c_void_p(out_) if out_ else None, M, 58, 58, G, C.c_void_p(ws) if ws else None, 0, bf, at, None)
    w = _lib.View(BASE, 58, 0)
    assert ex(w, w, 200, 3, 0, 0) == -1 and b'multiple of G' in lib.cdrl_last_error()
    assert ex(w, w, 200, 2, 0, 1) == -1 and b'bf16 activation storage' in lib.cdrl_last_error()
    assert ex(v, w, 200, 2, 0, 0) == -1 and ex(w, v, 200, 2, 0, 0) == -1 and b'null' in lib.cdrl_last_error()
    assert ex(w, w, 200, 2, 0, 0, out_=0) == -1 and ex(w, w, 200, 2, 0, 0, ws=0) == -1
    assert ex(w, _lib.View(BASE, 58, 1), 200, 2, 0, 0) == -1 and b'fit' in lib.cdrl_last_error()
    assert ex(w, w, 200, 2, 0, 0, shuf=58) == -1 and ex(w, w, 200, 2, 0, 2) == -1


def test_workspace_query(lib):
    """one size for every prologue, operand type and view of a shape: the largest plan's (an odd view sends a wide shape to the direct kernel)"""
    for M, N, K, G in ((300, 58, 58, 2), (2048, 232, 232, 4), (1026, 24, 58, 2), (1024, 16, 9, 1), (12288, 768, 464, 1)):
        need = max(query(lib, M, N, K, G, apro, dpro, 0, 0, bf, 0, a=a)['part_elems'] for apro in (0, 1) for dpro in (0, 1) for bf in (0, 1)
                   for a in (None, (K + 5, 1)))
        assert lib.cdrl_gemm_tn_ex_workspace_elems(M, N, K, G) == need
        if G == 1:
            assert lib.cdrl_gemm_tn_workspace_elems(M, N, K) == need
    assert lib.cdrl_gemm_tn_ex_workspace_elems(300, 58, 58, 7) == 0 and lib.cdrl_gemm_tn_ex_workspace_elems(0, 58, 58, 1) == 0


def test_reduce_plan_sweep(lib):
    out = (C.c_int32 * 4)()
    for n in (1, 3, 4, 24, 576, 648, 986, 2044, 2048, 3364, 4092, 4096, 4100, 10240, 10244, 13456, 53824):
        for nparts in (1, 3, 15, 16, 17, 64, 65, 127, 128, 129, 513, 2049):
            for stride in (n, n + 1, n + 4, 28 * n):
                for addr in (BASE, BASE + 4, BASE + 8, BASE + 16):
                    assert lib.cdrl_reduce_partials_plan(addr, nparts, n, stride, out, 4) == 4
                    form, grid = reduce_form(addr % 16 == 0, nparts, n, stride)
                    block = {0: (256, 1), 1: (256, 1), 2: (256, 1), 3: (256, 1), 4: (16, 64), 5: (4, 256)}[form]
                    assert tuple(out) == (form, grid) + block, (n, nparts, stride, addr, tuple(out))
    for bad in ((0, 4, 4), (3, 0, 4), (3, 8, 4)):
        assert lib.cdrl_reduce_partials_plan(BASE, *bad, out, 4) == -1 and lib.cdrl_last_error()
        assert lib.cdrl_reduce_partials_f32(C.c_void_p(BASE), *bad, C.c_void_p(BASE), 0, None) == -1
    assert lib.cdrl_reduce_partials_f32(None, 3, 4, 4, C.c_void_p(BASE), 0, None) == -1


def test_plan_of_every_gpu_case(lib):
    """the GPU module's cases, their expectations and the restatement agree (the same check_plan the GPU run starts every case with)"""
    for c in V.CASES + V.engine_cases(lib):
        p = V.plan_query(lib, c)
        V.check_plan(lib, p, c)
        ldd, cd, ctot = V.d_view(c)
        assert p == expected(c.G * c.Mg, c.N, c.K, c.G, c.apro, c.dpro, ctot, int(c.bf > 0), int(c.bf == 2), a=V.a_view(c), d=(ldd, cd)), V.case_id(c)
        L, cnt = V.chain_and_count(p, c)
        assert 2 <= cnt <= 12 and 2 <= L <= max(p['rows_per'], 2)
    for n, nparts, stride, aligned, acc, form, _ in V.REDUCE_CASES:
        assert reduce_form(bool(aligned), nparts, n, stride)[0] == form, (n, nparts, stride, aligned)


def test_coverage_on_the_host(lib):
    """What tests/test_gpu_tn_variants.py::test_coverage asserts on the GPU (the plan queries need none)."""
    V.test_coverage(lib)


def test_no_bf16_case_has_a_flagged_operand_pair():
    """the inputs of every bf16-operand case behind a prologue: the share of output elements with an operand pair that may round either
    way is below 1 % (in fact zero: flagged elements are drawn again)"""
    n = 0
    for c in V.CASES:
        if c.bf and (c.apro or c.dpro) and c.G * c.Mg <= 600:
            inp, ref, _ = V.inputs_of(c)
            assert ref.flagged_share < 0.01 and ref.flagged_share == 0.0 and np.all(ref.allow == 0.0), V.case_id(c)
            n += 1
    assert n > 40


def test_reference_pieces():
    """the reference's own building blocks against hand-computed values"""
    assert tn_ref.view_cols(4, 4, 8).tolist() == [2, 6, 3, 7]
    assert tn_ref.bf(np.array([1.0, 1.00390625, 1.01171875])).tolist() == [1.0, 1.0, 1.015625]
    f = lambda bits: np.array([bits], np.uint32).view(np.float32)       # noqa: E731
    assert [bool(tn_ref._near_tie(f(0x3F800000 | low))[0]) for low in (0x7FFE, 0x7FFF, 0x8000, 0x8001, 0x8002, 0)] == [0, 1, 1, 1, 0, 0]
    inp = tn_ref.draw(np.random.default_rng(0), 2, 2, 2, 2, 1, 1, 1)
    inp.a[:] = [[1, 2], [3, 4], [5, 6], [7, 8]]
    inp.d[:] = [[1, -1], [2, -2], [3, -3], [4, -4]]
    inp.y[:] = [[0, 1], [2, 3], [0.5, 1], [100, -100]]
    inp.ast[2:] = [[[2, 1], [1, 1]], [[0, 1], [0.5, -1]]]           # scale, shift per group
    inp.yst[:] = [[[1, 1], [0, 0]], [[2, 2], [1, 1]], [[1, 1], [1, 1]], [[0, 0], [0, 0]]]   # mean, invstd, scale, shift
    inp.coef[:] = [[[1, 2], [1, 1]], [[0.5, 0.5], [0, 0]], [[1, 0], [0, 1]]]
    a, d, dh = tn_ref.operands64(inp)
    assert a.tolist() == [[2, 3], [6, 5], [5.5, 5], [7.5, 7]]
    # z = y (scale 1, shift 0): open in (0, 6).  group 0: xhat = 2 (y - 1), k = (1, .5, 1) | (2, .5, 0); group 1: xhat = y, k = (1, 0, 0) | (1, 0, 1)
    assert d.tolist() == [[0 - 0.5 + 2, 2 * (-1 - 0.5)], [2 - 0.5 - 2, 2 * (-2 - 0.5)], [3.0, -3 - 1], [0.0, 0 + 100]]
    assert dh.tolist() == [[0 + 0.5 + 2, 2 * 1.5], [2 + 0.5 + 2, 2 * 2.5], [3.0, 3 + 1], [0.0, 100.0]]
    r = tn_ref.evaluate(inp)
    assert np.allclose(r.w, a.T @ d) and np.allclose(r.S, np.abs(a).T @ dh) and np.all(r.S >= np.abs(r.w))
    rb = tn_ref.evaluate(inp, True)
    assert np.allclose(rb.w, r.w, rtol=2 ** -6, atol=2 ** -6 * np.abs(r.S).max())
    part = tn_ref.draw_partials(np.random.default_rng(1), 2049, 5, 8)
    assert np.all(part * 1024 == np.round(part * 1024)) and np.abs(part).max() < 256
    assert np.array_equal(tn_ref.reduce_ref(part, 5), part[::-1, :5].astype(np.float64).sum(axis=0).astype(np.float32))
