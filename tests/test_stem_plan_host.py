"""cdrl_stem_plan against an independent restatement of the host decisions of the stem block (csrc/conv.hip: stem_plan, stem_fwd_geom;
csrc/cdrl_common.h: vcol_geom, col_geom) over a sweep of shapes, with the invariants the kernels rely on and every refusal with its code.
Also, on the CPU: the case table of tests/test_gpu_stem_variants.py (each case's asserted form, its coverage of REQUIRED and of the
default configuration's plan, the conditions on its inputs, the float32-numpy margins) and tests/stem_ref.py against hand-computed
values.  The query launches nothing and reads no memory.  No GPU."""
import itertools

import numpy as np
import pytest

from tests import bn_ref, stem_ref
from tests import test_gpu_stem_variants as V

F32 = np.float32
COUT, TWO_GB, ALIGN = 1, 2, 3


def cdiv(a, b):
    return -(-a // b)


def vcol(rows, Cc, maxb):
    vec = 4 if Cc % 4 == 0 else 2 if Cc % 2 == 0 else 1
    lanes = Cc // vec
    cx = min(lanes, 256)
    cy = max(256 // cx, 1)
    rb = cdiv(max(cdiv(rows, maxb), 2 * cy), cy) * cy
    return dict(vec=vec, cx=cx, cy=cy, nloop=cdiv(lanes, cx), rb=rb, nb=cdiv(rows, rb))


def col(rows, Cc, maxb):
    cx = 32
    while cx < min(Cc, 256):
        cx *= 2
    cy = 256 // cx
    rb = cdiv(max(cdiv(rows, maxb), 4 * cy), cy) * cy
    return rb, cdiv(rows, rb)


def slices_of(rows, rows_per, Mg):
    """the most time slices the rows [k rows_per, (k + 1) rows_per) of one workgroup come from -- by walking every workgroup"""
    return max((min(r0 + rows_per, rows) - 1) // Mg - r0 // Mg + 1 for r0 in range(0, rows, rows_per))


def expected(B, T, H, W, Cc, at=0, pooled=0, adj=0, aligned=1):
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    Hp, Wp = cdiv(Ho, 2), cdiv(Wo, 2)
    Mg, rows = B * Ho * Wo, B * T * Ho * Wo
    e = dict(Ho=Ho, Wo=Wo, Hp=Hp, Wp=Wp, fwd_vec=int(Cc % 4 == 0 and aligned))
    e['st_refusal'] = COUT if (Cc % 4 or Cc > 64) else 0 if aligned else ALIGN
    # band form: the tallest band of {8, 6, 4, 3, 2, 1} rows whose 2 R + 1 image rows fit 6 x 1024 floats; images below 2 GB; 4 <= Cout <= 64
    R = next((r for r in (8, 6, 4, 3, 2, 1) if (2 * r + 1) * W * 3 <= 6144), 0)
    band = Cc % 4 == 0 and 4 <= Cc <= 64 and B * T * H * W * 3 * 4 < 2 ** 31 and R > 0
    if band:
        nx = (2 * R + 1) * W * 3
        chunks = cdiv(nx, 1024)
        NB = cdiv(Ho, R)
        nbpg = max(1, min(512 // T, B * NB))
        cx = Cc // 4
        cy = 256 // cx
        lds = max((cdiv(nx, 4) * 4 + 4 + 28 * Cc) * 4, 8 * cy * cx * 8)
        e.update(st_form=0, R=R, NB=NB, nbpg=nbpg, px=2 if chunks <= 2 else 4 if chunks <= 4 else 6, NP=2, lds=lds, units_max=cdiv(B * NB, nbpg), part_rows=nbpg)
    else:
        rb = max(1, cdiv(Mg, 128))
        lds = 0
        if Cc % 4 == 0 and 4 <= Cc <= 1024:
            cx = Cc // 4
            lds = max(28 * Cc * 4, 8 * (256 // cx) * cx * 8)
        e.update(st_form=1, R=0, NB=0, nbpg=cdiv(Mg, rb), px=0, NP=4, lds=lds, units_max=1, part_rows=cdiv(Mg, rb))
    pf = vcol(B * T * Hp * Wp, Cc, 4096)
    e.update({'pf_' + k: v for k, v in pf.items()})
    pr = vcol(B * Hp * Wp, Cc, 128)
    v4 = int(pr['vec'] == 4 and pr['nloop'] == 1)
    e.update(pr_form=v4, pr_pooled=int(v4 and pooled), pr_nb=pr['nb'], pr_part_doubles=T * pr['nb'] * 2 * Cc)
    if Cc <= 32:
        rows_per = max(128, cdiv(cdiv(rows, 1024), 128) * 128)
        nblk = cdiv(rows, rows_per)
        e.update(fg_form=0, rows_per=rows_per, nblk=nblk, part_doubles=(nblk * 28 * Cc + 1) // 2, ws_doubles=(2048 * 28 * Cc + 1) // 2)
    else:
        rb, nb = col(rows, Cc, 1024)
        e.update(fg_form=2, rows_per=rb, nblk=nb, part_doubles=nb * 28 * Cc, ws_doubles=nb * 28 * Cc)
    e['slices_max'] = slices_of(rows, e['rows_per'], Mg)
    e['ff_refusal'] = COUT if (Cc % 4 or Cc > 32) else TWO_GB if rows * Cc * 4 >= 2 ** 31 else 0
    ok = not e['ff_refusal']
    e.update(ff_form=1 if ok else -1, NCH=(3 if Cc <= 24 else 4) if ok else 1, rowstats=int(ok and e['slices_max'] > 2), single=int(ok and adj))
    return e


SWEEP = [(B, T, H, W, Cc) for B, T in ((1, 1), (1, 4), (1, 6), (2, 3), (5, 64), (3, 600), (256, 4), (7, 2))
         for H, W in ((3, 3), (9, 9), (15, 15), (22, 33), (23, 120), (19, 150), (15, 200), (13, 280), (11, 400), (9, 600), (7, 682), (7, 683), (90, 120), (183, 183))
         for Cc in (4, 6, 8, 20, 24, 28, 30, 32, 40, 64, 68)]


def test_plan_matches_the_restatement(lib):
    for (B, T, H, W, Cc), (at, pooled, adj, aligned) in zip(SWEEP, itertools.cycle(itertools.product((0, 1), repeat=4))):
        got, want = V.plan(lib, B, T, H, W, Cc, at, pooled, adj, aligned), expected(B, T, H, W, Cc, at, pooled, adj, aligned)
        assert got == {k: want[k] for k in V.FIELDS}, ((B, T, H, W, Cc, at, pooled, adj, aligned), {k: (got[k], want[k]) for k in V.FIELDS if got[k] != want[k]})
        assert lib.cdrl_stem_fwd_stats_rows(B, T, H, W, Cc) == got['part_rows']
        assert lib.cdrl_stem_bwd_workspace_doubles(B, T, H, W, Cc) == got['ws_doubles']
        assert lib.cdrl_stem_block_bwd_workspace_doubles(B, T, H, W, Cc) == got['ws_doubles'] + got['pr_part_doubles']


def test_invariants(lib):
    """What the kernels rely on: the band fits px * 1024 floats and the LDS covers band, weights and the reduction scratch; no more
    workgroups per slice than units; the workspace queries cover what the plan writes; 32-bit offsets stay below 2^31; and no fused
    workgroup touches more time slices than its kernel form stages."""
    for B, T, H, W, Cc in SWEEP:
        p = V.plan(lib, B, T, H, W, Cc, 0, 1, 1)
        rows = B * T * p['Ho'] * p['Wo']
        if p['st_form'] == 0 and not p['st_refusal']:
            nx = (2 * p['R'] + 1) * W * 3
            assert nx <= p['px'] * 1024 and p['px'] in (2, 4, 6)
            cx = Cc // 4
            assert p['lds'] >= (cdiv(nx, 4) * 4 + 28 * Cc) * 4 and p['lds'] >= 8 * (256 // cx) * cx * 8 and p['lds'] <= 65536
            assert 1 <= p['nbpg'] <= B * p['NB'] and p['units_max'] * p['nbpg'] >= B * p['NB'] and T * p['nbpg'] <= max(512, T)
            assert B * T * H * W * 3 * 4 < 2 ** 31
            assert p['NB'] * p['R'] >= p['Ho'] > (p['NB'] - 1) * p['R']
        assert p['ws_doubles'] >= p['part_doubles']
        if p['fg_form'] == 0:
            assert p['rows_per'] % 128 == 0 and p['nblk'] <= 2048 and p['nblk'] * p['rows_per'] >= rows > (p['nblk'] - 1) * p['rows_per']
        if p['ff_form'] == 1:
            assert rows * Cc * 4 < 2 ** 31 and B * T * p['Hp'] * p['Wp'] * Cc * 4 < 2 ** 31
            assert p['slices_max'] <= (T if p['rowstats'] else 2), p
            assert p['slices_max'] == slices_of(rows, p['rows_per'], B * p['Ho'] * p['Wo'])
        assert p['pr_part_doubles'] == T * p['pr_nb'] * 2 * Cc


def test_refusals(lib):
    for Cc, st, ff in ((6, COUT, COUT), (68, COUT, COUT), (64, 0, COUT), (40, 0, COUT), (32, 0, 0), (24, 0, 0)):
        p = V.plan(lib, 2, 2, 9, 11, Cc)
        assert (p['st_refusal'], p['ff_refusal'], p['ff_form']) == (st, ff, -1 if ff else 1), (Cc, p)
    assert V.plan(lib, 2, 2, 9, 11, 24, aligned=0)['st_refusal'] == ALIGN and V.plan(lib, 2, 2, 9, 11, 24, aligned=0)['fwd_vec'] == 0
    assert V.plan(lib, 2, 2, 9, 11, 6, aligned=0)['st_refusal'] == COUT
    big = V.plan(lib, 256, 16, 183, 183, 24)                     # 33.9 M rows x 24 channels x 4 bytes
    assert big['ff_refusal'] == TWO_GB and big['ff_form'] == -1
    assert V.plan(lib, 512, 16, 183, 183, 24)['st_form'] == 1   # images of 2 GB or more: the window form
    out = (V.C.c_int32 * 40)()
    for bad in ((0, 1, 9, 9, 24), (1, 0, 9, 9, 24), (1, 1, 2, 9, 24), (1, 1, 9, 2, 24), (1, 1, 9, 9, 0)):
        assert lib.cdrl_stem_plan(*bad, 0, 0, 0, 1, out, 40) == -1 and lib.cdrl_last_error()
    assert lib.cdrl_stem_plan(1, 1, 9, 9, 24, 2, 0, 0, 1, out, 40) == -1
    assert lib.cdrl_stem_plan(1, 1, 9, 9, 24, 0, 0, 0, 1, None, 40) == -1
    assert lib.cdrl_stem_plan(1, 1, 9, 9, 24, 0, 0, 0, 1, out, 3) == len(V.FIELDS)


def test_the_workload_keeps_its_kernels(lib):
    """The benchmark's shape selects the two-slice instantiation of the fused filter gradient, the band forward and the pooled reduce."""
    for at in (0, 1):
        p = V.plan(lib, *V.ENGINE, at, 1, 1)
        assert (p['rowstats'], p['ff_form'], p['NCH'], p['slices_max'], p['single']) == (0, 1, 3, 2, 1)
        assert (p['st_form'], p['R'], p['px'], p['units_max']) == (0, 8, 6, 12) and (p['pr_form'], p['pr_pooled']) == (1, 1)


def test_case_table(lib):
    """Every case of the GPU module selects the form it is there for, and together they cover REQUIRED and the default configuration."""
    for c in V.FWD_CASES:
        for at in (0, 1):
            pl = V.plan(lib, c.B, c.T, c.H, c.W, c.C, at, aligned=int(not c.off))
            assert all(pl[k] == v for k, v in c.expect.items()), (V.fid(c), pl)
    for c in V.BWD_CASES:
        for dt in c.types:
            pl = V.plan(lib, c.B, c.T, c.H, c.W, c.C, int(dt == 'bf16'), c.pooled, c.adj)
            assert all(pl[k] == v for k, v in c.expect.items()), (V.bid(c, dt), pl)
    assert not V.coverage_gaps(lib)


@pytest.mark.parametrize('c,dt', V.BWD_PARAMS)
def test_backward_case_inputs(c, dt):
    """The conditions on a backward case's inputs and the float32-numpy margins, from the reference alone."""
    i = V.bwd_inputs(c, dt)
    V.input_conditions(c, dt, i)
    m = V.margins(c, i)
    print(V.bid(c, dt), ' '.join(f'{v:.2e}' for v in m), 'open', i.sums.nopen, 'six', i.sums.six)
    assert m[0] * V.MARGIN < V.TOL_BN and m[1] * V.MARGIN < V.TOL_BN and m[2] * V.MARGIN < V.TOL_DW and (c.real or m[3] * V.MARGIN < V.TOL_DW), m


def test_pool_case_inputs():
    """Ties on both clamps decide codes in every pool case that has more than a handful of windows."""
    for c in V.POOL_CASES:
        for at in (0, 1):
            y, stats = V.pool_inputs(c, at)
            pv, code, a = stem_ref.pool_fwd(y, stats, c.T, c.B, c.H, c.W, bf16=bool(at))
            z = bn_ref.z32(y, stats, c.T, c.B * c.H * c.W)
            assert stem_ref.ulp_margin(z, 6.0) == 0 and stem_ref.ulp_margin(z, 0.0) == 0
            if code.size >= 64:
                assert (pv == 0).any() and (pv == 6).any()
            assert ((code & 0x7f) <= 8).all() and (at or np.array_equal(code >= 128, (pv <= 0) | (pv >= 6)))       # (bf16: an open 5.99 is stored as 6.0)


def test_reference_by_hand():
    # a 3 x 3 image, one output pixel: y = b + sum x w; dw = x dy, db = dy
    x = np.arange(27, dtype=F32).reshape(1, 1, 3, 3, 3)
    w = np.zeros((3, 3, 3, 2), F32)
    w[0, 0, 0, 0], w[2, 2, 2, 0], w[1, 1, 1, 1] = 1.0, 2.0, -1.0          # taps 0 and 26 of channel 0, tap 13 of channel 1
    b = np.array([0.5, 0.25], F32)
    Pm = stem_ref.patches(x)
    assert Pm.shape == (1, 27) and np.array_equal(Pm[0], np.arange(27))
    assert np.array_equal(stem_ref.conv32(Pm, w, b), [[0.0 + 52.0 + 0.5, -13.0 + 0.25]])
    y64, mag = stem_ref.conv64(Pm, w, b)
    assert np.array_equal(y64, [[52.5, -12.75]]) and np.array_equal(mag, [[52.5, 13.25]])
    dw, db = stem_ref.filter_grad(Pm, np.array([[2.0, 3.0]], F32))
    assert np.array_equal(dw[:, 0], 2.0 * np.arange(27)) and np.array_equal(db, [2.0, 3.0])
    # frames are ordered f = t * B + b
    x2 = np.zeros((2, 3, 3, 3, 3), F32)
    x2[1, 2] = 7.0
    assert np.array_equal(stem_ref.patches(x2)[:, 0], [0, 0, 0, 0, 0, 7.0])
    # a 2 x 2 pool (one window, pad_before 0) with a tie: the first maximum in scan order wins; the clamped winner carries bit 7
    stats = np.array([[[0.0]], [[1.0]], [[2.0]], [[1.0]]], F32)            # a = clamp(2 y + 1, 0, 6)
    y = np.array([[1.0], [2.5], [3.0], [0.5]], F32)                        # a = 3, 6, 6 (clamped from 7), 2
    pv, code, a = stem_ref.pool_fwd(y, stats, 1, 1, 2, 2)
    assert a.ravel().tolist() == [3.0, 6.0, 6.0, 2.0] and pv.ravel().tolist() == [6.0] and code.ravel().tolist() == [0x80 | 1]
    y = np.array([[1.0], [2.0], [2.0], [0.5]], F32)                        # a = 3, 5, 5, 2: the tie at 5 goes to (0, 1)
    pv, code, a = stem_ref.pool_fwd(y, stats, 1, 1, 2, 2)
    assert pv.ravel().tolist() == [5.0] and code.ravel().tolist() == [1]
    assert stem_ref.pad_before(2) == 0 and stem_ref.pad_before(1) == 1 and stem_ref.pad_before(7) == 1 and stem_ref.pad_before(8) == 0
    # 'same' padding on a 1 x 3 row: two windows, pad 1 on both sides; window 0 sees columns 0..1 as kx 1..2, window 1 column 2 as kx 0... 1
    y = np.array([[0.5], [1.0], [0.25]], F32)
    pv, code, _ = stem_ref.pool_fwd(y, stats, 1, 1, 1, 3)
    assert stem_ref.pad_before(3) == 1 and pv.ravel().tolist() == [3.0, 3.0] and code.ravel().tolist() == [3 + 2, 3 + 0]
    # backward through those codes: both windows name column 1
    dz = stem_ref.pool_bwd(code, np.array([1.0, 10.0]).reshape(1, 1, 2, 1), 1, 3)
    assert dz.ravel().tolist() == [0.0, 11.0, 0.0]
    # a one-row slice: s1 = dp, s2 = dp xhat, k2 = s1, k3 = s2, dy = k1 (dz - k2 - xhat k3)
    stats = np.array([[[1.0]], [[0.5]], [[2.0]], [[1.0]]], F32)            # mean 1, invstd 0.5, scale 2, shift 1
    y = np.array([[2.0]], F32)                                             # z = 5 (open), xhat = 0.5
    pv, code, _ = stem_ref.pool_fwd(y, stats, 1, 1, 1, 1)
    assert pv.ravel().tolist() == [5.0] and code.ravel().tolist() == [4]
    dp = np.array([3.0], F32).reshape(1, 1, 1, 1)
    r = stem_ref.backward(np.ones((1, 27), F32), y, stats, code, dp, 1, 1, 1, 1)
    assert r.sums.s1.tolist() == [[3.0]] and r.sums.s2.tolist() == [[1.5]] and r.dgamma.tolist() == [1.5] and r.dbeta.tolist() == [3.0]
    assert r.dy.tolist() == [[2.0 * (3.0 - 3.0 - 0.5 * 1.5)]] and r.db.tolist() == [-1.5] and r.dw[:, 0].tolist() == [-1.5] * 27
    # the pooled form recovers y from a: (5 - 1) / 2 = 2
    s = stem_ref.bn_sums(y, stats, code, dp, 1, 1, 1, 1, pooled=pv)
    assert s.s2.tolist() == [[1.5]] and s.rec[0, 0] == 3.0 * 2.0 ** -23 * (5.0 + 1.0) / 2.0 * 0.5
    assert bn_ref.to_bf16(np.array([5.99], F32))[0] == 6.0                 # the stored-6.0 case exists in bf16 storage
