"""cdrl_dwconv_bn_plan_ex (every field of the plan) and cdrl_dwconv_bn_plan (its first 22) against an independent restatement of
the host planner of csrc/dwfused.hip (dwf_plan with dws_geom and dws2_geom: the arithmetic of dwf_geom and of the launch ladders of dwf_fwd / dwf_bwd as they stood before the plan struct), over a
sweep of shapes, with the invariants the kernels rely on, every refusal with its code and message, the workspace query, and, on the
CPU: the cases, the coverage assertion and the engine layers of tests/test_gpu_dw_variants.py, the CDRL_DWS=0 dispatch in a child
process, and the plans of the three measured configurations as literals.  The query launches nothing and reads no memory.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

from carla_driving_rl_agent_amd import _lib
from tests import nn_ref
from tests import test_gpu_dw_variants as V

KB = 1024
LDS_LIMIT = 150 * KB
OK, REFUSE_STRIDE, REFUSE_LDS, REFUSE_OFFSETS = 0, 1, 2, 3
BASE = 1 << 20
DWS_OFF = V.DWS_OFF
# cdrl_dwconv_bn_plan_ex: the 22 fields of cdrl_dwconv_bn_plan, then what the invariants below need
PLAN_FIELDS = V.PLAN_FIELDS + ('scchunk', 'sS', 'lds_fwd', 'lds_bwd', 'grid_fwd', 'grid_bwd', 'stile', 'refusal_fwd', 'refusal_bwd')


def plan(lib, G, B, H, W, Cc, stride):
    """every field; the first 22 are what cdrl_dwconv_bn_plan reports"""
    out = (C.c_int32 * len(PLAN_FIELDS))()
    assert lib.cdrl_dwconv_bn_plan_ex(G, B, H, W, Cc, stride, out, len(out)) == len(PLAN_FIELDS) == 31
    p = dict(zip(PLAN_FIELDS, out))
    assert V.plan(lib, G, B, H, W, Cc, stride) == {k: p[k] for k in V.PLAN_FIELDS}
    return p


def cdiv(a, b):
    return -(-a // b)


def same_out(n, s):
    return cdiv(n, s)


def pad_before(n, s):
    return max((same_out(n, s) - 1) * s + 3 - n, 0) // 2


def strip_lds(tile_floats, cchunk, cx, cy):
    """the D tile and the coefficient table [16][cchunk], or the reduce scratch: 10 float + 2 double quantities per channel pair lane"""
    return max((tile_floats + 16 * cchunk) * 4, cx * cy * (10 * 2 * 4 + 2 * 2 * 8))


def strips_s1(fpb, H, W, Cc):
    """dws_geom: whole rows first (one channel chunk), strips of 8 pixels with one strip per thread in 384 then 640 threads, strips of 4
    pixels with up to 3 per thread; F frames share a tile batch while they fit the 56 KB tile budget and the lanes"""
    if Cc % 2:
        return None
    for nch in range(1, 17):
        cchunk = cdiv(Cc // 2, nch) * 2
        if cchunk < 8 and nch > 1:
            break
        for sw, thr, rmax in ((8, 384, 1), (8, 640, 1), (4, 384, 3)):
            if sw == 8 and W <= 4:
                continue
            S = cdiv(W, sw)
            cx, lds1, NS1 = cchunk // 2, (H + 2) * (S * sw + 2) * cchunk * 4, H * S
            maxcy = thr // cx
            if maxcy < 1 or lds1 > 56 * KB:
                continue
            R = cdiv(NS1, maxcy)
            if R > rmax:
                continue
            F = 1
            while R == 1 and F * 2 <= fpb and fpb % (F * 2) == 0 and F * 2 * lds1 <= 56 * KB and F * 2 * NS1 <= maxcy:
                F *= 2
            cy = cdiv(F * NS1, R)
            return dict(sw=sw, S=S, R=R, F=F, cchunk=cchunk, nch=cdiv(Cc, cchunk), cx=cx, cy=cy, tile=F * lds1,
                        lds=strip_lds(F * lds1 // 4, cchunk, cx, cy))
    return None


def strips_s2(fpb, H, W, Cc):
    """dws2_geom: input strips of 8 pixels, the D tile of the output frame(s) within 60 KB, up to 384 threads"""
    if Cc % 2:
        return None
    Ho, Wo, S = same_out(H, 2), same_out(W, 2), cdiv(W, 8)
    NS1, Wdp = H * S, max(4 * S + 2, Wo + 2)
    for nch in range(1, 17):
        cchunk = cdiv(Cc // 2, nch) * 2
        if cchunk < 8 and nch > 1:
            break
        cx, lds1 = cchunk // 2, (Ho + 2) * Wdp * cchunk * 4
        maxcy = 384 // cx
        if maxcy < 1 or lds1 > 60 * KB:
            continue
        F = 1
        while F * 2 <= fpb and fpb % (F * 2) == 0 and F * 2 * lds1 <= 60 * KB and F * NS1 < maxcy:
            F *= 2
        cy = min(maxcy, F * NS1)
        return dict(sw=8, S=S, R=1, F=F, cchunk=cchunk, nch=cdiv(Cc, cchunk), cx=cx, cy=cy, tile=F * lds1,
                    lds=strip_lds(F * lds1 // 4, cchunk, cx, cy))
    return None


def expected(G, B, H, W, Cc, stride, strips=True):
    """every field of the query for an accepted (G, B, H, W, C, stride)"""
    Ho, Wo = same_out(H, stride), same_out(W, stride)
    vec = 4 if Cc % 4 == 0 else 2 if Cc % 2 == 0 else 1
    a_px, d_px = (H + 2) * (W + 2), (Ho + 2) * (Wo + 2)
    per_c = (a_px + d_px) * 4
    # 38 KB per workgroup; 52, then 76 KB while a chunk would hold fewer than 22 (stride 2: 8) channels and not the whole frame
    budget = 38 * KB
    for kb in (52, 76):
        mc = budget // per_c // vec * vec
        if mc >= Cc or mc >= (8 if stride == 2 else 22):
            break
        budget = max(budget, kb * KB)
    maxc = min(max(budget // per_c // vec * vec, vec), 256)
    if maxc >= Cc:
        nch, cchunk = 1, Cc
    else:
        cchunk = cdiv(Cc // vec, cdiv(Cc, maxc)) * vec
        nch = cdiv(Cc, cchunk)
    Po = Ho * Wo
    cx = cchunk // vec
    cy = max(min(256 // cx, Po), 1)
    # frame loop: small frames while 512 workgroups remain, any frame while 2048 remain
    fpb = 1
    while fpb < 8 and Po * cx * fpb * 2 <= 4096 and B % (fpb * 2) == 0 and G * (B // (fpb * 2)) * nch >= 512:
        fpb *= 2
    while fpb < 8 and B % (fpb * 2) == 0 and G * (B // (fpb * 2)) * nch >= 2048:
        fpb *= 2
    vec_bwd = min(vec, 2)
    cx_bwd = cchunk // vec_bwd
    cy_bwd = max(min(256 // cx_bwd, Po), 1)
    lds_fwd = max(a_px * cchunk * 4, 2 * cy * vec * cx * 8)
    lds_bwd = max((a_px + d_px) * cchunk * 4, 10 * cy_bwd * vec_bwd * cx_bwd * 8)
    fpb_bwd, d = fpb, None
    if strips and G * B * H * W * Cc * 8 < 1 << 31:
        geom = strips_s1 if stride == 1 else strips_s2
        d = geom(1, H, W, Cc)
        if d:
            fpb_bwd = 1
            while fpb_bwd < 8 and B % (fpb_bwd * 2) == 0 and G * (B // (fpb_bwd * 2)) * d['nch'] >= (512 if H * W <= 16 else 256):
                fpb_bwd *= 2
            d = geom(fpb_bwd, H, W, Cc)
    nb, nb_bwd = B // fpb, B // fpb_bwd
    e = dict(vec=vec, nch=nch, cchunk=cchunk, cy=cy, fpb=fpb, nb=nb, vec_bwd=vec_bwd, fpb_bwd=fpb_bwd, nb_bwd=nb_bwd, form=stride if d else 0,
             sw=0, R=0, F=0, snch=0, scy=0, pl=pad_before(W, 2), lds_bwd_over=int(lds_bwd > LDS_LIMIT), lds_fwd_over=int(lds_fwd > LDS_LIMIT),
             cx=cx, cx_bwd=cx_bwd, cy_bwd=cy_bwd, scx=0, scchunk=0, sS=0, lds_fwd=lds_fwd, lds_bwd=lds_bwd,
             grid_fwd=cdiv(G * nb, 8) * 8 * nch, grid_bwd=cdiv(G * nb_bwd, 8) * 8 * (d['nch'] if d else nch), stile=0,
             refusal_fwd=REFUSE_LDS if lds_fwd > LDS_LIMIT else OK, refusal_bwd=REFUSE_LDS if not d and lds_bwd > LDS_LIMIT else OK)
    if d:
        e.update(sw=d['sw'], R=d['R'], F=d['F'], snch=d['nch'], scy=d['cy'], scx=d['cx'], scchunk=d['cchunk'], sS=d['S'], lds_bwd=d['lds'],
                 stile=d['tile'])
    return e


def invariants(lib, p, G, B, H, W, Cc, stride):
    """what the kernels and the callers rely on, from the query alone"""
    Ho, Wo = same_out(H, stride), same_out(W, stride)
    assert p['cx'] * p['vec'] == p['cchunk'] and p['nch'] * p['cchunk'] >= Cc and 1 <= p['cx'] * p['cy'] <= 512 and p['cy'] <= Ho * Wo
    assert p['fpb'] * p['nb'] == B and p['fpb_bwd'] * p['nb_bwd'] == B
    assert p['cx_bwd'] * p['vec_bwd'] == p['cchunk'] and p['cx_bwd'] * p['cy_bwd'] <= 512
    assert p['lds_fwd_over'] == (p['lds_fwd'] > LDS_LIMIT) == (p['refusal_fwd'] == REFUSE_LDS) and p['refusal_fwd'] in (OK, REFUSE_LDS)
    if p['form'] == 0:
        assert p['fpb_bwd'] == p['fpb'] and p['nb_bwd'] == p['nb'] and p['grid_bwd'] == p['grid_fwd']
        assert p['lds_bwd_over'] == (p['lds_bwd'] > LDS_LIMIT) == (p['refusal_bwd'] == REFUSE_LDS)
        assert not any(p[k] for k in ('sw', 'R', 'F', 'snch', 'scy', 'scx', 'scchunk', 'sS', 'stile'))
    else:
        assert p['form'] == stride and Cc % 2 == 0 and p['refusal_bwd'] == OK
        assert 2 * p['scx'] == p['scchunk'] and p['snch'] * p['scchunk'] >= Cc
        assert p['scx'] * p['scy'] <= (640 if p['form'] == 1 else 512)
        assert p['fpb_bwd'] % p['F'] == 0 and p['sS'] * p['sw'] >= W > (p['sS'] - 1) * p['sw']
        if p['form'] == 1:
            assert p['sw'] in (4, 8) and 1 <= p['R'] <= 3 and (p['sw'] == 4 or p['R'] == 1)
            assert p['R'] * p['scy'] >= p['F'] * H * p['sS']            # every strip of a tile batch has a lane
        else:
            assert (p['sw'], p['R']) == (8, 1) and p['pl'] == pad_before(W, 2)
        assert p['stile'] <= (56 if p['form'] == 1 else 60) * KB and p['stile'] + 16 * p['scchunk'] * 4 <= p['lds_bwd'] <= LDS_LIMIT
    # the workspace: BatchNorm-sum rows, filter rows (either direction's count), the reduce rows of the BatchNorm that follows
    rows = max(p['nb'], p['nb_bwd'])
    nbm = max(nn_ref.vcol_geom(B * Ho * Wo, Cc)[5], nn_ref.vcol_geom(B * H * W, Cc)[5])
    ws = lib.cdrl_dwconv_bn_workspace_doubles(G, B, H, W, Cc, stride)
    assert ws == G * rows * 12 * Cc + G * nbm * 3 * Cc and ws >= G * max(p['nb'] * 2, p['nb_bwd'] * 12) * Cc


SMALL = tuple(range(1, 13))
HS = SMALL + (15, 22, 23, 30, 44, 45, 60, 73, 74, 90, 100)
WS = SMALL + (13, 15, 16, 23, 26, 30, 33, 60, 61, 90, 98, 100, 120, 130)
CS = (1, 2, 3, 6, 8, 24, 29, 58, 116, 232, 464)
GB = [(G, B) for B in (1, 2, 3, 8, 12, 64, 128, 256, 1024) for G in (1, 2, 4)]


def sweep():
    """every (H, W, C, stride) of HS x WS x CS x (1, 2) with 3 of the 27 (G, B) pairs, taken in turn"""
    i = 0
    for H in HS:
        for W in WS:
            for Cc in CS:
                for stride in (1, 2):
                    for _ in range(3):
                        i += 1
                        yield GB[i % len(GB)] + (H, W, Cc, stride)


def test_plan_sweep(lib):
    """field by field against the restatement, with the invariants; the sweep keeps the one-pixel frames, odd C, C = 2, both refusals
    and all three forms"""
    forms, refused, blocks, lds = [0, 0, 0], [0, 0], [0, 0, 0, 0], [0, 0]
    seen = set()
    for shape in sweep():
        p = plan(lib, *shape)
        assert p == expected(*shape, strips=not DWS_OFF), (shape, p, expected(*shape, strips=not DWS_OFF))
        invariants(lib, p, *shape)
        forms[p['form']] += 1
        refused[0] += p['refusal_fwd'] != OK
        refused[1] += p['refusal_bwd'] != OK
        if not p['refusal_fwd']:
            lds[0], blocks[0] = max(lds[0], p['lds_fwd']), max(blocks[0], p['cx'] * p['cy'])
        if p['form']:
            lds[1], blocks[p['form']] = max(lds[1], p['lds_bwd']), max(blocks[p['form']], p['scx'] * p['scy'])
        else:
            blocks[3] = max(blocks[3], p['cx_bwd'] * p['cy_bwd'])
        seen.add((shape[2] * shape[3] == 1, shape[4] % 2, shape[4] == 2, p['form']))
    print('forms', forms, 'refused fwd / bwd', refused, 'largest blocks fwd / form 1 / form 2 / form 0', blocks, 'largest LDS fwd / strips', lds)
    assert sum(forms) == len(HS) * len(WS) * len(CS) * 2 * 3 and refused[0] > 0 and refused[1] > 0
    assert {(True, 1, False, 0), (False, 1, False, 0), (False, 0, True, 0)} <= seen
    if DWS_OFF:
        assert forms[1] == forms[2] == 0
        return
    assert all(forms) and {(True, 0, True, 1), (True, 0, True, 2), (False, 0, True, 1), (False, 0, True, 2)} <= seen
    # what the full sweep of the planner before the plan struct showed (532,224 plans), reached by this thinner one as well
    assert blocks == [256, 640, 384, 256] and lds[0] <= 153408 and lds[1] <= 85376 and 64 * KB < lds[1]


def test_every_refusal_has_its_code_and_message(lib):
    out = (C.c_int32 * 40)()
    for q, n in ((lib.cdrl_dwconv_bn_plan, 22), (lib.cdrl_dwconv_bn_plan_ex, 31)):
        assert q(2, 4, 5, 7, 58, 1, out, 40) == n and q(2, 4, 5, 7, 58, 1, out, 3) == n and q(2, 4, 5, 7, 58, 1, None, 0) == n
        for stride in (0, 3, -1):
            assert q(2, 4, 5, 7, 58, stride, out, n) == -1 and b'stride must be 1 or 2' in lib.cdrl_last_error()
        for bad in ((0, 4, 5, 7, 58), (2, 0, 5, 7, 58), (2, 4, 0, 7, 58), (2, 4, 5, 0, 58), (2, 4, 5, 7, 0), (2, 4, 5, 7, -2)):
            assert q(*bad, 1, out, n) == -1 and b'bad shape' in lib.cdrl_last_error(), bad
        assert q(2, 4, 5, 7, 58, 1, None, n) == -1 and b'null output' in lib.cdrl_last_error()
    for stride in (0, 3, -1):
        assert lib.cdrl_dwconv_bn_workspace_doubles(2, 4, 5, 7, 58, stride) == 0
    # the LDS limit: the forward's tile alone and the pixel-mapped backward's pair of tiles (74x100 stride 2: the GPU module's 73x98
    # case is the largest accepted one of its kind)
    for shape, fwd, bwd in (((1, 2, 90, 120, 24, 1), REFUSE_LDS, REFUSE_LDS), ((1, 2, 90, 120, 24, 2), REFUSE_LDS, REFUSE_LDS),
                            ((2, 2, 74, 100, 24, 2), OK, REFUSE_LDS), ((2, 2, 73, 98, 24, 2), OK, OK), ((2, 2, 45, 61, 24, 1), OK, OK)):
        p = plan(lib, *shape)
        assert (p['refusal_fwd'], p['refusal_bwd'], p['form']) == (fwd, bwd, 0), (shape, p)
        assert (p['lds_fwd_over'], p['lds_bwd_over']) == (int(fwd != OK), int(bwd != OK))
    # the entries refuse on the host, before anything is launched or read (these pointers are not memory): the forward with the
    # plan's refusals, both directions with a bad stride
    ptr = C.c_void_p(BASE)
    fwd = lambda G, B, H, W, Cc, s: lib.cdrl_dwconv_bn_fwd(ptr, None, ptr, ptr, ptr, G, B, H, W, Cc, s, ptr, ptr, ptr, ptr, 1, ptr, ptr, 0, None)   # noqa: E731
    bwd = lambda G, B, H, W, Cc, s: lib.cdrl_dwconv_bn_bwd(ptr, None, ptr, ptr, ptr, ptr, G, B, H, W, Cc, s, *([ptr] * 10), 0, None)   # noqa: E731
    for stride in (1, 2):
        assert fwd(1, 2, 90, 120, 24, stride) == -1
        assert lib.cdrl_last_error() == b'dwf_fwd: frame 90x120 does not fit LDS even at 4 channels'
    assert fwd(2, 4, 5, 7, 58, 3) == -1 and lib.cdrl_last_error() == b'dwf_fwd: stride must be 1 or 2'
    assert bwd(2, 4, 5, 7, 58, 0) == -1 and lib.cdrl_last_error() == b'dwf_bwd: stride must be 1 or 2'


def test_cases_of_the_gpu_module(lib):
    """the `expect` dictionaries of tests/test_gpu_dw_variants.py hold (check_plan is what every GPU case starts with), the
    restatement agrees on them, and 74x100 next to the 73x98 case is refused as that module says"""
    for shape, combos, expect in V.CASES:
        V.check_plan(lib, shape, expect)
        p = plan(lib, *shape)
        assert p == expected(*shape, strips=not DWS_OFF), shape
        invariants(lib, p, *shape)


def test_coverage_on_the_host(lib):
    """What tests/test_gpu_dw_variants.py::test_coverage asserts on the GPU: REQUIRED_FWD and REQUIRED_BWD are covered by the cases,
    every depthwise layer of engine_layers() has a known, covered signature."""
    V.test_coverage(lib)


# (G, B, H, W, C, stride): form, SW | VEC, R, F, lanes of the backward that runs, fpb_bwd | forward VEC, channel chunks, lanes, fpb
WORKLOAD = {
    # 90x120, B = 256
    (4, 256, 22, 30, 58, 2): ((2, 8, 1, 1, 29, 13, 4), (2, 8, 4, 64, 4)),
    (4, 256, 22, 30, 24, 2): ((2, 8, 1, 1, 12, 32, 4), (4, 3, 2, 128, 4)),
    (4, 256, 11, 15, 58, 1): ((1, 8, 1, 1, 29, 22, 4), (2, 3, 10, 25, 2)),
    (4, 256, 11, 15, 116, 2): ((2, 8, 1, 1, 58, 6, 4), (4, 4, 8, 32, 8)),
    (4, 256, 6, 8, 116, 1): ((1, 8, 1, 1, 58, 6, 4), (4, 2, 15, 17, 4)),
    (4, 256, 6, 8, 232, 2): ((2, 8, 1, 1, 116, 3, 4), (4, 3, 20, 12, 4)),
    (4, 256, 3, 4, 232, 1): ((1, 4, 1, 1, 116, 3, 2), (4, 2, 29, 8, 4)),
    # 90x360, B = 64
    (4, 64, 22, 90, 58, 2): ((2, 8, 1, 1, 10, 38, 2), (2, 10, 3, 85, 2)),
    (4, 64, 22, 90, 24, 2): ((2, 8, 1, 1, 6, 64, 2), (4, 6, 1, 256, 2)),
    (4, 64, 11, 45, 58, 1): ((1, 8, 1, 1, 8, 66, 4), (2, 5, 6, 42, 1)),
    (4, 64, 11, 45, 116, 2): ((2, 8, 1, 1, 29, 13, 2), (4, 15, 2, 128, 4)),
    (4, 64, 6, 23, 116, 1): ((1, 8, 1, 1, 29, 18, 2), (4, 5, 6, 42, 2)),
    (4, 64, 6, 23, 232, 2): ((2, 8, 1, 1, 58, 6, 2), (4, 7, 9, 28, 2)),
    (4, 64, 3, 12, 232, 1): ((1, 8, 1, 1, 58, 6, 2), (4, 4, 15, 17, 2)),
    # 90x120, B = 1024, bf16 storage
    (4, 1024, 22, 30, 58, 2): ((2, 8, 1, 1, 29, 13, 8), (2, 8, 4, 64, 8)),
    (4, 1024, 22, 30, 24, 2): ((2, 8, 1, 1, 12, 32, 8), (4, 3, 2, 128, 8)),
    (4, 1024, 11, 15, 58, 1): ((1, 8, 1, 1, 29, 22, 8), (2, 3, 10, 25, 4)),
    (4, 1024, 11, 15, 116, 2): ((2, 8, 1, 1, 58, 6, 8), (4, 4, 8, 32, 8)),
    (4, 1024, 6, 8, 116, 1): ((1, 8, 1, 1, 58, 6, 8), (4, 2, 15, 17, 4)),
    (4, 1024, 6, 8, 232, 2): ((2, 8, 1, 1, 116, 3, 8), (4, 3, 20, 12, 8)),
    (4, 1024, 3, 4, 232, 1): ((1, 4, 1, 1, 116, 3, 8), (4, 2, 29, 8, 8)),
}


def test_the_workload_keeps_its_kernels(lib):
    """the depthwise layers of the three measured configurations: the plans the planner gave them before the plan struct, as literals"""
    assert {L[:6] for L in V.engine_layers()} == set(WORKLOAD)
    if DWS_OFF:
        return          # the literals are the default dispatch
    for shape, (bwd, fwd) in WORKLOAD.items():
        p = plan(lib, *shape)
        assert (p['form'], p['sw'], p['R'], p['F'], p['scx'], p['scy'], p['fpb_bwd']) == bwd, (shape, p)
        assert (p['vec'], p['nch'], p['cx'], p['cy'], p['fpb']) == fwd, (shape, p)
        assert p['refusal_fwd'] == p['refusal_bwd'] == OK and p['pl'] == shape[3] % 2


def test_pixel_mapped_everywhere_on_the_host():
    """CDRL_DWS=0 (read once per process: one child process): every plan has form 0 with the forward's frame loop and partial rows --
    the sweep, the GPU module's cases and its coverage assertion run there and assert it."""
    if DWS_OFF:
        return          # this IS the child
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k',
                        'test_plan_sweep or test_cases_of_the_gpu_module or test_coverage_on_the_host'], env=dict(os.environ, CDRL_DWS='0'),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert '3 passed' in r.stdout and 'skipped' not in r.stdout, r.stdout[-500:]
