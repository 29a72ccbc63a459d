"""Fused 1x1-conv backward (cdrl_pwconv_bwd_fused_fin -> pw_bwd_fused / pw_bwd_fused_reduce, csrc/gemm_pw_bwd.hip): every form its host
plan can dispatch, at op level, against the float64 contract of tests/pw_ref.py.

Each case first reads the plan (cdrl_pwconv_bwd_plan -- the struct the launchers dispatch on) and asserts the fields it is there for;
`test_coverage` then holds the union of the cases' plan signatures (form, kp, np, shuf, anorm, acc, fin) against REQUIRED, the hand-written
list of what the launch ladder can instantiate, and against every unit conv the float32 and the bf16-storage engine send here.

Nothing here can pass by luck: the partial-tile workspaces and fin_tot start as NaN, every output as a sentinel (or the random base when
accumulating); dA has guard rows above and below and guard columns left and right, dW / db / qpart / dbpart / fin_tot sit between guard
bands, and all of them must come back bit-intact; dz, y and a live inside larger allocations whose surroundings are NaN, so a read one
row or one column outside a view poisons the result; and every case runs a second time on the dirty workspace and must reproduce itself
bit for bit (fixed-order sums, no atomics).

Bounds: those of tests/test_gpu_ops.py for this op (float32: 1e-5 for da and dW, its db / coefficient bounds; bf16 storage: 6e-3 da,
5e-4 dW, 1e-4 db), and one float32 rounding of a double sum for the finalize-on-load dgamma / dbeta."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from oracle.spec import NetConfig, unit_plan
from tests import pw_ref
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
SENTINEL = -2.0 ** 100          # exact in float32 and bf16; no kernel output comes near it
GR = 2                          # guard rows above and below every 2-D tensor (even: keeps bf16 rows 8-byte aligned)

PLAN_FIELDS = ('ok', 'refusal', 'form', 'kp', 'np', 'bm', 'tiles', 'nbpg', 'wp_ks', 'shuf', 'anorm', 'acc', 'fin', 'coef_needed', 'lds_bytes',
               'qpart_elems', 'dbpart_elems', 'spart_offset')
FAKE = 1 << 20                  # a non-null, aligned address for probing the plan (the query reads no memory)

# a / da view forms: dense; the right half of a channel split; an odd-looking padded row.  dz: dense, padded, or through the shuffle
# of a ctot-channel tensor as its low (coff 0) or high (coff + N == ctot) part.
Case = namedtuple('Case', 'K N G Mg relu anorm acc fin a dz da bf16 ctot expect tag')


def mk(K, N, G=2, Mg=77, relu=1, anorm=0, acc=0, fin=0, a='dense', dz='dense', da='dense', bf16=0, ctot=0, tag='', **expect):
    return Case(K, N, G, Mg, relu, anorm, acc, fin, a, dz, da, bf16, ctot, expect, tag)


def a_view(c, which):
    """(ld, coff) of the a / da view"""
    form = getattr(c, which)
    return {'dense': (c.K, 0), 'split': (2 * c.K, c.K), 'pad': ((c.K + 6, 2) if which == 'a' else (c.K + 4, 2))}[form]


def dz_view(c):
    """(ld, coff, shuffle_ctot)"""
    if c.dz == 'dense':
        return c.N, 0, 0
    if c.dz == 'pad':
        return c.N + 10, 4, 0
    ctot = c.ctot or 2 * c.N
    return ctot, (0 if c.dz == 'lo' else ctot - c.N), ctot


def form_of(ld, coff, Cc, ctot=0):
    if ctot:
        return 'lo' if coff == 0 else 'hi' if coff + Cc == ctot else 'other'
    return 'dense' if (ld, coff) == (Cc, 0) else 'split' if (ld, coff) == (2 * Cc, Cc) else 'other'


def pad(c):
    return 64 if c <= 64 else 128


def bm_of(K, N):
    return 64 if pad(K) == 64 and pad(N) == 64 else 32


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
GS = (1, 2, 3, 4, 5, 8)
FIN_NBS = (1, 2, 3, 4, 7, 8, 9, 31, 33, 70)
CHANNEL_EDGES = ((8, 8), (24, 24), (24, 58), (32, 16), (34, 32), (32, 34), (58, 58), (64, 64), (62, 66), (64, 66), (58, 92), (116, 116),
                 (126, 128), (128, 128))
PADS_F32 = ((58, 58), (116, 116), (58, 92))          # 64/64, 128/128, 64 -> 128
CASES = []

# every instantiation: 3 paddings x shuffle x ANORM x accumulate, each with finalize-on-load and without (48 float32), 2 paddings x 8
# under bf16 storage; groups, row counts, views, ReLU6 and fin_nb vary along the way
i = 0
for K, N in PADS_F32:
    for shuf in (0, 1):
        for anorm in (0, 1):
            for acc in (0, 1):
                for fin in (0, 1):
                    i += 1
                    CASES.append(mk(K, N, G=GS[i % 6], Mg=(70, 33, 131, 97)[i % 4], relu=int(i % 3 != 0), anorm=anorm, acc=acc,
                                    fin=FIN_NBS[i % 10] if fin else 0, a=('dense', 'split', 'pad')[i % 3],
                                    dz=(('lo', 'hi')[(i // 2) % 2] if shuf else ('dense', 'pad')[(i // 2) % 2]), da=('pad', 'dense', 'split')[i % 3],
                                    tag='inst', kp=pad(K), np=pad(N), shuf=shuf, anorm_=anorm, acc_=acc, fin_=fin, form=0))
for K, N in PADS_F32[:2]:
    for shuf in (0, 1):
        for anorm in (0, 1):
            for acc in (0, 1):
                i += 1
                CASES.append(mk(K, N, G=GS[i % 6], Mg=(70, 33, 131, 97)[i % 4], relu=int(i % 3 != 0), anorm=anorm, acc=acc, bf16=1,
                                a=('dense', 'split', 'pad')[i % 3], dz=(('lo', 'hi')[i % 2] if shuf else ('dense', 'pad')[i % 2]),
                                da=('pad', 'dense', 'split')[i % 3], tag='inst', kp=pad(K), np=pad(N), shuf=shuf, anorm_=anorm, acc_=acc, fin_=0,
                                form=1))
# channel edges: the minimum, the weight pack's 2 -> 4 K-step boundary (N 32 | 34), the padding boundary (64 | 66, K 64 -> N 66), no
# padded column at all (128)
for j, (K, N) in enumerate(CHANNEL_EDGES):
    ks = 2 if N <= 32 else 4 if N <= 64 else 8
    CASES.append(mk(K, N, G=2, Mg=141, anorm=j % 2, dz=('dense', 'hi')[j % 2], tag='chan', kp=pad(K), np=pad(N), wp_ks=ks))
    CASES.append(mk(K, N, G=3, Mg=75, anorm=1 - j % 2, fin=(3, 9)[j % 2], dz=('lo', 'pad')[j % 2], acc=j % 2, tag='chan', kp=pad(K), np=pad(N),
                    wp_ks=ks, fin_=1))
    if pad(K) == pad(N):
        CASES.append(mk(K, N, G=2, Mg=141, anorm=j % 2, dz=('hi', 'dense')[j % 2], bf16=1, tag='chan', kp=pad(K), np=pad(N), wp_ks=ks))
# row edges for the 64-row and the 32-row form: fewer rows than a tile (nbpg == tiles), a tile exactly, one row more, ragged ends with
# Mg % 4 != 0; unequal tile counts per workgroup; many tiles per workgroup (the reduce's 32-wide loop: nbpg 256, and its 16- / 8-wide
# loops and tail: 216 partials in 8 slices of 27)
for K in (58, 116):
    BM = bm_of(K, K)
    for j, Mg in enumerate((1, 3, BM - 1, BM, BM + 1, 2 * BM + 5)):
        t = -(-Mg // BM)
        an = int(Mg > 1 and j % 2 == 1)         # (one row per group: xhat of the conv input is identically 0, its sums have no scale)
        CASES.append(mk(K, K, G=2, Mg=Mg, anorm=an, dz=('dense', 'lo')[j % 2], tag='rows', bm=BM, tiles=t, nbpg=t))
        CASES.append(mk(K, K, G=4, Mg=Mg, anorm=1 - an if Mg > 1 else 0, fin=(2, 7, 33)[j % 3], dz=('hi', 'dense')[j % 2], acc=j % 2, tag='rows',
                        bm=BM, tiles=t, nbpg=t))
        CASES.append(mk(K, K, G=2, Mg=Mg, anorm=an, dz=('dense', 'lo')[j % 2], bf16=1, tag='rows', bm=BM, tiles=t, nbpg=t))
    CASES.append(mk(K, K, G=4, Mg=101 * BM - 7, anorm=1, dz='hi', fin=4, tag='uneven', bm=BM, tiles=101, nbpg=64))
    CASES.append(mk(K, K, G=4, Mg=101 * BM - 7, anorm=1, dz='hi', bf16=1, tag='uneven', bm=BM, tiles=101, nbpg=64))
    CASES.append(mk(K, K, G=1, Mg=216 * BM - 3, anorm=1, dz='lo', tag='many', bm=BM, tiles=216, nbpg=216))
    CASES.append(mk(K, K, G=1, Mg=256 * BM + 5, anorm=1, dz='lo', fin=8, tag='many', bm=BM, tiles=257, nbpg=256))
    CASES.append(mk(K, K, G=1, Mg=256 * BM + 5, anorm=0, dz='dense', acc=1, tag='many', bm=BM, tiles=257, nbpg=256))
    # (generic coefficients: behind a true finalize the column sums of dy vanish, and a reduce that dropped them would go unnoticed)
    CASES.append(mk(K, K, G=1, Mg=256 * BM + 5, anorm=1, dz='hi', tag='many', bm=BM, tiles=257, nbpg=256))
    CASES.append(mk(K, K, G=8, Mg=32 * BM + 9, anorm=1, dz='lo', tag='many', bm=BM, tiles=33, nbpg=32))
# groups: G 8 (one reduce slice per group), G 3 (nb = 85, two unused reduce slots), G 5 (nb = 51), G 1 with ANORM; with all partials used
for j, G in enumerate(GS):
    for anorm in (0, 1):
        CASES.append(mk(58, 58, G=G, Mg=150, anorm=anorm, dz=('dense', 'hi')[anorm], fin=(0, 31)[(j + anorm) % 2], tag='groups', nbpg=3))
for G in (3, 5, 8):
    CASES.append(mk(116, 116, G=G, Mg=(256 // G) * 32 + 40, anorm=1, dz='hi', fin=2, tag='groups', nbpg=256 // G))
    CASES.append(mk(58, 58, G=G, Mg=(256 // G) * 64 + 70, anorm=1, dz='lo', bf16=1, tag='groups', nbpg=256 // G))
# views: the right half of a channel split as conv input (the engine's first unit conv of a stride-1 unit) and as accumulated output
for bf16 in (0, 1):
    CASES.append(mk(58, 58, Mg=90, a='split', da='split', acc=1, relu=0, dz='dense', bf16=bf16, tag='views'))
    CASES.append(mk(116, 116, Mg=90, a='pad', da='dense', dz='pad', bf16=bf16, tag='views'))
    CASES.append(mk(58, 58, Mg=90, a='pad', da='split', dz='lo', anorm=1, bf16=bf16, tag='views'))
    CASES.append(mk(116, 116, Mg=90, a='split', da='pad', dz='hi', anorm=1, bf16=bf16, tag='views'))
# finalize-on-load: fin_nb covers lane quarters that get no rows (1, 2, 3), the tail only (4, 7), the unrolled loop alone (31 -> per 8;
# 8 | per), unrolled + tail (33, 70); N covers column groups of 16 that end inside a wave (24, 58, 92, 116), at a wave and at NP (128)
for j, nb in enumerate(FIN_NBS):
    for k, N in enumerate((24, 58, 92, 116, 128)):
        K = 58 if N <= 92 else 116
        CASES.append(mk(K, N, G=(2, 3)[(j + k) % 2], Mg=(45, 130)[(j + k) % 2], relu=(j + k) % 2, anorm=(j + k // 2) % 2, fin=nb,
                        dz=('dense', 'hi', 'lo')[(j + k) % 3], tag='fin', fin_=1, coef_needed=0))
# bf16 storage with two resident workgroups per CU: tiles == 6 * (512 / G) is the threshold, one tile fewer falls back to 256 / G
CASES.append(mk(116, 116, G=8, Mg=12288, anorm=1, dz='hi', bf16=1, tag='two-wg', bm=32, tiles=384, nbpg=64))
CASES.append(mk(116, 116, G=8, Mg=12288 - 32, anorm=1, dz='hi', bf16=1, tag='two-wg', bm=32, tiles=383, nbpg=32))
CASES.append(mk(58, 58, G=8, Mg=24576, anorm=1, dz='lo', bf16=1, tag='two-wg', bm=64, tiles=384, nbpg=64))
# the engine's unit convs with their own channel counts and views (test_coverage matches every conv of both engines against the cases)
for bf16 in (0, 1):
    fin = 0 if bf16 else 5
    CASES.append(mk(24, 58, G=4, Mg=150, relu=0, acc=1, fin=fin, bf16=bf16, tag='engine'))                                   # s0.u0.pw1
    CASES.append(mk(24, 24, G=4, Mg=150, anorm=1, dz='lo', ctot=116, fin=fin, bf16=bf16, tag='engine'))                       # s0.u0.sc_pw
    CASES.append(mk(58, 58, G=4, Mg=150, relu=0, a='split', da='split', fin=fin, bf16=bf16, tag='engine'))                    # s0.u1.pw1
    CASES.append(mk(58, 58, G=4, Mg=150, anorm=1, dz='hi', ctot=116, fin=fin, bf16=bf16, tag='engine'))                       # s0.u1.pw2
    CASES.append(mk(116, 116, G=4, Mg=150, relu=0, acc=1, fin=fin, bf16=bf16, tag='engine'))                                  # s1.u0.pw1
    CASES.append(mk(116, 116, G=4, Mg=150, anorm=1, dz='hi', ctot=232, fin=fin, bf16=bf16, tag='engine'))                     # s1.u0.pw2
    CASES.append(mk(116, 116, G=4, Mg=150, anorm=1, dz='lo', ctot=232, fin=fin, bf16=bf16, tag='engine'))                     # s1.u0.sc_pw
    CASES.append(mk(116, 116, G=4, Mg=150, relu=0, a='split', da='split', fin=fin, bf16=bf16, tag='engine'))                  # s1.u1.pw1
CASES.append(mk(58, 92, G=4, Mg=150, anorm=1, dz='hi', ctot=116, fin=5, tag='engine'))                                       # s0.u0.pw2


def case_id(c):
    return (f"{'bf16' if c.bf16 else 'f32'}-{c.tag}-K{c.K}N{c.N}G{c.G}M{c.Mg}-r{c.relu}n{c.anorm}c{c.acc}f{c.fin}-{c.a}.{c.dz}{c.ctot or ''}.{c.da}")


PARAMS = [pytest.param(c, id=case_id(c)) for c in CASES]
assert len({case_id(c) for c in CASES}) == len(CASES)
assert all(c.G * c.Mg <= 200_000 for c in CASES)


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def plan_query(lib, c, pdz=FAKE, pa=FAKE, pda=FAKE):
    """the plan of a case for views at the given addresses; every other pointer the case would pass is probed as non-null"""
    ldz, cdz, ctot = dz_view(c)
    vz, va, vd = _lib.View(pdz, ldz, cdz), _lib.View(pa, *a_view(c, 'a')), _lib.View(pda, *a_view(c, 'da'))
    an = C.c_void_p(FAKE) if c.anorm else None
    fn = C.c_void_p(FAKE) if c.fin else None
    out = (C.c_int32 * len(PLAN_FIELDS))()
    n = lib.cdrl_pwconv_bwd_plan(C.byref(vz), ctot, C.byref(va), C.byref(vd), c.acc, c.G, c.Mg, c.N, c.K, an, an, an, an, an, an, fn, c.fin, fn, fn,
                                 fn, c.bf16, out, len(PLAN_FIELDS))
    assert n == len(PLAN_FIELDS), n
    return dict(zip(PLAN_FIELDS, out))


def signature(p):
    return (p['form'], p['kp'], p['np'], p['shuf'], p['anorm'], p['acc'], p['fin'])


def check_plan(p, c):
    assert p['ok'] == 1 and p['refusal'] == 0, (c, p)
    for k, v in c.expect.items():
        assert p[k.rstrip('_')] == v, (case_id(c), k, p)
    assert p['form'] == c.bf16 and p['bm'] == bm_of(c.K, c.N) and p['tiles'] == -(-c.Mg // p['bm']) and 1 <= p['nbpg'] <= p['tiles'], p
    assert p['lds_bytes'] <= 160 * 1024


# ---- REQUIRED: what the launch ladder of pw_bwd_fused can instantiate, written out from it -----------------------------------------
# pwb_kernel<KP, NP, SHUF, ANORM, ACC> for 64/64, 128/128, 64 -> 128, each with and without finalize-on-load (a kernel argument);
# pwb16_kernel<P, P, SHUF, ANORM, ACC> for P = 64 | 128 (no finalize-on-load under bf16 storage)
REQUIRED = ({(0, kp, np_, s, n, a, f) for kp, np_ in ((64, 64), (128, 128), (64, 128)) for s in (0, 1) for n in (0, 1) for a in (0, 1) for f in (0, 1)}
            | {(1, p, p, s, n, a, 0) for p in (64, 128) for s in (0, 1) for n in (0, 1) for a in (0, 1)})


def engine_convs():
    """(bf16, K, N, G, Mg, a (ld, coff), dz (ld, coff, ctot), da (ld, coff), act, anorm, acc, fin) of every unit conv of the default float32
    engine (finalize-on-load) and of the bf16-storage engine whose backward the fused form can take (K, N in 24..128), from the unit
    plan the engine is built from: pw1 reads the unit input (stride 2) or the right half of its channel split (stride 1) and writes
    (stride 2: accumulates) the gradient there, its dz is dense and already masked; pw2 / sc_pw read the dense depthwise output
    through its BatchNorm (ANORM) and gather dz through the unit's channel shuffle (main half: the high part, shortcut: the low part)."""
    for H, W, B in ((90, 120, 256), (90, 360, 64)):
        cfg = NetConfig(H=H, W=W)
        h, w = -(-((H - 3) // 2 + 1) // 2), -(-((W - 3) // 2 + 1) // 2)
        for u in unit_plan(cfg):
            s2 = u['stride'] == 2
            ho, wo = (-(-h // 2), -(-w // 2)) if s2 else (h, w)
            cin, c_out, sc = u['cin'], u['cout'], u['shortcut_c']
            xin = (cin, 0) if s2 else (cin, sc)
            convs = [(u['main_in'], u['mid'], B * h * w, xin, (u['mid'], 0, 0), xin, 0, 0, int(s2)),
                     (u['mid'], u['main_out'], B * ho * wo, (u['mid'], 0), (c_out, sc, c_out), (u['mid'], 0), 1, 1, 0)]
            if s2:
                convs.append((sc, sc, B * ho * wo, (sc, 0), (c_out, 0, c_out), (sc, 0), 1, 1, 0))
            for K, N, Mg, av, dzv, dav, act, anorm, acc in convs:
                if 24 <= K <= 128 and N <= 128:
                    for bf16 in (0, 1):
                        yield (bf16, K, N, cfg.T, Mg, av, dzv, dav, act, anorm, acc, int(not bf16))
            h, w = ho, wo


def record_of_case(c, p):
    ldz, cdz, ctot = dz_view(c)
    return (signature(p), c.K, c.N, form_of(*a_view(c, 'a'), c.K), form_of(ldz, cdz, c.N, ctot), form_of(*a_view(c, 'da'), c.K), c.relu)


def coverage_gaps(lib):
    have, records = set(), set()
    for c in CASES:
        p = plan_query(lib, c)
        have.add(signature(p))
        records.add(record_of_case(c, p))
    gaps = [('REQUIRED', s) for s in sorted(REQUIRED - have)] + [('unknown signature', s) for s in sorted(have - REQUIRED)]
    n = 0
    for bf16, K, N, G, Mg, av, dzv, dav, act, anorm, acc, fin in engine_convs():
        e = mk(K, N, G=G, Mg=Mg, relu=act, anorm=anorm, acc=acc, fin=5 if fin else 0, bf16=bf16)
        vz, va, vd = _lib.View(None, dzv[0], dzv[1]), _lib.View(None, *av), _lib.View(None, *dav)
        an, fn = (C.c_void_p(FAKE) if anorm else None), (C.c_void_p(FAKE) if fin else None)
        out = (C.c_int32 * len(PLAN_FIELDS))()
        lib.cdrl_pwconv_bwd_plan(C.byref(vz), dzv[2], C.byref(va), C.byref(vd), acc, G, Mg, N, K, an, an, an, an, an, an, fn, e.fin, fn, fn, fn, bf16,
                                 out, len(PLAN_FIELDS))
        p = dict(zip(PLAN_FIELDS, out))
        if not p['ok']:         # the engine asks pw_bwd_fused_supported (the same plan) and takes another backward form
            assert bf16 and p['refusal'] == 3 and (K, N) == (58, 92), (K, N, bf16, p)
            continue
        n += 1
        rec = (signature(p), K, N, form_of(av[0], av[1], K), form_of(dzv[0], dzv[1], N, dzv[2]), form_of(dav[0], dav[1], K), act)
        assert 'other' not in rec, rec
        if rec not in records:
            gaps.append(('engine conv', rec))
    assert n == 2 * (2 * 26 - 1), n     # (stages 0 and 1: 9 + 17 convs, two configurations, two engines, minus the refused conv)
    return gaps


def test_coverage(lib):
    """The plan signatures of this module's cases cover REQUIRED, contain nothing REQUIRED does not know, and every unit conv of both
    engines at the 90x120 and 90x360 configurations is matched by a case with the same signature, channel counts, view forms and
    activation.  Also holds the edge lists the module promises: rows, groups, fin_nb, channel pairs."""
    gaps = coverage_gaps(lib)
    assert not gaps, gaps
    for bm, K in ((64, 58), (32, 116)):
        for bf16 in (0, 1):
            rows = {c.Mg for c in CASES if c.bf16 == bf16 and bm_of(c.K, c.N) == bm}
            assert {1, 3, bm - 1, bm, bm + 1, 2 * bm + 5} <= rows, (bm, bf16)
    for an in (0, 1):
        assert {c.G for c in CASES if c.anorm == an and not c.bf16} == set(GS)
    assert {(c.fin, c.N) for c in CASES if c.tag == 'fin'} == {(nb, N) for nb in FIN_NBS for N in (24, 58, 92, 116, 128)}
    assert {(c.relu, c.anorm) for c in CASES if c.fin} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert set(CHANNEL_EDGES) <= {(c.K, c.N) for c in CASES if not c.bf16} and set(CHANNEL_EDGES) <= {(c.K, c.N) for c in CASES if c.fin}


def test_nine_groups_are_refused_by_the_plan(lib):
    p = plan_query(lib, mk(58, 58, G=9, Mg=100))
    assert p['ok'] == 0 and p['refusal'] == 5 and lib.cdrl_last_error(), p
    assert plan_query(lib, mk(58, 58, G=8, Mg=100))['ok'] == 1


# ---- guarded tensors ---------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


class Banded:
    """A 1-D tensor inside a larger one, with a band of `fill` on each side that must come back bit-intact."""

    def __init__(self, n, dtype, fill, band=256):
        self.whole = torch.full((band + n + band,), fill, dtype=dtype, device=DEV)
        self.t = self.whole[band:band + n]
        self.lo, self.hi = self.whole[:band], self.whole[band + n:]
        self.ref = self.lo.clone()

    def intact(self):
        return torch.equal(bits(self.lo), bits(self.ref)) and torch.equal(bits(self.hi), bits(self.ref))


class Framed:
    """A view (rows x C channels at column `cols`) of a [GR + M + GR][ld] tensor.  Inputs: everything around the payload is NaN.
    Outputs: the whole tensor starts as `base` (sentinel, or random when accumulating) and everything around the payload must come
    back bit-intact."""

    def __init__(self, M, ld, cols, dtype, payload=None, base=None):
        cols = torch.as_tensor(np.asarray(cols), dtype=torch.long)
        self.M, self.cols = M, cols.to(DEV)
        if base is None:
            whole = torch.full((GR + M + GR, ld), float('nan'), dtype=torch.float32)
            whole[GR:GR + M, cols] = torch.as_tensor(np.asarray(payload, np.float32))
        else:
            whole = torch.as_tensor(base).clone()
        self.whole = whole.to(dtype).to(DEV).contiguous()
        self.start = self.whole.clone() if base is not None else None
        self.ptr = self.whole.data_ptr() + GR * ld * self.whole.element_size()

    def payload(self):
        return self.whole[GR:GR + self.M][:, self.cols]

    def frame_intact(self):
        a, b = self.whole.clone(), self.start.clone()
        a[GR:GR + self.M, self.cols] = 0
        b[GR:GR + self.M, self.cols] = 0
        return torch.equal(bits(a), bits(b))


def sync():
    """A device fault ends the run: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device fault, stopping: {e}', returncode=3)


def clean(t):
    t = t.float()
    return bool(torch.isfinite(t).all()) and not bool((t == SENTINEL).any())


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


WORST = {}          # (tensor type, output) -> worst observed error / bound, printed by test_report
FIN_BITS = []       # finalize-on-load vs coefficient form: da, dW, db bit-equal?


def note(c, name, err, bound):
    assert err < bound or (err == 0.0 and bound == 0.0), f'{case_id(c)}: {name} {err:.3e} >= {bound:.3e}'
    key = ('bf16' if c.bf16 else 'f32', name)
    if bound > 0 and err / bound > WORST.get(key, (0.0, 0.0, ''))[0]:
        WORST[key] = (err / bound, err, case_id(c))


def launch(lib, c, t, coef, fin_part, out):
    """one call of the op on the case's tensors `t` into the outputs `out`"""
    ldz, cdz, ctot = dz_view(c)
    vz = _lib.View(t['dz'].ptr, ldz, cdz)
    va = _lib.View(t['a'].ptr, *a_view(c, 'a'))
    vd = _lib.View(out['da'].ptr, *a_view(c, 'da'))
    an = c.anorm
    lib.cdrl_set_op_activation_type(c.bf16)
    try:
        _lib.check(lib.cdrl_pwconv_bwd_fused_fin(
            C.byref(vz), ctot, c.relu, C.c_void_p(t['y'].ptr), P(t['yst']), P(coef), C.byref(va), P(t['ast']) if an else None,
            P(t['ga']) if an else None, P(t['ba']) if an else None, P(out['adg']) if an else None, P(out['adb']) if an else None,
            P(out['acf']) if an else None, P(t['w']), P(t['wp']), C.byref(vd), c.acc, P(out['dw'].t), P(out['db'].t), P(t['qpart'].t),
            P(t['dbpart'].t), P(fin_part), c.fin if fin_part is not None else 0, P(t['fin_tot'].t) if fin_part is not None else None,
            P(out['odg']) if fin_part is not None else None, P(out['odb']) if fin_part is not None else None, c.G, c.Mg, c.N, c.K, S()),
            case_id(c))
    finally:
        lib.cdrl_set_op_activation_type(0)
    sync()


def fresh_outputs(c, base, dt):
    K, N, G = c.K, c.N, c.G
    ld, coff = a_view(c, 'da')
    sent = lambda n: torch.full((n,), SENTINEL, device=DEV)       # noqa: E731
    return dict(da=Framed(G * c.Mg, ld, coff + np.arange(K), dt, base=base), dw=Banded(K * N, torch.float32, SENTINEL),
                db=Banded(N, torch.float32, SENTINEL), adg=sent(K), adb=sent(K), acf=sent(3 * G * K), odg=sent(N), odb=sent(N))


def outputs_of(c, out, fin):
    names = ['da', 'dw', 'db'] + (['adg', 'adb', 'acf'] if c.anorm else []) + (['odg', 'odb'] if fin else [])
    return {n: (out[n].whole if n == 'da' else out[n].t if n in ('dw', 'db') else out[n]) for n in names}


@pytest.mark.parametrize('c', PARAMS)
def test_variant(lib, c):
    K, N, G, Mg = c.K, c.N, c.G, c.Mg
    M = G * Mg
    dt = BF if c.bf16 else torch.float32
    rng = np.random.default_rng([11, K, N, G, Mg, c.relu, c.anorm, c.acc, c.fin, c.bf16, len(c.a), len(c.dz)])
    inp = pw_ref.draw(rng, G, Mg, K, N, c.relu, c.anorm, bool(c.bf16))
    fin_part = pw_ref.fin_partials(inp, rng, c.fin) if c.fin else None
    coef = None if c.fin else pw_ref.generic_coef(inp, rng)
    ref = pw_ref.evaluate(inp, coef, fin_part)
    ldz, cdz, ctot = dz_view(c)
    lda, ca = a_view(c, 'a')
    ldd, cd = a_view(c, 'da')
    t = dict(dz=Framed(M, ldz, pw_ref.view_cols(cdz, N, ctot), dt, payload=inp.dz), y=Framed(M, N, np.arange(N), dt, payload=inp.y),
             a=Framed(M, lda, ca + np.arange(K), dt, payload=inp.x), yst=dev(inp.yst), ast=dev(inp.ast), ga=dev(inp.ga), ba=dev(inp.ba),
             w=dev(inp.w))
    base = (pw_ref.bf(rng.standard_normal((GR + M + GR, ldd))) if c.bf16 else rng.standard_normal((GR + M + GR, ldd))).astype(np.float32)
    if not c.acc:
        base = np.full((GR + M + GR, ldd), SENTINEL, np.float32)
    out = fresh_outputs(c, base, dt)
    # the plan, for the very views of the launch
    p = plan_query(lib, c, t['dz'].ptr, t['a'].ptr, out['da'].ptr)
    check_plan(p, c)
    lib.cdrl_set_op_activation_type(c.bf16)
    try:
        assert (p['qpart_elems'], p['dbpart_elems']) == tuple(int(lib.cdrl_pwconv_bwd_fused_workspace(G, Mg, N, K, wh)) for wh in (0, 1))
    finally:
        lib.cdrl_set_op_activation_type(0)
    assert p['dbpart_elems'] == G * p['nbpg'] * p['np'] * (3 if c.bf16 else 1) and p['qpart_elems'] == G * p['nbpg'] * p['kp'] * p['np']
    assert p['spart_offset'] == (G * p['nbpg'] * p['np'] if c.bf16 and c.anorm else 0)
    t['wp'] = torch.zeros(int(lib.cdrl_pwconv_x3_packed_bytes(N)), dtype=torch.uint8, device=DEV)
    _lib.check(lib.cdrl_pwconv_x3_pack(P(t['w']), N, K, 1, N, P(t['wp']), S()))
    t['qpart'] = Banded(p['qpart_elems'], torch.float32, float('nan'), band=4096)
    t['dbpart'] = Banded(p['dbpart_elems'], torch.float64, float('nan'), band=1024)
    t['fin_tot'] = Banded(G * 2 * N, torch.float64, float('nan'))
    for b in (t['qpart'], t['dbpart'], t['fin_tot']):
        b.ref = torch.full_like(b.lo, float('nan'))
    CF, FP = (dev(coef) if coef is not None else None), (dev(fin_part, torch.float64) if c.fin else None)
    launch(lib, c, t, CF, FP, out)

    def guards(o):
        assert o['da'].frame_intact(), 'wrote outside the dA view'
        assert o['dw'].intact() and o['db'].intact(), 'wrote outside dW / db'
        assert t['qpart'].intact() and t['dbpart'].intact() and t['fin_tot'].intact(), 'wrote outside a workspace'
    guards(out)
    got = outputs_of(c, out, c.fin)
    assert all(clean(v if n != 'da' else out['da'].payload()) for n, v in got.items()), [n for n, v in got.items() if not clean(v)]
    # again, on the dirty workspace: bit-equal
    out2 = fresh_outputs(c, base, dt)
    launch(lib, c, t, CF, FP, out2)
    guards(out2)
    for (n, u), v in zip(got.items(), outputs_of(c, out2, c.fin).values()):
        assert torch.equal(bits(u), bits(v)), f'{n} not reproducible'
    # against the reference
    f64 = np.float64
    da = out['da'].payload().double().cpu().numpy()
    exp_da = ref.da + (base[GR:GR + M, cd:cd + K].astype(f64) if c.acc else 0.0)
    dw, db = out['dw'].t.cpu().numpy().reshape(K, N).astype(f64), out['db'].t.cpu().numpy().astype(f64)
    dwmax = np.abs(ref.dw).max()
    if c.bf16:
        note(c, 'da', rel_err(da, exp_da), 6e-3)
        note(c, 'dW', rel_err(dw, ref.dw), 5e-4)
        note(c, 'db', np.abs(db - ref.db).max(), 1e-4 * max(np.abs(ref.db).max(), 1e-3 * dwmax))
        tol = 5e-4
    else:
        note(c, 'da', rel_err(da, exp_da), 1e-5)
        note(c, 'dW', rel_err(dw, ref.dw), 1e-5)
        note(c, 'db', np.abs(db - ref.db).max(), 2e-5 * max(np.abs(ref.db).max(), 1e-4 * dwmax) + 1e-5 * dwmax)
        tol = 2e-5
    if c.anorm:
        cf = out['acf'].cpu().numpy().reshape(3, G, K).astype(f64)
        assert np.array_equal(cf[0], inp.ast[2].astype(f64)), 'a_coef k1 is not the scale row'
        sc = max(np.abs(ref.s2).max(), np.abs(ref.s1).max()) / Mg
        note(c, 'a_coef k2', np.abs(cf[1] - ref.a_coef[1]).max(), tol * sc)
        note(c, 'a_coef k3', np.abs(cf[2] - ref.a_coef[2]).max(), tol * sc)
        note(c, 'a_dgamma', rel_err(out['adg'].cpu().numpy(), ref.a_dgamma), tol)
        note(c, 'a_dbeta', np.abs(out['adb'].cpu().numpy() - ref.a_dbeta).max(), tol * np.abs(ref.a_dgamma).max())
    if c.fin:
        # one float32 rounding of a double sum, per channel
        for name, g_, r_, a_ in (('o_dbeta', out['odb'], ref.o_dbeta, ref.o_abs[0]), ('o_dgamma', out['odg'], ref.o_dgamma, ref.o_abs[1])):
            d = np.abs(g_.cpu().numpy().astype(f64) - r_)
            assert np.all(d <= 2.0 ** -23 * a_), (case_id(c), name, float((d - 2.0 ** -23 * a_).max()))
            WORST[('f32', name)] = max(WORST.get(('f32', name), (0.0, 0.0, '')), (float((d / np.maximum(a_, 1e-300)).max() / 2.0 ** -23), float(d.max()), case_id(c)))
        tot = t['fin_tot'].t.cpu().numpy().reshape(G, 2, N)
        assert np.allclose(tot, fin_part.sum(axis=1), rtol=1e-14, atol=1e-14 * np.abs(fin_part).sum(axis=1).max())
        # the same call in the coefficient form, with k2 / k3 as bn_bwd_finalize would leave them: da to the same bound
        out3 = fresh_outputs(c, base, dt)
        launch(lib, c, t, dev(ref.k.astype(np.float32)), None, out3)
        guards(out3)
        note(c, 'da (coefficient form)', rel_err(out3['da'].payload().double().cpu().numpy(), exp_da), 1e-5)
        FIN_BITS.append(all(torch.equal(bits(u), bits(v)) for u, v in zip(list(got.values())[:3], list(outputs_of(c, out3, 0).values())[:3])))


def test_report():
    """Prints what the cases observed (run the module with -s): worst error per output as a fraction of its bound, and how often the
    finalize-on-load form and the coefficient form gave bit-equal da / dW / db."""
    for (ty, name), (frac, err, cid) in sorted(WORST.items()):
        print(f'worst {ty} {name}: {err:.3e} = {frac:.3f} of its bound ({cid})')
    print(f'finalize-on-load vs coefficient form bit-equal in {sum(FIN_BITS)} of {len(FIN_BITS)} cases')
    assert all(frac <= 1.0 for frac, _, _ in WORST.values())
