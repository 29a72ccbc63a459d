"""Filter-gradient GEMM family  W[K][N] (+)= sum_m a'[m][K]^T d'[m][N]  (cdrl_gemm_tn_ex -> gemm_tn: csrc/gemm_tn_direct.hip, csrc/gemm_tn_lds.hip;
cdrl_reduce_partials_f32: csrc/gemm.hip): every form the host code can dispatch, at op level, against the float64 contract of tests/tn_ref.py.

Each case first reads the plan (cdrl_gemm_tn_plan / cdrl_reduce_partials_plan -- the structs the launchers dispatch on) and asserts the
fields it is there for; `test_coverage` holds the union of the cases' instantiations (kernel, MODE, NJW, APRO, DPRO) against REQUIRED, the
hand-written list of what the launch ladders can instantiate, and every product the three engines send to gemm_tn against the cases.

Nothing here can pass by luck: the workspace starts as NaN, the output as a sentinel (or a random base when accumulating) between guard
bands that must come back bit-intact; a, d and y live inside larger allocations whose surroundings are NaN (guard rows above and below,
guard columns left and right); every case runs a second time on the dirty workspace and must reproduce itself bit for bit.

Bounds.  The floor is what the suite already asks of this op: error over tensor maximum below 1e-5 (3e-5 with the D prologue) for float32
operands, 1e-5 against the exact product of the bf16 tensors under bf16 storage without prologues, 6e-3 against the unrounded product
for bf16 operands behind a prologue (tests/test_gpu_ops.py, test_gpu_bf16_storage.py, test_gpu_bf16.py).  On top of it EVERY ELEMENT is
held to a worst-case rounding bound
    |got - ref| <= (L + c) 2^-24 S [+ allow]                    S = |a'|^T D^ (tests/tn_ref.py), u = 2^-24
L = the longest row chain of one accumulator, from the plan: ceil(rows_per / (RS RS2)) rounded up to even (direct kernels), rows_per
(LDS kernel).  v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain: one rounding of the running sum (<= u S) per row.  A bf16 MFMA adds 16
exact products per instruction; it is charged one rounding per product = per row (six instructions per 16 rows in the plane-split form:
charged 16 roundings per 16 rows as well -- each instruction's aligned sum and final rounding within 16/6 u of the running magnitude).
c = the fixed number of other roundings, counted per form:
    1  the float32 rounding of the double sum of the partials (the reduce)
    1  second-order terms of all products (1 + delta)(1 + delta'), (L + c)^2 u^2 << u
    1  with RS2 = 2: the fold of the second half-workgroup's accumulator
    1  with the A prologue: the fused multiply-add (float32 operands only)
    5  with the D prologue (float32 operands only): relative to D^ the term xhat k3 carries the roundings of y - mean, (.) invstd,
       xhat k3, the subtraction and the product with k1 (5); dz - k2 carries its own subtraction, the second one and k1 (3)
    3  MODE 3 of the LDS kernel: the three dropped plane products x2 d3, x3 d2, x3 d3 <= (2 + 2^-8) u |x| |d|
bf16 operands: the reference reproduces the float32 prologues and the rounding, so c = 2 (+ 1 with RS2 = 2) and `allow` = 2^-8 |a'| |d'|
over the operand pairs tests/tn_ref.py flags (an operand within one float32 ulp of a bf16 tie may round the other way); the inputs are
chosen on the CPU such that no case has such a pair: flagged elements are drawn again (tests/test_gemm_tn_plan_host.py holds the share,
which the issue bounds by 1 %, at zero).
With accumulate the result is float32(base + float32(product)): one more rounding of |base + ref|.
Reduce: inputs are multiples of 2^-10 below 2^8, so the double sum is exact in any order and the result must EQUAL float32(sum) --
with accumulate float32(base + float32(sum))."""
import ctypes as C
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from oracle.spec import NetConfig, unit_plan
from tests import tn_ref
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
SENTINEL = -2.0 ** 100
GR = 2                          # guard rows above and below every 2-D tensor
U24 = 2.0 ** -24
LDS_F32 = os.environ.get('CDRL_TN_LDS_F32') == '1'      # the library reads it once per process: float32 LDS cases then run MODE 0, else MODE 3

PLAN_FIELDS = ('ok', 'refusal', 'kernel', 'mode', 'apro', 'dpro', 'NJW', 'WK', 'NSPL', 'RS', 'RS2', 'U', 'gy', 'gz', 'nspg', 'nsplit', 'rows_per',
               'part_slots', 'part_elems', 'reduce_form', 'dhalf')
REDUCE_FIELDS = ('form', 'grid', 'bx', 'by')
FAKE = 1 << 20
DIRECT, DIRECT_TR, LDS = 0, 1, 2
ROW_EDGES = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 127, 128, 129, 255, 256, 257, 511, 512, 513)

# bf: 0 float32 operands, 1 bf16 operands of float32 tensors, 2 bf16 tensors.  a: dense | split (right half) | pad | odd (odd offset);
# d: dense | pad | lo | hi (through the shuffle of a ctot-channel tensor, default 2 N; needs the D prologue)
Case = namedtuple('Case', 'K N G Mg apro dpro relu acc bf a d ctot expect tag')


def mk(K, N, G=2, Mg=77, apro=0, dpro=0, relu=0, acc=0, bf=0, a='dense', d='dense', ctot=0, tag='', **expect):
    assert dpro or (d in ('dense', 'pad') and not relu)
    return Case(K, N, G, Mg, apro, dpro, relu, acc, bf, a, d, ctot, expect, tag)


def a_view(c):
    return {'dense': (c.K, 0), 'split': (2 * c.K, c.K), 'pad': (c.K + 6, 2), 'odd': (c.K + 5, 1)}[c.a]


def d_view(c):
    """(ld, coff, shuffle_ctot)"""
    if c.d == 'dense':
        return c.N, 0, 0
    if c.d == 'pad':
        return c.N + 10, 4, 0
    ctot = c.ctot or 2 * c.N
    return ctot, (0 if c.d == 'lo' else ctot - c.N), ctot


def case_id(c):
    return f"{('f32', 'bf16op', 'bf16')[c.bf]}-{c.tag}-K{c.K}N{c.N}G{c.G}M{c.Mg}-a{c.apro}d{c.dpro}r{c.relu}c{c.acc}-{c.a}.{c.d}{c.ctot or ''}"


def lds_mode(bf):
    return (0 if LDS_F32 else 3, 1, 2)[bf]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
CASES = []
_rows = [0]


def next_rows(n=1):
    """the next row count(s) of ROW_EDGES, in turn: the edges are spread over the forms, not crossed with them"""
    _rows[0] += 1
    return ROW_EDGES[(7 * _rows[0]) % len(ROW_EDGES)]


A_FORMS, D_PLAIN, D_SHUF = ('dense', 'split', 'pad'), ('dense', 'pad'), ('lo', 'hi')
# every instantiation of the direct kernels: NJW x APRO x (U, MODE); tn_direct_kernel without, tn_direct_tr_kernel with the D prologue
NJW_SHAPES = {(DIRECT, 1): ((24, 24), (24, 58), (58, 58)), (DIRECT, 2): ((58, 128), (116, 58)), (DIRECT, 4): ((116, 80), (117, 116)),
              (DIRECT_TR, 1): ((24, 24), (58, 24), (58, 58)), (DIRECT_TR, 2): ((116, 58), (58, 116)), (DIRECT_TR, 4): ((80, 116), (116, 117))}
i = 0
for kern in (DIRECT, DIRECT_TR):
    for njw in (1, 2, 4):
        for apro in (0, 1):
            for bf in (0, 1, 2):
                for K, N in NJW_SHAPES[(kern, njw)]:
                    i += 1
                    dp = int(kern == DIRECT_TR)
                    CASES.append(mk(K, N, G=1 + i % 4, Mg=next_rows(), apro=apro, dpro=dp, relu=dp * (i % 2), acc=int(i % 5 == 0), bf=bf,
                                    a=A_FORMS[i % 3], d=(D_SHUF[i % 2] if dp and N % 2 == 0 and i % 3 else D_PLAIN[i % 2]), tag='inst',
                                    kernel=kern, NJW=njw, mode=bf, U=8 if (bf or dp) else 4))
# every instantiation of the LDS kernel: MODE x APRO x DPRO (float32 operands: MODE 3, or MODE 0 in the child process of
# test_lds_float32_mfma_forms)
for bf in (0, 1, 2):
    for apro in (0, 1):
        for dp in (0, 1):
            for K, N in ((116, 116), (232, 130)):
                i += 1
                CASES.append(mk(K, N, G=1 + i % 4, Mg=next_rows(), apro=apro, dpro=dp, relu=dp * (i % 2), acc=int(i % 5 == 0), bf=bf,
                                a=('dense', 'split', 'pad')[i % 3], d=(D_SHUF[i % 2] if dp and i % 3 else D_PLAIN[i % 2]),
                                tag='ldsf32' if bf == 0 else 'inst', kernel=LDS, mode=lds_mode(bf)))
# row edges: every count of ROW_EDGES on the direct kernel with 8-row batches (U 4: float32 without the D prologue), with 16-row batches
# (float32 with the D prologue, bf16 operands, bf16 tensors) and on the LDS kernel (chunks of 32; float32 and bf16 tensors); odd Mg with
# G > 1 makes group starts odd.  Mg < 8 with RS 4 leaves shares empty; 256 switches RS2; 256 / 512 (LDS) split a group over workgroups.
for j, Mg in enumerate(ROW_EDGES):
    G = (2, 3, 1, 4)[j % 4]
    CASES.append(mk(24, 24, G=G, Mg=Mg, apro=j % 2, tag='rows', kernel=DIRECT, U=4, RS=4, RS2=2 if Mg >= 256 else 1))
    CASES.append(mk(58, 24, G=G, Mg=Mg, dpro=1, relu=j % 2, tag='rows', kernel=DIRECT_TR, U=8, RS2=2 if Mg >= 256 else 1))
    CASES.append(mk(24, 58, G=G, Mg=Mg, bf=1 + j % 2, tag='rows', kernel=DIRECT, U=8, RS=2))
    CASES.append(mk(116, 116, G=G, Mg=Mg, apro=j % 2, bf=(0, 2)[j % 2], tag='ldsf32' if j % 2 == 0 else 'rows', kernel=LDS))
# column edges: 32 | 33, 64 | 65 tiles; 96 direct <-> LDS; 128 | 130 a second column block with one tile (idle waves, planned from the
# first block); widths that are 2 mod 4 (98, 102, 130) with and without the shuffle: dhalf on the LDS kernel, float32 and bf16 tensors
for j, (K, N) in enumerate(((32, 33), (33, 32), (64, 65), (65, 64), (96, 92), (92, 96), (96, 96), (128, 130), (130, 128), (98, 98), (130, 130),
                            (8, 16), (16, 8), (464, 98))):
    wide = K >= 96 and N >= 96 and K % 2 == 0 and N % 2 == 0
    kd, kt = (LDS, LDS) if wide else (DIRECT, DIRECT_TR)
    CASES.append(mk(K, N, G=2, Mg=75, apro=j % 2, tag='ldsf32' if wide else 'cols', kernel=kd))
    CASES.append(mk(K, N, G=3, Mg=41, dpro=1, relu=1, acc=j % 2, tag='ldsf32' if wide else 'cols', kernel=kt))
    CASES.append(mk(K, N, G=2, Mg=75, apro=1 - j % 2, dpro=j % 2, bf=2, tag='cols', kernel=(kt if j % 2 else kd)))
for bf in (0, 2):
    for N in (98, 102):
        for half in ('lo', 'hi'):
            CASES.append(mk(116, N, G=2, Mg=45, apro=int(half == 'lo'), dpro=1, relu=1, bf=bf, d=half, ctot=2 * N + 4 * int(half == 'hi'),
                            tag='ldsf32' if bf == 0 else 'dhalf', kernel=LDS, dhalf=1))
    CASES.append(mk(98, 102, G=2, Mg=45, dpro=1, bf=bf, d='pad', tag='ldsf32' if bf == 0 else 'dhalf', kernel=LDS, dhalf=0))
CASES.append(mk(116, 98, G=2, Mg=45, dpro=1, relu=1, bf=1, d='hi', tag='dhalf', kernel=LDS, dhalf=1))
# the fallback out of the LDS kernel for wide shapes: odd ld / offset / K / N, or an odd half of the shuffled tensor -> NJW 4
for bf in (0, 1, 2):
    CASES.append(mk(116, 116, G=2, Mg=65, apro=1, bf=bf, a='odd', tag='fallback', kernel=DIRECT, NJW=4))
    CASES.append(mk(116, 116, G=2, Mg=65, dpro=1, relu=1, bf=bf, d='hi', ctot=234, tag='fallback', kernel=DIRECT_TR, NJW=4))
    CASES.append(mk(117, 116, G=1, Mg=130, bf=bf, tag='fallback', kernel=DIRECT, NJW=4))
    CASES.append(mk(232, 117, G=2, Mg=65, dpro=1, bf=bf, tag='fallback', kernel=DIRECT_TR, NJW=4, gy=2))
# accumulate on every kernel
for bf in (0, 2):
    CASES.append(mk(58, 58, G=2, Mg=140, acc=1, bf=bf, tag='acc', kernel=DIRECT))
    CASES.append(mk(58, 58, G=2, Mg=140, apro=1, dpro=1, relu=1, acc=1, bf=bf, d='hi', tag='acc', kernel=DIRECT_TR))
    CASES.append(mk(116, 232, G=2, Mg=140, apro=1, dpro=1, relu=1, acc=1, bf=bf, d='lo', tag='ldsf32' if bf == 0 else 'acc', kernel=LDS))
# many partials: the float4 reduces behind the GEMM (16 slots and more)
CASES.append(mk(232, 232, G=4, Mg=512, apro=1, dpro=1, relu=1, d='hi', tag='ldsf32', kernel=LDS, part_slots=16, reduce_form=1))
CASES.append(mk(58, 92, G=4, Mg=1024, apro=1, dpro=1, relu=1, bf=2, d='hi', ctot=116, tag='parts', kernel=DIRECT_TR, part_slots=16, reduce_form=2))
CASES.append(mk(9, 16, G=1, Mg=1024, tag='parts', kernel=DIRECT, part_slots=16, reduce_form=2))

PARAMS = [pytest.param(c, id=case_id(c)) for c in CASES]
assert len({case_id(c) for c in CASES}) == len(CASES), [x for x in [case_id(c) for c in CASES] if [case_id(c) for c in CASES].count(x) > 1]


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def plan_query(lib, c, pa=FAKE, pd=FAKE):
    ldd, cd, ctot = d_view(c)
    va, vd = _lib.View(pa, *a_view(c)), _lib.View(pd, ldd, cd)
    out = (C.c_int32 * len(PLAN_FIELDS))()
    n = lib.cdrl_gemm_tn_plan(C.byref(va), C.byref(vd), c.G * c.Mg, c.N, c.K, c.G, c.apro, c.dpro, ctot, c.relu, int(c.bf > 0), int(c.bf == 2), out,
                              len(PLAN_FIELDS))
    assert n == len(PLAN_FIELDS), n
    return dict(zip(PLAN_FIELDS, out))


def signature(p, acc):
    return (p['kernel'], p['mode'], p['NJW'], p['apro'], p['dpro'], acc, p['reduce_form'], p['dhalf'])


def check_plan(lib, p, c):
    assert p['ok'] == 1 and p['refusal'] == 0, (case_id(c), p)
    for k, v in c.expect.items():
        assert p[k] == v, (case_id(c), k, p)
    assert (p['apro'], p['dpro']) == (c.apro, c.dpro) and (p['kernel'] == DIRECT_TR) == (c.dpro == 1 and p['kernel'] != LDS), p
    assert p['mode'] == (lds_mode(c.bf) if p['kernel'] == LDS else c.bf), (case_id(c), p)
    assert p['part_elems'] == p['part_slots'] * c.K * c.N <= lib.cdrl_gemm_tn_ex_workspace_elems(c.G * c.Mg, c.N, c.K, c.G), p
    if c.tag == 'ldsf32':
        assert p['kernel'] == LDS and c.bf == 0, case_id(c)


def chain_and_count(p, c):
    """(L, c) of the module docstring"""
    if p['kernel'] == LDS:
        L = p['rows_per']
        cnt = 2 + ((c.apro + 5 * c.dpro) if c.bf == 0 else 0) + (3 if p['mode'] == 3 else 0)
    else:
        L = -(-p['rows_per'] // (p['RS'] * p['RS2']))
        L += L % 2
        cnt = 2 + (p['RS2'] == 2) + ((c.apro + 5 * c.dpro) if c.bf == 0 else 0)
    return L, cnt


# ---- REQUIRED: what the launch ladders can instantiate, written out from them ---------------------------------------------------------
# tn_direct_kernel<NJW, APRO, false, U, MODE> (never with the D prologue: the plan maps that to the transposed kernel),
# tn_direct_tr_kernel<NJW, APRO, true, 8, MODE>, tn_lds_kernel<MODE, APRO, DPRO>; MODE 0 of the LDS kernel only under CDRL_TN_LDS_F32=1,
# which replaces MODE 3 for the process
REQUIRED = ({(DIRECT, m, w, a, 0) for m in (0, 1, 2) for w in (1, 2, 4) for a in (0, 1)}
            | {(DIRECT_TR, m, w, a, 1) for m in (0, 1, 2) for w in (1, 2, 4) for a in (0, 1)}
            | {(LDS, m, 0, a, d) for m in (lds_mode(0), 1, 2) for a in (0, 1) for d in (0, 1)})
REDUCE_REQUIRED = {(f, a) for f in range(6) for a in (0, 1)}


def engine_products():
    """(bf, K, N, G, M, a (ld, coff), d (ld, coff, ctot), apro, dpro, relu) of every product the float32, bf16-operand and bf16-storage
    engines send to gemm_tn at the default NetConfig (90 x 120 images, minibatch 256), from the unit plan the engines are built from:
    the unit convs the fused backward (tests/test_gpu_pw_bwd_variants.py) does not take keep the two-kernel form with the D prologue
    -- all of them in the bf16-operand engine, otherwise those wider than 128 channels or padded differently under bf16 storage --; the
    head conv and the dense / GRU layers are plain products (the dense and GRU ones in float32 in every engine); a conv without the
    fused BatchNorm backward sends its plain form with the A prologue alone."""
    cfg = NetConfig(H=90, W=120)
    B, T = 256, cfg.T
    for bf in (0, 1, 2):
        h, w = -(-((cfg.H - 3) // 2 + 1) // 2), -(-((cfg.W - 3) // 2 + 1) // 2)
        for u in unit_plan(cfg):
            s2 = u['stride'] == 2
            ho, wo = (-(-h // 2), -(-w // 2)) if s2 else (h, w)
            cin, c_out, sc = u['cin'], u['cout'], u['shortcut_c']
            xin = (cin, 0) if s2 else (cin, sc)
            convs = [(u['main_in'], u['mid'], T * B * h * w, xin, (u['mid'], 0, 0), 0, 0),
                     (u['mid'], u['main_out'], T * B * ho * wo, (u['mid'], 0), (c_out, sc, c_out), 1, 1)]
            if s2:
                convs.append((sc, sc, T * B * ho * wo, (sc, 0), (c_out, 0, c_out), 1, 1))
            for K, N, M, av, dv, apro, relu in convs:
                yield (bf, K, N, T, M, av, dv, apro, 1, relu)
                if apro:
                    yield (bf, K, N, T, M, av, (N, 0, 0), 1, 0, 0)
            h, w = ho, wo
        yield (bf, cfg.stage_channels[-1], cfg.last_channels, 1, T * B * h * w, (cfg.stage_channels[-1], 0), (cfg.last_channels, 0, 0), 0, 0, 0)
    cat = cfg.rnn_image + 3 * cfg.rnn_small
    dense = [(d, cfg.feat_units, T * B) for d in (cfg.road, cfg.vehicle, cfg.navigation)] + [(cfg.feat_units, cfg.feat_units, T * B)]
    dense += [(cat, cfg.dyn_units, B), (cfg.dyn_units, cfg.head_units, B), (cfg.head_units, cfg.head_units, B)]
    dense += [(cfg.last_channels, 3 * cfg.rnn_image, T * B), (cfg.rnn_image, 3 * cfg.rnn_image, T * B), (cfg.feat_units, 3 * cfg.rnn_small, T * B),
              (cfg.rnn_small, 3 * cfg.rnn_small, T * B)]
    for K, N, M in dense:
        yield (0, K, N, 1, M, (K, 0), (N, 0, 0), 0, 0, 0)


def fused_takes(lib, bf, K, N, G, Mg, av, dv, apro):
    """the engines' choice of the fused backward for a unit conv (engine.hip: plan_pw): float32 and bf16 storage, G <= 8, Cin >= 24, the
    fused plan accepts the views, a normalised input is dense"""
    if bf == 1 or K < 24 or (apro and av != (K, 0)):
        return False
    vz, va = _lib.View(None, dv[0], dv[1]), _lib.View(None, *av)
    an = C.c_void_p(FAKE) if apro else None
    out = (C.c_int32 * 18)()
    lib.cdrl_pwconv_bwd_plan(C.byref(vz), dv[2], C.byref(va), C.byref(va), 0, G, Mg, N, K, an, an, an, an, an, an, None, 0, None, None, None,
                             int(bf == 2), out, 18)
    return out[0] == 1


def engine_cases(lib):
    """one small case per distinct plan signature of the engines' products: same channels, groups, views and prologues, the smallest
    row count of a short list that keeps the product's signature (kernel, instantiation, reduce form)"""
    want = {}
    for bf, K, N, G, M, av, dv, apro, dpro, relu in engine_products():
        if dpro and fused_takes(lib, bf, K, N, G, M // G, av, dv, apro):
            continue
        form_a = {(K, 0): 'dense', (2 * K, K): 'split'}[av]
        form_d = 'dense' if dv[2] == 0 else 'lo' if dv[1] == 0 else 'hi'
        assert dv[2] == 0 or dv[1] in (0, dv[2] - N)
        big = mk(K, N, G=G, Mg=M // G, apro=apro, dpro=dpro, relu=relu, bf=bf, a=form_a, d=form_d, ctot=dv[2], tag='engine')
        assert d_view(big) == dv, (big, dv)
        sig = signature(plan_query(lib, big), 0)
        want.setdefault((sig, K, N, G, form_a, form_d, dv[2], relu), big)
    cases = []
    for (sig, K, N, G, fa, fd, ctot, relu), big in sorted(want.items()):
        for Mg in (64, 150, 256, 300, 512, 1024, 2048, 4096):
            small = big._replace(Mg=Mg)
            if signature(plan_query(lib, small), 0) == sig:
                cases.append(small)
                break
        else:
            raise AssertionError(f'no small case keeps the signature of {case_id(big)}')
    return cases


def coverage_gaps(lib):
    sigs = {signature(plan_query(lib, c), c.acc) for c in CASES}
    have = {s[:5] for s in sigs}
    gaps = [('REQUIRED', s) for s in sorted(REQUIRED - have)] + [('unknown instantiation', s) for s in sorted(have - REQUIRED)]
    gaps += [('no accumulate', k) for k in (DIRECT, DIRECT_TR, LDS) if not any(s[0] == k and s[5] == 1 for s in sigs)]
    gaps += [('no dhalf', m) for m in (lds_mode(0), 1, 2) if not any(s[0] == LDS and s[1] == m and s[7] == 1 for s in sigs)]
    rsigs = {(reduce_plan(lib, 0 if al else 4, nparts, n, stride)['form'], acc) for n, nparts, stride, al, acc, _, _ in REDUCE_CASES}
    gaps += [('reduce', s) for s in sorted(REDUCE_REQUIRED - rsigs)]
    return gaps


def test_coverage(lib):
    """The cases' plans cover REQUIRED (52 kernel instantiations: 18 + 18 direct, 12 of the LDS kernel in this process and its MODE 0
    in the child process of test_lds_float32_mfma_forms) and contain nothing REQUIRED does not know; every kernel accumulates once; dhalf
    is reached in every LDS mode; the reduce cases cover the six forms with and without accumulate; every engine product has a small
    case with its plan signature (test_engine_products runs them); the row edges are all present on each batch geometry."""
    gaps = coverage_gaps(lib)
    assert not gaps, gaps
    assert len(REQUIRED) == 48 and len(engine_cases(lib)) >= 8
    plans = [(c, plan_query(lib, c)) for c in CASES]
    for name, sel in (('U4', lambda c, p: p['kernel'] != LDS and p['U'] == 4), ('U8', lambda c, p: p['kernel'] != LDS and p['U'] == 8),
                      ('bf16 direct', lambda c, p: p['kernel'] != LDS and c.bf > 0), ('LDS', lambda c, p: p['kernel'] == LDS)):
        rows = {c.Mg for c, p in plans if sel(c, p)}
        assert set(ROW_EDGES) <= rows, (name, sorted(set(ROW_EDGES) - rows))
    assert any(c.Mg % 2 and c.G > 1 and c.bf == 2 for c in CASES)
    assert any(p['kernel'] != LDS and p['RS'] == 4 and c.Mg < 8 for c, p in plans)          # empty shares
    assert {p['RS2'] for c, p in plans if p['kernel'] != LDS} == {1, 2} and any(p['nspg'] > 1 for c, p in plans)
    assert any(p['gz'] == 2 and c.N == 130 for c, p in plans) and any(p['gy'] == 2 and c.K == 130 for c, p in plans)


# ---- guarded tensors ---------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


class Banded:
    """A 1-D tensor inside a larger one, with a band of `fill` on each side that must come back bit-intact."""

    def __init__(self, n, dtype, fill, band=256, value=None):
        self.whole = torch.full((band + n + band,), fill, dtype=dtype, device=DEV)
        self.t = self.whole[band:band + n]
        if value is not None:
            self.t.copy_(value)
        self.lo, self.hi = self.whole[:band], self.whole[band + n:]
        self.ref = self.lo.clone()

    def intact(self):
        return torch.equal(bits(self.lo), bits(self.ref)) and torch.equal(bits(self.hi), bits(self.ref))


def framed(M, ld, cols, dtype, payload):
    """(tensor, address of row 0 of the view): the payload at columns `cols` of rows GR .. GR + M of a NaN tensor [GR + M + GR][ld]"""
    whole = torch.full((GR + M + GR, ld), float('nan'), dtype=torch.float32)
    whole[GR:GR + M, torch.as_tensor(np.asarray(cols), dtype=torch.long)] = torch.as_tensor(np.asarray(payload, np.float32))
    whole = whole.to(dtype).to(DEV).contiguous()
    return whole, whole.data_ptr() + GR * ld * whole.element_size()


def sync():
    """A device fault ends the run: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device fault, stopping: {e}', returncode=3)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


WORST = {}          # (operand type, check) -> worst observed error / bound, printed by test_report


def note(c, name, err, bound):
    assert err <= bound, f'{case_id(c)}: {name} {err:.3e} > {bound:.3e}'
    key = (('f32', 'bf16op', 'bf16')[c.bf], name)
    if bound > 0 and err / bound > WORST.get(key, (0.0, 0.0, ''))[0]:
        WORST[key] = (err / bound, err, case_id(c))


def inputs_of(c):
    key = [7, c.K, c.N, c.G, c.Mg, c.apro, c.dpro, c.relu, c.acc, c.bf, len(c.a), len(c.d), c.ctot]
    return tn_ref.draw_clean(key, c.G, c.Mg, c.K, c.N, c.apro, c.dpro, c.relu, c.bf == 2, c.bf > 0)


def run_case(lib, c):
    K, N, G, Mg = c.K, c.N, c.G, c.Mg
    M = G * Mg
    dt = BF if c.bf == 2 else torch.float32
    inp, ref, rng = inputs_of(c)
    assert ref.flagged_share < 0.01, (case_id(c), ref.flagged_share)
    lda, ca = a_view(c)
    ldd, cd, ctot = d_view(c)
    ta, pa = framed(M, lda, ca + np.arange(K), dt, inp.a)
    td, pd = framed(M, ldd, tn_ref.view_cols(cd, N, ctot), dt, inp.d)
    ty, py = framed(M, N, np.arange(N), dt, inp.y)
    ast, yst, coef = dev(inp.ast), dev(inp.yst), dev(inp.coef)
    p = plan_query(lib, c, pa, pd)
    check_plan(lib, p, c)
    assert p == plan_query(lib, c), 'the plan depends on the addresses'
    ws = Banded(int(lib.cdrl_gemm_tn_ex_workspace_elems(M, N, K, G)), torch.float32, float('nan'), band=4096)
    ws.ref = torch.full_like(ws.lo, float('nan'))
    base = rng.standard_normal(K * N).astype(np.float32) * np.float32(np.abs(ref.w).mean()) if c.acc else None
    va, vd = _lib.View(pa, lda, ca), _lib.View(pd, ldd, cd)

    def launch():
        out = Banded(K * N, torch.float32, SENTINEL, value=dev(base) if c.acc else None)
        _lib.check(lib.cdrl_gemm_tn_ex(C.byref(va), P(ast) if c.apro else None, C.byref(vd), C.c_void_p(py) if c.dpro else None,
                                       P(yst) if c.dpro else None, P(coef) if c.dpro else None, ctot, c.relu, P(out.t), M, N, K, G, P(ws.t), c.acc,
                                       int(c.bf > 0), int(c.bf == 2), S()), case_id(c))
        sync()
        assert out.intact() and ws.intact(), 'wrote outside the output or the workspace'
        return out.t.clone()
    got_t = launch()
    assert bool(torch.isfinite(got_t).all()) and not bool((got_t == SENTINEL).any()), 'an output element was poisoned or never written'
    assert torch.equal(bits(got_t), bits(launch())), 'not reproducible on the dirty workspace'
    got = got_t.double().cpu().numpy().reshape(K, N)
    b64 = base.astype(np.float64).reshape(K, N) if c.acc else 0.0
    want = ref.w + b64
    L, cnt = chain_and_count(p, c)
    bound = (L + cnt) * U24 * ref.S + ref.allow
    if c.acc:
        bound = bound + U24 * (np.abs(want) + bound)
    err = np.abs(got - want)
    name = ('direct', 'direct-tr', 'lds')[p['kernel']] + f" mode {p['mode']}"
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert worst <= 1.0, f'{case_id(c)}: element {np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)} is {worst:.3f} of its bound'
    note(c, f'{name}: worst element / bound', worst, 1.0)
    scale = np.abs(ref.w).max() + 1e-30
    if c.bf == 0:
        note(c, f'{name}: tensor scale', float(err.max() / scale), 3e-5 if c.dpro else 1e-5)
    elif c.bf == 2 and not c.apro and not c.dpro:
        note(c, f'{name}: tensor scale, exact product of bf16 tensors', float(err.max() / scale), 1e-5)
    else:
        full = tn_ref.evaluate(inp, False).w
        note(c, f'{name}: tensor scale, unrounded product', rel_err(got - b64, full), 6e-3)


@pytest.mark.parametrize('c', PARAMS)
def test_variant(lib, c):
    run_case(lib, c)


def test_engine_products(lib):
    """every product of the three engines that reaches gemm_tn, at a small row count with the product's own plan signature"""
    cases = engine_cases(lib)
    for c in cases:
        run_case(lib, c)
    print('\n' + '\n'.join(f'{case_id(c)}: {plan_query(lib, c)}' for c in cases))


def test_lds_float32_mfma_forms():
    """MODE 0 of the LDS kernel (float32 operands on v_mfma_f32_32x32x2_f32) needs CDRL_TN_LDS_F32=1, which the library reads once per
    process: every float32 case that plans the LDS kernel, and the coverage with MODE 0 in the place of MODE 3, in one child process."""
    if LDS_F32:
        return
    env = dict(os.environ, CDRL_TN_LDS_F32='1')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-k', 'ldsf32 or test_coverage'], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'skipped' not in r.stdout, r.stdout[-500:]


# ---- the partial reduce -------------------------------------------------------------------------------------------------------------
# (n, nparts, stride, 16-byte aligned part, accumulate, expected form): 0 few, 1 / 2 / 3 float4 with 16 / 4 / 1 column lanes, 4 / 5 scalar
# with 16 / 4 column lanes.  The second trip of a kernel's split loop needs nparts > 128 (v4<16>: 16 lanes x 8), 512 (v4<4>), 2048
# (v4<1>, scalar<4>), 512 (scalar<16>).
REDUCE_CASES = []
for n in (4096, 4100):
    for j, nparts in enumerate((1, 3, 4, 5, 15)):
        REDUCE_CASES.append((n, nparts, n + 4 * (j % 2), 1, j % 2, 0))
REDUCE_CASES += [(13456, 16, 13456, 1, 0, 1), (13456, 17, 13460, 1, 1, 1), (13456, 129, 13456, 1, 0, 1),
                 (3364, 16, 3364, 1, 0, 2), (3364, 513, 3364, 1, 1, 2), (576, 100, 576, 1, 0, 2),
                 (576, 128, 576, 1, 0, 3), (576, 2049, 580, 1, 1, 3),
                 (986, 64, 986, 1, 0, 4), (986, 64, 986, 1, 1, 4), (13456, 17, 13456, 0, 0, 4), (3364, 16, 3365, 1, 0, 4), (576, 60, 577, 1, 1, 4), (3364, 513, 3365, 1, 1, 4),
                 (4096, 3, 4096, 0, 0, 4),
                 (986, 65, 986, 1, 0, 5), (986, 2049, 990, 1, 1, 5), (576, 128, 576, 0, 0, 5),
                 # the stem's rows [27 Cout filter sums | Cout bias sums]: n = 27 Cout, and n = Cout at offset 27 Cout (Cout 24)
                 (27 * 24, 40, 28 * 24, 1, 0, 2), (24, 40, 28 * 24, 1, 1, 2, 27 * 24), (27 * 24, 200, 28 * 24, 1, 0, 3), (24, 8, 28 * 24, 1, 0, 4, 27 * 24)]
REDUCE_CASES = [(r + (0,))[:7] for r in REDUCE_CASES]      # last field: the column of a row the reduce starts at


def reduce_plan(lib, addr, nparts, n, stride):
    out = (C.c_int32 * 4)()
    assert lib.cdrl_reduce_partials_plan(addr, nparts, n, stride, out, 4) == 4
    return dict(zip(REDUCE_FIELDS, out))


@pytest.mark.parametrize('n,nparts,stride,aligned,acc,form,col0', REDUCE_CASES)
def test_reduce(lib, n, nparts, stride, aligned, acc, form, col0):
    rng = np.random.default_rng([n, nparts, stride, aligned, acc])
    part = tn_ref.draw_partials(rng, nparts, n, stride)
    # the partials inside a NaN band; one float further when the misaligned path is wanted; what lies beyond n in a row is NaN as well
    # unless the row is the stem's (stride > n + 4: the other reduce's columns, finite)
    host = part.copy()
    if stride <= n + 4:
        host[:, n:] = np.nan
    off = 0 if aligned else 1
    buf = Banded(nparts * stride + off, torch.float32, float('nan'), band=1024)
    buf.t[off:].copy_(dev(np.roll(host, col0, axis=1).reshape(-1)))      # (columns [col0, col0 + n) of every row hold the partials)
    src = buf.t[off + col0:]
    assert (src.data_ptr() % 16 == 0) == bool(aligned)
    p = reduce_plan(lib, src.data_ptr(), nparts, n, stride)
    assert p['form'] == form, p
    base = rng.integers(-1000, 1000, n + 8).astype(np.float32) * np.float32(2.0 ** -3) if acc else None
    out = Banded(n + 8, torch.float32, SENTINEL, value=dev(base) if acc else None)
    start = out.t.clone()
    _lib.check(lib.cdrl_reduce_partials_f32(P(src), nparts, n, stride, P(out.t), acc, S()))
    sync()
    assert out.intact() and torch.equal(bits(out.t[n:]), bits(start[n:])), 'wrote beyond n'
    want = tn_ref.reduce_ref(part, n, base[:n] if acc else None)
    got = out.t[:n].cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (int((got != want).sum()), float(np.abs(got - want).max()))


def test_report():
    """Prints what the cases observed (run the module with -s): the worst figure per kernel and check as a fraction of its bound."""
    for (ty, name), (frac, err, cid) in sorted(WORST.items()):
        print(f'worst {ty} {name}: {err:.3e} = {frac:.3f} of its bound ({cid})')
    assert all(frac <= 1.0 for frac, _, _ in WORST.values())
