"""Dense GEMM family  c[M][N] (+)= a'[M][K] B(k, n) + bias  (cdrl_gemm_nn_ex -> gemm_nn: csrc/gemm.hip, with its split-K slab reduce and the
activation fused into it), the dense activations (cdrl_act_fwd / cdrl_act_bwd), the bias-gradient path (cdrl_colsum, cdrl_reduce_partials)
and cdrl_permute_bt (csrc/bn.hip): every form the host code can dispatch, at op level, against the float64 contract of tests/nn_ref.py.

Each GEMM case first reads the plan (cdrl_gemm_nn_plan -- the struct the launcher dispatches on), asserts the fields it is there for and
holds the whole plan to the restatement of the ladder in tests/nn_ref.py; `test_coverage` holds the union of the cases' instantiations
(kernel, NT, WR, BT, VEC) against REQUIRED, the hand-written list of what the ladder can instantiate, and `test_engine_products` every
product add_dense / add_gru send to gemm_nn against the cases.

Nothing here can pass by luck: a, B and bias live inside larger NaN allocations (guard rows above and below, guard columns left and
right); c is a sentinel (or the base when accumulating) whose surroundings must come back bit-intact; the workspace starts as NaN
between guard bands; act_out is a sentinel between guard bands; every case runs a second time on the dirty workspace and must
reproduce itself bit for bit.

Exactness contract.  Every case runs once with exact inputs -- integers |a| <= 1023 (10 mantissa bits: operands silently rounded to bf16
would change), |b| <= 15, integer bias and base, S = sum |a||b| + |bias| (+ |base|) < 2^24 per element (asserted on the CPU), so every
partial sum is representable in any order and under any split: the output must EQUAL the exact value -- and once with standard-normal
operands, where EVERY ELEMENT is held to the worst-case rounding bound
    |got - ref| <= (L + c) 2^-24 S
L = the accumulator's chain length from the plan: K (v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain: one rounding of the running sum,
<= 2^-24 S, per k), or kchunk + gz under split-K (one slab's chain, then the gz additions of the reduce); c = 2 for the bias addition and
the second-order terms, + 1 when accumulating.  Both are derived, not measured.

Fused activation: act_out must be bit-equal to cdrl_act_fwd of the c the same call wrote (both go through act_value of
csrc/cdrl_common.h), and that c bit-equal to the c of the same call without act_out.

Activations on their own.  relu6 forward and backward are exact.  For swish6 / tanh / sigmoid the error depends on the device's expf /
tanhf, so it is measured against the float64 reference in units of 2^-24 max(|ref|, tiny) and asserted at four times the largest
measured value (MEASURED below; the margin is for inputs other than the tested ones).  tiny = 2^-100 for values (below it results are
subnormal or flushed: an absolute scale), and 1 for derivatives: 1 - t^2, s (1 - s) and s (1 + x (1 - s)) are differences of terms of
magnitude <= 1 each carrying its own relative rounding, so their error scales with 2^-24 of the terms, not of the difference (tanh'(5) =
1.8e-4 computed from t = 0.99991 cannot be better than 2^-24 absolute).  Measured on an MI355X over the inputs of nn_ref.act_inputs
(n = 2048 * 256 + 1), largest per quantity:
    swish6 2.744 (value, x = -1.213) and 9.055 (derivative, x = 5.959: the rounding of 1 - s, s = 0.9974, times x), tanh 2.398 and 2.384,
    sigmoid 2.068 and 1.496 -- none above 16 units; asserted at 10.98 / 36.22, 9.59 / 9.54, 8.27 / 5.98.
Finding: act_bwd decided the swish6 gate on the rounded float32 product x sigmoid(x) < 6.0f, which reaches 6.0f at x = 6.01465607, one
float32 below x*, where the true product is still below 6: the gradient was 0 there instead of 1.0.  The gate is now decided on x
(x < 6.01465654f, the smallest float32 above x*); the neighbours of x* in the inputs are its regression test.
The open / closed side of the swish6 gate (x sigmoid(x) < 6, clamp at x* = 6.01466) must agree with the float64 rule at every tested
input, the float32 neighbours of x* on both sides included.

Bias gradient: integer-valued inputs, so the double sums are exact: the result must EQUAL float32(sum), float32(base + float32(sum)) when
accumulating.  cdrl_permute_bt is a bit-exact gather."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from oracle.spec import NetConfig, unit_plan
from tests import nn_ref
from tests.nn_ref import RT, SPLITK, TILE, cdiv

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -2.0 ** 100
GR = 2                          # guard rows above and below every 2-D tensor
U24 = 2.0 ** -24
FAKE = 1 << 20
ROW_EDGES = (1, 63, 64, 65, 127, 128, 129)
K_EDGES = (1, 2, 3, 31, 32, 33, 63, 64, 65)
# N -> (NT, gy): written out by hand from the column-block balancing (129 -> 2 blocks of 3 tiles, 232 -> 2 x 4, 320 -> 3 x 4)
N_EDGES = {1: (1, 1), 32: (1, 1), 33: (2, 1), 64: (2, 1), 65: (3, 1), 96: (3, 1), 97: (4, 1), 128: (4, 1), 129: (3, 2), 130: (3, 2), 160: (3, 2),
           232: (4, 2), 320: (4, 3)}
# largest measured error per (activation, quantity) in units of 2^-24 max(|ref|, tiny) -- see the module docstring; asserted at 4 x
MEASURED = {('swish6', 'value'): 2.744, ('swish6', 'deriv'): 9.055, ('tanh', 'value'): 2.398, ('tanh', 'deriv'): 2.384,
            ('sigmoid', 'value'): 2.068, ('sigmoid', 'deriv'): 1.496}
TINY = {'value': 2.0 ** -100, 'deriv': 1.0}

# a: dense | pad (even offset 2, ld = 2 mod 4 for K = 0 mod 4) | pad4 (16-byte aligned rows) | oddld | oddoff | p4 (pointer = 4 mod 8) |
#    p8 (pointer = 8 mod 16);  c: dense | pad;  b: '' | 'b8' (pointer = 8 mod 16)
# act: None = no act_out; 0..4 = act_out given.  done: 1 = act_done given, 0 = null
Case = namedtuple('Case', 'M K N order a c b bias acc ws act done tag expect')


def mk(M, K, N, order='w', a='dense', c='dense', b='', bias=1, acc=0, ws=0, act=None, done=1, tag='', **expect):
    return Case(M, K, N, order, a, c, b, bias, acc, ws, act, done, tag, expect)


def a_view(c):
    """(ld, coff, pointer offset in floats mod 4)"""
    K = c.K
    even = K + K % 2
    return {'dense': (K, 0, 0), 'pad': (even + 6, 2, 0), 'pad4': (cdiv(K, 4) * 4 + 8, 4, 0), 'oddld': (even + 5, 0, 0), 'oddoff': (even + 6, 1, 0),
            'p4': (K, 0, 1), 'p8': (K, 0, 2)}[c.a]


def c_view(c):
    return {'dense': (c.N, 0), 'pad': (c.N + 10, 4)}[c.c]


def case_id(c):
    act = '' if c.act is None else f'-{nn_ref.ACT_NAMES[c.act]}{"" if c.done else ".nodone"}'
    return f'{c.tag}-M{c.M}K{c.K}N{c.N}-{c.order}-{c.a}.{c.c}{c.b}-b{c.bias}c{c.acc}w{c.ws}{act}'


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
CASES = []
# tile kernel: every (NT, WR) x BT x VEC at every N edge; the row and K edges one per case in rotation; VEC off each way in rotation
VEC_OFF = ('oddk', 'oddld', 'oddoff', 'p4')
i = 0
for N, (NT, gy) in N_EDGES.items():
    for bt in (0, 1):
        for vec in (0, 1):
            i += 1
            M = ROW_EDGES[(3 * i) % len(ROW_EDGES)]
            way = VEC_OFF[(i // 2) % 4]
            if vec:
                K, a = (2, 32, 64)[i % 3], ('dense', 'pad', 'p8')[(i // 3) % 3]
            elif way == 'oddk':
                K, a = (1, 3, 31, 33, 63, 65)[(i // 8) % 6 if N not in (32, 129) else (i // 8 + 3) % 6], 'dense'
            else:
                K, a = K_EDGES[(2 * i) % 9], way
            if bt and K == 1:       # (W^T with K = 1 is W: sbn = 1)
                K = 3
            CASES.append(mk(M, K, N, order='wt' if bt else 'w', a=a, c=('dense', 'pad')[i % 2], bias=int(i % 3 != 0), acc=int(i % 4 == 1), ws=int(i % 5 == 0),
                            tag='tile', kernel=TILE, NT=NT, WR=2 if NT % 2 == 0 else 4, BT=bt, VEC=vec, gy=gy, gx=cdiv(M, 64 if NT % 2 == 0 else 128), gz=1))
# the K edges a rotation can miss, on both tile heights, VEC on and off
for j, K in enumerate(K_EDGES):
    CASES.append(mk(ROW_EDGES[j % 7], K, (64, 96)[j % 2], order=('w', 'wt')[j % 2], c='pad', acc=j % 2, tag='tilek', kernel=TILE, VEC=int(K % 2 == 0)))
    CASES.append(mk(ROW_EDGES[(j + 3) % 7], K, (32, 128)[j % 2], order=('wt', 'w')[j % 2] if K > 1 else 'w', a='oddoff', tag='tilek', kernel=TILE, VEC=0))
# row-stacked kernel: 96-row tiles end in a partial tile at 2048 / 2049 and exactly at 2144; 2 .. 8 slices with a 4- or 8-wide tail
RT_M, RT_N = (2048, 2049, 2143, 2144), (132, 232)
for j, K in enumerate((64, 68, 96, 100, 128, 160, 232)):
    for o, order in enumerate(('w', 'wt')):
        i = 2 * j + o
        CASES.append(mk(RT_M[i % 4], K, RT_N[(j + o) % 2], order=order, a=('dense', 'pad4')[i % 2], c='pad', bias=int(i % 3 != 0), acc=int(i % 3 == 1), tag='rt',
                        kernel=RT, NT=3, BT=o, a16=1, b16=1, gx=cdiv(RT_M[i % 4], 96), gy=2))
CASES.append(mk(2049, 100, 129, order='wt', c='pad', tag='rt', kernel=RT, gy=2))
CASES.append(mk(2144, 64, 129, order='wt', a='pad4', acc=1, tag='rt', kernel=RT, gy=2))
# ... and back to the tile kernel: offset 2, a B pointer = 8 mod 16, a pointer = 8 mod 16, N % 4 != 0 forward, M below 2048
CASES.append(mk(2048, 128, 132, a='pad', c='pad', tag='rtfall', kernel=TILE, a16=0, b16=1, NT=3, WR=4))
CASES.append(mk(2049, 100, 232, order='wt', a='pad', tag='rtfall', kernel=TILE, a16=0, NT=4, WR=2))
CASES.append(mk(2143, 96, 232, b='b8', c='pad', acc=1, tag='rtfall', kernel=TILE, a16=1, b16=0))
CASES.append(mk(2144, 68, 132, order='wt', b='b8', tag='rtfall', kernel=TILE, a16=1, b16=0))
CASES.append(mk(2048, 64, 232, a='p8', tag='rtfall', kernel=TILE, a16=0, VEC=1))
CASES.append(mk(2049, 64, 130, tag='rtfall', kernel=TILE, a16=1, b16=0))
CASES.append(mk(2047, 64, 132, tag='rtfall', kernel=TILE, a16=1, b16=1))
# split-K: the eight instantiations, the chunk tails, the engine shapes, the grid-stride loop of the reduce (M N > 2048 * 256)
CASES.append(mk(1, 256, 33, ws=1, tag='splitk', kernel=SPLITK, NT=2, BT=0, VEC=1, gz=8, kchunk=32, ws_elems=8 * 33, reduce_grid=1))
CASES.append(mk(65, 257, 128, ws=1, bias=0, tag='splitk', kernel=SPLITK, NT=4, BT=0, VEC=0, gz=5, kchunk=64))
CASES.append(mk(64, 300, 64, order='wt', ws=1, c='pad', acc=1, tag='splitk', kernel=SPLITK, NT=2, BT=1, VEC=1, gz=5, kchunk=64))
CASES.append(mk(64, 300, 64, a='oddoff', ws=1, act=nn_ref.TANH, tag='splitk', kernel=SPLITK, NT=2, BT=0, VEC=0, gz=5, kchunk=64))
CASES.append(mk(1, 256, 33, order='wt', a='p4', ws=1, bias=0, act=nn_ref.NONE, tag='splitk', kernel=SPLITK, NT=2, BT=1, VEC=0, gz=8))
CASES.append(mk(65, 257, 128, order='wt', ws=1, c='pad', acc=1, act=nn_ref.SIGMOID, tag='splitk', kernel=SPLITK, NT=4, BT=1, VEC=0, gz=5))
CASES.append(mk(256, 352, 512, ws=1, tag='splitk', kernel=SPLITK, NT=4, BT=0, VEC=1))
CASES.append(mk(256, 512, 352, order='wt', ws=1, bias=0, tag='splitk', kernel=SPLITK, NT=4, BT=1, VEC=1))
CASES.append(mk(256, 512, 320, ws=1, act=nn_ref.SWISH6, tag='splitk', kernel=SPLITK, NT=4, BT=0, VEC=1, act_fused=1))
CASES.append(mk(256, 512, 320, ws=1, act=nn_ref.RELU6, done=0, tag='splitk', kernel=SPLITK, NT=4))
CASES.append(mk(256, 320, 512, order='wt', ws=1, bias=0, tag='splitk', kernel=SPLITK, NT=4, BT=1))
CASES.append(mk(1024, 768, 768, ws=1, act=nn_ref.RELU6, tag='splitk', kernel=SPLITK, NT=4, BT=0, gz=6, kchunk=128, reduce_grid=2048))
CASES.append(mk(1024, 768, 768, order='wt', ws=1, bias=0, acc=1, c='pad', tag='splitk', kernel=SPLITK, NT=4, BT=1, gz=6, reduce_grid=2048))
CASES.append(mk(2048, 256, 64, ws=1, acc=1, act=nn_ref.SWISH6, tag='splitk', kernel=SPLITK, NT=2, gz=8, kchunk=32))
# ... and its neighbours that must not split: M above 2048, K below 256, an odd tile count, no workspace; act_out then stays untouched
CASES.append(mk(2049, 256, 64, ws=1, act=nn_ref.RELU6, tag='nosplit', kernel=TILE, NT=2, WR=2, act_fused=0))
CASES.append(mk(64, 255, 64, ws=1, act=nn_ref.SWISH6, tag='nosplit', kernel=TILE, NT=2, WR=2, VEC=0))
CASES.append(mk(64, 256, 96, ws=1, act=nn_ref.TANH, tag='nosplit', kernel=TILE, NT=3, WR=4))
CASES.append(mk(64, 256, 64, ws=0, tag='nosplit', kernel=TILE, NT=2, WR=2))


def engine_products():
    """Every product add_dense and add_gru (csrc/engine.hip) send to gemm_nn at the default NetConfig for minibatch B in {1, 37, 256}:
    dicts of M, K, N, order ('w' forward, 'wt' backward-data), ws (a split-K workspace is passed: the layer allocates one when either
    direction qualifies), act (the activation the forward asks the reduce to fuse, or None), acc, dense_out.  The linear heads run in
    heads.hip, the GRU steps in rnn.hip; every output here is a dense tensor.
    The pointwise convs of the default unit plan whose planner choice is the gemm_nn fallback (plan_pw: neither the fused persistent
    kernel nor the split-precision GEMM takes them): there are NONE -- every unit conv has even K, N <= 256 with a supported tile
    mapping (asserted below from the planner's own predicates, restated), and the 464 -> 768 head conv goes to gemm_x3 (K % 4 == 0)."""
    cfg = NetConfig()
    T = cfg.T
    cat = cfg.rnn_image + 3 * cfg.rnn_small
    for u in unit_plan(cfg):            # pw_nn_supported (csrc/gemm_pw.hip) for the convs of a unit, dense even views
        convs = [(u['main_in'], u['mid']), (u['mid'], u['main_out'])] + ([(u['shortcut_c'], u['shortcut_c'])] if u['stride'] == 2 else [])
        for K, N in convs + [(N, K) for K, N in convs]:
            nt, ksm = (4 if N > 128 else cdiv(N, 32)), (16 if K <= 32 else 32 if K <= 64 else 64 if K <= 128 else 128)
            assert K <= 256 and N <= 256 and K % 2 == 0 and not (nt == 3 and ksm > 32) and not (ksm == 128 and nt != 4), (K, N)
    assert cfg.stage_channels[-1] % 4 == 0 and cfg.last_channels % 4 == 0
    for B in (1, 37, 256):
        TB = T * B

        def layer(M, K, N, act=None, need_din=True):
            ws = M <= 2048 and (K >= 256 or N >= 256)
            yield dict(M=M, K=K, N=N, order='w', ws=ws, act=act if ws else None, acc=0, dense_out=True)
            if need_din:
                yield dict(M=M, K=N, N=K, order='wt', ws=ws, act=None, acc=0, dense_out=True)
        for D in (cfg.road, cfg.vehicle, cfg.navigation):
            yield from layer(TB, D, cfg.feat_units, nn_ref.RELU6, need_din=False)
            yield from layer(TB, cfg.feat_units, cfg.feat_units, nn_ref.RELU6)
        yield from layer(TB, cfg.last_channels, 3 * cfg.rnn_image)
        yield from layer(TB, cfg.feat_units, 3 * cfg.rnn_small)
        yield from layer(B, cat, cfg.dyn_units)
        yield from layer(B, cfg.dyn_units, cfg.head_units, nn_ref.SWISH6)
        yield from layer(B, cfg.head_units, cfg.head_units, nn_ref.SWISH6)


# one small case per distinct engine product shape: M of minibatch 37 (its plan signature does not depend on the minibatch, see
# test_engine_products)
_seen = set()
for p in engine_products():
    key = (p['K'], p['N'], p['order'], p['ws'], p['act'])
    if key not in _seen and p['M'] in (37, 148):
        _seen.add(key)
        CASES.append(mk(p['M'], p['K'], p['N'], order=p['order'], ws=int(p['ws']), act=p['act'], bias=int(p['order'] == 'w'), tag='engine'))

PARAMS = [pytest.param(c, id=case_id(c)) for c in CASES]
assert len({case_id(c) for c in CASES}) == len(CASES), [x for x in [case_id(c) for c in CASES] if [case_id(c) for c in CASES].count(x) > 1]

# ---- REQUIRED: what the ladder can instantiate, written out from it ---------------------------------------------------------------
# gemm_nn_kernel<NT, BT, VEC, WR> for (NT, WR) in {(1, 4), (3, 4), (2, 2), (4, 2)} without split-K (16), (2, 2) and (4, 2) with it (8),
# gemm_nn_rt_kernel<3, BT> (2); splitk_reduce_kernel with and without act_out, with and without accumulate
REQUIRED = ({(TILE, nt, wr, bt, v) for nt, wr in ((1, 4), (3, 4), (2, 2), (4, 2)) for bt in (0, 1) for v in (0, 1)}
            | {(SPLITK, nt, 2, bt, v) for nt in (2, 4) for bt in (0, 1) for v in (0, 1)}
            | {(RT, 3, 0, bt, 0) for bt in (0, 1)})
REDUCE_REQUIRED = {(act_out, acc) for act_out in (0, 1) for acc in (0, 1)}


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def plan_of(lib, M, N, K, a_addr, a_ld, a_coff, b_addr, sbk, sbn, ws):
    va = _lib.View(a_addr, a_ld, a_coff)
    out = (C.c_int32 * len(nn_ref.PLAN_FIELDS))()
    n = lib.cdrl_gemm_nn_plan(C.byref(va), b_addr, sbk, sbn, M, N, K, int(ws), out, len(out))
    assert n == len(nn_ref.PLAN_FIELDS), (n, lib.cdrl_last_error())
    return dict(zip(nn_ref.PLAN_FIELDS, out))


def case_addresses(c, base_a=FAKE, base_b=FAKE):
    """(address of a, address of B) with the case's pointer alignment on top of 16-byte aligned bases"""
    return base_a + 4 * a_view(c)[2], base_b + (8 if c.b == 'b8' else 0)


def plan_query(lib, c, a_addr=None, b_addr=None):
    fa, fb = case_addresses(c)
    lda, ca, _ = a_view(c)
    sbk, sbn = nn_ref.b_strides(c.order, c.K, c.N)
    return plan_of(lib, c.M, c.N, c.K, a_addr or fa, lda, ca, b_addr or fb, sbk, sbn, c.ws)


def check_plan(lib, p, c, a_addr=None, b_addr=None):
    for k, v in c.expect.items():
        assert p[k] == v, (case_id(c), k, p)
    fa, fb = case_addresses(c)
    lda, ca, _ = a_view(c)
    sbk, sbn = nn_ref.b_strides(c.order, c.K, c.N)
    assert p == nn_ref.expected_plan(c.M, c.N, c.K, a_addr or fa, lda, ca, b_addr or fb, sbk, sbn, c.ws), (case_id(c), p)
    assert p['ws_elems'] <= lib.cdrl_gemm_nn_workspace_elems(c.M, c.N, c.K)
    assert (p['kernel'] == SPLITK) == (c.tag == 'splitk') or c.tag == 'engine', (case_id(c), p)


def chain(p, c):
    """(L, c) of the module docstring"""
    L = p['kchunk'] + p['gz'] if p['kernel'] == SPLITK else c.K
    return L, 2 + c.acc


def coverage_gaps(lib):
    plans = [(c, plan_query(lib, c)) for c in CASES]
    have = {nn_ref.signature(p) for c, p in plans}
    gaps = [('REQUIRED', s) for s in sorted(REQUIRED - have)] + [('unknown instantiation', s) for s in sorted(have - REQUIRED)]
    red = {(int(c.act is not None and c.done), c.acc) for c, p in plans if p['kernel'] == SPLITK}
    gaps += [('reduce', s) for s in sorted(REDUCE_REQUIRED - red)]
    gaps += [('reduce act', a) for a in range(5) if not any(p['kernel'] == SPLITK and c.act == a and c.done for c, p in plans)]
    return gaps


def test_coverage(lib):
    """The cases' plans cover REQUIRED (26 kernel instantiations) and contain nothing REQUIRED does not know; the reduce runs with and
    without act_out and accumulate and with each of the five activations; every edge the issue names is present on its kernel."""
    gaps = coverage_gaps(lib)
    assert not gaps, gaps
    assert len(REQUIRED) == 26
    plans = [(c, plan_query(lib, c)) for c in CASES]
    tile = [(c, p) for c, p in plans if p['kernel'] == TILE and c.M < 2047]
    for nt_wr in ((1, 4), (3, 4), (2, 2), (4, 2)):
        assert set(ROW_EDGES) <= {c.M for c, p in tile if (p['NT'], p['WR']) == nt_wr}, nt_wr
    assert set(K_EDGES) <= {c.K for c, p in tile if p['WR'] == 2} and set(K_EDGES) <= {c.K for c, p in tile if p['WR'] == 4}
    assert set(N_EDGES) <= {c.N for c, p in tile}
    off = [c for c, p in tile if not p['VEC']]
    assert any(c.K % 2 for c in off) and {'oddld', 'oddoff', 'p4'} <= {c.a for c in off}
    rt = [c for c, p in plans if p['kernel'] == RT]
    assert {c.M for c in rt} == set(RT_M) and {c.K for c in rt} == {64, 68, 96, 100, 128, 160, 232} and {c.N for c in rt} == {129, 132, 232}
    assert {(c.order, c.acc) for c in rt} == {('w', 0), ('w', 1), ('wt', 0), ('wt', 1)} and all(c.order == 'wt' for c in rt if c.N == 129)
    assert sum(c.tag == 'rtfall' for c, p in plans if p['kernel'] == TILE) >= 4
    sk = {(c.M, c.K, c.N) for c, p in plans if p['kernel'] == SPLITK}
    assert {(1, 256, 33), (65, 257, 128), (64, 300, 64), (256, 352, 512), (256, 512, 320), (1024, 768, 768), (2048, 256, 64)} <= sk
    assert {c.order for c, p in plans if (c.M, c.K, c.N) == (1024, 768, 768)} == {'w', 'wt'}
    assert not {(2049, 256, 64), (64, 255, 64), (64, 256, 96)} & sk
    assert any(c.act is not None and not c.done and p['kernel'] == SPLITK for c, p in plans)
    assert any(c.act is not None and c.ws and p['kernel'] != SPLITK for c, p in plans)


def engine_matches(lib):
    """(product, matching cases) for every engine product: same plan signature, same K, N, B order"""
    sigs = {}
    for c in CASES:
        sigs.setdefault((nn_ref.signature(plan_query(lib, c)), c.K, c.N, c.order), []).append(c)
    out = []
    for p in engine_products():
        sbk, sbn = nn_ref.b_strides(p['order'], p['K'], p['N'])
        plan = plan_of(lib, p['M'], p['N'], p['K'], FAKE, p['K'], 0, FAKE, sbk, sbn, p['ws'])
        out.append((p, plan, sigs.get((nn_ref.signature(plan), p['K'], p['N'], p['order']), [])))
    return out


def test_engine_products(lib):
    """every product of the engine that reaches gemm_nn has a case with its plan signature, K, N and B order (test_variant runs them);
    a product whose forward fuses an activation has a case that fuses the same one"""
    ms = engine_matches(lib)
    assert len(ms) == 3 * 19
    for p, plan, cases in ms:
        assert cases, (p, plan)
        if p['act'] is not None and plan['kernel'] == SPLITK:
            assert any(c.act == p['act'] and c.done for c in cases), p
    print('\n' + '\n'.join(f"{p}: {nn_ref.signature(plan)} gz {plan['gz']} kchunk {plan['kchunk']}" for p, plan, _ in ms if p['M'] in (256, 1024)))


# ---- guarded tensors ---------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


class Banded:
    """A 1-D tensor inside a larger one, with a band of `fill` on each side that must come back bit-intact.  shift: elements the
    payload starts past a 256-byte boundary."""

    def __init__(self, n, dtype, fill, band=256, value=None, shift=0):
        self.whole = torch.full((band + shift + n + band,), fill, dtype=dtype, device=DEV)
        self.t = self.whole[band + shift:band + shift + n]
        if value is not None:
            self.t.copy_(value)
        self.lo, self.hi = self.whole[:band + shift], self.whole[band + shift + n:]
        self.ref_lo, self.ref_hi = self.lo.clone(), self.hi.clone()

    def intact(self):
        return torch.equal(bits(self.lo), bits(self.ref_lo)) and torch.equal(bits(self.hi), bits(self.ref_hi))


def framed(M, ld, coff, payload, shift=0, fill=float('nan')):
    """(device tensor, address of row 0 of the view, host copy): the payload at columns [coff, coff + cols) of rows GR .. GR + M of a
    `fill` tensor [GR + M + GR][ld]; the view's row 0 starts `shift` floats past a 16-byte boundary"""
    cols = payload.shape[1]
    assert coff >= 0 and coff + cols <= ld
    pre = (-(GR * ld) % 4 + shift) % 4
    host = np.full(pre + (GR + M + GR) * ld + 4, fill, np.float32)
    body = host[pre:pre + (GR + M + GR) * ld].reshape(GR + M + GR, ld)
    body[GR:GR + M, coff:coff + cols] = payload
    t = torch.as_tensor(host).to(DEV)
    addr = t.data_ptr() + 4 * (pre + GR * ld)
    assert t.data_ptr() % 16 == 0 and addr % 16 == 4 * shift
    return t, addr, host


def sync():
    """A device fault ends the run: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device fault, stopping: {e}', returncode=3)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


WORST = {}          # (kernel name, check) -> (worst error / bound, case), printed by test_report
REPORT = []


def run_case(lib, c, exact):
    M, K, N = c.M, c.K, c.N
    inp = nn_ref.draw([11, M, K, N, len(c.a), len(c.order), c.acc, int(exact)], M, K, N, c.bias, c.acc, exact)
    if exact:
        assert nn_ref.exact_condition(inp), case_id(c)
    ref, Smag = nn_ref.product(inp.A, inp.B, inp.bias, inp.base)
    lda, ca, shift = a_view(c)
    ldc, cc = c_view(c)
    sbk, sbn = nn_ref.b_strides(c.order, K, N)
    ta, pa, _ = framed(M, lda, ca, inp.A, shift)
    tb = Banded(K * N, torch.float32, float('nan'), value=dev(nn_ref.b_flat(inp.B, c.order)), shift=2 if c.b == 'b8' else 0)
    assert tb.t.data_ptr() % 16 == (8 if c.b == 'b8' else 0)
    tbias = Banded(N, torch.float32, float('nan'), value=dev(inp.bias)) if c.bias else None
    p = plan_of(lib, M, N, K, pa, lda, ca, tb.t.data_ptr(), sbk, sbn, c.ws)
    check_plan(lib, p, c, pa, tb.t.data_ptr())
    assert p == plan_query(lib, c), 'the plan depends on more than the alignment of the addresses'
    nws = int(lib.cdrl_gemm_nn_workspace_elems(M, N, K))
    ws = Banded(max(nws, 16), torch.float32, float('nan'), band=4096) if c.ws else None
    payload = inp.base if c.acc else np.full((M, N), SENTINEL, np.float32)
    va = _lib.View(pa, lda, ca)
    mask = np.zeros((GR + M + GR, ldc), bool)
    mask[GR:GR + M, cc:cc + N] = True

    def launch(act_out):
        tc, pc, host = framed(M, ldc, cc, payload, fill=SENTINEL)
        vc = _lib.View(pc, ldc, cc)
        ao = Banded(M * N, torch.float32, SENTINEL) if act_out else None
        done = C.c_int(-7)
        _lib.check(lib.cdrl_gemm_nn_ex(C.byref(va), P(tb.t), sbk, sbn, P(tbias.t) if c.bias else None, C.byref(vc), M, N, K, c.acc, P(ws.t) if c.ws else None,
                                       P(ao.t) if act_out else None, c.act or 0, C.byref(done) if (c.done and act_out) else None, S()), case_id(c))
        sync()
        got = tc.cpu().numpy()
        body = got[len(got) - 4 - (GR + M + GR) * ldc:len(got) - 4].reshape(GR + M + GR, ldc)
        hbody = host[len(host) - 4 - (GR + M + GR) * ldc:len(host) - 4].reshape(GR + M + GR, ldc)
        assert np.array_equal(body[~mask].view(np.int32), hbody[~mask].view(np.int32)) and np.array_equal(got[:len(got) - 4 - mask.size].view(np.int32),
                                                                                                          host[:len(host) - 4 - mask.size].view(np.int32)), 'wrote outside the view c'
        assert tb.intact() and (ws is None or ws.intact()) and (ao is None or ao.intact()) and (tbias is None or tbias.intact()), 'wrote outside a buffer'
        return body[GR:GR + M, cc:cc + N].copy(), ao, done.value

    with_act = c.act is not None
    got, ao, done = launch(with_act)
    assert np.isfinite(got).all() and not (got == SENTINEL).any(), 'an output element was poisoned or never written'
    again, ao2, _ = launch(with_act)
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), 'not reproducible on the dirty workspace'
    if c.ws and p['kernel'] != SPLITK:
        assert bool(torch.isnan(ws.t).all()), 'the workspace was written without split-K'
    name = ('tile', 'row-stacked', 'split-K')[p['kernel']]
    if exact:
        bad = int((got.astype(np.float64) != ref).sum())
        assert bad == 0, f'{case_id(c)}: {bad} of {got.size} elements differ from the exact value (worst {np.abs(got - ref).max():.3e})'
        err_txt = 'exact'
    else:
        L, cnt = chain(p, c)
        bound = (L + cnt) * U24 * Smag
        frac = np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)
        worst = float(frac.max())
        assert worst <= 1.0, f'{case_id(c)}: element {np.unravel_index(np.argmax(frac), frac.shape)} is {worst:.3f} of its bound'
        if worst > WORST.get(name, (0.0, ''))[0]:
            WORST[name] = (worst, case_id(c))
        err_txt = f'{worst:.4f} of the bound, {float(np.abs(got - ref).max() / np.abs(ref).max()):.2e} of the tensor maximum'
    REPORT.append(f"{case_id(c)}: {nn_ref.signature(p)} grid {p['gx']}x{p['gy']}x{p['gz']} kchunk {p['kchunk']}: {err_txt}")
    if not with_act:
        return
    fused = bool(c.done and p['kernel'] == SPLITK)
    assert done == (int(fused) if c.done else -7), (case_id(c), done)
    if not fused:
        assert bool((ao.t == SENTINEL).all()) and bool((ao2.t == SENTINEL).all()), 'act_out was written although the call did not report it'
        return
    z = dev(got)
    want = Banded(M * N, torch.float32, SENTINEL)
    _lib.check(lib.cdrl_act_fwd(P(z), P(want.t), M * N, c.act, S()))
    sync()
    assert want.intact() and torch.equal(bits(ao.t), bits(want.t)) and torch.equal(bits(ao2.t), bits(want.t)), 'act_out differs from cdrl_act_fwd of the c the call wrote'
    plain, _, _ = launch(False)
    assert np.array_equal(plain.view(np.int32), got.view(np.int32)), 'c depends on whether act_out is given'
    a64 = nn_ref.act_fwd(got.astype(np.float64), c.act)
    assert float(nn_ref.units(want.t.cpu().numpy(), a64.reshape(-1), TINY['value']).max()) <= 4 * max([1.0] + [v for (a, q), v in MEASURED.items() if q == 'value'])


@pytest.mark.parametrize('c', PARAMS)
def test_variant(lib, c):
    run_case(lib, c, True)
    run_case(lib, c, False)


def test_refusals(lib):
    """what cdrl_gemm_nn_ex refuses is refused through its return code and cdrl_last_error, before any launch"""
    t = torch.zeros(64 * 64, device=DEV)
    v, bad_a, bad_c = _lib.View(t.data_ptr(), 64, 0), _lib.View(t.data_ptr(), 64, 1), _lib.View(t.data_ptr(), 63, 0)
    ex = lambda a, c, ws, ao, act: lib.cdrl_gemm_nn_ex(C.byref(a), P(t), 64, 1, None, C.byref(c), 64, 64, 64, 0, ws, ao, act, None, S())      # noqa: E731
    assert ex(bad_a, v, None, None, 0) == -1 and b'fit' in lib.cdrl_last_error()
    assert ex(v, bad_c, None, None, 0) == -1 and b'fit' in lib.cdrl_last_error()
    assert ex(v, v, None, P(t), 1) == -1 and b'workspace' in lib.cdrl_last_error()
    assert ex(v, v, None, None, 5) == -1 and ex(v, v, None, None, -1) == -1 and b'activation' in lib.cdrl_last_error()
    sync()
    assert bool((t == 0).all())


# ---- activations on their own ------------------------------------------------------------------------------------------------------
ACT_WORST = {}


@pytest.fixture(scope='module')
def act_reference():
    """inputs and float64 references of the largest activation case, computed once"""
    n = 2048 * 256 + 1
    x = nn_ref.act_inputs(n)
    da = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    da[da == 0] = 1.0
    x64 = x.astype(np.float64)
    return x, da, {a: (nn_ref.act_fwd(x64, a), nn_ref.act_deriv(x64, a)) for a in range(5)}


@pytest.mark.parametrize('n', (1, 255, 256, 257, 2048 * 256 + 1))
def test_activations(lib, act_reference, n):
    """forward and backward of the five activations (the last n runs the grid-stride loop); the inputs are a prefix-independent draw
    for the small n and the shared large one otherwise"""
    if n == 2048 * 256 + 1:
        x, da, refs = act_reference
    else:
        x = nn_ref.act_inputs(n)
        da = np.random.default_rng(n).standard_normal(n).astype(np.float32) + np.float32(3.0)
        refs = {a: (nn_ref.act_fwd(x.astype(np.float64), a), nn_ref.act_deriv(x.astype(np.float64), a)) for a in range(5)}
    xz, xd = Banded(n, torch.float32, float('nan'), value=dev(x)), Banded(n, torch.float32, float('nan'), value=dev(da))
    problems = []           # every figure is printed before anything about the measured quantities is asserted
    for act in range(5):
        out, dz = Banded(n, torch.float32, SENTINEL), Banded(n, torch.float32, SENTINEL)
        _lib.check(lib.cdrl_act_fwd(P(xz.t), P(out.t), n, act, S()))
        _lib.check(lib.cdrl_act_bwd(P(xz.t), P(xd.t), P(dz.t), n, act, S()))
        sync()
        assert out.intact() and dz.intact() and xz.intact() and xd.intact()
        v, g = out.t.cpu().numpy(), dz.t.cpu().numpy()
        val, der = refs[act]
        name = nn_ref.ACT_NAMES[act]
        if act in (nn_ref.NONE, nn_ref.RELU6):
            assert np.array_equal(v.view(np.int32), val.astype(np.float32).view(np.int32)) or np.array_equal(v, val.astype(np.float32)), name
            want = np.where(der != 0, da, np.float32(0.0)).astype(np.float32)
            assert np.array_equal(g, want), (name, int((g != want).sum()))
            continue
        if act == nn_ref.SWISH6:
            # the gate, where the derivative cannot underflow (x > 0; the clamp sits at x* = 6.0147): closed <=> the gradient is 0
            pos = x > 0
            closed, want_closed = (g == 0)[pos], ~nn_ref.swish6_open(x.astype(np.float64))[pos]
            if not np.array_equal(closed, want_closed):
                problems.append((name, 'gate', [repr(float(t)) for t in x[pos][closed != want_closed][:8]]))
        uv = nn_ref.units(v, val, TINY['value'])
        # dz = da act'(z): the error of the derivative in its units, times |da| (the product with da is one more rounding, measured along)
        ud = np.abs(g.astype(np.float64) - der * da.astype(np.float64)) / (U24 * np.maximum(np.abs(der), TINY['deriv']) * np.abs(da.astype(np.float64)))
        for q, u in (('value', uv), ('deriv', ud)):
            w = float(u.max())
            if w > ACT_WORST.get((name, q), (0.0, 0.0))[0]:
                ACT_WORST[(name, q)] = (w, float(x[int(np.argmax(u))]))
            print(f'n {n} {name} {q}: worst {w:.3f} units at x = {float(x[int(np.argmax(u))])!r}')
            if not w <= 4 * MEASURED[(name, q)]:
                problems.append((name, q, w, float(x[int(np.argmax(u))])))
    assert not problems, problems


# ---- the bias-gradient path -------------------------------------------------------------------------------------------------------
COLSUM_ROWS = (1, 2, 255, 256, 257, 1024)


@pytest.mark.parametrize('Cn', (1, 2, 5, 16, 96, 320, 512, 768, 1028))
def test_colsum_then_reduce(lib, Cn):
    """column sums of integer-valued rows through dense, padded and alignment-breaking views, folded by cdrl_reduce_partials"""
    vec, cx, cy, nloop, _, _ = nn_ref.vcol_geom(1024, Cn)
    assert (vec, nloop) == {1: (1, 1), 2: (2, 1), 5: (1, 1), 16: (4, 1), 96: (4, 1), 320: (4, 1), 512: (4, 1), 768: (4, 1), 1028: (4, 2)}[Cn]
    for j, rows in enumerate(COLSUM_ROWS):
        rng = np.random.default_rng([Cn, rows])
        x = rng.integers(-4095, 4096, (rows, Cn)).astype(np.float32)
        ld, coff, shift = ((Cn, 0, 0), (Cn + 8, 4, 0), (Cn + 7, 1, 0), (Cn + 8, 0, 1), (Cn + 6, 2, 0), (Cn + 8, 4, 2))[(j + Cn) % 6]
        tx, px, _ = framed(rows, ld, coff, x, shift)
        nb = lib.cdrl_colsum_partial_rows(rows, Cn)
        assert nb == nn_ref.vcol_geom(rows, Cn)[5]
        part = Banded(nb * Cn, torch.float64, float('nan'))
        vx = _lib.View(px, ld, coff)
        _lib.check(lib.cdrl_colsum(C.byref(vx), rows, Cn, P(part.t), S()))
        acc = j % 2
        base = rng.integers(-1000, 1000, Cn).astype(np.float32) if acc else None
        out = Banded(Cn, torch.float32, SENTINEL, value=dev(base) if acc else None)
        _lib.check(lib.cdrl_reduce_partials(P(part.t), nb, Cn, 0, Cn, P(out.t), None, acc, S()))
        sync()
        assert part.intact() and out.intact()
        exact = x.astype(np.float64).sum(axis=0)
        assert np.array_equal(part.t.cpu().numpy().reshape(nb, Cn).sum(axis=0), exact), (rows, 'partials')
        want = nn_ref.f32_sum(x, base)
        assert np.array_equal(out.t.cpu().numpy().view(np.int32), want.view(np.int32)), (rows, ld, coff, shift)


@pytest.mark.parametrize('nparts', (1, 63, 64, 65, 511, 512, 513, 1025))
def test_reduce_partials(lib, nparts):
    """the double-partials reduce on its own: both CX forms (asserted through the query), one and two outputs with the boundary inside a
    block, rows longer than n, with and without accumulate"""
    for j, (n1, n2, stride) in enumerate(((37, 0, 37), (19, 18, 41), (2053, 0, 2053), (2043, 10, 2060), (1, 0, 3), (3, 1, 4))):
        n = n1 + n2
        cxw = 16 if (cdiv(n, 16) >= 128 or nparts <= 64) else 4
        assert lib.cdrl_reduce_partials_cx(nparts, n1, n2) == cxw == nn_ref.reduce_cx(nparts, n)
        rng = np.random.default_rng([nparts, n1, n2])
        host = rng.integers(-(1 << 20), 1 << 20, (nparts, stride)).astype(np.float64)
        buf = host.copy()
        buf[:, n:] = np.nan
        part = Banded(nparts * stride, torch.float64, float('nan'), value=dev(buf.reshape(-1), torch.float64))
        acc = (j + nparts) % 2
        b1 = rng.integers(-1000, 1000, n1).astype(np.float32) if acc else None
        b2 = rng.integers(-1000, 1000, max(n2, 1)).astype(np.float32) if acc else None
        o1 = Banded(n1, torch.float32, SENTINEL, value=dev(b1) if acc else None)
        o2 = Banded(max(n2, 1), torch.float32, SENTINEL, value=dev(b2) if acc else None)
        start2 = o2.t.clone()
        _lib.check(lib.cdrl_reduce_partials(P(part.t), nparts, n1, n2, stride, P(o1.t), P(o2.t) if n2 else None, acc, S()))
        sync()
        assert part.intact() and o1.intact() and o2.intact()
        assert np.array_equal(o1.t.cpu().numpy().view(np.int32), nn_ref.f32_sum(host[:, :n1], b1).view(np.int32)), (n1, n2, stride, 'out1')
        if n2:
            assert np.array_equal(o2.t.cpu().numpy().view(np.int32), nn_ref.f32_sum(host[:, n1:n], b2).view(np.int32)), (n1, n2, stride, 'out2')
        else:
            assert torch.equal(bits(o2.t), bits(start2))
    assert lib.cdrl_reduce_partials(None, 4, 4, 0, 4, None, None, 0, S()) == -1 and lib.cdrl_last_error()


@pytest.mark.parametrize('B,T,D', ((1, 1, 1), (3, 4, 9), (37, 4, 5), (256, 4, 4)))
def test_permute_bt(lib, B, T, D):
    x = np.random.default_rng([B, T, D]).standard_normal(B * T * D).astype(np.float32)
    src = Banded(B * T * D, torch.float32, float('nan'), value=dev(x))
    dst = Banded(B * T * D, torch.float32, SENTINEL)
    _lib.check(lib.cdrl_permute_bt(P(src.t), P(dst.t), B, T, D, S()))
    sync()
    assert src.intact() and dst.intact()
    assert np.array_equal(dst.t.cpu().numpy().view(np.int32), nn_ref.permute_bt(x, B, T, D).view(np.int32))


def test_report():
    """Prints what the cases observed (run the module with -s): plan signature and error per case, the worst Gaussian figure per kernel as a
    fraction of its bound, the measured activation errors."""
    print('\n' + '\n'.join(REPORT))
    for name, (frac, cid) in sorted(WORST.items()):
        print(f'worst {name}: {frac:.4f} of its bound ({cid})')
    for (name, q), (w, x) in sorted(ACT_WORST.items()):
        print(f'activation {name} {q}: {w:.3f} units at x = {x!r} (asserted at {4 * MEASURED[(name, q)]:.1f})')
    assert all(frac <= 1.0 for frac, _ in WORST.values())
