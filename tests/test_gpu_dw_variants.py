"""Fused depthwise block (cdrl_dwconv_bn_fwd / _bwd, csrc/dwfused.hip): every kernel variant its host planner can dispatch, at op
level, against the float64 autograd reference (float32 tensors) or the exact storage contract (bf16 tensors) of tests/dw_ref.py.

The planner picks the instantiation and the loop structure from (G, B, H, W, C, stride) alone, so each case first reads the plan
(cdrl_dwconv_bn_plan -- the struct the launchers dispatch on) and asserts the variant it is there for; `test_coverage` then holds
the union of the cases' variant signatures against REQUIRED, the hand-written list of what the launch ladders of dwf_fwd / dwf_bwd
can select, and against the depthwise layers of the engine's configurations.

Nothing here can pass by luck: workspaces start as NaN, outputs as a sentinel, y / dx / the workspace sit between sentinel bands that
must come back bit-intact, and every backward runs a second time on the dirty workspace and must reproduce itself bit for bit
(fixed-order sums, no atomics).

ReLU6 decisions: with up to 1e7 elements per case a handful of pre-BN outputs lie within float32 rounding of a kink, where kernel and
float64 reference legitimately take different branches (an O(1) difference in that element's gradient).  As in the engine-level
tests (tests/util.py::engine_decisions) the reference is evaluated on the regions of z = fmaf(scale, x, shift) of the float32
statistics block the kernels read -- the expression they evaluate -- and is then a smooth function of its inputs.

CDRL_DWS=0 (read once per process) sends every shape to the pixel-mapped backward: `test_pixel_mapped_everywhere` runs the
float32 cases of this module again in a child process with it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from oracle.spec import NetConfig, unit_plan
from tests import dw_ref
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
DWS_OFF = os.environ.get('CDRL_DWS', '').strip() not in ('',) and int(os.environ['CDRL_DWS']) == 0
SENTINEL = -2.0 ** 100          # exact in float32 and bf16; no kernel output comes near it

PLAN_FIELDS = ('vec', 'nch', 'cchunk', 'cy', 'fpb', 'nb', 'vec_bwd', 'fpb_bwd', 'nb_bwd', 'form', 'sw', 'R', 'F', 'snch', 'scy', 'pl',
               'lds_bwd_over', 'lds_fwd_over', 'cx', 'cx_bwd', 'cy_bwd', 'scx')


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def plan(lib, G, B, H, W, Cc, stride):
    out = (C.c_int32 * len(PLAN_FIELDS))()
    n = lib.cdrl_dwconv_bn_plan(G, B, H, W, Cc, stride, out, len(PLAN_FIELDS))
    _lib.check(0 if n == len(PLAN_FIELDS) else -1, 'cdrl_dwconv_bn_plan')
    return dict(zip(PLAN_FIELDS, out))


def fwd_sig(p, stride, pre, dt):
    """forward variant: (stride, VEC, several channel chunks, frame loop, PRE, tensor type) -- dwf_fwd_kernel<stride, VEC, PRE, T>"""
    return (stride, p['vec'], p['nch'] > 1, p['fpb'] > 1, int(bool(pre)), dt)


def bwd_sig(p, stride, pre, dt):
    """backward variant: (form, stride, SW | VEC, R, PL, F > 1, frame loop, several channel chunks, PRE, tensor type) --
    form 1: dws_bwd_kernel<SW, R, PRE, T>, form 2: dws2_bwd_kernel<PL, PRE, T>, form 0: dwf_bwd_kernel<stride, VEC, PRE, T>"""
    if p['form'] == 0:
        return (0, stride, p['vec_bwd'], 0, 0, False, p['fpb_bwd'] > 1, p['nch'] > 1, int(bool(pre)), dt)
    return (p['form'], stride, p['sw'], p['R'], p['pl'] if p['form'] == 2 else 0, p['F'] > 1, p['fpb_bwd'] > 1, p['snch'] > 1,
            int(bool(pre)), dt)


# ---- the cases: (G, B, H, W, C, stride), the (pre, tensor type) combinations it runs with, the plan it is there for ---------------
ALL4 = ((1, 'f32'), (0, 'f32'), (1, 'bf16'), (0, 'bf16'))
CASES = [
    # forward and backward frame loops: the loop structure of the 90x120 workload (B = 256: fpb 2 | 4 | 8, fpb_bwd 2 | 4)
    ((4, 256, 3, 4, 232, 1), ((1, 'f32'), (1, 'bf16')), dict(fpb=4, fpb_bwd=2, form=1, sw=4, R=1, F=1)),
    ((4, 128, 6, 8, 116, 1), ((1, 'f32'), (1, 'bf16')), dict(fpb=2, fpb_bwd=2, form=1, sw=8, R=1, F=1, scx=58, scy=6)),
    ((4, 128, 11, 15, 58, 1), ((1, 'f32'), (1, 'bf16')), dict(fpb=2, fpb_bwd=2, form=1, sw=8, R=1, F=1, scx=29, scy=22, nch=3)),
    ((4, 128, 6, 8, 232, 2), ALL4, dict(fpb=2, fpb_bwd=2, form=2, pl=0, F=1)),
    ((4, 128, 11, 15, 116, 2), ALL4, dict(fpb=4, fpb_bwd=2, form=2, pl=1, F=1)),                # 9.8 M input elements: the largest
    ((4, 128, 11, 15, 58, 2), ((1, 'f32'), (1, 'bf16')), dict(vec=2, nch=2, fpb=2, form=2)),     # forward <2, 2> with chunks AND a frame loop
    ((2, 3, 11, 15, 58, 1), ((1, 'f32'),), dict(vec=2, nch=3, fpb=1, fpb_bwd=1, form=1, sw=8, scx=29, scy=22)),      # odd B: no loop
    # frames sharing one tile batch
    ((4, 512, 3, 4, 24, 1), ((1, 'f32'), (0, 'f32'), (1, 'bf16')), dict(form=1, sw=4, R=1, F=4, fpb_bwd=4)),
    ((8, 1024, 3, 4, 24, 1), ((1, 'f32'),), dict(form=1, sw=4, R=1, F=8, fpb=8, fpb_bwd=8)),
    ((4, 128, 5, 7, 58, 1), ((1, 'f32'), (0, 'bf16')), dict(form=1, sw=8, R=1, F=2)),
    ((4, 128, 5, 7, 58, 2), ALL4, dict(form=2, pl=1, F=2)),
    ((4, 512, 4, 6, 24, 2), ((0, 'f32'), (1, 'f32'), (0, 'bf16')), dict(form=2, pl=0, F=8)),
    # strips of 4 pixels with 2 and 3 strips per thread
    ((4, 2, 4, 4, 232, 1), ALL4, dict(form=1, sw=4, R=2)),
    ((4, 2, 5, 3, 232, 1), ((1, 'f32'),), dict(form=1, sw=4, R=2, scy=3)),                       # 5 strips on 3 lanes: partial second strip
    ((4, 2, 7, 4, 232, 1), ALL4, dict(form=1, sw=4, R=3)),
    ((2, 256, 7, 4, 116, 1), ((1, 'f32'),), dict(form=1, sw=4, R=2, fpb_bwd=2)),                 # ... inside a frame loop
    # every strip instantiation without loops, both PRE, both tensor types
    ((2, 3, 5, 7, 58, 1), ALL4, dict(form=1, sw=8, R=1, F=1, fpb_bwd=1, snch=1)),
    ((2, 3, 3, 4, 58, 1), ALL4, dict(form=1, sw=4, R=1, F=1, fpb_bwd=1, snch=1)),
    ((2, 3, 6, 8, 58, 2), ALL4, dict(form=2, pl=0, F=1, fpb_bwd=1, snch=1)),
    ((2, 3, 5, 7, 116, 2), ALL4, dict(form=2, pl=1, F=1, fpb_bwd=1, snch=1)),
    # pixel-mapped backward: odd C (VEC = 1 forward and backward), and even C when no strip plan fits LDS
    ((2, 3, 5, 7, 29, 1), ALL4, dict(form=0, vec=1, vec_bwd=1)),
    ((2, 3, 5, 7, 29, 2), ALL4, dict(form=0, vec=1, vec_bwd=1)),
    ((2, 512, 3, 4, 29, 1), ((1, 'f32'),), dict(form=0, vec=1, vec_bwd=1, fpb=2, fpb_bwd=2)),    # its frame loop
    ((2, 2, 45, 61, 24, 1), ALL4, dict(form=0, vec_bwd=2, nch=6, lds_bwd_over=0)),
    ((2, 2, 73, 98, 24, 2), ALL4, dict(form=0, vec_bwd=2, nch=6, lds_bwd_over=0)),               # (74x100: refused)
    # strip forms with channel chunks; with a frame loop on top: the wide frames of the 90x360 configuration at B = 64
    ((2, 2, 44, 60, 24, 2), ((0, 'f32'),), dict(form=2, pl=0, snch=2, fpb_bwd=1)),
    ((4, 64, 3, 12, 232, 1), ((1, 'f32'),), dict(form=1, sw=8, R=1, snch=2, fpb_bwd=2)),
    ((2, 128, 4, 26, 232, 2), ((1, 'f32'), (0, 'f32')), dict(form=2, pl=0, snch=2, fpb_bwd=2)),
    ((2, 128, 5, 23, 232, 2), ((1, 'f32'), (0, 'f32')), dict(form=2, pl=1, snch=2, fpb_bwd=2)),
]
BWD_ONLY_FIELDS = ('fpb_bwd', 'form', 'sw', 'R', 'F', 'snch', 'scx', 'scy')


def case_id(shape, pre, dt):
    return f"{dt}-{'x'.join(map(str, shape[:5]))}s{shape[5]}p{pre}"


PARAMS = [pytest.param(shape, pre, expect, id=case_id(shape, pre, dt)) for shape, combos, expect in CASES for pre, dt in combos if dt == 'f32']
PARAMS_BF16 = [pytest.param(shape, pre, expect, id=case_id(shape, pre, dt)) for shape, combos, expect in CASES for pre, dt in combos
               if dt == 'bf16']


def check_plan(lib, shape, expect):
    p = plan(lib, *shape)
    for k, v in expect.items():
        if DWS_OFF and k in BWD_ONLY_FIELDS:
            continue
        assert p[k] == v, (shape, k, p)
    if DWS_OFF:
        assert p['form'] == 0 and p['fpb_bwd'] == p['fpb'] and p['nb_bwd'] == p['nb'], (shape, p)
    assert not p['lds_fwd_over'] and not (p['form'] == 0 and p['lds_bwd_over']), (shape, p)
    return p


# ---- REQUIRED: what the launch ladders of dwf_fwd / dwf_bwd (csrc/dwfused.hip) can select, written out from them ------------------
TYPES = ('f32', 'bf16')
# dwf_fwd: stride 1 | 2, g.vec 4 | 2 | 1, pre_stats or not, float | bf16_t; with one or several channel chunks and with or without the
# frame loop where the planner produces them (VEC = 1 needs an odd C: several chunks only for frames no case needs)
REQUIRED_FWD = (
    {(s, v, False, False, pre, dt) for s in (1, 2) for v in (1, 2) for pre in (0, 1) for dt in TYPES}
    | {(s, 4, True, False, pre, dt) for s in (1, 2) for pre in (0, 1) for dt in TYPES}
    | {(1, 4, True, True, 1, dt) for dt in TYPES} | {(1, 2, True, True, 1, dt) for dt in TYPES}           # the workloads' loops
    | {(2, 4, True, True, pre, dt) for pre in (0, 1) for dt in TYPES} | {(2, 2, True, True, 1, dt) for dt in TYPES}
    | {(1, 2, True, False, 1, 'f32'), (1, 4, False, True, 1, 'f32'), (2, 4, False, True, 0, 'f32'), (1, 1, False, True, 1, 'f32')})
NOLOOP = (False, False, False)
REQUIRED_BWD = (
    # dws_bwd_kernel<SW, R, PRE, T>: d.sw == 4 -> d.R 1 | 2 | 3, else <8, 1>
    {(1, 1, sw, R, 0) + NOLOOP + (pre, dt) for sw, R in ((8, 1), (4, 1), (4, 2), (4, 3)) for pre in (0, 1) for dt in TYPES}
    | {(1, 1, sw, 1, 0, False, True, False, 1, dt) for sw in (8, 4) for dt in TYPES}                       # fpb_bwd loop
    | {(1, 1, 4, 2, 0, False, True, False, 1, 'f32')}
    | {(1, 1, 4, 1, 0, True, True, False, pre, 'f32') for pre in (0, 1)} | {(1, 1, 4, 1, 0, True, True, False, 1, 'bf16')}      # F > 1
    | {(1, 1, 8, 1, 0, True, True, False, 1, 'f32'), (1, 1, 8, 1, 0, True, True, False, 0, 'bf16')}
    | {(1, 1, 8, 1, 0, False, True, True, 1, 'f32')}                                                       # channel chunks + loop
    # dws2_bwd_kernel<PL, PRE, T>: pl = same_pad_before(W, 2)
    | {(2, 2, 8, 1, pl) + NOLOOP + (pre, dt) for pl in (0, 1) for pre in (0, 1) for dt in TYPES}
    | {(2, 2, 8, 1, pl, False, True, False, pre, dt) for pl in (0, 1) for pre in (0, 1) for dt in TYPES}
    | {(2, 2, 8, 1, 1, True, True, False, pre, dt) for pre in (0, 1) for dt in TYPES}
    | {(2, 2, 8, 1, 0, True, True, False, 0, 'f32'), (2, 2, 8, 1, 0, True, True, False, 1, 'f32'), (2, 2, 8, 1, 0, True, True, False, 0, 'bf16')}
    | {(2, 2, 8, 1, 0, False, False, True, 0, 'f32')}
    | {(2, 2, 8, 1, pl, False, True, True, pre, 'f32') for pl in (0, 1) for pre in (0, 1)}
    # dwf_bwd_kernel<stride, VEC, PRE, T>: g.vec_bwd 2 | 1 (in-process: odd C, or no strip plan fits -- then always in channel chunks)
    | {(0, s, 1, 0, 0, False, False, False, pre, dt) for s in (1, 2) for pre in (0, 1) for dt in TYPES}
    | {(0, s, 2, 0, 0, False, False, True, pre, dt) for s in (1, 2) for pre in (0, 1) for dt in TYPES}
    | {(0, 1, 1, 0, 0, False, True, False, 1, 'f32')})


def known_signature(sig):
    """Every value a signature can take with today's ladders: a plan outside this (a new strip width, a fourth strip per thread, ...)
    is an instantiation REQUIRED does not know about."""
    if len(sig) == 6:
        return sig[0] in (1, 2) and sig[1] in (1, 2, 4) and sig[4] in (0, 1) and sig[5] in TYPES
    form, s, a, R, pl = sig[:5]
    return ((form == 0 and s in (1, 2) and a in (1, 2) and R == 0 and pl == 0 and not sig[5])
            or (form == 1 and s == 1 and (a, R) in ((8, 1), (4, 1), (4, 2), (4, 3)) and pl == 0)
            or (form == 2 and s == 2 and (a, R) == (8, 1) and pl in (0, 1))) and sig[8] in (0, 1) and sig[9] in TYPES


def engine_layers():
    """(G, B, H, W, C, stride, pre, tensor type) of every depthwise layer of the engine's three measured configurations, from the unit
    plan the engine is built from: stem conv 3x3 / 2 'valid', max-pool 3x3 / 2 'same', then the units (main branch: BN + ReLU6 in front
    of the depthwise; the stride-2 units' shortcut branch: none)."""
    for H, W, B, dt in ((90, 120, 256, 'f32'), (90, 360, 64, 'f32'), (90, 120, 1024, 'bf16')):
        cfg = NetConfig(H=H, W=W)
        h, w = -(-((H - 3) // 2 + 1) // 2), -(-((W - 3) // 2 + 1) // 2)
        for u in unit_plan(cfg):
            yield (cfg.T, B, h, w, u['mid'], u['stride'], 1, dt)
            if u['stride'] == 2:
                yield (cfg.T, B, h, w, u['cin'], 2, 0, dt)
                h, w = -(-h // 2), -(-w // 2)


def test_coverage(lib):
    """The variant signatures of this module's cases, computed through the plan query, cover REQUIRED and the signature of every
    depthwise layer of the engine's configurations; nothing is waived.  Prints the table case -> plan fields."""
    fwd, bwd = set(), set()
    for shape, combos, expect in CASES:
        p = plan(lib, *shape)
        print(shape, ' '.join(f'{k}={p[k]}' for k in PLAN_FIELDS), '| threads bwd', p['scx'] * p['scy'] if p['form'] else p['cx_bwd'] * p['cy_bwd'])
        for pre, dt in combos:
            fwd.add(fwd_sig(p, shape[5], pre, dt))
            bwd.add(bwd_sig(p, shape[5], pre, dt))
    assert all(known_signature(s) for s in fwd | bwd), [s for s in fwd | bwd if not known_signature(s)]
    if DWS_OFF:         # the pixel-mapped form throughout: the cases' own plans are the check (REQUIRED describes the default dispatch)
        assert all(s[0] == 0 for s in bwd), sorted(s for s in bwd if s[0])
        return
    assert not REQUIRED_FWD - fwd, sorted(REQUIRED_FWD - fwd)
    assert not REQUIRED_BWD - bwd, sorted(REQUIRED_BWD - bwd)
    missing = []
    for L in engine_layers():
        p = plan(lib, *L[:6])
        f, b = fwd_sig(p, L[5], L[6], L[7]), bwd_sig(p, L[5], L[6], L[7])
        assert known_signature(f) and known_signature(b), (L, f, b)
        if f not in fwd:
            missing.append((L, 'forward', f))
        if b not in bwd:
            missing.append((L, 'backward', b))
    assert not missing, missing


# ---- guarded tensors ---------------------------------------------------------------------------------------------------------------

class Banded:
    """A tensor inside a larger one, with a band of `band` elements of `fill` on each side."""

    def __init__(self, shape, dtype, band, fill):
        n = int(np.prod(shape))
        band = -(-band // 64) * 64              # keeps the payload's alignment
        self.whole = torch.full((band + n + band,), fill, dtype=dtype, device=DEV)
        self.t = self.whole[band:band + n].view(shape)
        self.lo, self.hi = self.whole[:band], self.whole[band + n:]
        self.ref = self.lo.clone()

    @staticmethod
    def bits(t):
        return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])

    def intact(self):
        return torch.equal(self.bits(self.lo), self.bits(self.ref)) and torch.equal(self.bits(self.hi), self.bits(self.ref))


def sync():
    """A device fault ends the run: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device fault, stopping: {e}', returncode=3)


def clean(t):
    """no NaN and no sentinel left"""
    return bool(torch.isfinite(t).all()) and not bool((t == SENTINEL).any())


def sentinel(shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def run_case(lib, shape, pre, at, X, DO, w, b, bn_pre, bn_post, Y=None, post=None, backward=True):
    """Forward (unless Y / post, a common state, are given) and two backwards of one case on guarded tensors.  X / DO: device tensors of
    the tensor type `at` (0 float32, 1 bf16); bn_pre = (gamma, beta, moving_mean, moving_var) device vectors or None, bn_post
    likewise (its moving statistics are updated in place).  Returns a dict of the outputs."""
    G, B, H, W, Cc, stride = shape
    N, Ho, Wo = G * B, -(-H // stride), -(-W // stride)
    dt = BF if at else torch.float32
    r = {}
    lib.cdrl_set_op_activation_type(at)
    try:
        pre_stats = None
        if pre:
            pre_stats = sentinel((4 * G * Cc,))
            tmp = torch.empty((N * H * W, Cc), dtype=dt, device=DEV)
            ws0 = torch.full((G * 256 * 2 * Cc,), float('nan'), dtype=torch.float64, device=DEV)
            _lib.check(lib.cdrl_bn_train_fwd(P(X), G, B * H * W, Cc, P(bn_pre[0]), P(bn_pre[1]), P(bn_pre[2]), P(bn_pre[3]), 1, 1, P(tmp), Cc,
                                             0, 0, P(pre_stats), P(ws0), S()))
            del tmp
        r['pre_stats'] = pre_stats
        nws = int(lib.cdrl_dwconv_bn_workspace_doubles(G, B, H, W, Cc, stride))
        ws = Banded((nws,), torch.float64, 1024, float('nan'))              # 8 KB bands
        if Y is None:
            y = Banded((N, Ho, Wo, Cc), dt, max(Wo * Cc, 1024), SENTINEL)
            post = sentinel((4 * G * Cc,))
            _lib.check(lib.cdrl_dwconv_bn_fwd(P(X), P(pre_stats), P(w), P(b), P(y.t), G, B, H, W, Cc, stride, P(bn_post[0]), P(bn_post[1]),
                                              P(bn_post[2]), P(bn_post[3]), 1, P(post), P(ws.t), S()))
            sync()
            assert y.intact() and ws.intact(), 'forward wrote outside y / the workspace'
            assert clean(y.t.float()) and clean(post) and clean(bn_post[2]) and clean(bn_post[3])
            Y = y.t
        r['y'], r['post'] = Y, post
        if not backward:
            return r
        runs = []
        for _ in range(2):          # the second one on the dirty workspace
            dx = Banded((N, H, W, Cc), dt, max(W * Cc, 1024), SENTINEL)
            dw, db = sentinel((3, 3, Cc, 1)), sentinel((Cc,))
            vecs = [sentinel((Cc,)) for _ in range(4)]
            coefs = [sentinel((3 * G * Cc,)) for _ in range(2)]
            _lib.check(lib.cdrl_dwconv_bn_bwd(P(X), P(pre_stats), P(DO), P(Y), P(post), P(w), G, B, H, W, Cc, stride, P(dx.t), P(dw), P(db),
                                              P(vecs[0]), P(vecs[1]), P(coefs[0]), P(vecs[2]), P(vecs[3]), P(coefs[1]), P(ws.t), S()))
            sync()
            assert dx.intact() and ws.intact(), 'backward wrote outside dx / the workspace'
            outs = [dx.t.float(), dw, db, vecs[0], vecs[1], coefs[0]] + ([vecs[2], vecs[3], coefs[1]] if pre else [])
            assert all(clean(t) for t in outs), [clean(t) for t in outs]
            runs.append((dx.t, dw, db, vecs, coefs))
        a, c = runs
        assert torch.equal(Banded.bits(a[0]), Banded.bits(c[0])) and torch.equal(a[1], c[1]) and torch.equal(a[2], c[2]), 'not reproducible'
        assert all(torch.equal(u, v) for u, v in zip(a[3][:4 if pre else 2] + a[4][:2 if pre else 1], c[3][:4 if pre else 2] + c[4][:2 if pre else 1]))
        r['bwd'] = a
    finally:
        lib.cdrl_set_op_activation_type(0)
    return r


def seed_of(shape, pre):
    return [7, int(bool(pre))] + list(shape)


def relu6_regions(x, pre_stats, G, Cc):
    """(inside, above) of relu6(z), z = fmaf(scale, x, shift) in float32 as the kernels evaluate it: the float64 product of two float32
    numbers is exact, so rounding the float64 sum to float32 reproduces fmaf.  x: (G, B, H, W, C) float32; (G, B, C, H, W) booleans."""
    st = pre_stats.cpu().double().view(4, G, Cc)
    z = (torch.from_numpy(x).double() * st[2].view(G, 1, 1, 1, Cc) + st[3].view(G, 1, 1, 1, Cc)).float().permute(0, 1, 4, 2, 3)
    return ((z > 0.0) & (z < 6.0)), (z >= 6.0)


def bound_of(name, tol, got, inp, ref, decisions, cache):
    """The op's bound `tol`; a quantity that exceeds it is held to 4 x the distance of the SAME composition evaluated in float32 from the
    float64 one (tests/util.py::check3, slack 4) -- never to anything the kernel produced."""
    if rel_err(got, getattr(ref, name)) < tol:
        return tol
    if 'r32' not in cache:
        cache['r32'] = dw_ref.evaluate(inp, torch.float32, decisions)
    noise = rel_err(getattr(cache['r32'], name), getattr(ref, name))
    print(f'{name}: kernel {rel_err(got, getattr(ref, name)):.3e}, float32 composition {noise:.3e}, bound {tol:.1e}')
    return max(tol, 4.0 * noise)


@pytest.mark.parametrize('shape,pre,expect', PARAMS)
def test_variant_f32(lib, shape, pre, expect):
    """float32 tensors against float64 autograd, with the bounds of test_dwconv_bn_fused: y, statistics, moving statistics 1e-5;
    dx, dw, dgamma, dbeta of both BatchNorms 2e-5; db (analytically zero) < 1e-4 max|dw|."""
    p = check_plan(lib, shape, expect)
    G, B, H, W, Cc, stride = shape
    inp = dw_ref.draw(np.random.default_rng(seed_of(shape, pre)), G, B, H, W, Cc, stride, pre)
    dev = lambda a: torch.as_tensor(a).to(DEV).contiguous()                          # noqa: E731
    bn = {n: tuple(dev(inp.f32[f'{n}.{k}']) for k in ('gamma', 'beta', 'moving_mean', 'moving_var')) for n in ('pre', 'post')}
    r = run_case(lib, shape, pre, 0, dev(inp.x), dev(inp.dout), dev(inp.w), dev(inp.b), bn['pre'] if pre else None, bn['post'])
    with dw_ref.cpu_threads():
        decisions = relu6_regions(inp.x, r['pre_stats'], G, Cc) if pre else None
        ref = dw_ref.evaluate(inp, decisions=decisions)
        cache = {}

        def check(name, got, tol):
            got = got.float().cpu().numpy()
            e, bound = rel_err(got, getattr(ref, name)), bound_of(name, tol, got, inp, ref, decisions, cache)
            if e >= bound:
                d = np.abs(got.astype(np.float64) - getattr(ref, name))
                worst = np.unravel_index(int(d.argmax()), d.shape)
                raise AssertionError(f'{name}: {e:.3e} >= {bound:.3e}; worst element {worst} (frame, ..., channel) of {d.shape}; plan {p}')

        st = r['post'].view(4, G, Cc)
        check('y', r['y'], 1e-5)
        check('mean', st[0], 1e-5)
        check('rstd', st[1], 1e-5)
        check('moving_mean', bn['post'][2], 1e-5)
        check('moving_var', bn['post'][3], 1e-5)
        dx, dw, db, vecs, _ = r['bwd']
        check('dx', dx, 2e-5)
        check('dw', dw, 2e-5)
        # the bias feeds a train-mode BN: its true gradient is 0, the computed one is rounding noise of the sums
        assert db.abs().max().item() < 1e-4 * dw.abs().max().item()
        check('dgamma_post', vecs[0], 2e-5)
        check('dbeta_post', vecs[1], 2e-5)
        if pre:
            check('dgamma_pre', vecs[2], 2e-5)
            check('dbeta_pre', vecs[3], 2e-5)


@pytest.mark.parametrize('shape,pre,expect', PARAMS_BF16)
def test_variant_bf16_storage(lib, shape, pre, expect):
    """bf16 tensors against the float32-tensor run of the same kernels on the same values, with the contract and the bounds of
    test_dwconv_bn_bf16_storage (activations: the rounded float32 results; sums: identical; statistics: those of the stored y)."""
    check_plan(lib, shape, expect)
    G, B, H, W, Cc, stride = shape
    c = dw_ref.bf16_inputs(np.random.default_rng(seed_of(shape, pre)), G, B, H, W, Cc, stride, DEV)

    def bn(gamma, beta):
        return gamma, beta, torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
    fw = {at: run_case(lib, shape, pre, at, X, DO, c.w, c.b, bn(c.g1, c.b1) if pre else None, bn(c.g2, c.b2), backward=bool(at))
          for at, X, DO in ((0, c.xb.float(), c.dob.float()), (1, c.xb, c.dob))}
    dw_ref.check_bf16_forward(fw[0]['y'], fw[1]['y'], fw[1]['post'], G, Cc)
    # backward from a COMMON state: the rounded y and its statistics
    yb, post = fw[1]['y'], fw[1]['post']
    o0 = run_case(lib, shape, pre, 0, c.xb.float(), c.dob.float(), c.w, c.b, bn(c.g1, c.b1) if pre else None, None, Y=yb.float(), post=post)
    dw_ref.check_bf16_backward(o0['bwd'], fw[1]['bwd'], pre)


@pytest.mark.parametrize('stride', [1, 2])
def test_frame_too_large_is_refused(lib, stride):
    """A 90x120 frame fits LDS at no channel chunk.  What the code promises, and the plan query reports (lds_fwd_over; lds_bwd_over with
    form 0): the forward refuses it too, not only the backward -- both on the host, with an error that names the frame, instead of
    launching the depthwise kernel.  y / the statistics, resp. dx / dw / db stay untouched (the backward's BatchNorm-backward sums
    of the FOLLOWING BatchNorm, a separate kernel in front, have run by then)."""
    G, B, H, W, Cc = 1, 2, 90, 120, 24
    Ho, Wo = -(-H // stride), -(-W // stride)
    p = plan(lib, G, B, H, W, Cc, stride)
    assert p['form'] == 0 and p['lds_bwd_over'] == 1 and p['lds_fwd_over'] == 1, p
    rng = np.random.default_rng(stride)
    t = lambda *s: torch.as_tensor(rng.standard_normal(s).astype(np.float32)).to(DEV)      # noqa: E731
    x, dout, yin, w, b = t(G * B, H, W, Cc), t(G * B, Ho, Wo, Cc), t(G * B, Ho, Wo, Cc), t(3, 3, Cc, 1), t(Cc)
    ones, zeros = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    ws = torch.zeros(int(lib.cdrl_dwconv_bn_workspace_doubles(G, B, H, W, Cc, stride)), dtype=torch.float64, device=DEV)
    y, post = sentinel((G * B, Ho, Wo, Cc)), sentinel((4 * G * Cc,))
    with pytest.raises(_lib.CdrlError, match='90x120'):
        _lib.check(lib.cdrl_dwconv_bn_fwd(P(x), None, P(w), P(b), P(y), G, B, H, W, Cc, stride, P(ones), P(zeros), P(zeros.clone()),
                                          P(ones.clone()), 1, P(post), P(ws), S()))
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((post == SENTINEL).all())
    stats = torch.stack([zeros, ones, ones, zeros]).view(4, 1, Cc).expand(4, G, Cc).contiguous()      # mean, rstd, scale, shift
    dx, dw, db = sentinel((G * B, H, W, Cc)), sentinel((3, 3, Cc, 1)), sentinel((Cc,))
    vecs = [sentinel((Cc,)) for _ in range(4)]
    coefs = [sentinel((3 * G * Cc,)) for _ in range(2)]
    with pytest.raises(_lib.CdrlError, match='90x120'):
        _lib.check(lib.cdrl_dwconv_bn_bwd(P(x), None, P(dout), P(yin), P(stats), P(w), G, B, H, W, Cc, stride, P(dx), P(dw), P(db), P(vecs[0]),
                                          P(vecs[1]), P(coefs[0]), P(vecs[2]), P(vecs[3]), P(coefs[1]), P(ws), S()))
    torch.cuda.synchronize()
    assert bool((dx == SENTINEL).all()) and bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all())


def test_pixel_mapped_everywhere():
    """CDRL_DWS=0: the pixel-mapped backward for EVERY float32 case of this module, against float64 (the strip forms are its
    replacement for most shapes; in the default dispatch it only runs for odd C and for frames no strip plan fits).  The switch is
    read once per process: child process.  There the cases assert form 0 from the plan query and the coverage test checks that
    instead of REQUIRED."""
    if DWS_OFF:
        return          # this IS the child
    env = dict(os.environ, CDRL_DWS='0')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-p', 'no:cacheprovider', '-k',
                        'test_variant_f32 or test_coverage'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'skipped' not in r.stdout and 'deselected' in r.stdout, r.stdout[-500:]
