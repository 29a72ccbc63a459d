"""BatchNorm family (csrc/bn.hip) at op level, in the argument forms the engine runs it with: every kernel form the host dispatchers
bn_apply / bn_bwd_reduce / bn_bwd_apply can select, bn_act_gap_fwd, gather_view and bn_inference_stats_many, against the plain
float64 reference of tests/bn_ref.py.

The dispatchers choose between a fast kernel and the generic skeleton from the views' shape and alignment, so each case first reads
cdrl_bn_plan -- the structs the launchers dispatch on -- and asserts the form it is there for; `test_coverage` then holds the union
of the cases' signatures against REQUIRED, the hand-written list of what the three launch ladders can select, and against the
signature of every BatchNorm of the engine's default configuration (oracle.spec.unit_plan).

The statistics block is drawn (random float32 mean, invstd, scale of both signs, shift), so apply and backward are tested against
exact inputs, separately from colstats / finalize; one case per tensor type takes real statistics from cdrl_bn_train_fwd.
ReLU6 regions follow tests/util.py::engine_decisions: the mask comes from z = fmaf(scale, y, shift) in float32.

Nothing here can pass by luck: outputs start as the sentinel -2**100 and workspaces as NaN, every output view sits inside a wider
buffer whose other columns and a band of rows before and after must come back bit-intact, every backward runs a second time on
the dirty workspace and must reproduce itself bit for bit, and the partials of the reduce step are summed on the host and compared
with the reference sums channel by channel.

Bounds (none of them comes from what the kernels produce):
  forward, float32     |got - ref64| <= 2^-23 |ref64| per element (one fmaf rounding is half an ulp; the bound grants one)
  forward, bf16        <= 2^-8 |ref64|;  pass-through and copy outputs: bit-equal to the source
  gap forward          <= P 2^-23 |ref64| + 2^-23 (sequential float32 sum of P non-negative terms, then one division)
  partial sums         <= 2^-22 x the sum of the terms' magnitudes (each term: a float32 subtraction, a product and, in the
                       broadcast form, a division, 3 x 2^-24; the accumulation is double)
  coefficients         k1 bit-equal to the scale; k2, k3: the partial sums' bound over Mg plus one float32 rounding
  dgamma, dbeta        rel_err < 2e-5 (tests/test_gpu_ops.py::test_bn_train)
  dy, float32          2e-5 PER CHANNEL (bn_ref.channel_err); the same formula in float32 numpy meets it with a margin of 4 on
                       every case's inputs (asserted here and in tests/test_bn_plan_host.py: worst value 1.4e-6)
  dy, bf16             the float32 result rounded once: 2^-8 (|ref64| + e) + e per element, e = 2e-5 x the channel's max |ref64|"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from oracle.spec import NetConfig, unit_plan
from tests import bn_ref
from tests.util import rel_err

BF = torch.bfloat16
SENTINEL = -2.0 ** 100          # exact in float32 and bf16; no kernel output comes near it
BAND = 8                        # guard rows in front of and behind every 2-D buffer (8 rows keep a 16-byte aligned payload)
PAD = 4                         # guard columns at the end of every row of a wide buffer
TOL = 2e-5
F32_NUMPY_MARGIN = 4.0          # the float32-numpy evaluation of dy must meet TOL / 4 (worst observed over all cases: 1.4e-6)
PLAN_FIELDS = ('form', 'vec', 'cx', 'cy', 'nloop', 'rb', 'nb', 'al0', 'al1', 'al2')
TYPES = ('f32', 'bf16')


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ref_of(v):
    return C.byref(v) if v is not None else None


def bits(t):
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def sync():
    """A device fault ends the run: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device fault, stopping: {e}', returncode=3)


class Buf:
    """A [rows][ld] tensor inside a larger one: BAND rows of `fill` in front and behind.  `view(coff)` is the cdrl_view of its columns
    from coff on; `check(cols)` asserts that the bands and every column outside `cols` still hold the fill, bit for bit."""

    def __init__(self, rows, ld, dtype, device, fill=SENTINEL):
        self.rows, self.ld, self.fill = rows, ld, fill
        self.whole = torch.full((rows + 2 * BAND, ld), fill, dtype=dtype, device=device)
        self.t = self.whole[BAND:BAND + rows]

    def put(self, cols, a):
        self.t[:, torch.as_tensor(np.asarray(cols), device=self.whole.device)] = torch.as_tensor(a).to(self.whole.device).to(self.whole.dtype)
        return self

    def view(self, coff):
        return _lib.View(self.t.data_ptr(), self.ld, coff)

    def get(self, cols):
        return self.t.cpu()[:, torch.as_tensor(np.asarray(cols))]

    def check(self, cols, what):
        w = self.whole.cpu()
        mask = torch.ones(w.shape, dtype=torch.bool)
        mask[BAND:BAND + self.rows, torch.as_tensor(np.asarray(cols, dtype=np.int64))] = False
        rest = w[mask]
        if np.isnan(self.fill):
            assert bool(torch.isnan(rest).all()), f'{what}: written outside its view'
        else:
            assert bool((rest == self.fill).all()), f'{what}: written outside its view'
        inside = w[BAND:BAND + self.rows][:, torch.as_tensor(np.asarray(cols, dtype=np.int64))].float()
        assert bool(torch.isfinite(inside).all()) and not bool((inside == SENTINEL).any()), f'{what}: elements left unwritten'


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# C -> (vec, cx, cy) of vcol_geom, rb = 2 cy for these small row counts: 24: 4, 6, 42 | 57: 1, 57, 4 | 58: 2, 29, 8 | 116: 4, 29, 8 |
# 232: 4, 58, 4 | 768: 4, 192, 1 (no LDS tree) | 514: 2, 257 lanes -> nloop 2 | 1028: 4, 257 lanes -> nloop 2.
# Rows per group: 1; cy - 1 (fewer rows than row lanes); rb; k rb + 1 (a tail block of one row: every unroll slot but the first is
# clamped); k rb + 2 cy + 1 (a tail that ends inside the 4-row unroll).  G in {1, 3, 4}.

def case(C_, G, Mg, types=TYPES, shuffle=1, relu6=1, pass_=0, y_pad=0, out_odd=0, ps_odd=0, pgd_odd=0, nostats=0, bcast=0, fwd=1, bwd=1,
         real=0, expect=()):
    """expect: the forms of the launchers the case runs, in the order apply, reduce, backward apply; shuffle: through the de-interleave of a 2 C-channel tensor;
    pass_: the identity half rides along; y_pad: y is a non-dense view (ld = C + 8, coff 4); out_odd: plain store at an odd column;
    ps_odd / pgd_odd: pass_src / pass_gdst start at an odd column; bcast: rows per frame of the pooled gradient (forward: the fused
    global average pool); real: statistics from cdrl_bn_train_fwd."""
    return SimpleNamespace(C=C_, G=G, Mg=Mg, types=types, shuffle=shuffle, relu6=relu6, pass_=pass_, y_pad=y_pad, out_odd=out_odd, ps_odd=ps_odd,
                           pgd_odd=pgd_odd, nostats=nostats, bcast=bcast, fwd=fwd, bwd=bwd and not nostats, real=real, expect=expect)


def _rows(cy, k=2):
    rb = 2 * cy
    return [m for m in (1, cy - 1, rb, k * rb + 1, k * rb + 2 * cy + 1) if m > 0]


FAST = (1, 1, 1)
CASES = []
# the unit's last BatchNorm: shuffle + ReLU6, with and without the identity half -- fast apply / reduce / backward apply, VEC 2 and 4
for C_, cy in ((58, 8), (116, 8)):
    for i, Mg in enumerate(_rows(cy)):
        CASES.append(case(C_, (1, 3, 4)[i % 3], Mg, pass_=i % 2, expect=FAST))
        CASES.append(case(C_, (3, 4, 1)[i % 3], Mg, pass_=1 - i % 2, expect=FAST, types=('f32',) if i % 2 else ('bf16',)))
for i, Mg in enumerate(_rows(42, 1)):
    CASES.append(case(24, (4, 1, 3)[i % 3], Mg, pass_=i % 2, expect=FAST))
for i, Mg in enumerate(_rows(4)):
    CASES.append(case(232, (3, 4, 1)[i % 3], Mg, pass_=1 - i % 2, expect=FAST))
CASES += [
    case(232, 1, 4097, pass_=1, expect=FAST),                       # reduce: rb 36, nine rows per thread (two full unrolls and a tail)
    case(768, 3, 5, expect=FAST), case(768, 1, 1, pass_=1, expect=FAST), case(768, 4, 2, pass_=1, expect=FAST),      # cy 1 with shuffle
    # plain BatchNorms (bn1, bn2, sc_bn1): generic apply and reduce, fast backward apply with ctot 0, ReLU6 on and off
    case(116, 3, 33, shuffle=0, relu6=1, expect=(0, 0, 1)), case(116, 4, 49, shuffle=0, relu6=0, expect=(0, 0, 1)),
    case(58, 4, 33, shuffle=0, relu6=1, expect=(0, 0, 1)), case(58, 3, 7, shuffle=0, relu6=0, expect=(0, 0, 1)),
    case(24, 1, 85, shuffle=0, relu6=1, expect=(0, 0, 1)), case(232, 4, 17, shuffle=0, relu6=0, expect=(0, 0, 1)),
    # shuffle without ReLU6: the apply ladder does not look at the activation (fast), the reduce ladder does (generic)
    case(116, 3, 17, relu6=0, expect=(1, 0, 1)), case(58, 4, 49, relu6=0, pass_=1, expect=(1, 0, 1)),
    case(57, 3, 17, relu6=0, expect=(0, 0, 0)),                     # ... and in the generic apply
    # VEC 1
    case(57, 1, 1, expect=(0, 0, 0)), case(57, 4, 3, shuffle=0, expect=(0, 0, 0)), case(57, 3, 8, pass_=1, expect=(0, 0, 0)),
    case(57, 1, 17, shuffle=0, relu6=0, expect=(0, 0, 0)), case(57, 4, 25, expect=(0, 0, 0)),
    # nloop 2
    case(514, 3, 5, expect=(0, 0, 0)), case(514, 1, 2, shuffle=0, relu6=0, expect=(0, 0, 0)), case(1028, 3, 5, pass_=1, expect=(0, 0, 0)),
    case(1028, 4, 1, shuffle=0, expect=(0, 0, 0)),
    # views that drop to the generic path
    case(58, 3, 33, shuffle=0, out_odd=1, bwd=0, expect=(0,)), case(116, 4, 17, shuffle=0, out_odd=1, relu6=0, bwd=0, expect=(0,)),
    case(116, 3, 33, pass_=1, ps_odd=1, bwd=0, expect=(0,)), case(58, 4, 49, pass_=1, ps_odd=1, bwd=0, expect=(0,)),
    case(116, 3, 33, pass_=1, pgd_odd=1, fwd=0, expect=(0, 1)), case(58, 4, 49, pass_=1, pgd_odd=1, fwd=0, expect=(0, 1)),
    case(116, 4, 33, y_pad=1, expect=(1, 0, 0)), case(58, 3, 49, y_pad=1, pass_=1, expect=(1, 0, 0)),
    case(232, 3, 25, y_pad=1, shuffle=0, relu6=0, expect=(0, 0, 0)),
    # the pure concat-and-shuffle copy (float32 only, as the engine enforces)
    case(58, 1, 49, types=('f32',), relu6=0, nostats=1, expect=(0,)), case(116, 1, 33, types=('f32',), relu6=0, nostats=1, expect=(0,)),
    case(57, 1, 25, types=('f32',), relu6=0, nostats=1, expect=(0,)),
    # head BatchNorm fused with the global average pool: P 12 rows per frame, 5 frames per group (rb does not divide by P: frames
    # straddle blocks), and P 1
    case(768, 4, 60, shuffle=0, bcast=12, expect=(0, 1)), case(116, 4, 60, shuffle=0, bcast=12, expect=(0, 1)),
    case(58, 4, 60, shuffle=0, bcast=12, expect=(0, 1)), case(768, 3, 5, shuffle=0, bcast=1, expect=(0, 1)),
    case(57, 4, 60, shuffle=0, bcast=12, expect=(0, 0)), case(1028, 4, 60, shuffle=0, bcast=12, expect=(0, 0)),
    # real statistics
    case(116, 4, 165, pass_=1, real=1, expect=FAST), case(58, 3, 97, shuffle=0, real=1, expect=(0, 0, 1)),
]


def case_id(c, dt):
    flags = ''.join(f for f, on in (('s', c.shuffle), ('r', c.relu6), ('p', c.pass_), ('Y', c.y_pad), ('O', c.out_odd), ('I', c.ps_odd), ('D', c.pgd_odd),
                                    ('N', c.nostats), ('R', c.real)) if on)
    return f'{dt}-C{c.C}-G{c.G}-M{c.Mg}-{flags or "plain"}' + (f'-P{c.bcast}' if c.bcast else '') + ('' if c.fwd and c.bwd else '-fwd' if c.fwd else '-bwd')


PARAMS = [pytest.param(c, dt, id=case_id(c, dt)) for c in CASES for dt in c.types]


def setup(c, dt, device, seed_extra=0):
    """Inputs and every buffer of a case (on `device`: the host test builds them on the CPU to read the plan of the same layout)."""
    at = int(dt == 'bf16')
    tt = BF if at else torch.float32
    G, Mg, Cc = c.G, c.Mg, c.C
    R = G * Mg
    assert R * Cc < 1_000_000
    inp = bn_ref.draw(np.random.default_rng([11, Cc, G, Mg, c.shuffle, c.relu6, c.pass_, c.bcast, at, seed_extra]), G, Mg, Cc, bf16=bool(at), bcast=c.bcast)
    ctot = 2 * Cc if c.shuffle else 0
    width = 2 * Cc + PAD
    b = SimpleNamespace(inp=inp, at=at, tt=tt, ctot=ctot, R=R)
    y_ld, b.y_coff = (Cc + 8, 4) if c.y_pad else (Cc, 0)
    b.y = Buf(R, y_ld, tt, device, fill=0.5).put(b.y_coff + np.arange(Cc), inp.y)
    b.stats = None if c.nostats else torch.as_tensor(inp.stats).to(device).contiguous()
    # forward: `out` is the unit's 2 C-channel output (identity half at 0, this BatchNorm's half at C), or a plain store at column 1
    b.out_coff = 1 if c.out_odd else Cc
    b.out = Buf(R, width, tt, device)
    b.out_cols = bn_ref.view_cols(b.out_coff, Cc, ctot)
    b.pass_cols = bn_ref.view_cols(0, Cc, ctot)
    b.ps_coff = 1 if c.ps_odd else 0
    b.x = Buf(R, width, tt, device, fill=0.25).put(b.ps_coff + np.arange(Cc), inp.ident) if c.pass_ else None
    b.gap = Buf(R // c.bcast, Cc, torch.float32, device) if c.bcast else None
    # backward: `dout` is the gradient of the same 2 C-channel tensor (read through the shuffle), or the pooled gradient
    if c.bcast:
        b.dout, b.d_coff = Buf(R // c.bcast, Cc, torch.float32, device, fill=0.125).put(np.arange(Cc), inp.d), 0
    else:
        b.dout, b.d_coff = Buf(R, width, tt, device, fill=0.125).put(bn_ref.view_cols(Cc, Cc, ctot), inp.d), Cc
        if c.pass_:
            b.dout.put(b.pass_cols, inp.gident)
    b.pgd_coff = 1 if c.pgd_odd else 0
    b.dy = Buf(R, Cc, tt, device)
    return b


def views(c, b, gx=None):
    """(y, out, dout, pass_src, pass_dst, pass_gsrc, pass_gdst) as cdrl_view structures (None: absent)"""
    p = c.pass_
    return (b.y.view(b.y_coff), b.out.view(b.out_coff), b.dout.view(b.d_coff), b.x.view(b.ps_coff) if p else None, b.out.view(0) if p else None,
            b.dout.view(0) if p else None, (gx if gx is not None else b.x).view(b.pgd_coff) if p else None)


def plan(lib, c, b):
    """{'apply' | 'reduce' | 'bapply': {field: value}} of cdrl_bn_plan for the case's own buffers"""
    v = views(c, b)
    out = (C.c_int32 * 30)()
    n = lib.cdrl_bn_plan(ref_of(v[0]), ref_of(v[1]), ref_of(v[2]), b.ctot, c.G, c.Mg, c.C, int(not c.nostats), c.relu6, ref_of(v[3]), ref_of(v[4]),
                         ref_of(v[5]), ref_of(v[6]), C.c_void_p(b.dy.t.data_ptr()), c.bcast, b.at, out, 30)
    _lib.check(0 if n == 30 else -1, 'cdrl_bn_plan')
    return {k: dict(zip(PLAN_FIELDS, out[10 * i:10 * i + 10])) for i, k in enumerate(('apply', 'reduce', 'bapply'))}


def signatures(c, pl, dt):
    """What a case exercises, as dictionaries REQUIRED entries and the engine's BatchNorms are matched against."""
    sigs = []
    if c.fwd and c.bcast:
        sigs.append(dict(op='gap', P=c.bcast, dt=dt))
    elif c.fwd:
        a = pl['apply']
        sigs.append(dict(op='apply', form=a['form'], vec=a['vec'], nloop=a['nloop'], shuffle=c.shuffle, relu6=c.relu6, pass_=c.pass_, stats=int(not c.nostats),
                         al_out=a['al1'], al_pass=a['al2'] if c.pass_ else 1, cy1=int(a['cy'] == 1), dt=dt))
    if c.bwd:
        r, a = pl['reduce'], pl['bapply']
        dense = int(not c.y_pad)
        sigs.append(dict(op='reduce', form=r['form'], vec=r['vec'], nloop=r['nloop'], shuffle=c.shuffle, relu6=c.relu6, pass_=c.pass_, dense=dense,
                         bcast=int(c.bcast > 0), al_pass=r['al2'] if c.pass_ else 1, cy1=int(r['cy'] == 1), dt=dt))
        sigs.append(dict(op='bapply', form=a['form'], vec=a['vec'], nloop=a['nloop'], shuffle=c.shuffle, relu6=c.relu6, dense=dense, bcast=int(c.bcast > 0),
                         cy1=int(a['cy'] == 1), dt=dt))
    return sigs


# ---- REQUIRED: what the launch ladders of bn_apply_t / bn_bwd_reduce / bn_bwd_apply (csrc/bn.hip) can select, written out from them.
# An entry is matched by a signature that agrees on every key it names.  (The apply ladder does not look at the activation, so
# "shuffle without ReLU6" is a fast form there for VEC >= 2 and a generic one for VEC 1; both are listed.)
def _req():
    for dt in TYPES:
        for vec in (4, 2):
            for p in (0, 1):
                yield dict(op='apply', form=1, vec=vec, pass_=p, dt=dt)
                yield dict(op='reduce', form=1, vec=vec, pass_=p, dt=dt)
            for sh in (0, 1):
                for r in (0, 1):
                    yield dict(op='bapply', form=1, vec=vec, shuffle=sh, relu6=r, dt=dt)
        for vec in (4, 2, 1):
            yield dict(op='apply', form=0, vec=vec, nloop=1, dt=dt)
        for op in ('apply', 'reduce', 'bapply'):
            yield dict(op=op, form=0, nloop=2, vec=4, dt=dt)
            yield dict(op=op, form=0, nloop=2, vec=2, dt=dt)
        yield dict(op='apply', form=1, shuffle=1, relu6=0, dt=dt)
        yield dict(op='apply', form=0, shuffle=1, relu6=0, dt=dt)
        yield dict(op='apply', form=0, shuffle=0, al_out=0, dt=dt)
        yield dict(op='apply', form=0, shuffle=1, pass_=1, al_pass=0, dt=dt)
        yield dict(op='apply', form=1, cy1=1, dt=dt)
        yield dict(op='reduce', form=0, shuffle=1, relu6=0, dt=dt)
        yield dict(op='reduce', form=0, dense=0, dt=dt)
        yield dict(op='reduce', form=0, vec=1, dt=dt)
        yield dict(op='reduce', form=0, bcast=1, dt=dt)
        yield dict(op='reduce', form=0, bcast=1, cy1=1, dt=dt)
        yield dict(op='reduce', form=0, shuffle=1, relu6=1, pass_=1, al_pass=0, dt=dt)
        yield dict(op='reduce', form=1, cy1=1, dt=dt)
        yield dict(op='bapply', form=1, bcast=1, cy1=1, dt=dt)
        yield dict(op='bapply', form=1, bcast=1, cy1=0, dt=dt)
        yield dict(op='bapply', form=0, vec=1, dt=dt)
        yield dict(op='bapply', form=0, dense=0, dt=dt)
        yield dict(op='bapply', form=0, bcast=1, dt=dt)
        yield dict(op='gap', P=1, dt=dt)
        yield dict(op='gap', P=12, dt=dt)
    yield dict(op='apply', form=0, stats=0, dt='f32')


REQUIRED = list(_req())


def matches(req, sig):
    return all(sig.get(k) == v for k, v in req.items())


def engine_batchnorms():
    """(Mg, C, shuffle, act, pass, gap) of every BatchNorm of the engine's default configuration that goes through these launchers,
    from the unit plan the engine is built from (stem conv 3x3 / 2 'valid', max-pool 3x3 / 2 'same', the units, the head with its fused
    average pool).  CDRL_FUSED_PASS is on by default: every stride-1 unit's bn3 carries the identity half."""
    cfg, B = NetConfig(), 256
    h, w = -(-((cfg.H - 3) // 2 + 1) // 2), -(-((cfg.W - 3) // 2 + 1) // 2)
    for u in unit_plan(cfg):
        ho, wo = (-(-h // 2), -(-w // 2)) if u['stride'] == 2 else (h, w)
        yield (B * h * w, u['mid'], 0, 1, 0, 0)                                     # bn1
        yield (B * ho * wo, u['mid'], 0, 0, 0, 0)                                   # bn2
        yield (B * ho * wo, u['main_out'], 1, 1, int(u['stride'] == 1), 0)          # bn3
        if u['stride'] == 2:
            yield (B * ho * wo, u['shortcut_c'], 0, 0, 0, 0)                        # sc_bn1
            yield (B * ho * wo, u['shortcut_c'], 1, 1, 0, 0)                        # sc_bn2
        h, w = ho, wo
    yield (B * h * w, cfg.last_channels, 0, 1, 0, h * w)                            # head: BatchNorm + ReLU6 + global average pool


def engine_signatures(lib, dt):
    """The signatures of engine_batchnorms() for dense, aligned views (every engine tensor is 256-byte aligned)."""
    for Mg, Cc, sh, act, ps, gp in engine_batchnorms():
        at = int(dt == 'bf16')
        ctot = 2 * Cc if sh else 0
        base = 1 << 20
        dense, wide = _lib.View(base, Cc, 0), _lib.View(base, 2 * Cc, Cc)
        wide0 = _lib.View(base, 2 * Cc, 0)
        pv = [ref_of(wide0) if ps else None] * 4
        out = (C.c_int32 * 30)()
        n = lib.cdrl_bn_plan(ref_of(dense), ref_of(wide if sh else dense), ref_of(wide if sh else dense), ctot, 4, Mg, Cc, 1, act, pv[0], pv[1], pv[2], pv[3],
                             C.c_void_p(base), gp, at, out, 30)
        assert n == 30, (Mg, Cc)
        pl = {k: dict(zip(PLAN_FIELDS, out[10 * i:10 * i + 10])) for i, k in enumerate(('apply', 'reduce', 'bapply'))}
        c = case(Cc, 4, Mg, shuffle=sh, relu6=act, pass_=ps, bcast=gp)
        for s in signatures(c, pl, dt):
            if s['op'] == 'gap':
                s['P'] = 12 if gp > 1 else 1            # the pool's loop: one row, or several
            yield (Mg, Cc, sh, act, ps, gp), s


def case_signatures(lib, device):
    sigs = []
    for c in CASES:
        for dt in c.types:
            pl = plan(lib, c, setup(c, dt, device))
            sigs += signatures(c, pl, dt)
    return sigs


def coverage_gaps(lib, device):
    sigs = case_signatures(lib, device)
    missing = [r for r in REQUIRED if not any(matches(r, s) for s in sigs)]
    for dt in TYPES:
        for layer, s in engine_signatures(lib, dt):
            if s not in sigs:
                missing.append((layer, s))
    return missing


@pytest.mark.gpu
def test_coverage(lib):
    """The signatures of this module's cases, computed through the plan query on the cases' own buffers, cover REQUIRED and the
    signature of every BatchNorm of the engine's default configuration, in both tensor types; nothing is waived."""
    missing = coverage_gaps(lib, 'cuda:0')
    assert not missing, missing


# ---- running a case ---------------------------------------------------------------------------------------------------------------

def check_plan(lib, c, b):
    pl = plan(lib, c, b)
    forms = [pl[k]['form'] for k, on in (('apply', c.fwd and not c.bcast), ('reduce', c.bwd), ('bapply', c.bwd)) if on]
    assert tuple(forms) == tuple(c.expect), (pl, c.expect)
    return pl


def real_statistics(lib, c, b):
    """The statistics block of the case's y from cdrl_bn_train_fwd (colstats + finalize; its own apply output is not used)."""
    dev = b.y.whole.device
    gamma, beta = (torch.as_tensor(v).to(dev) for v in bn_ref.draw_affine(c.C))
    mm, mv = torch.zeros(c.C, device=dev), torch.ones(c.C, device=dev)
    stats = torch.full((4 * c.G * c.C,), SENTINEL, device=dev)
    tmp = torch.empty((b.R, c.C), dtype=b.tt, device=dev)
    ws = torch.full((c.G * 256 * 2 * c.C,), float('nan'), dtype=torch.float64, device=dev)
    _lib.check(lib.raw.cdrl_bn_train_fwd(P(b.y.t), c.G, c.Mg, c.C, P(gamma), P(beta), P(mm), P(mv), 1, c.relu6, P(tmp), c.C, 0, 0, P(stats), P(ws), b.at, S()))
    sync()
    st = stats.view(4, c.G, c.C)
    y64 = b.inp.y.astype(np.float64).reshape(c.G, c.Mg, c.C)
    assert rel_err(st[0].cpu().numpy(), y64.mean(axis=1)) < 1e-5 and rel_err(st[1].cpu().numpy(), 1.0 / np.sqrt(y64.var(axis=1) + bn_ref.EPS)) < 1e-5
    return st.contiguous()


def forward_case(lib, c, b):
    G, Mg, Cc, inp = c.G, c.Mg, c.C, b.inp
    stats_np = None if c.nostats else b.stats.cpu().numpy()
    if c.bcast:
        _lib.check(lib.cdrl_bn_act_gap_fwd(P(b.y.t), P(b.stats), P(b.gap.t), G, Mg // c.bcast, c.bcast, Cc, c.relu6, b.at, S()))
        sync()
        b.gap.check(np.arange(Cc), 'gap out')
        ref = bn_ref.gap(bn_ref.apply(inp.y, stats_np, G, Mg, c.relu6), c.bcast)
        got = b.gap.t.cpu().numpy().astype(np.float64)
        assert c.relu6          # the bound is that of a sum of non-negative terms
        err = np.abs(got - ref) - (c.bcast * 2.0 ** -23 * np.abs(ref) + 2.0 ** -23)
        assert err.max() <= 0, f'gap forward: worst excess {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}'
        return
    v = views(c, b)
    _lib.check(lib.cdrl_bn_apply(ref_of(v[0]), G, Mg, Cc, P(b.stats), c.relu6, ref_of(v[1]), b.ctot, ref_of(v[3]), ref_of(v[4]), b.at, S()))
    sync()
    b.out.check(np.concatenate([b.out_cols, b.pass_cols]) if c.pass_ else b.out_cols, 'out')
    got = b.out.get(b.out_cols)
    if c.nostats:
        assert torch.equal(bits(got), bits(torch.as_tensor(inp.y))), 'copy: not bit-equal to the source'
    else:
        ref = bn_ref.apply(inp.y, stats_np, G, Mg, c.relu6)
        err = np.abs(got.double().numpy() - ref) - (2.0 ** -8 if b.at else 2.0 ** -23) * np.abs(ref)
        assert err.max() <= 0, f'apply: worst excess {err.max():.3e} at (row, channel) {np.unravel_index(err.argmax(), err.shape)}'
    if c.pass_:
        assert torch.equal(bits(b.out.get(b.pass_cols)), bits(torch.as_tensor(inp.ident).to(b.tt))), 'identity half: not bit-equal to the source'
        assert torch.equal(bits(b.x.whole.cpu()), bits(b.x_before)), 'pass_src was written'


def f32_numpy_noise(c, inp, stats_np, ref):
    """dy by the same formula in float32 numpy against the float64 reference, per channel: must meet the bound with a margin"""
    r32 = bn_ref.backward(inp.y, inp.d, stats_np, c.G, c.Mg, c.relu6, c.bcast, dtype=np.float32)
    return bn_ref.channel_err(r32.dy, ref.dy)


def backward_case(lib, c, b, pl):
    G, Mg, Cc, inp, dev = c.G, c.Mg, c.C, b.inp, b.y.whole.device
    stats_np = b.stats.cpu().numpy()
    ref = bn_ref.backward(inp.y, inp.d, stats_np, G, Mg, c.relu6, c.bcast)
    noise = f32_numpy_noise(c, inp, stats_np, ref)
    print(f'float32-numpy dy error per channel: {noise:.3e}')
    assert noise * F32_NUMPY_MARGIN < TOL, noise
    nb = pl['reduce']['nb']
    assert nb == pl['bapply']['nb']
    n1, n2 = G * nb * 2 * Cc, G * nb * Cc
    ws = Buf(1, n1 + n2, torch.float64, dev, fill=float('nan'))
    runs = []
    for _ in range(2):          # the second one on the dirty workspace
        dy = Buf(b.R, Cc, b.tt, dev)
        gx = Buf(b.R, 2 * Cc + PAD, b.tt, dev) if c.pass_ else None
        dgamma, dbeta, coef = (torch.full((n,), SENTINEL, device=dev) for n in (Cc, Cc, 3 * G * Cc))
        v = views(c, b, gx)
        _lib.check(lib.cdrl_bn_bwd(ref_of(v[2]), b.ctot, ref_of(v[0]), G, Mg, Cc, P(b.stats), c.relu6, P(dgamma), P(dbeta), P(dy.t), P(coef), P(ws.t),
                                   ref_of(v[5]), ref_of(v[6]), c.bcast, b.at, S()))
        sync()
        dy.check(np.arange(Cc), 'dy')
        ws.check(np.arange(n1 + n2), 'workspace')
        for t in (dgamma, dbeta, coef):
            assert bool(torch.isfinite(t).all()) and not bool((t == SENTINEL).any())
        if c.pass_:
            gx.check(b.pgd_coff + np.arange(Cc), 'pass_gdst')
        runs.append((dy, gx, dgamma, dbeta, coef, ws.t.clone()))
    a, r2 = runs
    assert torch.equal(bits(a[0].t), bits(r2[0].t)) and all(torch.equal(bits(p), bits(q)) for p, q in zip(a[2:], r2[2:])), 'not reproducible'
    assert torch.equal(bits(b.dout.whole.cpu()), bits(b.dout_before)) and torch.equal(bits(b.y.whole.cpu()), bits(b.y_before)), 'an input was written'
    dy, gx, dgamma, dbeta, coef, wsv = a
    # the partials of the reduce step, summed on the host
    part = wsv[0, :n1].cpu().numpy().reshape(G, nb, 2, Cc).sum(axis=1)
    for q, (s, mag) in enumerate(((ref.s1, ref.a1), (ref.s2, ref.a2))):
        err = np.abs(part[:, q] - s) - 2.0 ** -22 * mag
        assert err.max() <= 0, f'partial sums {q}: worst excess {err.max():.3e} at (group, channel) {np.unravel_index(err.argmax(), err.shape)}'
    assert rel_err(dgamma.cpu().numpy(), ref.dgamma) < TOL and rel_err(dbeta.cpu().numpy(), ref.dbeta) < TOL
    cf = coef.cpu().numpy().reshape(3, G, Cc)
    # coefficients: k1 is the statistics block's scale itself; k2, k3 are the sums over Mg (bound of the partial sums) rounded to float32
    assert np.array_equal(cf[0], stats_np[2])
    for q, mag in ((1, ref.a1), (2, ref.a2)):
        err = np.abs(cf[q] - ref.k[q]) - (2.0 ** -22 * mag / Mg + 2.0 ** -24 * np.abs(ref.k[q]))
        assert err.max() <= 0, f'coef {q}: worst excess {err.max():.3e}'
    got = dy.t.cpu().double().numpy()
    if b.at:
        e = TOL * np.abs(ref.dy).max(axis=0, keepdims=True)
        err = np.abs(got - ref.dy) - (2.0 ** -8 * (np.abs(ref.dy) + e) + e)
        assert err.max() <= 0, f'dy: worst excess {err.max():.3e} at (row, channel) {np.unravel_index(err.argmax(), err.shape)}'
    else:
        e = bn_ref.channel_err(got, ref.dy)
        print(f'dy error per channel: {e:.3e}')
        assert e < TOL, f'dy: {e:.3e} per channel'
    if c.pass_:
        assert torch.equal(bits(gx.get(b.pgd_coff + np.arange(Cc))), bits(torch.as_tensor(inp.gident).to(b.tt))), 'identity gradient: not bit-equal'


@pytest.mark.gpu
@pytest.mark.parametrize('c,dt', PARAMS)
def test_variant(lib, c, dt):
    """One case: the plan it is there for, then forward (apply, copy or the fused average pool) and two backwards on guarded buffers
    against tests/bn_ref.py with the bounds of the module docstring."""
    b = setup(c, dt, 'cuda:0')
    pl = check_plan(lib, c, b)
    if c.real:
        b.stats = real_statistics(lib, c, b)
    b.y_before, b.dout_before = b.y.whole.cpu().clone(), b.dout.whole.cpu().clone()
    if c.pass_:
        b.x_before = b.x.whole.cpu().clone()
    if c.fwd:
        forward_case(lib, c, b)
    if c.bwd:
        backward_case(lib, c, b, pl)


@pytest.mark.gpu
@pytest.mark.parametrize('Cc,rows,shuffle,accumulate', [(24, 37, 1, 0), (24, 70, 0, 1), (58, 70, 1, 1), (58, 33, 0, 0), (116, 300, 1, 1)])
def test_gather_view(lib, Cc, rows, shuffle, accumulate):
    """gather_view: dst (plain view) = or += src read through the shuffle; C below and above the 32 channel lanes, one and several
    blocks.  A copy is bit-equal to the source; an accumulation is the single float32 addition."""
    rng = np.random.default_rng([Cc, rows, shuffle, accumulate])
    ctot, width = (2 * Cc if shuffle else 0), 2 * Cc + PAD
    src_np, pre_np = rng.standard_normal((rows, Cc)).astype(np.float32), rng.standard_normal((rows, Cc)).astype(np.float32)
    src = Buf(rows, width, torch.float32, 'cuda:0', fill=0.125).put(bn_ref.view_cols(Cc, Cc, ctot), src_np)
    dst = Buf(rows, width, torch.float32, 'cuda:0')
    dcols = 1 + np.arange(Cc)
    if accumulate:
        dst.put(dcols, pre_np)
    sv, dv = src.view(Cc), dst.view(1)
    before = src.whole.cpu().clone()
    _lib.check(lib.cdrl_gather_view(ref_of(sv), ctot, rows, Cc, ref_of(dv), accumulate, S()))
    sync()
    dst.check(dcols, 'dst')
    assert torch.equal(bits(src.whole.cpu()), bits(before))
    want = pre_np + src_np if accumulate else src_np
    assert torch.equal(bits(dst.get(dcols)), bits(torch.as_tensor(want)))


@pytest.mark.gpu
@pytest.mark.parametrize('G', [1, 4])
def test_inference_stats(lib, G):
    """bn_inference_stats_many: three layers of different widths in one launch (none a multiple of the 64-thread block, one below it).
    invstd is one float32 rounding of the float64 value (2^-24), computed with the float32 constant 1e-3f, which sits 4.7e-11 above 1e-3:
    at most 2.4e-8 of var + eps here, together under 2^-23; scale one more product; shift two products and a subtraction."""
    rng = np.random.default_rng(G)
    Cs = (24, 116, 100)
    vec = lambda a: torch.as_tensor(np.asarray(a, np.float32)).cuda()                   # noqa: E731
    layers = [SimpleNamespace(C=Cc, gamma=vec(rng.uniform(0.5, 1.5, Cc) * rng.choice([-1, 1], Cc)), beta=vec(rng.standard_normal(Cc)),
                              mm=vec(rng.standard_normal(Cc)), mv=vec(rng.uniform(0.0, 2.0, Cc)), stats=Buf(1, 4 * G * Cc, torch.float32, 'cuda:0'))
              for Cc in Cs]
    n = len(layers)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])                      # noqa: E731
    table = torch.zeros(int(lib.cdrl_bn_inference_stats_table_bytes(n)), dtype=torch.uint8, device='cuda:0')
    _lib.check(lib.cdrl_bn_inference_stats(n, arr([L.gamma for L in layers]), arr([L.beta for L in layers]), arr([L.mm for L in layers]),
                                           arr([L.mv for L in layers]), arr([L.stats.t for L in layers]), (C.c_int * n)(*([G] * n)), (C.c_int * n)(*Cs),
                                           P(table), S()))
    sync()
    for L in layers:
        L.stats.check(np.arange(4 * G * L.C), 'stats')
        got = L.stats.t.cpu().double().numpy().reshape(4, G, L.C)
        g, bt, m, v = (t.cpu().double().numpy() for t in (L.gamma, L.beta, L.mm, L.mv))
        ref = bn_ref.inference_stats(g, bt, m, v, G)
        assert np.array_equal(got[0], ref[0])
        assert (np.abs(got[1] - ref[1]) <= 2.0 ** -23 * np.abs(ref[1])).all()
        assert (np.abs(got[2] - ref[2]) <= 2.0 ** -22 * np.abs(ref[2])).all()
        assert (np.abs(got[3] - ref[3]) <= 2.0 ** -21 * (np.abs(bt) + np.abs(m * ref[2]))).all()


@pytest.mark.gpu
def test_bad_views_are_refused(lib):
    """The wrappers check that every view's channels stay inside its rows before anything is launched."""
    t = torch.full((16, 8), SENTINEL, device='cuda:0')
    ok, short = _lib.View(t.data_ptr(), 8, 0), _lib.View(t.data_ptr(), 8, 4)
    st = torch.ones(4 * 8, device='cuda:0')
    for args in ((ref_of(ok), 1, 16, 8, P(st), 0, ref_of(short), 0, None, None, 0), (ref_of(ok), 1, 16, 8, P(st), 0, ref_of(ok), 12, None, None, 0),
                 (ref_of(ok), 1, 16, 8, None, 1, ref_of(ok), 0, None, None, 0), (ref_of(ok), 1, 16, 8, P(st), 0, ref_of(ok), 0, ref_of(ok), None, 0)):
        with pytest.raises(_lib.CdrlError):
            _lib.check(lib.cdrl_bn_apply(*args, S()))
    torch.cuda.synchronize()
    assert bool((t == SENTINEL).all())
