"""The 1x1-conv forward / backward-data family at op level: every instantiation the three launch ladders hold -- pw_nn_kernel<KSM, NT, PRO,
EPI, MODE, ACC> (csrc/gemm_pw.hip, through cdrl_pwconv_ex), pw_x3_kernel<KP, NT, PRO, EPI> / pw_x3_wide_kernel<PRO, EPI> (cdrl_pwconv_x3)
and pw_x3_wide_bwd_kernel<SH, EPI, ACC> (cdrl_pwconv_x3_wide_bwd, csrc/gemm_pw_x3.hip) -- against the float64 contract of tests/pwf_ref.py.

Each case first reads the plan (the struct the launcher dispatches on) and must land on the signature it was written for; REQUIRED*, the
hand-written lists of what the ladders instantiate, are held against the cases here and against the plan sweep in
tests/test_pw_plan_host.py.  A test function is one (KSM, NT) pair: 30 signatures, small launches.

Shapes: rows per group 1, bm - 1, bm, bm + 1, 3 bm + 5 (wide forms: 1, 31, 32, 33, 65); G = 128 where a workgroup must own more than
one tile; K at each padding's first and last even value, N at each column-tile count's first and last value (even under bf16 storage,
whose epilogue stores column pairs).  Operands sit in padded views with the offsets each form allows -- the dz view of the
BatchNorm-backward prologue also at an odd offset in odd rows, which the plan says needs no alignment -- framed by NaN; outputs start
as a sentinel, partial buffers as NaN between bands; everything around a payload must come back bit-intact, and every case runs a second
time on the dirty partial buffers and must reproduce itself bit for bit.

Contract: small-integer operands -> the exact value in every mode; standard-normal operands -> every element within
pwf_ref.bound of float64 (derivation there); bf16 storage -> bit for bit the bf16 rounding of what the float32-tensor form of the same
mode produces from the widened inputs; partials, summed in float64, against float64 sums of the values the kernel stored (rtol 1e-9,
atol 1e-6; under bf16 storage the BatchNorm-sum epilogue sums the float32 values in front of the storage rounding); the ReLU6 mask of tests/pw_ref.py, no element excluded."""
import ctypes as C
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from tests import pwf_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
SENTINEL = -2.0 ** 100          # exact in float32 and bf16; no kernel output comes near it
GR = 2                          # guard rows above and below every 2-D tensor (even: keeps the view pointers 16-byte aligned)
BAND = 256
FAKE = 1 << 20                  # a non-null, aligned address for probing the plans (the queries read no memory)

# ---- REQUIRED: what the launch ladders instantiate, written out from them -----------------------------------------------------------
NN_PAIRS = ((16, 1), (16, 2), (16, 3), (16, 4), (32, 1), (32, 2), (32, 3), (32, 4), (64, 1), (64, 2), (64, 4), (128, 4))
NN_PRO_EPI = ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0), (2, 2))
REQUIRED = {(ksm, nt, pro, epi, mode, acc) for ksm, nt in NN_PAIRS for pro, epi in NN_PRO_EPI for mode in (0, 1, 2)
            for acc in ((0, 1) if epi == 0 else (0,))}
REQUIRED_X3 = ({(0, kp, nt, pro, epi) for kp in (32, 64, 128) for nt in (1, 2, 4) for pro in (0, 1) for epi in (0, 1)}
               | {(1, 256, 4, pro, epi) for pro in (0, 1) for epi in (0, 1)})
REQUIRED_X3B = {(sh, epi, acc) for sh in (0, 1) for epi, acc in ((0, 0), (1, 0), (0, 1))}
assert (len(REQUIRED), len(REQUIRED_X3), len(REQUIRED_X3B)) == (360, 40, 6)

NN_KS = {16: (2, 32), 32: (34, 64), 64: (66, 128), 128: (130, 256)}
NN_NS = {1: (1, 32), 2: (33, 64), 3: (65, 96), 4: (97, 128, 129, 232, 256)}
NN_NS_EVEN = {1: (2, 32), 2: (34, 64), 3: (66, 96), 4: (98, 128, 130, 232, 256)}
X3_KS = {32: (4, 32), 64: (34, 64), 128: (66, 128)}
X3_NS = {1: (1, 32), 2: (33, 64), 4: (65, 96, 97, 128)}
WIDE_MG = (1, 31, 32, 33, 65)

# a / c: 'dense', 'pad' (ld + 6 | + 8, offset 2 | 4), 'split' (the right half of a tensor twice as wide).  dz (prologue 2): those, 'odd'
# (odd row length, odd offset), or through the channel shuffle of a 2 K-channel tensor as its low / high part.
Case = namedtuple('Case', 'entry sig G Mg K N pro epi acc mode a c packed wt relu6')


def bm_of(nt):
    return 32 * (4 // (1 if nt == 3 else nt))


def nn_cases(ksm, nt):
    out, i = [], 0
    for pro, epi in NN_PRO_EPI:
        for mode in (0, 1, 2):
            for acc in ((0, 1) if epi == 0 else (0,)):
                bm = bm_of(nt)
                ns = (NN_NS_EVEN if mode == 2 else NN_NS)[nt]
                Mg = (1, bm - 1, bm, bm + 1, 3 * bm + 5)[i % 5]
                G = 128 if i == 4 else (2, 3, 1, 4)[i % 4]
                a = (('dense', 'odd', 'lo', 'hi', 'pad') if pro == 2 else ('dense', 'pad', 'split'))[i % (5 if pro == 2 else 3)]
                out.append(Case('nn', (ksm, nt, pro, epi, mode, acc), G, Mg, NN_KS[ksm][i % 2], ns[i % len(ns)], pro, epi, acc, mode, a,
                                ('pad', 'dense', 'split')[i % 3], int(mode > 0 or i % 2), (i // 2) % 2, int(i % 3 != 0)))
                i += 1
    return out


def x3_cases():
    out, i = [], 0
    for kp in (32, 64, 128):
        for nt in (1, 2, 4):
            for pro in (0, 1):
                for epi in (0, 1):
                    bm = 32 * (4 // nt)
                    G, Mg = (128, 4 * bm + 3) if i % 4 == 1 else ((2, 3, 1)[i % 3], (1, bm - 1, bm, bm + 1, 3 * bm + 5)[i % 5])
                    out.append(Case('x3', (0, kp, nt, pro, epi), G, Mg, X3_KS[kp][i % 2], X3_NS[nt][i % len(X3_NS[nt])], pro, epi, 0, 0,
                                    ('dense', 'pad', 'split')[i % 3], ('pad', 'dense')[i % 2], 1, i % 2, 0))
                    i += 1
    for j, (K, N) in enumerate(((132, 1), (256, 33), (64, 129), (232, 232), (4, 256), (256, 256), (128, 232), (140, 97))):
        for pro, epi in ((j % 2, (j // 2) % 2), (1 - j % 2, 1 - (j // 2) % 2)):
            out.append(Case('x3', (1, 256, 4, pro, epi), (2, 3, 1)[j % 3], WIDE_MG[(j + pro) % 5], K, N, pro, epi, 0, 0, ('dense', 'pad4')[j % 2],
                            ('pad', 'dense')[j % 2], 1, j % 2, 0))
    return out


def x3b_cases():
    out, j = [], 0
    for K, N in ((132, 64), (232, 232), (4, 129), (256, 256), (128, 232)):
        for sh in (0, 1):
            for epi, acc in ((0, 0), (1, 0), (0, 1)):
                out.append(Case('x3b', (sh, epi, acc), (2, 3, 1)[j % 3], WIDE_MG[j % 5], K, N, 2, 2 if epi else 0, acc, 0,
                                (('lo', 'hi')[j % 2] if sh else ('dense', 'pad4')[j % 2]), ('pad', 'dense', 'split')[j % 3], 1, 1, int(j % 3 != 0)))
                j += 1
    return out


CASES = [c for ksm, nt in NN_PAIRS for c in nn_cases(ksm, nt)] + x3_cases() + x3b_cases()


def case_id(c):
    return f'{c.entry}-{"-".join(map(str, c.sig))}-G{c.G}-Mg{c.Mg}-K{c.K}-N{c.N}-{c.a}-{c.c}'


def a_view(c):
    """(ld, coff, shuffle_ctot) of the operand view"""
    K = c.K
    return {'dense': (K, 0, 0), 'pad': (K + 6, 2, 0), 'pad4': (K + 8, 4, 0), 'split': (2 * K, K, 0), 'odd': (K + 5, 3, 0), 'lo': (2 * K, 0, 2 * K),
            'hi': (2 * K, K, 2 * K)}[c.a]


def c_view(c):
    N = c.N
    return {'dense': (N, 0), 'pad': (N + 4, 2), 'split': (2 * N, N)}[c.c]


def plan_query(lib, c, a_addr=FAKE, y_addr=FAKE):
    """the plan of a case as a dict (entry 'nn' / 'x3' / 'x3b'), and the query's return code"""
    ld, coff, ctot = a_view(c)
    va, vc = _lib.View(a_addr, ld, coff), _lib.View(FAKE, *c_view(c))
    if c.entry == 'nn':
        names, out = R.NN_FIELDS, (C.c_int32 * len(R.NN_FIELDS))()
        rc = lib.cdrl_pwconv_plan(C.byref(va), C.byref(vc), y_addr if c.pro == 2 else 0, c.G, c.Mg, c.N, c.K, c.pro, c.epi, c.acc, c.packed,
                                  int(c.mode > 0), int(c.mode == 2), int(c.epi != 0), out, len(names))
    elif c.entry == 'x3':
        names, out = R.X3_FIELDS, (C.c_int32 * len(R.X3_FIELDS))()
        rc = lib.cdrl_pwconv_x3_plan(C.byref(va), C.byref(vc), c.G, c.Mg, c.N, c.K, c.pro, c.epi, 1, 0, out, len(names))
    else:
        names, out = R.X3B_FIELDS, (C.c_int32 * len(R.X3B_FIELDS))()
        rc = lib.cdrl_pwconv_x3_wide_bwd_plan(C.byref(va), C.byref(vc), c.G, c.Mg, c.N, c.K, ctot, int(c.epi != 0), c.acc, 1, out, len(names))
    return dict(zip(names, out)), rc


def signature(c, p):
    return {'nn': R.nn_signature, 'x3': R.x3_signature, 'x3b': R.x3b_signature}[c.entry](p)


def check_plan(c, p, rc):
    assert rc == 0 and p['ok'] == 1 and p['refusal'] == 0, (case_id(c), p)
    assert signature(c, p) == c.sig, (case_id(c), p)
    if c.entry == 'x3b':
        assert (p['rows'], p['gx'], p['gy']) == (R.cdiv(c.Mg, 32), c.G * R.cdiv(c.Mg, 32), R.cdiv(c.N, 128))
        return
    assert p['nbpg'] >= 1 and p['gx'] == c.G * p['nbpg'] and p['tiles_g'] == R.cdiv(c.Mg, p['bm']) >= p['nbpg']
    if c.entry == 'nn':
        assert p['nbpg'] * p['tpb'] >= p['tiles_g'] > p['nbpg'] * (p['tpb'] - 1) and p['bm'] == bm_of(c.sig[1]) and p['gy'] == R.cdiv(c.N, 128)


def test_coverage(lib):
    """the cases' plans are accepted, land on their signatures, and together are exactly REQUIRED; the edge lists the module promises"""
    have = {'nn': set(), 'x3': set(), 'x3b': set()}
    for c in CASES:
        p, rc = plan_query(lib, c)
        check_plan(c, p, rc)
        have[c.entry].add(signature(c, p))
    assert have['nn'] == REQUIRED and have['x3'] == REQUIRED_X3 and have['x3b'] == REQUIRED_X3B
    nn = [c for c in CASES if c.entry == 'nn']
    for ksm, nt in NN_PAIRS:
        grp = [c for c in nn if c.sig[:2] == (ksm, nt)]
        bm = bm_of(nt)
        assert len(grp) == 30 and {c.Mg for c in grp} == {1, bm - 1, bm, bm + 1, 3 * bm + 5} and {c.K for c in grp} == set(NN_KS[ksm])
        assert {c.N for c in grp if c.mode < 2} == set(NN_NS[nt])
        # G = 128 at 3 bm + 5 rows: four tiles per group, and workgroups with two or more of them wherever the grid target is below four
        big = [plan_query(lib, c)[0] for c in grp if c.G == 128]
        assert len(big) == 1 and all(p['tiles_g'] == 4 for p in big) and all((p['tpb'] >= 2) == (p['nbpg'] < 4) for p in big)
    assert any(p['tpb'] == 2 and p['tiles_g'] % p['nbpg'] for p in (plan_query(lib, c)[0] for c in nn if c.G == 128)), 'no uneven split'
    assert {c.a for c in nn if c.pro == 2} == {'dense', 'odd', 'lo', 'hi', 'pad'}
    x3p = [plan_query(lib, c)[0] for c in CASES if c.entry == 'x3' and c.G == 128]
    assert x3p and all(p['tiles_g'] == 5 and p['nbpg'] == 4 for p in x3p)
    assert {c.Mg for c in CASES if c.entry == 'x3b'} == set(WIDE_MG) == {c.Mg for c in CASES if c.entry == 'x3' and c.sig[0] == 1}


# ---- guarded tensors ---------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


class Banded:
    """A dense tensor inside a larger 1-D one; the bands of `fill` on each side must come back bit-intact."""

    def __init__(self, shape, dtype, fill, data=None):
        n = int(np.prod(shape))
        self.whole = torch.full((BAND + n + BAND,), fill, dtype=dtype, device=DEV)
        self.t = self.whole[BAND:BAND + n].view(*shape)
        if data is not None:
            self.t.copy_(torch.as_tensor(np.asarray(data, np.float64)).to(dtype))
        self.ref = self.whole[:BAND].clone()

    def intact(self):
        return torch.equal(bits(self.whole[:BAND]), bits(self.ref)) and torch.equal(bits(self.whole[-BAND:]), bits(self.ref))

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())


class Framed:
    """M rows x `cols` (column indices inside a row of ld elements) of a [GR + M + GR][ld] tensor filled with `fill`: NaN around an
    input, the sentinel around an output, where everything but the payload must come back bit-intact."""

    def __init__(self, M, ld, cols, dtype, fill, data=None):
        self.whole = torch.full((GR + M + GR, ld), fill, dtype=dtype, device=DEV)
        self.cols = torch.as_tensor(np.asarray(cols), device=DEV)
        self.M, self.dtype = M, dtype
        if data is not None:
            self.set(data)
        self.mask = torch.ones_like(self.whole, dtype=torch.bool)
        self.mask[GR:GR + M, self.cols] = False
        self.before = self.whole.clone()

    def set(self, data):
        self.whole[GR:GR + self.M, self.cols] = torch.as_tensor(np.asarray(data, np.float64)).to(self.dtype).to(DEV)

    def get(self):
        return self.whole[GR:GR + self.M, self.cols].double().cpu().numpy()

    def intact(self):
        return torch.equal(bits(self.whole)[self.mask], bits(self.before)[self.mask])

    def view(self, coff):
        return _lib.View(self.whole[GR].data_ptr(), self.whole.shape[1], coff)


def rng_of(c, exact):
    return np.random.default_rng(zlib.crc32(repr((c, exact)).encode()))


def run_case(lib, c, exact, mode=None, inp=None):
    """One case on the device, twice (the second time on the dirty partial buffers).  Returns the inputs, the stored output
    [M][N] float64, the partial sums [G][2][N] and [G][K] (or None) and the plan."""
    mode = c.mode if mode is None else mode
    G, Mg, K, N, M = c.G, c.Mg, c.K, c.N, c.G * c.Mg
    p, rc = plan_query(lib, c._replace(mode=mode, sig=c.sig[:4] + (mode, c.sig[5])) if c.entry == 'nn' else c)
    assert rc == 0, (case_id(c), p)
    r = inp or R.draw(rng_of(c, exact), G, Mg, K, N, c.pro, c.epi, c.acc, exact, bf16=c.mode == 2, relu6=bool(c.relu6))
    td = BF if mode == 2 else torch.float32
    f32t = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(DEV)      # noqa: E731
    ld, coff, ctot = a_view(c)
    A = Framed(M, ld, R.view_cols(coff, K, ctot), td, float('nan'), r.a)
    cld, ccoff = c_view(c)
    Cf = Framed(M, cld, ccoff + np.arange(N), td, SENTINEL, r.base)
    y = Banded((M, K), td, float('nan'), r.y) if c.pro == 2 else None
    ey = Banded((M, N), td, float('nan'), r.ey) if c.epi == 2 else None
    stats, coef, estats, bias = f32t(r.stats), f32t(r.coef), f32t(r.estats), f32t(r.bias)
    nbpg = p['rows'] if c.entry == 'x3b' else p['nbpg']
    part = Banded((G, nbpg, 2, N), torch.float64, float('nan')) if c.epi else None
    part2 = Banded((G, nbpg, K), torch.float64, float('nan')) if c.pro == 2 else None
    w_mem = np.ascontiguousarray(r.w.T if c.wt else r.w, np.float32)          # B(k, n) = w[k * sbk + n * sbn]
    sbk, sbn = (1, K) if c.wt else (N, 1)
    W = f32t(w_mem)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    bptr = lambda b: None if b is None else b.ptr                        # noqa: E731
    wp = None
    if c.entry == 'nn' and (c.packed or mode > 0):
        wp = torch.full((int(lib.cdrl_pwconv_pack_elems(N, K)),), float('nan'), device=DEV)
        assert wp.numel() == p['packed_elems']
        assert lib.cdrl_pwconv_pack(ptr(W), K, N, sbk, sbn, ptr(wp), int(mode > 0), None) == 0, lib.cdrl_last_error()
    elif c.entry != 'nn':
        nbytes = int(lib.cdrl_pwconv_x3_packed_bytes_n(K, N))
        wp = torch.zeros((nbytes // 4,), device=DEV)
        assert lib.cdrl_pwconv_x3_pack(ptr(W), K, N, sbk, sbn, ptr(wp), None) == 0, lib.cdrl_last_error()

    def launch():
        va, vc = A.view(coff), Cf.view(ccoff)
        if c.entry == 'nn':
            return lib.cdrl_pwconv_ex(C.byref(va), ptr(stats), bptr(y), ptr(coef), ctot, c.relu6, bptr(part2), ptr(W), sbk, sbn, ptr(bias), C.byref(vc),
                                      c.acc, G, Mg, N, K, c.epi, bptr(ey), ptr(estats), bptr(part), ptr(wp), int(mode > 0), int(mode == 2), None)
        if c.entry == 'x3':
            return lib.cdrl_pwconv_x3(C.c_void_p(va.p), ld, coff, ptr(stats), ptr(wp), ptr(bias), C.c_void_p(vc.p), cld, ccoff, G, Mg, N, K, bptr(part), None)
        return lib.cdrl_pwconv_x3_wide_bwd(C.c_void_p(va.p), ld, coff, ctot, c.relu6, y.ptr, ptr(stats), ptr(coef), ptr(wp), C.c_void_p(vc.p), cld, ccoff,
                                           c.acc, G, Mg, N, K, part2.ptr, bptr(ey), ptr(estats), bptr(part), None)

    assert launch() == 0, (case_id(c), lib.cdrl_last_error())
    torch.cuda.synchronize()
    first = [Cf.whole.clone()] + [b.whole.clone() for b in (part, part2) if b is not None]
    if c.acc:
        Cf.set(r.base)
    assert launch() == 0, (case_id(c), lib.cdrl_last_error())
    torch.cuda.synchronize()
    second = [Cf.whole] + [b.whole for b in (part, part2) if b is not None]
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, second)), f'{case_id(c)}: the second run differs'
    assert A.intact() and Cf.intact() and all(b.intact() for b in (y, ey, part, part2) if b is not None), f'{case_id(c)}: guard band'
    ps = None if part is None else part.t.double().sum(dim=1).cpu().numpy()
    ps2 = None if part2 is None else part2.t.double().sum(dim=1).cpu().numpy()
    return r, Cf.get(), ps, ps2, p


def reference(c, r, mode):
    """(float64 output, S, a' float32) for the inputs r in compute mode `mode`; x3b has no bias"""
    ap = R.prologue(c.pro, r.a, c.G, c.Mg, r.stats, r.coef, r.y, relu6=bool(c.relu6), bf16=mode > 0)
    apf = ap if mode == 0 else R.prologue(c.pro, r.a, c.G, c.Mg, r.stats, r.coef, r.y, relu6=bool(c.relu6))
    c64, s = R.product(ap, r.w, None if c.entry == 'x3b' else r.bias, r.base, bf16=mode > 0)
    return c64, s, apf


def check_partials(c, r, stored, ps, ps2, apf):
    """statistics / BatchNorm-sum partials against float64 sums of the stored values; column sums of the transformed operand"""
    close = lambda a, b: np.allclose(a, b, rtol=1e-9, atol=1e-6)        # noqa: E731
    if c.epi:           # (cases with an epilogue do not accumulate: the stored values are the summed ones)
        want = R.stats_partials(stored, c.G, c.Mg) if c.epi == 1 else R.bnred_partials(stored, r.ey, r.estats, c.G, c.Mg)
        assert close(ps, want), (case_id(c), float(np.abs(ps - want).max()))
    if c.pro == 2:
        want2 = apf.astype(np.float64).reshape(c.G, c.Mg, c.K).sum(axis=1)
        assert close(ps2, want2), (case_id(c), float(np.abs(ps2 - want2).max()))


WORST = {}


def check_case(lib, c):
    x3 = c.entry != 'nn'
    # small integers: the exact value (bf16 storage: its bf16 rounding)
    r, out, ps, ps2, _ = run_case(lib, c, True)
    assert R.exact_condition(r, bf16=c.mode > 0), case_id(c)
    c64, _, apf = reference(c, r, c.mode)
    want = R.bf(c64) if c.mode == 2 else c64
    assert np.array_equal(out, want), (case_id(c), float(np.abs(out - want).max()))
    check_partials(c, r, c64 if c.epi == 2 else out, ps, ps2, apf)
    # standard normal: every element within the bound of the float64 product
    r, out, ps, ps2, _ = run_case(lib, c, False)
    c64, s, apf = reference(c, r, c.mode)
    stored = out
    if c.mode == 2:     # bit for bit the bf16 rounding of the float32-tensor form on the widened inputs
        out = run_case(lib, c, False, mode=1, inp=r)[1]
        assert np.array_equal(stored, R.bf(out)), (case_id(c), float(np.abs(stored - R.bf(out)).max()))
    lim = R.bound(c.K, s, x3=x3)
    ratio = float((np.abs(out - c64) / np.maximum(lim, 1e-300)).max())
    key = ('x3' if x3 else 'f32' if c.mode == 0 else 'bf16', c.K)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= 1.0, (case_id(c), ratio)
    # (bf16 storage: the statistics epilogue sums the rounded values it stores, the BatchNorm-sum epilogue the float32 values in front of
    #  the storage rounding -- those the float32-tensor form stores)
    check_partials(c, r, out if c.epi == 2 else stored, ps, ps2, apf)


@pytest.mark.parametrize('pair', NN_PAIRS, ids=lambda p: f'ksm{p[0]}-nt{p[1]}')
def test_pw_nn(lib, pair):
    """the 30 instantiations of one (KSM, NT) pair"""
    for c in nn_cases(*pair):
        check_case(lib, c)
    print('worst |error| / bound so far:', {k: round(v, 4) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize('form', (0, 1), ids=('persistent', 'wide'))
def test_pw_x3(lib, form):
    for c in x3_cases():
        if c.sig[0] == form:
            check_case(lib, c)
    print('worst |error| / bound so far:', {k: round(v, 4) for k, v in sorted(WORST.items())})


def test_pw_x3_wide_bwd(lib):
    for c in x3b_cases():
        check_case(lib, c)
    print('worst |error| / bound so far:', {k: round(v, 4) for k, v in sorted(WORST.items())})


def test_refusals_launch_nothing(lib):
    """what the plans refuse is refused by the entries, in the plan's words, with the output untouched"""
    c = nn_cases(16, 1)[0]._replace(G=2, Mg=5, K=32, N=32, a='dense', c='dense')
    out = torch.full((10, 32), SENTINEL, device=DEV)
    a = torch.zeros((10, 32), device=DEV)
    w = torch.zeros((32, 32), device=DEV)
    va, vc = _lib.View(a.data_ptr(), 32, 0), _lib.View(out.data_ptr(), 32, 0)
    call = lambda G, Mg, K, epi: lib.cdrl_pwconv_ex(C.byref(va), None, None, None, 0, 0, None, C.c_void_p(w.data_ptr()), 32, 1, None, C.byref(vc), 0, G, Mg,      # noqa: E731
                                                    32, K, epi, None, None, None, None, 0, 0, None)
    for args, word in (((0, 5, 32, 0), b'nothing to launch'), ((2, 0, 32, 0), b'nothing to launch'), ((2, 5, 0, 0), b'column pair'),
                       ((2, 5, 31, 0), b'not supported'), ((2, 5, 32, 1), b'partial buffer')):
        assert call(*args) == -1 and word in lib.cdrl_last_error(), (args, lib.cdrl_last_error())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and plan_query(lib, c)[1] == 0
