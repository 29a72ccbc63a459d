"""The 1x1-conv forward / backward-data family (csrc/gemm_pw.hip: pw_nn; csrc/gemm_pw_x3.hip: pw_x3, pw_x3_wide_bwd) -- shared by
tests/test_pw_plan_host.py and tests/test_gpu_pw_variants.py.  numpy only.

Part 1 restates the host dispatch as the commit before the plan structs had it (pw_nn_supported / pw_nn_plan / the four-level launch
ladder / launch_pw_bf's LDS size; pw_x3_supported / pw_x3_partial_rows / the CDRL_X3 ladder; pw_x3_wide_bwd_supported), from that
source and as tables, not as the new code's control flow.  The refusals that commit did not have -- G, Mg, N < 1 and K < 2, which
reached a zero-sized or meaningless launch -- are marked NEW.

Part 2 is the float64 reference of the op, written from the definitions:
    C[m, n] (+)= sum_k a'[m, k] W[k, n] + bias[n]          rows of group g contiguous, G groups of Mg rows
    prologue 0: a' = A;   1: a' = scale[g, k] A + shift[g, k] (one float32 rounding: fmaf);
             2: a' = k1 (mask dz - k2 - xhat(y) k3) -- the BatchNorm-backward apply, evaluated in float32 step by step as written
                (the kernels are built without contraction), dz optionally gathered through the channel shuffle
    epilogue 1: per group (sum c, sum c^2);   2: (sum c, sum c xhat(ey)) with xhat = (ey - mean) * invstd in float32
    modes 1 / 2: a' and W enter the product rounded to bf16.
Nothing here follows a kernel's loop structure."""
from types import SimpleNamespace

import numpy as np

from tests.pw_ref import F32, F64, bf, shuffle_map, stats_of, view_cols  # noqa: F401  (re-exported)

U = 2.0 ** -24                  # unit roundoff of float32


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- part 1: dispatch
# pw_nn_kernel<KSM, NT, PRO, EPI, MODE, ACC>: the (KSM, NT) pairs the ladder instantiates, the prologue / epilogue pairs, ACC for EPI 0
NN_PAIRS = ((16, 1), (16, 2), (16, 3), (16, 4), (32, 1), (32, 2), (32, 3), (32, 4), (64, 1), (64, 2), (64, 4), (128, 4))
NN_PRO_EPI = ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0), (2, 2))
NN_ONE_PER_CU = ((32, 3), (64, 1), (64, 2), (128, 4))          # __launch_bounds__(256, 1): more than 256 VGPRs
NN_REFUSALS = dict(dims=1, shape=2, tile=3, align=4, pro_epi=5, part=6, big=7, storage=8)
X3_REFUSALS = dict(dims=1, shape=2, align=3, packed=4, big=5, nbpg=6)
X3B_REFUSALS = dict(dims=1, shape=2, align=3, operands=4, epi_acc=5, big=6)
NN_FIELDS = ('ok', 'refusal', 'ksm', 'nt', 'pro', 'epi', 'mode', 'acc', 'wc', 'wr', 'bm', 'tiles_g', 'nbpg', 'tpb', 'gx', 'gy', 'occ', 'lds_bytes',
             'packed_elems')
X3_FIELDS = ('ok', 'refusal', 'form', 'kp', 'nt', 'pro', 'epi', 'bm', 'tiles_g', 'nbpg', 'gx', 'gy', 'packed_bytes')
X3B_FIELDS = ('ok', 'refusal', 'sh', 'epi', 'acc', 'rows', 'gx', 'gy')


def nn_ksm(K):
    """K pairs padded to 16, 32, 64 or 128"""
    return next(k for k in (16, 32, 64, 128) if 2 * k >= K or k == 128)


def nn_geometry(G, Mg, N, K):
    """pw_nn_plan of that commit (bm, tpb, nbpg) with the numbers it derived on the way"""
    nt, ksm = (4 if N > 128 else cdiv(N, 32)), nn_ksm(K)
    wc = 1 if nt == 3 else nt
    wr = 4 // wc
    bm = 32 * wr
    tiles = cdiv(Mg, bm)
    occ = 1 if (ksm, nt) in NN_ONE_PER_CU or ksm == 128 else (3 if ksm <= 32 and nt != 1 else 2)
    gy = cdiv(N, 128)
    nbpg = min(tiles, max(1, 256 * occ // (G * gy)))
    return dict(ksm=ksm, nt=nt, wc=wc, wr=wr, bm=bm, tiles_g=tiles, nbpg=nbpg, tpb=cdiv(tiles, nbpg), gx=G * nbpg, gy=gy, occ=occ)


def nn_lds_bytes(ksm, nt, pro):
    """launch_pw_bf: the A tile (+ 14 KSM floats of coefficients under the BatchNorm-backward prologue), no less than the epilogue's
    [WR][2][32 NT] doubles and the 512 doubles of the column-sum scratch"""
    wr = 4 // (1 if nt == 3 else nt)
    return max(4 * (32 * wr * (2 * ksm + 2) + (14 * ksm if pro == 2 else 0)), 8 * wr * 2 * 32 * nt, 8 * 512)


def nn_expected(G, Mg, N, K, pro, epi, acc, packed, packed_bf16, at, has_part, a_addr, a_ld, a_coff, y_addr=0):
    """The plan cdrl_pwconv_plan must report: the reasons to refuse in the order the new plan checks them (that commit's own order
    behind the NEW ones), and the fields"""
    p = dict.fromkeys(NN_FIELDS, 0)
    p.update(pro=pro, epi=epi, mode=2 if at else int(bool(packed and packed_bf16)), acc=int(bool(acc) and epi == 0))
    why = []
    if G < 1 or Mg < 1 or N < 1:
        why.append('dims')                              # NEW
    else:
        g = nn_geometry(G, Mg, N, K)
        p.update(g, lds_bytes=nn_lds_bytes(g['ksm'], g['nt'], pro), packed_elems=cdiv(N, 32) * 2 * 32 * g['ksm'])
        if K < 2:
            why.append('dims')                          # NEW
        if K > 256 or N > 256 or K % 2:
            why.append('shape')
        if (g['ksm'], g['nt']) not in NN_PAIRS:
            why.append('tile')
        # that commit held the operand view to 8 bytes -- under the BatchNorm-backward prologue a dense view of y instead (the dz view
        # is not looked at: the kernel decides per launch whether it can load pairs)
        addr, ld, coff = (y_addr, K, 0) if pro == 2 else (a_addr, a_ld, a_coff)
        if ld % 2 or coff % 2 or addr % 8:
            why.append('align')
        if epi != 0 and not has_part:
            why.append('part')
        if G * Mg * a_ld * 4 >= 2 ** 31 or G * Mg * K * 4 >= 2 ** 31:
            why.append('big')
        if at and not (packed and packed_bf16):
            why.append('storage')
        if (pro, epi) not in NN_PRO_EPI:
            why.append('pro_epi')
    p['ok'], p['refusal'] = int(not why), (NN_REFUSALS[why[0]] if why else 0)
    return p, why


def nn_signature(p):
    return (p['ksm'], p['nt'], p['pro'], p['epi'], p['mode'], p['acc'])


def x3_expected(G, Mg, N, K, pro, epi, packed, nbpg, a_addr, a_ld, a_coff):
    """pw_x3 of that commit: pw_x3_supported's two clauses (the first for K, N <= 128, the second for everything up to 256), the wide
    form for K or N above 128, pw_x3_partial_rows; NEW: dims, and a caller's nbpg beyond the tile count (that commit launched
    workgroups without a tile)"""
    p = dict.fromkeys(X3_FIELDS, 0)
    wide = K > 128 or N > 128
    kp = 256 if wide else next(k for k in (32, 64, 128, 256) if k >= K or k == 256)
    nt = 4 if wide or N > 64 else (1 if N <= 32 else 2)
    blocks = cdiv(N, 128) if wide else 1
    p.update(form=int(wide), kp=kp, nt=nt, pro=int(pro), epi=int(epi), packed_bytes=3 * (kp // 16) * 2 * 128 * 8 * 2 * blocks)
    why = []
    if G < 1 or Mg < 1 or N < 1:
        return dict(p, refusal=X3_REFUSALS['dims']), ['dims']       # NEW
    bm = 32 if wide else 32 * (4 // nt)
    tiles = cdiv(Mg, bm)
    own = tiles if wide else min(tiles, max(1, 512 // G))
    p.update(bm=bm, tiles_g=tiles, nbpg=own, gx=G * own, gy=blocks)
    clause1 = 4 <= K <= 128 and 1 <= N <= 128 and K % 2 == 0
    clause2 = 4 <= K <= 256 and 1 <= N <= 256 and K % 4 == 0
    al1, al2 = a_ld % 2 == 0 and a_coff % 2 == 0 and a_addr % 16 == 0, a_ld % 4 == 0 and a_coff % 4 == 0 and a_addr % 16 == 0
    if not (clause1 or clause2):
        why.append('shape')
    elif not ((clause1 and al1) or (clause2 and al2)):
        why.append('align')
    if not packed:
        why.append('packed')
    if G * Mg * a_ld * 4 >= 2 ** 31:
        why.append('big')
    if nbpg > 0:
        if (wide and nbpg != tiles) or nbpg > tiles:
            why.append('nbpg')
        elif not why:
            p.update(nbpg=nbpg, gx=G * nbpg)
    p['ok'], p['refusal'] = int(not why), (X3_REFUSALS[why[0]] if why else 0)
    return p, why


def x3_signature(p):
    return (p['form'], p['kp'], p['nt'], p['pro'], p['epi'])


def x3b_expected(G, Mg, N, K, shuffle_ctot, epi, acc, operands, dz_addr, dz_ld, dz_coff, c_ld):
    p = dict.fromkeys(X3B_FIELDS, 0)
    p.update(sh=int(shuffle_ctot != 0), epi=int(epi), acc=int(acc != 0), rows=cdiv(Mg, 32))
    if G < 1 or Mg < 1:
        return dict(p, refusal=X3B_REFUSALS['dims']), ['dims']      # NEW
    p.update(gx=G * p['rows'], gy=cdiv(N, 128))
    why = []
    if not (K > 128 or N > 128) or K > 256 or N > 256 or K % 4:
        why.append('shape')
    if dz_addr % 16 or dz_ld % 2 or ((dz_coff % 2 or (shuffle_ctot // 2) % 2) if shuffle_ctot else (dz_ld % 4 or dz_coff % 4)):
        why.append('align')
    if not operands:
        why.append('operands')
    if epi and acc:
        why.append('epi_acc')
    if G * Mg * max(dz_ld, K, c_ld) * 4 >= 2 ** 31:
        why.append('big')
    p['ok'], p['refusal'] = int(not why), (X3B_REFUSALS[why[0]] if why else 0)
    return p, why


def x3b_signature(p):
    return (p['sh'], p['epi'], p['acc'])


# ---------------------------------------------------------------------------------------------------------------- part 2: the op
def f32(x):
    return np.asarray(x, F32)


def fma32(a, b, c):
    """fmaf on float32 arrays: the float64 product of two float32 numbers is exact, the sum is rounded twice only where the float64 sum
    is inexact AND lands on a float32 tie -- pw_ref's ReLU6 rule covers the one place that matters (the mask, below)"""
    return (f32(a).astype(F64) * f32(b).astype(F64) + f32(c).astype(F64)).astype(F32)


def relu6_mask(y, scale, shift):
    """open where 0 < z < 6, z = fmaf(scale, y, shift): decided on the float32 value wherever the float64 value lies within 1e-4 of a
    kink, in float64 elsewhere (tests/pw_ref.py)"""
    z64 = f32(scale).astype(F64) * f32(y).astype(F64) + f32(shift).astype(F64)
    z32 = z64.astype(F32)
    near = np.abs(z64 - np.round(z64 / 6.0) * 6.0) <= 1e-4
    return np.where(near, (z32 > 0) & (z32 < 6), (z64 > 0) & (z64 < 6))


def rows_of(v, Mg):
    """[G][C] -> [G * Mg][C]"""
    return np.repeat(np.asarray(v), Mg, axis=0)


def prologue(pro, a, G, Mg, stats=None, coef=None, y=None, relu6=False, bf16=False):
    """a' as float32 [G*Mg][K] the way the kernels form it (see the module docstring); `a` is A, or the LOGICAL dz columns"""
    a = f32(a)
    if pro == 1:
        a = fma32(rows_of(stats[2], Mg), a, rows_of(stats[3], Mg))
    elif pro == 2:
        y = f32(y)
        mean, inv, sc, sh = (rows_of(f32(stats[i]), Mg) for i in range(4))
        k1, k2, k3 = (rows_of(f32(coef[i]), Mg) for i in range(3))
        d = np.where(relu6_mask(y, sc, sh), a, F32(0)) if relu6 else a
        xh = (y - mean) * inv
        a = k1 * ((d - k2) - xh * k3)
    return a if not bf16 else bf(a).astype(F32)


def product(ap, w, bias=None, base=None, bf16=False):
    """(C, S): the float64 product of the float32 a' and W (+ bias, + the old output) and S = sum |a'| |w| (+ |bias| + |base|)"""
    a64, w64 = f32(ap).astype(F64), (bf(w) if bf16 else f32(w).astype(F64))
    c, s = a64 @ w64, np.abs(a64) @ np.abs(w64)
    for t in (bias, base):
        if t is not None:
            c, s = c + np.asarray(t, F64), s + np.abs(np.asarray(t, F64))
    return c, s


def stats_partials(c_stored, G, Mg):
    """epilogue 1 from the values the kernel stored: [G][2][N]"""
    c = np.asarray(c_stored, F64).reshape(G, Mg, -1)
    return np.stack([c.sum(axis=1), (c * c).sum(axis=1)], axis=1)


def bnred_partials(c_stored, ey, estats, G, Mg):
    """epilogue 2: (sum c, sum c xhat(ey)), xhat in float32 as the kernel forms it"""
    xh = ((f32(ey) - rows_of(f32(estats[0]), Mg)) * rows_of(f32(estats[1]), Mg)).astype(F64).reshape(G, Mg, -1)
    c = np.asarray(c_stored, F64).reshape(G, Mg, -1)
    return np.stack([c.sum(axis=1), (c * xh).sum(axis=1)], axis=1)


def bound(K, s, x3=False, extra=0):
    """Per-element bound on |c - float64|, in units of S.  Float32 MFMA chain and bf16-operand chain: the products are exact or rounded
    once, every one of the K accumulations rounds once, each against a partial sum no larger than S: (1 + u)^K - 1 <= K u (1 + K u)
    -- K u plus a second-order term below u for K <= 256.  c = 3: that second-order unit, the bias add, the accumulate add.
    x3 (csrc/mfma_x3.h): each operand is the sum of three bf16 numbers up to a last rounding below u (2 u for the pair of operands),
    three of the nine plane products are dropped (2^-24 + 2^-24 + 2^-32 of the product: 2 u + 2^-8 u), the six kept ones are exact
    and go through 6 K accumulations; c = 3 + 5."""
    n_acc = 6 * K if x3 else K
    return (n_acc + 3 + (5 if x3 else 0) + extra) * U * np.asarray(s, F64)


def draw(rng, G, Mg, K, N, pro, epi, acc, exact, bf16=False, relu6=True):
    """One case's logical tensors.  exact: small integers (products and sums exact in float32, prologue coefficients powers of two,
    everything representable in bf16); else standard normal (bf16: rounded to it where the tensors are stored as bf16)."""
    M = G * Mg
    r = SimpleNamespace(G=G, Mg=Mg, K=K, N=N, pro=pro, epi=epi, acc=acc, stats=None, coef=None, y=None, ey=None, estats=None, base=None, relu6=relu6)
    q = (lambda x: bf(x).astype(F32)) if bf16 else f32
    if exact:
        ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(F32)      # noqa: E731
        pow2 = lambda shape: (2.0 ** rng.integers(-1, 2, shape)).astype(F32)           # noqa: E731
        r.a, r.w, r.bias = ints(-3, 3, (M, K)), ints(-2, 2, (K, N)), ints(-8, 8, N)
        if pro == 1:        # a' = 2^e a + integer: |a'| <= 6 + 4
            r.stats = np.stack([np.zeros((G, K), F32), np.ones((G, K), F32), pow2((G, K)), ints(-4, 4, (G, K))])
        if pro == 2:        # xhat = (y - mean) * 2^e, a' = 2^e ((dz - k2) - xhat k3): integers / 4, |a'| <= 2 (3 + 2 + 4 * 2 * 2) = 42
            r.y = ints(-2, 2, (M, K))
            r.stats = np.stack([ints(-2, 2, (G, K)), pow2((G, K)), pow2((G, K)), ints(-1, 7, (G, K)) * F32(0.5)])
            r.coef = np.stack([pow2((G, K)), ints(-2, 2, (G, K)), ints(-2, 2, (G, K))])
        if epi == 2:
            r.ey, r.estats = ints(-3, 3, (M, N)), np.stack([ints(-2, 2, (G, N)), pow2((G, N)), np.ones((G, N), F32), np.zeros((G, N), F32)])
        if acc:
            r.base = ints(-64, 64, (M, N))
    else:
        r.a, r.w, r.bias = q(rng.standard_normal((M, K))), f32(rng.standard_normal((K, N))), f32(rng.standard_normal(N))
        if pro == 1:
            r.stats = np.stack([f32(rng.standard_normal((G, K))), f32(rng.uniform(0.5, 2, (G, K))), f32(rng.uniform(0.5, 2, (G, K))),
                                f32(rng.standard_normal((G, K)))])
        if pro == 2:
            r.y = q(rng.standard_normal((M, K)) * 2 + 1)
            r.stats = stats_of(r.y, rng.uniform(0.5, 1.5, K).astype(F32), rng.uniform(1.0, 3.0, K).astype(F32), G, Mg)
            r.coef = np.stack([r.stats[2], f32(rng.uniform(-0.3, 0.3, (G, K))), f32(rng.uniform(-0.3, 0.3, (G, K)))])
        if epi == 2:
            r.ey = q(rng.standard_normal((M, N)))
            r.estats = np.stack([f32(rng.standard_normal((G, N)) * 0.1), f32(rng.uniform(0.5, 2, (G, N))), np.ones((G, N), F32), np.zeros((G, N), F32)])
        if acc:
            r.base = q(rng.standard_normal((M, N)))
    return r


def exact_condition(r, bf16=False):
    """every product and partial sum of the integer case is a multiple of 2^-4 below 2^24 * 2^-4, and (bf16) a' and W are bf16 numbers"""
    ap = prologue(r.pro, r.a, r.G, r.Mg, r.stats, r.coef, r.y, relu6=r.relu6)
    _, s = product(ap, r.w, r.bias, r.base)
    fine = np.all(ap.astype(F64) * 16 == np.round(ap.astype(F64) * 16)) and s.max() * 16 < 2 ** 24
    return bool(fine and (not bf16 or (np.array_equal(bf(ap), ap.astype(F64)) and np.array_equal(bf(r.w), r.w.astype(F64)))))
