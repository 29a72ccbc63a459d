"""Plain float64 reference of the filter-gradient GEMM family (csrc/gemm_tn_direct.hip, csrc/gemm_tn_lds.hip; cdrl_gemm_tn_ex) and of its
partial reduce (csrc/gemm.hip; cdrl_reduce_partials_f32), written from the contract -- shared by tests/test_gpu_tn_variants.py and
tests/test_gemm_tn_plan_host.py.  numpy only; nothing here follows a kernel's loop structure.

The op, rows of group g contiguous (rows [g*Mg, (g+1)*Mg)):
    W[k][n] = sum_m a'[m][k] d'[m][n]
    a' = scale[g][k] a + shift[g][k]                         (A prologue: rows 2 and 3 of the statistics block ast [4][G][K]), or a
    d' = k1 (mask dz - k2 - xhat(y) k3)                      (D prologue), or d
         xhat(y) = (y - mean) invstd from yst [4][G][N], k1..k3 = coef [3][G][N], dz = the view d (plain or through the channel shuffle:
         the caller lays the logical columns out), mask = ReLU6 open at z = fmaf(scale, y, shift) evaluated in float32 as every engine
         kernel does (float64 product of two float32 numbers, rounded once: tests/util.py::engine_decisions builds it the same way).
Next to W the reference returns the magnitude matrix S = |a'|^T D^, D^ = |k1| (|mask dz| + |k2| + |xhat k3|) (or |d|): what the terms of
an output element add up to before anything cancels -- the scale of its rounding errors.

bf16 operands: the prologues run in float32, then both operands are rounded to bf16 (nearest even); products and sums are exact.  The
float32 prologue values are reproduced here: a' is one fused multiply-add; d' is (y - mean) invstd, dz - k2, then either a rounded
product and a subtraction or one fused multiply-subtract (a compiler may contract it), then the product with k1.  An operand is FLAGGED
when its float32 value, in either evaluation, lies within one float32 ulp of the midpoint of two bf16 numbers, or the two evaluations
round to different bf16 numbers: the kernel may round such an operand the other way.  `allow` holds 2^-8 |a'| |d'| summed over the
flagged pairs of every output element, `flagged_share` the share of output elements with such a pair.  Operands that reach the rounding
without arithmetic (no prologue) round the same way everywhere and are never flagged."""
from types import SimpleNamespace

import numpy as np

from tests.bn_ref import F32, shuffle_map, to_bf16, view_cols  # noqa: F401  (re-exported for the test modules)

F64 = np.float64


def bf(x):
    """round to bf16 (nearest even), widened to float64"""
    return to_bf16(np.asarray(x, F32)).astype(F64)


def rows(v, Mg):
    """[G][C] -> [G*Mg][C]"""
    return np.repeat(np.asarray(v), Mg, axis=0)


def draw(rng, G, Mg, K, N, apro, dpro, relu, bf16_storage=False):
    """Inputs of one case.  a [M][K], d [M][N] (logical columns), y [M][N] float32 (bf16 values under bf16 storage); ast [4][G][K],
    yst [4][G][N], coef [3][G][N] float32.  Scales have both signs; z = scale y + shift crosses both ReLU6 kinks; k2 / k3 are generic
    (not the means a true finalize would give: every term of the prologue carries weight)."""
    M = G * Mg
    q = (lambda v: to_bf16(v.astype(F32))) if bf16_storage else (lambda v: v.astype(F32))
    a = q(rng.standard_normal((M, K)) * rng.uniform(0.5, 2.0, K) + rng.uniform(-1, 1, K))
    d = q(rng.standard_normal((M, N)) * rng.uniform(0.5, 2.0, N))
    y = q(rng.standard_normal((M, N)) * 1.5 + 0.4)
    sgn = lambda shape: rng.choice([-1.0, 1.0], shape)     # noqa: E731
    ast = np.stack([rng.uniform(-1, 1, (G, K)), rng.uniform(0.5, 2, (G, K)), rng.uniform(0.5, 1.5, (G, K)) * sgn((G, K)),
                    rng.uniform(-0.5, 0.5, (G, K))]).astype(F32)
    mean, inv = rng.uniform(0.1, 0.7, (G, N)), rng.uniform(0.5, 0.8, (G, N))
    sc = rng.uniform(1.0, 3.0, (G, N)) * inv * sgn((G, N))
    yst = np.stack([mean, inv, sc, rng.uniform(1.0, 4.0, (G, N)) - mean * sc]).astype(F32)
    coef = np.stack([yst[2], rng.uniform(-0.4, 0.4, (G, N)), rng.uniform(-0.4, 0.4, (G, N))]).astype(F32)
    return SimpleNamespace(G=G, Mg=Mg, K=K, N=N, apro=apro, dpro=dpro, relu=relu, a=a, d=d, y=y, ast=ast, yst=yst, coef=coef)


def mask_of(inp):
    """ReLU6 open, decided on the float32 fmaf(scale, y, shift)"""
    if not (inp.dpro and inp.relu):
        return np.ones(inp.d.shape, bool)
    z = (rows(inp.yst[2], inp.Mg).astype(F64) * inp.y.astype(F64) + rows(inp.yst[3], inp.Mg).astype(F64)).astype(F32)
    return (z > 0) & (z < 6)


def operands64(inp):
    """(a', d', D^) in float64"""
    Mg = inp.Mg
    a = inp.a.astype(F64)
    if inp.apro:
        a = rows(inp.ast[2], Mg).astype(F64) * a + rows(inp.ast[3], Mg).astype(F64)
    d = inp.d.astype(F64)
    if not inp.dpro:
        return a, d, np.abs(d)
    dz = d * mask_of(inp)
    xh = (inp.y.astype(F64) - rows(inp.yst[0], Mg).astype(F64)) * rows(inp.yst[1], Mg).astype(F64)
    k1, k2, k3 = (rows(inp.coef[i], Mg).astype(F64) for i in range(3))
    return a, k1 * (dz - k2 - xh * k3), np.abs(k1) * (np.abs(dz) + np.abs(k2) + np.abs(xh * k3))


def _near_tie(x32):
    """float32 values within one float32 ulp of the midpoint of two bf16 numbers (low 16 bits 0x7fff, 0x8000 or 0x8001)"""
    low = np.ascontiguousarray(x32, F32).view(np.uint32) & 0xFFFF
    return (low >= 0x7FFF) & (low <= 0x8001)


def operands32(inp):
    """the float32 prologue values as the kernels compute them, and the flags: (a' float32, flagged a, d' float32, flagged d)"""
    Mg = inp.Mg
    a = inp.a
    fa = np.zeros(a.shape, bool)
    if inp.apro:
        a = (rows(inp.ast[2], Mg).astype(F64) * a.astype(F64) + rows(inp.ast[3], Mg).astype(F64)).astype(F32)       # fmaf
        fa = _near_tie(a)
    d = inp.d
    fd = np.zeros(d.shape, bool)
    if inp.dpro:
        dz = np.where(mask_of(inp), d, F32(0))
        xh = ((inp.y - rows(inp.yst[0], Mg)).astype(F32) * rows(inp.yst[1], Mg)).astype(F32)
        k1, k2, k3 = (rows(inp.coef[i], Mg) for i in range(3))
        t = (dz - k2).astype(F32)
        v1 = (t - (xh * k3).astype(F32)).astype(F32)                                        # rounded product, then the subtraction
        v2 = (t.astype(F64) - xh.astype(F64) * k3.astype(F64)).astype(F32)                  # one fused multiply-subtract
        d, d2 = (k1 * v1).astype(F32), (k1 * v2).astype(F32)
        fd = _near_tie(d) | _near_tie(d2) | (to_bf16(d) != to_bf16(d2))
    return a, fa, d, fd


def evaluate(inp, bf16_operands=False):
    """W [K][N], S [K][N] in float64.  bf16 operands: of the rounded operands, with `allow` [K][N] and `flagged_share`."""
    r = SimpleNamespace(allow=0.0, flagged_share=0.0)
    if not bf16_operands:
        a, d, dh = operands64(inp)
        r.w, r.S = a.T @ d, np.abs(a).T @ dh
        return r
    a32, fa, d32, fd = operands32(inp)
    a, d = bf(a32), bf(d32)
    r.w, r.S = a.T @ d, np.abs(a).T @ np.abs(d)
    r.allow = 2.0 ** -8 * ((np.abs(a) * fa).T @ np.abs(d) + np.abs(a).T @ (np.abs(d) * fd))
    hit = (fa.astype(F64).T @ np.ones(d.shape) + np.ones(a.shape).T @ fd.astype(F64)) > 0
    r.flagged_share = float(hit.mean())
    return r


def draw_clean(key, G, Mg, K, N, apro, dpro, relu, bf16_storage, bf16_operands, rounds=50):
    """draw() from the seed `key`; for bf16 operands behind a prologue the flagged elements (their a, or their d and y) are then drawn
    again until none is left: the inputs are CHOSEN such that no operand can round either way.  Returns (inputs, reference, rng) -- the
    rng goes on to draw the accumulate base."""
    rng = np.random.default_rng(list(key))
    inp = draw(rng, G, Mg, K, N, apro, dpro, relu, bf16_storage)
    if bf16_operands and (apro or dpro):
        q = (lambda v: to_bf16(v.astype(F32))) if bf16_storage else (lambda v: v.astype(F32))
        for _ in range(rounds):
            _, fa, _, fd = operands32(inp)
            if not fa.any() and not fd.any():
                break
            inp.a[fa] = q(rng.standard_normal(int(fa.sum())) * 1.3 + 0.2)
            inp.d[fd] = q(rng.standard_normal(int(fd.sum())) * 1.3)
            inp.y[fd] = q(rng.standard_normal(int(fd.sum())) * 1.5 + 0.4)
    return inp, evaluate(inp, bf16_operands), rng


# ---- the partial reduce -------------------------------------------------------------------------------------------------------------
def draw_partials(rng, nparts, n, stride):
    """[nparts][stride] float32, multiples of 2^-10 below 2^8: any double sum of up to 2^27 of them is exact in every order"""
    return (rng.integers(-(1 << 18) + 1, 1 << 18, (nparts, stride)).astype(F64) * 2.0 ** -10).astype(F32)


def reduce_ref(part, n, base=None):
    """float32(sum_p part[p][:n]) -- with a base: float32(base + float32(sum))"""
    s = part[:, :n].astype(F64).sum(axis=0).astype(F32)
    return s if base is None else (base.astype(F64) + s.astype(F64)).astype(F32)
