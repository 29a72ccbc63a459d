"""Plain float64 reference of the fused 1x1-conv backward (csrc/gemm_pw_bwd.hip: cdrl_pwconv_bwd_fused / cdrl_pwconv_bwd_fused_fin),
written from the definitions -- shared by tests/test_gpu_pw_bwd_variants.py and tests/test_pw_bwd_plan_host.py.  numpy only; nothing here
follows a kernel's loop structure.

The op, for y = a W + b followed by a train-mode BatchNorm (+ ReLU6) whose output gradient is dz (core/architectures.py:130-141 under
autograd), rows of group g contiguous:
    dy = k1 (mask dz - k2 - xhat(y) k3)          k1 = the BatchNorm's scale row, k2 = mean(mask dz), k3 = mean(mask dz xhat(y))
    da = dy W^T,   dW = a^T dy,   db = column sums of dy
ANORM (a_stats): a = gamma xhat(x) + beta is itself a BatchNorm output applied on load; the op then also returns that BatchNorm's backward
sums: a_dbeta = sum da, a_dgamma = sum da xhat(x), a_coef = [scale row, sum_g da / Mg, sum_g da xhat / Mg].
Finalize-on-load: k2 / k3 are not given but folded from per-chunk sums [G][fin_nb][2][N] (sum mask dz, sum mask dz xhat(y)), and
o_dbeta / o_dgamma = their totals over chunks and groups.

ReLU6: the mask is decided on z = fmaf(scale, y, shift) in float32 (the expression the kernels evaluate) wherever the float64 value lies
within 1e-4 of a kink, in float64 elsewhere; no element is excluded from any comparison.

bf16 storage (`bf16=True`): x, y, dz hold bf16 values; the prologue runs in float32; dy, xhat(x) (or x) and W enter the products rounded
to bf16, products and sums are exact; the ANORM sums are those of the resulting da against the ROUNDED xhat."""
from types import SimpleNamespace

import numpy as np

from tests.bn_ref import EPS, F32, shuffle_map, to_bf16, view_cols  # noqa: F401  (re-exported for the test modules)

F64 = np.float64


def bf(x):
    """round to bf16 (nearest even), widened to float64"""
    return to_bf16(np.asarray(x, F32)).astype(F64)


def _rows(v, Mg):
    """[G][C] -> [G][1][C] float64"""
    return np.asarray(v, F64)[:, None, :]


def stats_of(v, gamma, beta, G, Mg):
    """[4][G][C] float32 block of a train-mode BatchNorm over v [G*Mg][C]: mean, invstd, scale, shift"""
    vg = np.asarray(v, F64).reshape(G, Mg, -1)
    mean = vg.mean(axis=1).astype(F32)
    inv = (1.0 / np.sqrt(vg.var(axis=1) + EPS)).astype(F32)
    sc = (gamma[None].astype(F32) * inv).astype(F32)
    return np.stack([mean, inv, sc, (beta[None].astype(F32) - mean * sc).astype(F32)]).astype(F32)


def draw(rng, G, Mg, K, N, relu, anorm, bf16=False):
    """Inputs of one case: x [G*Mg][K] (the raw conv input), W [K][N], the BatchNorm in front (gamma ga, beta ba, statistics ast
    [4][G][K]; used with anorm), the stored conv output y, the statistics yst [4][G][N] of the BatchNorm behind, the gradient dz
    [G*Mg][N] (logical columns: the caller lays them out plain or through the shuffle), and the ReLU6 mask."""
    M = G * Mg
    x = rng.standard_normal((M, K)) * rng.uniform(0.5, 2.0, K) + rng.uniform(-1, 1, K)
    x = bf(x) if bf16 else x.astype(F32).astype(F64)
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(F32)
    ga, ba = rng.uniform(0.5, 1.5, K).astype(F32), rng.uniform(-0.5, 0.5, K).astype(F32)
    ast = stats_of(x, ga, ba, G, Mg)
    xg = x.reshape(G, Mg, K)
    xh_a = (xg - _rows(ast[0], Mg)) * _rows(ast[1], Mg)
    a_val = xh_a * ga.astype(F64) + ba.astype(F64) if anorm else xg
    y = a_val @ w.astype(F64) + rng.standard_normal(N).astype(F32).astype(F64)
    y = (bf(y) if bf16 else y.astype(F32).astype(F64)).reshape(M, N)
    gy, by = rng.uniform(0.5, 1.5, N).astype(F32), rng.uniform(1.0, 3.0, N).astype(F32)
    yst = stats_of(y, gy, by, G, Mg)
    dz = rng.standard_normal((M, N))
    dz = bf(dz) if bf16 else dz.astype(F32).astype(F64)
    mask = np.ones((G, Mg, N), bool)
    if relu:
        z64 = _rows(yst[2], Mg) * y.reshape(G, Mg, N) + _rows(yst[3], Mg)
        z32 = z64.astype(F32)               # = fmaf(scale, y, shift): the float64 product of two float32 numbers is exact
        near = np.abs(z64 - np.round(z64 / 6.0) * 6.0) <= 1e-4
        mask = np.where(near, (z32 > 0) & (z32 < 6), (z64 > 0) & (z64 < 6))
    return SimpleNamespace(G=G, Mg=Mg, K=K, N=N, relu=relu, anorm=anorm, bf16=bf16, x=x, w=w, ga=ga, ba=ba, ast=ast, y=y, yst=yst, dz=dz,
                           mask=mask, xh_a=xh_a, a_val=a_val)


def sums(inp):
    """(mask dz, mask dz xhat(y)) as [G][Mg][N] float64: the terms of the BatchNorm-backward sums of the BatchNorm behind the conv"""
    G, Mg, N = inp.G, inp.Mg, inp.N
    dzm = inp.dz.reshape(G, Mg, N) * inp.mask
    xh_y = (inp.y.reshape(G, Mg, N) - _rows(inp.yst[0], Mg)) * _rows(inp.yst[1], Mg)
    return dzm, dzm * xh_y, xh_y


def generic_coef(inp, rng):
    """[3][G][N] float32 coefficients as bn_bwd_finalize leaves them, k2 / k3 moved off their true values: the bias gradient --
    analytically zero behind a train-mode BatchNorm -- and every term that rides on it is exercised"""
    t1, t2, _ = sums(inp)
    k2 = t1.mean(axis=1) + rng.uniform(-0.3, 0.3, (inp.G, inp.N))
    k3 = t2.mean(axis=1) + rng.uniform(-0.3, 0.3, (inp.G, inp.N))
    return np.stack([inp.yst[2], k2.astype(F32), k3.astype(F32)]).astype(F32)


def fin_partials(inp, rng, fin_nb):
    """[G][fin_nb][2][N] float64: each group's rows split into fin_nb contiguous chunks of unequal length (empty ones included when the
    cuts coincide), the two sums per chunk"""
    t1, t2, _ = sums(inp)
    part = np.zeros((inp.G, fin_nb, 2, inp.N), F64)
    for g in range(inp.G):
        cuts = np.concatenate([[0], np.sort(rng.integers(0, inp.Mg + 1, fin_nb - 1)), [inp.Mg]]).astype(int)
        for b in range(fin_nb):
            part[g, b, 0] = t1[g, cuts[b]:cuts[b + 1]].sum(axis=0)
            part[g, b, 1] = t2[g, cuts[b]:cuts[b + 1]].sum(axis=0)
    return part


def evaluate(inp, coef=None, fin_part=None):
    """The whole contract.  coef [3][G][N] float32 (k1, k2, k3), or fin_part [G][fin_nb][2][N]: k1 = the scale row, k2 / k3 =
    sum_b part / Mg in float64, o_dbeta / o_dgamma = the totals.  Returns da [G*Mg][K], dw, db, the coefficients used, and with anorm
    a_coef [3][G][K], a_dgamma, a_dbeta (+ s1, s2 [G][K])."""
    G, Mg, K, N = inp.G, inp.Mg, inp.K, inp.N
    r = SimpleNamespace()
    dzm, _, xh_y = sums(inp)
    if fin_part is not None:
        k1, k2, k3 = inp.yst[2].astype(F64), fin_part[:, :, 0].sum(axis=1) / Mg, fin_part[:, :, 1].sum(axis=1) / Mg
        r.o_dbeta, r.o_dgamma = fin_part[:, :, 0].sum(axis=(0, 1)), fin_part[:, :, 1].sum(axis=(0, 1))
        r.o_abs = np.abs(fin_part[:, :, 0]).sum(axis=(0, 1)), np.abs(fin_part[:, :, 1]).sum(axis=(0, 1))
    else:
        k1, k2, k3 = (coef[i].astype(F64) for i in range(3))
    r.k = np.stack([k1, k2, k3])
    dy = _rows(k1, Mg) * (dzm - _rows(k2, Mg) - xh_y * _rows(k3, Mg))
    w = inp.w.astype(F64)
    ga, ba = inp.ga.astype(F64), inp.ba.astype(F64)
    r.db = dy.sum(axis=(0, 1))
    if inp.bf16:
        dyb, wb = bf(dy), bf(w)
        a_op = bf(inp.xh_a) if inp.anorm else inp.x.reshape(G, Mg, K)
        da = dyb @ wb.T
        q = np.einsum('gmk,gmn->kn', a_op, dyb)
        r.dw = ga[:, None] * q + ba[:, None] * r.db[None, :] if inp.anorm else q
        xs = a_op
    else:
        da = dy @ w.T
        r.dw = np.einsum('gmk,gmn->kn', inp.a_val, dy)
        xs = inp.xh_a
    r.da = da.reshape(G * Mg, K)
    if inp.anorm:
        r.s1, r.s2 = da.sum(axis=1), (da * xs).sum(axis=1)
        r.a_coef = np.stack([inp.ast[2].astype(F64), r.s1 / Mg, r.s2 / Mg])
        r.a_dgamma, r.a_dbeta = r.s2.sum(axis=0), r.s1.sum(axis=0)
    return r
