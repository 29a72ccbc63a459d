"""Plain float64 reference of the stem block (csrc/conv.hip, pool_bn_bwd_reduce in csrc/bn.hip): conv 3x3 / stride 2 'valid' ->
BatchNorm + ReLU6 -> max-pool 3x3 / stride 2 'same', forward and backward, written from the definitions -- shared by
tests/test_gpu_stem_variants.py and tests/test_stem_plan_host.py.  numpy only; nothing here follows a kernel's loop structure.

Layout: observations x (B, T, H, W, 3); frames are ordered f = t * B + b; every activation is 2-D [rows][C] with rows = (f, oy, ox), so
the rows of time slice t are contiguous.  Filters w (3, 3, 3, C) = [ky][kx][ci][co], as a matrix [27][C].  A statistics block is
[4][T][C] float32: mean, invstd, scale, shift (tests/bn_ref.py).  `dtype` of the evaluating functions: float64 is the reference, float32
evaluates the same formulas with every elementwise operation rounded to float32 -- what float32 arithmetic itself loses."""
from types import SimpleNamespace

import numpy as np

from tests.bn_ref import F32, relu6_open, to_bf16, z32

WIDE = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else np.float64


def conv_out(n):
    return (n - 3) // 2 + 1


def same_out(n):
    return -(-n // 2)


def pad_before(n):
    """TF 'SAME' for a window of 3 and stride 2: pad_before = floor(total / 2)"""
    return max((same_out(n) - 1) * 2 + 3 - n, 0) // 2


def patches(x):
    """(B, T, H, W, 3) -> the im2col matrix [T*B*Ho*Wo][27], columns ordered (ky, kx, ci)"""
    B, T, H, W, _ = x.shape
    Ho, Wo = conv_out(H), conv_out(W)
    xf = np.transpose(x, (1, 0, 2, 3, 4)).reshape(T * B, H, W, 3)
    cols = [xf[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2, :] for ky in range(3) for kx in range(3)]
    return np.stack(cols, axis=3).reshape(T * B * Ho * Wo, 27)


def conv64(P, w, b):
    """y = P w + b in float64, and mag = |b| + sum |x w| per element"""
    P64, w64, b64 = P.astype(np.float64), w.reshape(27, -1).astype(np.float64), b.astype(np.float64)
    return P64 @ w64 + b64, np.abs(P64) @ np.abs(w64) + np.abs(b64)


def conv32(P, w, b):
    """The float32 value the definition fixes: the bias, then the 27 taps in order, each one fused multiply-add.  The product of two
    float32 numbers is exact in a wider type and the sum is rounded to float32 once (64-bit mantissa where the platform has it, which
    leaves no room for a double rounding to matter)."""
    w2 = w.reshape(27, -1)
    acc = np.broadcast_to(b.astype(F32), (P.shape[0], w2.shape[1])).copy()
    for k in range(27):
        acc = (P[:, k:k + 1].astype(WIDE) * w2[k].astype(WIDE) + acc.astype(WIDE)).astype(F32)
    return acc


def slice_sums(y, T):
    """per-slice sums of y and y^2 [T][C] in float64, with the sums of magnitudes"""
    y3 = y.astype(np.float64).reshape(T, -1, y.shape[1])
    return y3.sum(axis=1), (y3 * y3).sum(axis=1), np.abs(y3).sum(axis=1)


def pool_fwd(y, stats, T, B, H, W, bf16=False):
    """BatchNorm + ReLU6 + max-pool as the kernel defines it: a = clamp(fmaf(scale, y, shift), 0, 6) in float32, the FIRST strict maximum
    in (ky, kx) scan order over the window positions inside the image, code ky * 3 + kx with bit 7 set where the winner is clamped.
    y [T*B*H*W][C] holds the stored values (widened).  Returns (values [N][Hp][Wp][C] float32 -- rounded to bf16 with bf16 --, codes
    uint8, a [N][H][W][C] float32)."""
    N, C = T * B, y.shape[1]
    a = np.clip(z32(y, stats, T, B * H * W), F32(0), F32(6)).astype(F32).reshape(N, H, W, C)
    Hp, Wp, pt, pl = same_out(H), same_out(W), pad_before(H), pad_before(W)
    best = np.full((N, Hp, Wp, C), -np.inf, F32)
    code = np.zeros((N, Hp, Wp, C), np.uint8)
    for ky in range(3):
        iy = 2 * np.arange(Hp) + ky - pt
        for kx in range(3):
            ix = 2 * np.arange(Wp) + kx - pl
            ok = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]
            cand = a[:, np.clip(iy, 0, H - 1)][:, :, np.clip(ix, 0, W - 1)]
            upd = ok[None, :, :, None] & (cand > best)
            best = np.where(upd, cand, best)
            code = np.where(upd, np.uint8(ky * 3 + kx), code)
    code = np.where(relu6_open(best), code, code | np.uint8(0x80)).astype(np.uint8)
    return (to_bf16(best) if bf16 else best), code, a


def pool_targets(code, H, W):
    """flat pre-pool row (n, iy, ix) each pooled element's code points at: [N][Hp][Wp][C] int64"""
    N, Hp, Wp, C = code.shape
    k = (code & 0x7f).astype(np.int64)
    iy = 2 * np.arange(Hp)[None, :, None, None] - pad_before(H) + k // 3
    ix = 2 * np.arange(Wp)[None, None, :, None] - pad_before(W) + k % 3
    assert (iy >= 0).all() and (iy < H).all() and (ix >= 0).all() and (ix < W).all()
    return (np.arange(N)[:, None, None, None] * H + iy) * W + ix


def pool_bwd(code, dp, H, W, dtype=np.float64):
    """dz [N*H*W][C]: every pooled gradient goes to the position its code names"""
    N, Hp, Wp, C = code.shape
    dz = np.zeros((N * H * W, C), dtype)
    np.add.at(dz, (pool_targets(code, H, W), np.arange(C)[None, None, None, :]), dp.astype(dtype))
    return dz


def _rows(v, Mg):
    return np.repeat(np.asarray(v), Mg, axis=0)


def bn_sums(y, stats, code, dp, T, B, H, W, pooled=None, six_from_y=False, lane_ok=None, dtype=np.float64):
    """The BatchNorm backward sums over the pooled gradient, per slice [T][C]: s1 = sum dz, s2 = sum dz xhat, with the sums of their
    terms' magnitudes a1, a2 (float64 accumulation for both dtypes: every implementation under test accumulates in double).
    Gather form (pooled None): the pre-pool value the code points at, mask relu6_open(z32) of it, xhat = (y - mean) invstd.
    Pooled form: pooled = the stored pooled activation a; mask 0 < a < 6, y = (a - shift) / scale -- `rec` is then the recovery error
    bound sum |dp| 2^-23 (|a| + |shift|) / |scale| invstd of the terms of s2.  six_from_y (bf16 storage): an activation stored as
    exactly 6.0 may be an open one rounded up, so those elements take mask and value from the raw conv output, as the apply side does
    (`six`: how many of them are open).  lane_ok [T][C] bool: where False the element takes the gather form (the per-thread fall-back of
    channels whose statistics would amplify the recovery error)."""
    dt = dtype
    N, Hp, Wp, C = code.shape
    Mp = B * Hp * Wp
    st = [_rows(stats[i], Mp).astype(dt) for i in range(4)]
    d = dp.reshape(N * Hp * Wp, C).astype(dt)
    yg = np.take_along_axis(y, pool_targets(code, H, W).reshape(-1, C), axis=0)
    og = relu6_open(z32(yg, stats, T, Mp))
    six = 0
    if pooled is None:
        open_, yv = og, yg.astype(dt)
        rec = np.zeros((T, C))
    else:
        a = pooled.reshape(N * Hp * Wp, C)
        open_ = relu6_open(a)
        yv = (a.astype(dt) - st[3]) / st[2]
        if six_from_y:
            s6 = (a == F32(6)) & og
            six = int(s6.sum())
            open_ = open_ | s6
            yv = np.where(s6, yg.astype(dt), yv)
        if lane_ok is not None:
            keep = _rows(lane_ok, Mp)
            open_, yv = np.where(keep, open_, og), np.where(keep, yv, yg.astype(dt))
        rec = (np.where(open_ if lane_ok is None else open_ & keep, np.abs(d), 0) * 2.0 ** -23 * (np.abs(a) + np.abs(st[3])) / np.abs(st[2]) * np.abs(st[1])).astype(np.float64)
        rec = rec.reshape(T, Mp, C).sum(axis=1)
    xh = (yv - st[0]) * st[1]
    t1 = np.where(open_, d, dt(0)).astype(np.float64).reshape(T, Mp, C)
    t2 = (np.where(open_, d, dt(0)) * xh).astype(np.float64).reshape(T, Mp, C)
    return SimpleNamespace(s1=t1.sum(axis=1), s2=t2.sum(axis=1), a1=np.abs(t1).sum(axis=1), a2=np.abs(t2).sum(axis=1), rec=rec, open=open_, nopen=int(open_.sum()), six=six)


def backward(P, y, stats, code, dp, T, B, H, W, sums=None, dtype=np.float64):
    """Backward of the block from the pooled gradient.  H, W: the conv output's (pre-pool) size.  dz is scattered through the codes and
    masked by relu6_open(z32) of the raw conv output; k2 = s1 / Mg, k3 = s2 / Mg (from `sums` when given -- the pooled form's --, else
    the gather form's own); dy = k1 (dz - k2 - xhat k3); dw = P^T dy [27][C], db = sum dy."""
    dt = dtype
    Mg = B * H * W
    if sums is None:
        sums = bn_sums(y, stats, code, dp, T, B, H, W, dtype=dt)
    dz = np.where(relu6_open(z32(y, stats, T, Mg)), pool_bwd(code, dp, H, W, dt), dt(0))
    xh = (y.astype(dt) - _rows(stats[0], Mg).astype(dt)) * _rows(stats[1], Mg).astype(dt)
    k2, k3 = (sums.s1 / Mg).astype(dt), (sums.s2 / Mg).astype(dt)
    dy = _rows(stats[2], Mg).astype(dt) * (dz - _rows(k2, Mg) - xh * _rows(k3, Mg))
    dw = (P.astype(dt).T @ dy).astype(np.float64)
    return SimpleNamespace(sums=sums, dgamma=sums.s2.sum(axis=0), dbeta=sums.s1.sum(axis=0), k=(stats[2].astype(np.float64), sums.s1 / Mg, sums.s2 / Mg),
                           dy=dy, dw=dw, db=dy.astype(np.float64).sum(axis=0))


def filter_grad(P, dy, dtype=np.float64):
    """dw = P^T dy [27][C], db = sum dy"""
    return (P.astype(dtype).T @ dy.astype(dtype)).astype(np.float64), dy.astype(dtype).sum(axis=0).astype(np.float64)


def ulp_margin(z, at):
    """elements of a float32 array within one float32 ulp of `at` (a ReLU6 decision there would be a coin toss)"""
    z = np.asarray(z, F32)
    return int((np.abs(z.astype(np.float64) - at) <= np.spacing(F32(max(at, 2.0 ** -100)))).sum()) if at else int((np.abs(z) <= np.finfo(F32).tiny).sum())
