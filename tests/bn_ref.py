"""Plain float64 reference of the BatchNorm family (csrc/bn.hip), written from the definitions -- shared by
tests/test_gpu_bn_variants.py and tests/test_bn_plan_host.py.  numpy only; nothing here follows a kernel's loop structure.

Tensors are 2-D [rows][channels] with the rows of group g contiguous: rows [g*Mg, (g+1)*Mg).  A statistics block is [4][G][C]
float32: mean, invstd, scale, shift.  `dtype` of the evaluating functions: float64 is the reference; float32 evaluates the same
formula with every elementwise operation rounded to float32 (what float32 arithmetic itself loses -- the measure behind the
per-channel bound of the GPU tests)."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32
EPS = 1e-3


def shuffle_map(c, ctot):
    """channel_shuffle as a destination permutation: concat index c -> column (c & 1) * (ctot / 2) + (c >> 1)"""
    c = np.asarray(c)
    return (c & 1) * (ctot // 2) + (c >> 1)


def view_cols(coff, C, shuffle_ctot):
    """columns of a buffer row that the C channels of a view at `coff` occupy, plain or through the shuffle"""
    c = coff + np.arange(C)
    return shuffle_map(c, shuffle_ctot) if shuffle_ctot else c


def to_bf16(x):
    """float32 array rounded to bf16 (nearest even), returned widened to float32"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(F32).reshape(np.shape(x))


def _per_row(v, G, Mg):
    """[G][C] -> [G*Mg][C]"""
    return np.repeat(np.asarray(v), Mg, axis=0)


def z32(y, stats, G, Mg):
    """z = fmaf(scale, y, shift) as every kernel evaluates it: the float64 product of two float32 numbers is exact, so rounding the
    float64 sum to float32 reproduces the fused multiply-add."""
    return (y.astype(np.float64) * _per_row(stats[2], G, Mg).astype(np.float64) + _per_row(stats[3], G, Mg).astype(np.float64)).astype(F32)


def relu6_open(z):
    return (z > 0.0) & (z < 6.0)


def apply(y, stats, G, Mg, relu6):
    """relu6(scale * y + shift) in float64 (rounding is monotonic: clamping the exact value is the exact value of the clamped fmaf)"""
    z = y.astype(np.float64) * _per_row(stats[2], G, Mg).astype(np.float64) + _per_row(stats[3], G, Mg).astype(np.float64)
    return np.clip(z, 0.0, 6.0) if relu6 else z


def gap(a, P):
    """mean over each frame's P rows: [N*P][C] -> [N][C]"""
    return a.reshape(-1, P, a.shape[1]).mean(axis=1)


def backward(y, d, stats, G, Mg, relu6, bcast=0, dtype=np.float64):
    """BatchNorm(+ReLU6) backward from a given statistics block.  d: the incoming gradient [G*Mg][C], or with bcast > 0 the pooled
    gradient [G*Mg / bcast][C] of a global average pool over bcast rows.  Returns the per-group sums s1 = sum dz, s2 = sum dz * xhat
    ([G][C]) with the sums of their terms' magnitudes (a1, a2), dgamma, dbeta ([C]) and dy ([G*Mg][C]);
    dy = scale * (dz - mean(dz) - xhat * mean(dz * xhat)), dgamma = sum dz * xhat, dbeta = sum dz.
    The ReLU6 mask always comes from z32 (tests/util.py::engine_decisions)."""
    dt = dtype
    C = y.shape[1]
    d = d.astype(dt)
    if bcast:
        d = np.repeat(d, bcast, axis=0) / dt(bcast)
    dz = np.where(relu6_open(z32(y, stats, G, Mg)), d, dt(0)) if relu6 else d
    xhat = (y.astype(dt) - _per_row(stats[0], G, Mg).astype(dt)) * _per_row(stats[1], G, Mg).astype(dt)
    # the sums themselves are exact in every implementation under test (double accumulation): float64 here for both dtypes
    t1, t2 = dz.astype(np.float64).reshape(G, Mg, C), (dz.astype(np.float64) * xhat.astype(np.float64)).reshape(G, Mg, C)
    s1, s2 = t1.sum(axis=1), t2.sum(axis=1)
    k2, k3 = (s1 / Mg).astype(dt), (s2 / Mg).astype(dt)
    dy = _per_row(stats[2], G, Mg).astype(dt) * (dz - _per_row(k2, G, Mg) - xhat * _per_row(k3, G, Mg))
    return SimpleNamespace(s1=s1, s2=s2, a1=np.abs(t1).sum(axis=1), a2=np.abs(t2).sum(axis=1), dgamma=s2.sum(axis=0), dbeta=s1.sum(axis=0),
                           dy=dy.astype(np.float64), k=(stats[2].astype(np.float64), s1 / Mg, s2 / Mg))


def channel_err(got, ref):
    """max over channels of max|diff[:, c]| / max|ref[:, c]|: a small-magnitude channel cannot hide behind a large one.  A channel
    whose reference is all zero must be reproduced exactly."""
    diff = np.abs(np.asarray(got, np.float64) - ref).max(axis=0)
    scale = np.abs(ref).max(axis=0)
    return float(np.max(np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(diff > 0, np.inf, 0.0))))


def inference_stats(gamma, beta, mov_mean, mov_var, G):
    """[4][G][C] float64: mean, 1 / sqrt(var + eps), gamma * invstd, beta - mean * gamma * invstd"""
    inv = 1.0 / np.sqrt(mov_var.astype(np.float64) + EPS)
    g, b, m = gamma.astype(np.float64), beta.astype(np.float64), mov_mean.astype(np.float64)
    return np.stack([np.tile(v, (G, 1)) for v in (m, inv, g * inv, b - m * g * inv)])


def draw(rng, G, Mg, C, bf16=False, bcast=0):
    """Inputs of one case.  Per-channel scales s (of y) and t (of the gradient) are log-uniform in [1e-2, 1e2]; the statistics block
    is drawn, not computed: mean and invstd near those of y (so xhat is O(1)), scale of both signs, shift such that z = scale * y +
    shift crosses both ReLU6 kinks.  bf16: y and the gradient hold bf16 values (widened exactly); the pooled gradient of the
    bcast form stays float32."""
    R = G * Mg
    s = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), C))
    t = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), C))
    y = (s * (rng.standard_normal((R, C)) * 1.5 + 0.4)).astype(F32)
    d = (t * rng.standard_normal((R // bcast if bcast else R, C))).astype(F32)
    ident = (s * rng.standard_normal((R, C))).astype(F32)           # the unit's identity half
    gident = (t * rng.standard_normal((R, C))).astype(F32)          # ... and its gradient
    if bf16:
        y, ident, gident = to_bf16(y), to_bf16(ident), to_bf16(gident)
        if not bcast:
            d = to_bf16(d)
    mean = (s * (0.4 + rng.uniform(-0.3, 0.3, (G, C)))).astype(F32)
    invstd = (rng.uniform(0.8, 1.25, (G, C)) / (1.5 * s)).astype(F32)
    gam = rng.uniform(1.0, 3.0, (G, C)) * rng.choice([-1.0, 1.0], (G, C))
    scale = (gam * invstd).astype(F32)
    shift = (rng.uniform(1.0, 4.0, (G, C)) - mean * scale).astype(F32)
    return SimpleNamespace(y=y, d=d, ident=ident, gident=gident, stats=np.stack([mean, invstd, scale, shift]).astype(F32))


def draw_affine(C):
    """gamma (both signs) and beta of the cases that take real statistics"""
    rng = np.random.default_rng(C)
    return (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F32), rng.uniform(1.0, 3.0, C).astype(F32)


def train_stats(y, gamma, beta, G, Mg):
    """[4][G][C] float32 statistics block of training-mode BatchNorm (biased variance, eps 1e-3), float64 arithmetic rounded once"""
    yg = y.astype(np.float64).reshape(G, Mg, -1)
    mean, inv = yg.mean(axis=1), 1.0 / np.sqrt(yg.var(axis=1) + EPS)
    return np.stack([mean, inv, gamma * inv, beta - mean * gamma * inv]).astype(F32)
