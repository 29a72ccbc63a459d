"""Plain float64 reference of the dense GEMM family (csrc/gemm.hip: gemm_nn with its split-K slab reduce; csrc/bn.hip: the dense
activations, the bias-gradient column sums and their reduce, permute_bt), written from the contract -- shared by
tests/test_gpu_nn_variants.py and tests/test_gemm_nn_plan_host.py.  numpy only; nothing here follows a kernel's loop structure.

The op:  C[m][n] (+)= sum_k A'[m][k] B(k, n) + bias[n],  A'[m][k] = a[m * ld + coff + k],  B(k, n) = b[k * sbk + n * sbn]
(forward: sbk = N, sbn = 1; backward-data through W^T: sbk = 1, sbn = K).  Next to C the reference returns the magnitude
S = sum_k |A'| |B| + |bias| (+ |base|): what the terms of an output element add up to before anything cancels -- the scale of its
rounding errors.

Activations (act 0 none, 1 relu6, 2 swish6, 3 tanh, 4 sigmoid) follow the oracle: relu6 has gradient 1 strictly inside (0, 6) and 0
elsewhere (at +-0 and 6 too); swish6 = min(x sigmoid(x), 6) with gradient sigmoid(x) (1 + x (1 - sigmoid(x))) where x sigmoid(x) < 6
and 0 where x sigmoid(x) >= 6.

`expected_plan` restates the dispatch ladder of gemm_nn AS THE COMMIT BEFORE THE PLAN STRUCT HAD IT (with its 64-row-tile threshold of
1 << 30 blocks and the four-way switch on the tile count behind it): the plan query is held to it."""
from types import SimpleNamespace

import numpy as np

F32, F64 = np.float32, np.float64
NONE, RELU6, SWISH6, TANH, SIGMOID = range(5)
ACT_NAMES = ('none', 'relu6', 'swish6', 'tanh', 'sigmoid')
PLAN_FIELDS = ('kernel', 'NT', 'WR', 'BT', 'VEC', 'gx', 'gy', 'gz', 'kchunk', 'ws_elems', 'reduce_grid', 'act_fused', 'a16', 'b16')
TILE, RT, SPLITK = 0, 1, 2
NO_CHUNK = 1 << 30


def cdiv(a, b):
    return -(-a // b)


# ---- the product ---------------------------------------------------------------------------------------------------------------------
def b_strides(order, K, N):
    """(sbk, sbn) of a dense weight: 'w' = W[K][N] read forward, 'wt' = W[N][K] read transposed (backward-data)"""
    return {'w': (N, 1), 'wt': (1, K)}[order]


def b_flat(Bm, order):
    """the flat array that holds the logical B [K][N] in the given order"""
    return np.ascontiguousarray(Bm if order == 'w' else Bm.T).reshape(-1)


def b_logical(flat, K, N, sbk, sbn):
    """B(k, n) = flat[k * sbk + n * sbn]"""
    return np.asarray(flat)[np.arange(K)[:, None] * sbk + np.arange(N)[None, :] * sbn]


def a_logical(whole, M, ld, coff, K):
    """A'[m][k] = whole[m * ld + coff + k]"""
    return np.asarray(whole).reshape(-1)[np.arange(M)[:, None] * ld + coff + np.arange(K)[None, :]]


def product(A, Bm, bias=None, base=None):
    """(C, S) in float64 for logical A [M][K], B [K][N], bias [N] or None, base [M][N] (accumulate) or None"""
    A, Bm = np.asarray(A, F64), np.asarray(Bm, F64)
    c, s = A @ Bm, np.abs(A) @ np.abs(Bm)
    if bias is not None:
        c, s = c + np.asarray(bias, F64), s + np.abs(np.asarray(bias, F64))
    if base is not None:
        c, s = c + np.asarray(base, F64), s + np.abs(np.asarray(base, F64))
    return c, s


def draw(key, M, K, N, bias, acc, exact):
    """Operands of one case.  exact: integers |a| <= 1023 (10 mantissa bits: a path that rounded to bf16 would change them), |b| <= 15,
    integer bias and base -- with S < 2^24 every partial sum is an integer below 2^24, exactly representable in float32 in any order
    and under any split.  Otherwise standard normal."""
    rng = np.random.default_rng(list(key))
    if exact:
        A = rng.integers(-1023, 1024, (M, K)).astype(F32)
        Bm = rng.integers(-15, 16, (K, N)).astype(F32)
        b = rng.integers(-4095, 4096, N).astype(F32) if bias else None
        base = rng.integers(-4095, 4096, (M, N)).astype(F32) if acc else None
    else:
        A = rng.standard_normal((M, K)).astype(F32)
        Bm = rng.standard_normal((K, N)).astype(F32)
        b = rng.standard_normal(N).astype(F32) if bias else None
        base = rng.standard_normal((M, N)).astype(F32) if acc else None
    return SimpleNamespace(A=A, B=Bm, bias=b, base=base)


def exact_condition(inp):
    """the exactness condition of the integer cases: integer operands within their ranges and S < 2^24 for every element"""
    _, s = product(inp.A, inp.B, inp.bias, inp.base)
    ints = all(x is None or np.array_equal(x, np.round(x)) for x in (inp.A, inp.B, inp.bias, inp.base))
    return bool(ints and np.abs(inp.A).max() <= 1023 and np.abs(inp.B).max() <= 15 and s.max() < 2.0 ** 24)


# ---- activations ---------------------------------------------------------------------------------------------------------------------
def sigmoid(x):
    x = np.asarray(x, F64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def swish(x):
    return np.asarray(x, F64) * sigmoid(x)


def swish6_open(x):
    """the gate of swish6's gradient: x sigmoid(x) < 6"""
    return swish(x) < 6.0


def relu6_open(x):
    x = np.asarray(x, F64)
    return (x > 0.0) & (x < 6.0)


def act_fwd(x, act):
    x = np.asarray(x, F64)
    if act == RELU6:
        return np.minimum(np.maximum(x, 0.0), 6.0)
    if act == SWISH6:
        return np.minimum(swish(x), 6.0)
    if act == TANH:
        return np.tanh(x)
    if act == SIGMOID:
        return sigmoid(x)
    return x.copy()


def act_deriv(x, act):
    x = np.asarray(x, F64)
    if act == RELU6:
        return relu6_open(x).astype(F64)
    if act == SWISH6:
        s = sigmoid(x)
        return np.where(swish6_open(x), s * (1.0 + x * (1.0 - s)), 0.0)
    if act == TANH:
        return 1.0 / np.cosh(np.minimum(np.abs(x), 350.0)) ** 2
    if act == SIGMOID:
        e = np.exp(-np.abs(x))
        return e / (1.0 + e) ** 2
    return np.ones_like(x)


def swish6_clamp():
    """x* with x* sigmoid(x*) = 6 by float64 bisection (about 6.0147), and the float32 numbers on both sides of it: (x*, below, above)"""
    lo, hi = 6.0, 6.1
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if float(swish(mid)) < 6.0:
            lo = mid
        else:
            hi = mid
    x = F32(lo)
    below = x if F64(x) <= lo else np.nextafter(x, F32(0))
    above = np.nextafter(below, F32(10))
    assert float(swish(below)) < 6.0 <= float(swish(above))
    return lo, below, above


def act_inputs(n, seed=0):
    """n float32 inputs: the special points first (as many as fit), the rest a normal fill scaled to cross every kink"""
    _, below, above = swish6_clamp()
    nxt = lambda v, to: np.nextafter(F32(v), F32(to))        # noqa: E731
    special = [0.0, -0.0, 6.0, nxt(0, 1), nxt(0, -1), np.finfo(F32).tiny, -np.finfo(F32).tiny, nxt(6, 0), nxt(6, 7),
               below, above, nxt(below, 0), nxt(above, 7), 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1.0, -1.0, 3.0, 5.9, 6.01, 6.02]
    rng = np.random.default_rng([n, seed])
    x = (rng.standard_normal(n) * 4.0).astype(F32)
    k = min(n, len(special))
    pos = rng.permutation(n)[:k]
    x[pos] = np.asarray(special[:k], F32)
    return x


def units(got, ref, tiny=2.0 ** -100):
    """per-element error in units of 2^-24 max(|ref|, tiny)"""
    return np.abs(np.asarray(got, F64) - ref) / (2.0 ** -24 * np.maximum(np.abs(ref), tiny))


# ---- the bias-gradient path -------------------------------------------------------------------------------------------------------
def vcol_geom(rows, C, max_blocks=128):
    """the block geometry of the column sums: (vec, cx, cy, nloop, rb, nb)"""
    vec = 4 if C % 4 == 0 else 2 if C % 2 == 0 else 1
    lanes = C // vec
    cx = min(lanes, 256)
    nloop = cdiv(lanes, cx)
    cy = max(256 // cx, 1)
    rb = max(cdiv(rows, max_blocks), 2 * cy)
    rb = cdiv(rb, cy) * cy
    return vec, cx, cy, nloop, rb, cdiv(rows, rb)


def reduce_cx(nparts, n):
    return 16 if (cdiv(n, 16) >= 128 or nparts <= 64) else 4


def f32_sum(part, base=None):
    """float32(sum over axis 0) of exactly summable doubles -- with a base: float32(base + float32(sum))"""
    s = np.asarray(part, F64).sum(axis=0).astype(F32)
    return s if base is None else (np.asarray(base, F64) + s.astype(F64)).astype(F32)


def permute_bt(x, B, T, D):
    """(B, T, D) -> (T, B, D)"""
    return np.ascontiguousarray(np.asarray(x).reshape(B, T, D).transpose(1, 0, 2)).reshape(-1)


# ---- the dispatch ladder of gemm_nn, as the parent commit has it ----------------------------------------------------------------------
def expected_plan(M, N, K, a_addr, a_ld, a_coff, b_addr, sbk, sbn, has_ws):
    e = dict.fromkeys(PLAN_FIELDS, 0)
    e['kernel'] = -1
    if M <= 0 or N <= 0:
        return e
    bt = int(sbn != 1)
    vec = int(K % 2 == 0 and a_ld % 2 == 0 and a_coff % 2 == 0 and a_addr % 8 == 0)
    a16 = int(K % 4 == 0 and a_ld % 4 == 0 and a_coff % 4 == 0 and a_addr % 16 == 0)
    b16 = int(b_addr % 16 == 0 and ((sbk == 1 and sbn % 4 == 0) if bt else (sbn == 1 and sbk % 4 == 0 and N % 4 == 0)))

    def tiles():
        nt = min(cdiv(N, 32), 4)
        ncb = cdiv(N, 32 * nt)
        return cdiv(cdiv(N, ncb), 32)
    e.update(BT=bt, VEC=vec, a16=a16, b16=b16, gz=1, kchunk=NO_CHUNK)
    # 1. split-K: a workspace, M <= 2048, K >= 256, an even tile count, more than one split left after rounding the chunk to 32
    if has_ws and M <= 2048 and K >= 256:
        nt = tiles()
        if nt % 2 == 0:
            gy, gx = cdiv(N, 32 * nt), cdiv(M, 64)
            nsplit = min(cdiv(512, gx * gy), 8)
            kchunk = cdiv(cdiv(K, nsplit), 32) * 32
            nsplit = cdiv(K, kchunk)
            if nsplit > 1:
                e.update(kernel=SPLITK, NT=nt, WR=2, gx=gx, gy=gy, gz=nsplit, kchunk=kchunk, ws_elems=nsplit * M * N,
                         reduce_grid=min(cdiv(M * N, 256), 2048), act_fused=1)
                return e
    nt = tiles()
    gy = cdiv(N, 32 * nt)
    # 2. row-stacked 96 x 128 tiles
    if N >= 129 and K >= 64 and M >= 2048 and a16 and b16:
        e.update(kernel=RT, NT=3, WR=0, VEC=0, gx=cdiv(M, 96), gy=cdiv(N, 128))
        return e
    # 3. the tile kernel: 64-row tiles below the threshold (1 << 30 blocks: always) when the tile count is even, else 128-row tiles
    threshold = 1 << 30
    small = nt % 2 == 0 and cdiv(M, 128) * gy < threshold
    if small:
        e.update(kernel=TILE, NT=2 if nt == 2 else 4, WR=2, gx=cdiv(M, 64), gy=gy)
    else:
        e.update(kernel=TILE, NT={1: 1, 2: 2, 3: 3}.get(nt, 4), WR=4, gx=cdiv(M, 128), gy=gy)
    return e


def signature(p, acc=0, act_out=0):
    """what a plan instantiates: (kernel, NT, WR, BT, VEC) -- for split-K the reduce's (accumulate, act_out) rides along"""
    return (p['kernel'], p['NT'], p['WR'], p['BT'], p['VEC'])


def vec_addresses_aligned(M, K, a_addr, a_ld, a_coff, kchunk, gz):
    """every float2 address the tile kernel forms under VEC -- a + (m * ld + coff + kb + k0 + kk) for even kk inside a split's range --
    is 8-byte aligned: checked over the first rows (the row term repeats with period 2) and every slab start"""
    for z in range(gz):
        kb = z * kchunk if gz > 1 else 0
        kend = min(kchunk, K - kb) if gz > 1 else K
        for m in range(min(M, 4)):
            for k in (0, 2, 30, 32, max(kend - 2, 0) // 2 * 2):
                if k < kend and (a_addr + 4 * (m * a_ld + a_coff + kb + k)) % 8:
                    return False
    return True
