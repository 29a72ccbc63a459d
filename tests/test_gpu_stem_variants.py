"""Stem block (csrc/conv.hip, pool_bn_bwd_reduce in csrc/bn.hip) at op level: conv 3x3 / s2 'valid' -> BatchNorm + ReLU6 -> max-pool
3x3 / s2 'same', every form the host plan (StemPlan, reported by cdrl_stem_plan) can select, against the plain float64 reference of
tests/stem_ref.py.

Each case first reads cdrl_stem_plan and asserts the form it is there for; `test_coverage` holds the union of the cases' signatures
against REQUIRED, the hand-written list of what the ladders can select, and against the plan of the engine's default configuration
(B 256, T 4, 90 x 120, 24 channels, both storage types), which is queried and never run.

The statistics block of the backward cases is drawn (mean, invstd, scale of both signs, shift; independent from slice to slice); one
case per storage type takes real statistics through cdrl_bn_train_fwd.  The backward cases take the pool's codes and pooled values from
the reference (the pool forward has its own cases, bit for bit), so every piece is tested against exact inputs.

Nothing here can pass by luck: outputs start as the sentinel -2**100 and workspaces as NaN, every output sits inside a wider buffer
whose guard elements must come back bit-intact, every backward runs a second time on the dirty workspace and must reproduce itself
bit for bit, and the conditions on the inputs (every form-specific branch entered, no ReLU6 decision within an ulp of a kink) are
asserted from the reference alone, here and in tests/test_stem_plan_host.py.

Bounds (none of them comes from what the kernels produce):
  y                    bit-equal to the 27-fmaf chain (stem_ref.conv32) and to cdrl_stem_fwd; bf16 storage: to_bf16 of it;
                       |y - y64| <= 28 2^-24 (|b| + sum |x w|) per element
  statistics partials  summed on the host: 1e-12 of sum |y| and of sum y^2 (tests/test_gpu_ops.py::test_stem_fwd_with_statistics)
  pool forward         values and all eight bits of every code bit-equal, both storage types; plain max-pool the same
  BatchNorm partials   summed on the host: 2^-22 x the sum of the terms' magnitudes (tests/test_gpu_bn_variants.py); pooled form: plus
                       the recovery error the kernel's comment states, sum |dz| 2^-23 (|a| + |shift|) / |scale| invstd
  dgamma, dbeta        rel_err < 2e-5;  dw: rel_err < 1e-5 unfused, < 3e-5 fused;  db: the same against its own reference (with real
                       statistics it cancels: |db| < 1e-4 max |dw|)  (tests/test_gpu_ops.py)
  bf16 storage         gather form: bit-equal to the float32 run on the same stored inputs (test_stem_block_bf16_storage)
  margin               the float32-numpy evaluation of stem_ref meets each rel_err bound with a margin of 4 on every case's inputs
                       (asserted here and in the host test).
Worst observed on an MI355X (124 cases, 5.3 s): y at 0.20 of its bound; statistics 0 and 4.4e-15; BatchNorm partials at 0.77 of their
bound (a pooled case); dgamma 2.7e-7, dbeta 4.6e-8, dw 4.8e-7 fused and 1.7e-7 unfused, db 2.2e-6; the float32-numpy evaluation:
dgamma 2.7e-7, dw 1.2e-6, db 8.3e-7.  On the commit before the ROWSTATS form the multi-slice cases gave dw 4.8e-1 (B 1, T 4, 15 x 15)
and 2.3 (B 1, T 6, 9 x 9) with dgamma and dbeta unchanged."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from tests import bn_ref, stem_ref
from tests.bn_ref import F32, to_bf16
from tests.util import rel_err

BF = torch.bfloat16
SENTINEL = -2.0 ** 100
GUARD = 64                      # guard elements in front of and behind every buffer (keeps the payload 128-byte aligned)
TOL_BN, TOL_DW, TOL_DW_UNFUSED = 2e-5, 3e-5, 1e-5
MARGIN = 4.0
TYPES = ('f32', 'bf16')
FIELDS = ('Ho', 'Wo', 'Hp', 'Wp', 'fwd_vec', 'st_refusal', 'st_form', 'R', 'NB', 'nbpg', 'px', 'NP', 'lds', 'units_max', 'part_rows', 'pf_vec', 'pf_cx', 'pf_cy',
          'pf_nloop', 'pf_rb', 'pf_nb', 'pr_form', 'pr_pooled', 'pr_nb', 'fg_form', 'ff_refusal', 'ff_form', 'NCH', 'rowstats', 'rows_per', 'nblk', 'slices_max',
          'single', 'part_doubles', 'ws_doubles', 'pr_part_doubles')
ENGINE = (256, 4, 90, 120, 24)


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bits(t):
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def sync():
    """A device fault ends the run: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'device fault, stopping: {e}', returncode=3)


def plan(lib, B, T, H, W, Cout, at=0, pooled=0, adj=0, aligned=1):
    out = (C.c_int32 * 40)()
    n = lib.cdrl_stem_plan(B, T, H, W, Cout, at, pooled, adj, aligned, out, 40)
    assert n == len(FIELDS), n
    return dict(zip(FIELDS, out[:n]))


class Flat:
    """n elements inside a larger tensor: GUARD elements of `fill` in front and behind (`off` more in front: an unaligned payload)."""

    def __init__(self, n, dtype, fill=SENTINEL, off=0, device='cuda:0'):
        self.n, self.fill = n, fill
        self.whole = torch.full((n + 2 * GUARD + off,), fill, dtype=dtype, device=device)
        self.t = self.whole[GUARD + off:GUARD + off + n]

    def put(self, a):
        self.t.copy_(torch.as_tensor(np.ascontiguousarray(a)).reshape(-1).to(self.whole.dtype))
        return self

    def check(self, what, written=None):
        w = self.whole.cpu()
        lo = self.t.data_ptr() - self.whole.data_ptr()
        lo //= self.whole.element_size()
        rest = torch.cat([w[:lo], w[lo + self.n:]])
        if isinstance(self.fill, float) and np.isnan(self.fill):
            assert bool(torch.isnan(rest).all()), f'{what}: written outside'
        else:
            assert bool((rest == self.fill).all()), f'{what}: written outside'
        inside = w[lo:lo + (self.n if written is None else written)]
        if inside.dtype != torch.uint8:
            inside = inside.double()
            assert bool(torch.isfinite(inside).all()) and not bool((inside == SENTINEL).any()), f'{what}: elements left unwritten'

    def np(self):
        t = self.t.cpu()
        return (t.float() if t.dtype == BF else t).numpy().copy()


# ---- forward cases ---------------------------------------------------------------------------------------------------------------
def fcase(B, T, H, W, Cc, off=0, stats=1, expect=None):
    return SimpleNamespace(B=B, T=T, H=H, W=W, C=Cc, off=off, stats=stats and not off and Cc % 4 == 0, expect=expect or {})


FWD_CASES = [
    fcase(2, 2, 9, 11, 6, expect=dict(fwd_vec=0, st_refusal=1)),                         # scalar forward: Cout % 4
    fcase(2, 2, 9, 11, 24, off=1),                                                       # ... and y one float off
    fcase(2, 2, 22, 33, 24, expect=dict(st_form=0, R=8, px=2)),                          # px 2; odd W * 3 with an even H
    fcase(1, 3, 23, 58, 24, expect=dict(st_form=0, R=8, px=4)),
    fcase(1, 2, 23, 120, 24, expect=dict(st_form=0, R=8, px=6, NB=2)),                   # R 8 .. 1, H = 2 R + 7: the last band is shorter than R
    fcase(1, 2, 19, 150, 24, expect=dict(st_form=0, R=6, NB=2)),
    fcase(1, 2, 15, 200, 24, expect=dict(st_form=0, R=4, NB=2)),
    fcase(1, 2, 13, 280, 24, expect=dict(st_form=0, R=3, NB=2)),
    fcase(1, 2, 11, 400, 24, expect=dict(st_form=0, R=2, NB=3)),
    fcase(1, 2, 9, 600, 24, expect=dict(st_form=0, R=1, NB=4)),
    fcase(1, 2, 7, 700, 8, expect=dict(st_form=1)),                                      # window form in the process: W > 682
    fcase(5, 64, 21, 9, 24, expect=dict(st_form=0, nbpg=8, units_max=2)),                # 10 units on 8 workgroups per slice
    fcase(2, 300, 5, 120, 24, expect=dict(st_form=0, R=8, px=6, nbpg=1, units_max=2)),   # the workload's band geometry, several units
    fcase(2, 600, 5, 5, 24, expect=dict(st_form=0, nbpg=1)),                             # T > 512
    fcase(2, 2, 11, 13, 4, expect=dict(st_form=0)), fcase(2, 2, 11, 13, 20, expect=dict(st_form=0)),
    fcase(2, 2, 11, 13, 28, expect=dict(st_form=0)), fcase(2, 2, 11, 13, 64, expect=dict(st_form=0)),
]


def fid(c):
    return f'B{c.B}-T{c.T}-{c.H}x{c.W}-C{c.C}' + ('-off' if c.off else '')


@functools.lru_cache(maxsize=4)
def fwd_inputs(B, T, H, W, Cc):
    rng = np.random.default_rng([3, B, T, H, W, Cc])
    x = rng.uniform(0.0, 1.0, (B, T, H, W, 3)).astype(F32)
    w = (rng.standard_normal((3, 3, 3, Cc)) * 0.4).astype(F32)
    b = rng.standard_normal(Cc).astype(F32)
    Pm = stem_ref.patches(x)
    y64, mag = stem_ref.conv64(Pm, w, b)
    return SimpleNamespace(x=x, w=w, b=b, y32=stem_ref.conv32(Pm, w, b), y64=y64, mag=mag)


def fwd_signatures(c, pl, dt):
    sigs = []
    if dt == 'f32':
        sigs.append(dict(op='fwd', vec=pl['fwd_vec'], c4=int(c.C % 4 == 0)))
    if c.stats:
        band = pl['st_form'] == 0
        sigs.append(dict(op='stats', form=pl['st_form'], R=pl['R'], px=pl['px'], multi=int(pl['units_max'] > 1), short=int(band and pl['Ho'] % pl['R'] != 0),
                         oddw=(c.W * 3) % 2, C=c.C, tbig=int(c.T > 512), dt=dt))
    return sigs


# ---- pool forward cases ----------------------------------------------------------------------------------------------------------
POOL_GRIDS = ((1, 1), (2, 2), (2, 5), (5, 2), (6, 7), (7, 6), (7, 7), (8, 8))
POOL_CASES = [SimpleNamespace(C=Cc, H=h, W=w, B=2, T=2) for Cc in (24, 6, 5) for h, w in POOL_GRIDS]


def pool_inputs(c, at):
    """y over both kinks, scale of both signs, and a shift that clamps a large share of every window to 0 or to 6: ties decide the code"""
    rng = np.random.default_rng([5, c.C, c.H, c.W, at])
    rows = c.T * c.B * c.H * c.W
    y = (rng.standard_normal((rows, c.C)) * 1.5 + 0.4).astype(F32)
    if at:
        y = to_bf16(y)
    scale = (rng.uniform(1.0, 3.0, (c.T, c.C)) * rng.choice([-1.0, 1.0], (c.T, c.C))).astype(F32)
    shift = rng.uniform(-1.0, 7.0, (c.T, c.C))
    slot = (np.arange(c.C)[None, :] + np.arange(c.T)[:, None]) % 4         # one slot in four far below 0, one far above 6: whole windows tie
    shift = np.where(slot == 0, shift - 7.0, np.where(slot == 1, shift + 7.0, shift)).astype(F32)
    stats = np.stack([np.zeros_like(scale), np.ones_like(scale), scale, shift]).astype(F32)
    return y, stats


# ---- backward cases --------------------------------------------------------------------------------------------------------------
def bcase(B, T, H, W, Cc, pooled=0, adj=0, real=0, thr=0, six=0, types=TYPES, expect=None):
    return SimpleNamespace(B=B, T=T, H=H, W=W, C=Cc, pooled=pooled, adj=adj, real=real, thr=thr, six=six, types=types, expect=expect or {})


BWD_CASES = [
    # rows of three and more time slices in one workgroup: 49 rows per slice (workgroup 0 holds slices 0, 1, 2), and 16 (a wave's 32 rows span two)
    bcase(1, 4, 15, 15, 24, expect=dict(rowstats=1, slices_max=3, NCH=3)), bcase(1, 4, 15, 15, 24, pooled=1, adj=1, expect=dict(rowstats=1, slices_max=3)),
    bcase(1, 6, 9, 9, 24, adj=1, expect=dict(rowstats=1, slices_max=6)), bcase(1, 6, 9, 9, 32, pooled=1, expect=dict(rowstats=1, NCH=4)),
    bcase(1, 1, 3, 3, 24, expect=dict(rowstats=0, slices_max=1, nblk=1)),                                                     # one row in all
    bcase(1, 1, 3, 3, 8, pooled=1, adj=1, expect=dict(slices_max=1)),
    # rows no multiple of 128, all four (Ho, Wo) parities, Cout 8 .. 32, db adjacent and apart, both forms
    bcase(3, 2, 21, 27, 24, adj=1, expect=dict(rowstats=0, slices_max=2, NCH=3)),                                             # Ho 10, Wo 13
    bcase(3, 2, 23, 27, 24, pooled=1, expect=dict(rowstats=0, NCH=3)),                                                        # Ho 11, Wo 13
    bcase(2, 3, 23, 29, 8, pooled=1, adj=1, expect=dict(rowstats=0, NCH=3)),                                                  # Ho 11, Wo 14
    bcase(2, 3, 21, 29, 28, expect=dict(rowstats=0, NCH=4)),                                                                  # Ho 10, Wo 14
    bcase(2, 2, 21, 27, 32, pooled=1, adj=1, expect=dict(rowstats=0, NCH=4)), bcase(2, 2, 23, 29, 28, pooled=1, expect=dict(NCH=4)),
    bcase(2, 2, 23, 27, 32, adj=1, expect=dict(NCH=4)), bcase(2, 2, 21, 29, 8, expect=dict(NCH=3)),
    # pooled form: channels on each side of each of the three fall-back thresholds, spread over the four-channel lanes
    bcase(3, 2, 23, 29, 24, pooled=1, adj=1, thr=1, expect=dict(pr_pooled=1)),
    # bf16 pooled: stored activations of exactly 6.0 whose ReLU6 is open
    bcase(3, 2, 31, 31, 24, pooled=1, adj=1, six=1, types=('bf16',), expect=dict(pr_pooled=1)),
    # real statistics
    bcase(3, 2, 21, 29, 24, pooled=1, adj=1, real=1, types=('f32',)), bcase(3, 2, 21, 29, 24, adj=1, real=1, types=('bf16',)),
    # rows_per 256: the smallest shape that gets there (132496 rows on 1024 workgroups)
    bcase(4, 4, 183, 183, 24, pooled=1, adj=1, expect=dict(rows_per=256, rowstats=0, slices_max=2)),
]


def bid(c, dt):
    return f'{dt}-B{c.B}-T{c.T}-{c.H}x{c.W}-C{c.C}-' + ('pooled' if c.pooled else 'gather') + ''.join(f for f, on in (('-adj', c.adj), ('-real', c.real), ('-thr', c.thr), ('-six', c.six)) if on)


BWD_PARAMS = [pytest.param(c, dt, id=bid(c, dt)) for c in BWD_CASES for dt in c.types]


def pooled_lane_ok(stats):
    """[T][C] bool: the four channels of a lane take the pooled shortcut together, only where all of them have |scale| >= 0.05,
    |shift| <= 8 and |gamma| = |scale| / invstd >= 0.25 (float32, as the header states the thresholds)"""
    ok = (np.abs(stats[2]) >= F32(0.05)) & (np.abs(stats[3]) <= F32(8.0)) & (np.abs(stats[2]) >= F32(0.25) * np.abs(stats[1]))
    return np.repeat(ok.reshape(ok.shape[0], -1, 4).all(axis=2), 4, axis=1)


def threshold_sides(stats):
    """per threshold (below / above): channels that fail only this one, and channels that pass all three"""
    sc, sh, inv = np.abs(stats[2]), np.abs(stats[3]), np.abs(stats[1])
    t = [sc >= F32(0.05), sh <= F32(8.0), sc >= F32(0.25) * inv]
    return [int((~t[i] & t[(i + 1) % 3] & t[(i + 2) % 3]).sum()) for i in range(3)], int((t[0] & t[1] & t[2]).sum())


@functools.lru_cache(maxsize=2)
def _bwd_base(B, T, H, W, Cc):
    rng = np.random.default_rng([7, B, T, H, W, Cc])
    x = rng.uniform(0.0, 1.0, (B, T, H, W, 3)).astype(F32)
    w = (rng.standard_normal((3, 3, 3, Cc)) * 0.4).astype(F32)
    b = rng.standard_normal(Cc).astype(F32)
    Pm = stem_ref.patches(x)
    return x, Pm, stem_ref.conv32(Pm, w, b)


def draw_stats(rng, c, y, Mg):
    y3 = y.astype(np.float64).reshape(c.T, Mg, c.C)
    ym, ys = y3.mean(axis=1), np.maximum(y3.std(axis=1), 0.5)
    mean = ym + ys * rng.uniform(-0.3, 0.3, ym.shape)
    invstd = rng.uniform(0.8, 1.25, ym.shape) / ys
    gamma = rng.uniform(1.0, 3.0, ym.shape) * rng.choice([-1.0, 1.0], ym.shape)
    scale = gamma * invstd
    shiftc = rng.uniform(1.0, 4.0, ym.shape)
    if c.thr:
        # channel c of slice t: (c + 4 t) % 16 picks the side -- 1: |scale| 0.03 (invstd 0.1: gamma 0.3), 2: |scale| 0.06, 3: |shift| 9,
        # 4: |shift| 7.5, 5: gamma 0.2 (invstd 1, scale 0.2), 6: gamma 0.3, the rest ordinary.  Lanes of four channels: two of every four
        # lanes mix failing and passing channels (and fall back whole), two pass whole.
        side = (np.arange(c.C)[None, :] + 4 * np.arange(c.T)[:, None]) % 16
        sgn = np.sign(gamma)
        for s, (iv, sc) in {1: (0.1, 0.03), 2: (0.1, 0.06), 5: (1.0, 0.2), 6: (1.0, 0.3)}.items():
            invstd = np.where(side == s, iv, invstd)
            scale = np.where(side == s, sgn * sc, scale)
        shift = shiftc - mean * scale
        shift = np.where(side == 3, 9.0 * sgn, np.where(side == 4, 7.5 * sgn, shift))       # (their ReLU6 stays open in the tail of y)
    else:
        shift = shiftc - mean * scale
    return np.stack([mean, invstd, scale, shift]).astype(F32)


def bwd_inputs(c, dt, stats=None):
    """Everything a backward case reads, and its references.  stats: a statistics block to use instead of the drawn one (real statistics
    from the GPU); a `real` case without it takes bn_ref.train_stats (the host test)."""
    at = int(dt == 'bf16')
    x, Pm, y = _bwd_base(c.B, c.T, c.H, c.W, c.C)
    if at:
        y = to_bf16(y)
    Ho, Wo = stem_ref.conv_out(c.H), stem_ref.conv_out(c.W)
    Hp, Wp = stem_ref.same_out(Ho), stem_ref.same_out(Wo)
    Mg = c.B * Ho * Wo
    rng = np.random.default_rng([9, c.B, c.T, c.H, c.W, c.C, c.pooled, c.thr, at])
    gamma, beta = bn_ref.draw_affine(c.C)
    if stats is None:
        stats = bn_ref.train_stats(y, gamma, beta, c.T, Mg) if c.real else draw_stats(rng, c, y, Mg)
    pv, code, _ = stem_ref.pool_fwd(y, stats, c.T, c.B, Ho, Wo, bf16=bool(at))
    tsc = np.exp(rng.uniform(np.log(0.1), np.log(10.0), c.C))
    dp = (tsc * (rng.standard_normal((c.T * c.B, Hp, Wp, c.C)) + 0.5)).astype(F32)
    if at:
        dp = to_bf16(dp)
    i = SimpleNamespace(x=x, P=Pm, y=y, stats=stats, pv=pv, code=code, dp=dp, Ho=Ho, Wo=Wo, Hp=Hp, Wp=Wp, Mg=Mg, at=at, gamma=gamma, beta=beta)
    i.lane_ok = pooled_lane_ok(stats) if c.pooled else None
    kw = dict(pooled=pv if c.pooled else None, six_from_y=bool(at), lane_ok=i.lane_ok)
    i.sums = stem_ref.bn_sums(y, stats, code, dp, c.T, c.B, Ho, Wo, **kw)
    i.ref = stem_ref.backward(Pm, y, stats, code, dp, c.T, c.B, Ho, Wo, sums=i.sums)
    s32 = stem_ref.bn_sums(y, stats, code, dp, c.T, c.B, Ho, Wo, dtype=F32, **kw)
    i.r32 = stem_ref.backward(Pm, y, stats, code, dp, c.T, c.B, Ho, Wo, sums=s32, dtype=F32)
    return i


def margins(c, i):
    """the float32-numpy evaluation against the float64 reference: (dgamma, dbeta, dw, db) relative errors"""
    return (rel_err(i.r32.dgamma, i.ref.dgamma), rel_err(i.r32.dbeta, i.ref.dbeta), rel_err(i.r32.dw, i.ref.dw), rel_err(i.r32.db, i.ref.db))


def input_conditions(c, dt, i):
    """From the reference alone: every branch the case is there for is entered, and no ReLU6 decision sits within an ulp of a kink."""
    z = bn_ref.z32(i.y, i.stats, c.T, i.Mg)
    assert stem_ref.ulp_margin(z, 0.0) == 0 and stem_ref.ulp_margin(z, 6.0) == 0, 'a ReLU6 decision within one ulp of a kink'
    assert i.sums.nopen > 0, 'no open element'
    if c.six:
        assert i.sums.six > 0, 'no stored 6.0 with an open ReLU6'
    if c.thr:
        fails, passes = threshold_sides(i.stats)
        assert min(fails) > 0 and passes > 0, (fails, passes)
        lanes = i.lane_ok.reshape(c.T, -1, 4)[:, :, 0]
        assert lanes.any() and (~lanes).any(), 'the thresholds leave no lane on one side'
        mixed = pooled_lane_ok(i.stats) != ((np.abs(i.stats[2]) >= F32(0.05)) & (np.abs(i.stats[3]) <= F32(8.0)) & (np.abs(i.stats[2]) >= F32(0.25) * np.abs(i.stats[1])))
        assert mixed.any(), 'no lane mixes passing and failing channels'
    # window B of the gather: a pre-pool pixel reached from the pooled row / column before its own (even tap parity)
    k = i.code & 0x7f
    if i.Hp > 1:
        assert (k // 3 == 2).any(), 'no winner in the last window row (window B along y)'
    if i.Wp > 1:
        assert (k % 3 == 2).any(), 'no winner in the last window column (window B along x)'
    assert (i.code >= 128).any() or i.Mg < 16, 'no clamped winner'


def bwd_signatures(c, pl, dt):
    return [dict(op='reduce', form=pl['pr_form'], pooled=pl['pr_pooled'], dt=dt),
            dict(op='filter', form=1, NCH=pl['NCH'], rowstats=pl['rowstats'], big=int(pl['rows_per'] > 128), slices=min(pl['slices_max'], 3), single=pl['single'], dt=dt,
                 hpar=pl['Ho'] % 2, wpar=pl['Wo'] % 2, C=c.C, ragged=int((c.B * c.T * pl['Ho'] * pl['Wo']) % 128 != 0))]


UNFUSED = ((2, 3, 13, 15, 24, 0), (2, 3, 13, 15, 30, 0), (2, 3, 13, 15, 40, 2))     # (B, T, H, W, Cout, form of stem_bwd_filter)


# ---- REQUIRED: what the ladders of stem_plan (csrc/conv.hip) can select, written out from them ------------------------------------
def _req():
    yield dict(op='fwd', vec=1)
    yield dict(op='fwd', vec=0, c4=0)
    yield dict(op='fwd', vec=0, c4=1)                   # unaligned y
    for dt in TYPES:
        for R in (8, 6, 4, 3, 2, 1):
            yield dict(op='stats', form=0, R=R, dt=dt)
        for px in (2, 4, 6):
            yield dict(op='stats', form=0, px=px, dt=dt)
        yield dict(op='stats', form=0, multi=1, dt=dt)
        yield dict(op='stats', form=0, multi=0, dt=dt)
        yield dict(op='stats', form=0, short=1, dt=dt)
        yield dict(op='stats', form=0, oddw=1, dt=dt)
        yield dict(op='stats', form=0, tbig=1, dt=dt)
        yield dict(op='stats', form=1, dt=dt)
        for Cc in (4, 8, 20, 24, 28, 64):
            yield dict(op='stats', C=Cc, dt=dt)
        for vec in (4, 2, 1):
            yield dict(op='pool', vec=vec, dt=dt)
        for hp in (0, 1):
            for wp in (0, 1):
                yield dict(op='pool', hpar=hp, wpar=wp, dt=dt)
                yield dict(op='filter', form=1, hpar=hp, wpar=wp, dt=dt)
        for pooled in (0, 1):
            yield dict(op='reduce', form=1, pooled=pooled, dt=dt)
        for nch in (3, 4):
            for rs in (0, 1):
                yield dict(op='filter', form=1, NCH=nch, rowstats=rs, dt=dt)
        for single in (0, 1):
            yield dict(op='filter', form=1, single=single, dt=dt)
        for sl in (1, 2, 3):
            yield dict(op='filter', form=1, slices=sl, dt=dt)
        yield dict(op='filter', form=1, big=1, dt=dt)
        yield dict(op='filter', form=1, ragged=1, dt=dt)
        for Cc in (8, 24, 28, 32):
            yield dict(op='filter', form=1, C=Cc, dt=dt)
    yield dict(op='reduce', form=0)                     # the generic column reduce (C % 4 != 0: cdrl_bn_train_bwd_pooled)
    yield dict(op='filter', form=0, C=24)
    yield dict(op='filter', form=0, C=30)
    yield dict(op='filter', form=2)


REQUIRED = list(_req())
ENGINE_KEYS = {'stats': ('op', 'form', 'R', 'px', 'multi', 'dt'), 'pool': ('op', 'vec', 'dt'), 'reduce': ('op', 'form', 'pooled', 'dt'),
               'filter': ('op', 'form', 'NCH', 'rowstats', 'big', 'slices', 'single', 'dt')}


def matches(req, sig):
    return all(sig.get(k) == v for k, v in req.items())


def case_signatures(lib):
    sigs = []
    for c in FWD_CASES:
        for dt in TYPES:
            sigs += fwd_signatures(c, plan(lib, c.B, c.T, c.H, c.W, c.C, int(dt == 'bf16'), aligned=int(not c.off)), dt)
    for c in POOL_CASES:
        for dt in TYPES:
            pl = plan(lib, c.B, c.T, 2 * c.H + 1, 2 * c.W + 1, c.C, int(dt == 'bf16'))           # conv output H x W
            assert (pl['Ho'], pl['Wo']) == (c.H, c.W)
            sigs.append(dict(op='pool', vec=pl['pf_vec'], dt=dt, hpar=c.H % 2, wpar=c.W % 2))
    for c in BWD_CASES:
        for dt in c.types:
            sigs += bwd_signatures(c, plan(lib, c.B, c.T, c.H, c.W, c.C, int(dt == 'bf16'), c.pooled, c.adj), dt)
    sigs.append(dict(op='reduce', form=plan(lib, 2, 2, 15, 13, 6)['pr_form']))
    for B, T, H, W, Cc, form in UNFUSED:
        sigs.append(dict(op='filter', form=plan(lib, B, T, H, W, Cc)['fg_form'], C=Cc))
    return sigs


def engine_signatures(lib):
    """the default configuration's plan: queried, never run.  The engine hands the pooled activations over and keeps db behind dw."""
    B, T, H, W, Cc = ENGINE
    for dt in TYPES:
        pl = plan(lib, B, T, H, W, Cc, int(dt == 'bf16'), 1, 1)
        assert pl['rowstats'] == 0 and pl['ff_form'] == 1 and pl['st_form'] == 0, pl      # the forms that serve the workload are the two-slice ones
        c = SimpleNamespace(B=B, T=T, H=H, W=W, C=Cc, stats=1, off=0)
        for s in fwd_signatures(c, pl, dt)[-1:] + [dict(op='pool', vec=pl['pf_vec'], dt=dt)] + bwd_signatures(c, pl, dt):
            yield {k: s[k] for k in ENGINE_KEYS[s['op']]}


def coverage_gaps(lib):
    sigs = case_signatures(lib)
    missing = [r for r in REQUIRED if not any(matches(r, s) for s in sigs)]
    missing += [('engine', e) for e in engine_signatures(lib) if not any(matches(e, s) for s in sigs)]
    return missing


@pytest.mark.gpu
def test_coverage(lib):
    """The cases' signatures, through the plan query, cover REQUIRED and the default configuration's plan in both storage types."""
    missing = coverage_gaps(lib)
    assert not missing, missing


# ---- running the cases -----------------------------------------------------------------------------------------------------------
def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).to('cuda:0')
    return t.to(dtype) if dtype is not None else t


@pytest.mark.gpu
@pytest.mark.parametrize('c', FWD_CASES, ids=fid)
@pytest.mark.parametrize('dt', TYPES)
def test_forward(lib, c, dt):
    """cdrl_stem_fwd (float32) and cdrl_stem_fwd_stats in the form the plan names: y bit for bit, the partials summed on the host."""
    at = int(dt == 'bf16')
    if at and not c.stats:
        return                  # the plain forward has no bf16 form: the float32 parameter runs it
    pl = plan(lib, c.B, c.T, c.H, c.W, c.C, at, aligned=int(not c.off))
    assert all(pl[k] == v for k, v in c.expect.items()), (pl, c.expect)
    i = fwd_inputs(c.B, c.T, c.H, c.W, c.C)
    X, Wd, Bd = dev(i.x), dev(i.w), dev(i.b)
    n = i.y32.size
    if not at:
        y0 = Flat(n, torch.float32, off=c.off)
        _lib.check(lib.cdrl_stem_fwd(P(X), P(Wd), P(Bd), P(y0.t), c.B, c.T, c.H, c.W, c.C, S()))
        sync()
        y0.check('y')
        got = y0.np().reshape(i.y32.shape)
        assert np.array_equal(got.view(np.uint32), i.y32.view(np.uint32)), 'plain forward: not the 27-fmaf chain'
        err = np.abs(got.astype(np.float64) - i.y64) - 28 * 2.0 ** -24 * i.mag
        print(f'plain forward: worst |y - y64| / bound {float((np.abs(got - i.y64) / (28 * 2.0 ** -24 * i.mag)).max()):.3f}')
        assert err.max() <= 0
    if not c.stats:
        if c.C % 4 == 0:        # the statistics forward refuses an unaligned y
            part = Flat(8, torch.float64, fill=float('nan'))
            assert lib.raw.cdrl_stem_fwd_stats(P(X), P(Wd), P(Bd), P(y0.t), P(part.t), c.B, c.T, c.H, c.W, c.C, 0, S()) != 0
        return
    rows_p = pl['part_rows']
    assert rows_p == lib.cdrl_stem_fwd_stats_rows(c.B, c.T, c.H, c.W, c.C)
    y1 = Flat(n, BF if at else torch.float32)
    part = Flat(c.T * rows_p * 2 * c.C, torch.float64, fill=float('nan'))
    _lib.check(lib.raw.cdrl_stem_fwd_stats(P(X), P(Wd), P(Bd), P(y1.t), P(part.t), c.B, c.T, c.H, c.W, c.C, at, S()))
    sync()
    y1.check('y')
    part.check('partials')
    want = to_bf16(i.y32) if at else i.y32
    assert np.array_equal(y1.np().reshape(want.shape).view(np.uint32), want.view(np.uint32)), 'statistics forward: y not bit-equal'
    s, q, amag = stem_ref.slice_sums(want, c.T)
    pt = part.np().reshape(c.T, rows_p, 2, c.C).sum(axis=1)
    e1, e2 = float((np.abs(pt[:, 0] - s) / amag).max()), float((np.abs(pt[:, 1] - q) / q).max())
    print(f'statistics: sum {e1:.2e}, sum of squares {e2:.2e} (bound 1e-12)')
    assert e1 < 1e-12 and e2 < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize('c', POOL_CASES, ids=lambda c: f'C{c.C}-{c.H}x{c.W}')
@pytest.mark.parametrize('dt', TYPES)
def test_pool_forward(lib, c, dt):
    """cdrl_maxpool_bn_fwd: values and all eight bits of every code; float32 also cdrl_maxpool_fwd / _bwd on the activated tensor."""
    at = int(dt == 'bf16')
    tt = BF if at else torch.float32
    N = c.T * c.B
    y, stats = pool_inputs(c, at)
    pv, code, a = stem_ref.pool_fwd(y, stats, c.T, c.B, c.H, c.W, bf16=bool(at))
    if code.size >= 64:
        assert (pv == 0).any() and (pv == 6).any() and ((code & 0x7f) > 0).any(), 'no clamped winners: ties would not decide anything'
    pl = plan(lib, c.B, c.T, 2 * c.H + 1, 2 * c.W + 1, c.C, at)
    assert pl['pf_vec'] == {24: 4, 6: 2, 5: 1}[c.C] and (pl['Hp'], pl['Wp']) == code.shape[1:3]
    Y, St = dev(y, tt), dev(stats)
    p, am = Flat(pv.size, tt), Flat(code.size, torch.uint8, fill=0xEE)
    before = Y.clone()
    _lib.check(lib.raw.cdrl_maxpool_bn_fwd(P(Y), P(St), c.T, c.B, P(p.t), P(am.t), N, c.H, c.W, c.C, at, S()))
    sync()
    p.check('pooled')
    am.check('codes')
    assert torch.equal(bits(Y), bits(before))
    assert np.array_equal(p.np().view(np.uint32).ravel(), pv.view(np.uint32).ravel()), 'pooled values not bit-equal'
    assert np.array_equal(am.np().ravel(), code.ravel()), 'codes differ'
    if at:
        return
    A = dev(a)
    p2, am2 = Flat(pv.size, torch.float32), Flat(code.size, torch.uint8, fill=0xEE)
    _lib.check(lib.cdrl_maxpool_fwd(P(A), P(p2.t), P(am2.t), N, c.H, c.W, c.C, S()))
    dp = np.random.default_rng(c.C + c.H).integers(-8, 9, code.shape).astype(F32)        # small integers: the sums are exact in any order
    DP, da = dev(dp), Flat(a.size, torch.float32)
    _lib.check(lib.cdrl_maxpool_bwd(P(am.t), P(DP), P(da.t), N, c.H, c.W, c.C, S()))      # the fused forward's codes: bit 7 is masked away
    sync()
    p2.check('plain pooled')
    da.check('plain da')
    assert np.array_equal(p2.np().view(np.uint32).ravel(), pv.view(np.uint32).ravel()) and np.array_equal(am2.np().ravel(), (code & 0x7f).ravel())
    assert np.array_equal(da.np().reshape(-1, c.C), stem_ref.pool_bwd(code, dp, c.H, c.W, F32))


def real_statistics(lib, c, i):
    """the statistics block of the case's y from cdrl_bn_train_fwd (its own apply output is not used)"""
    tt = BF if i.at else torch.float32
    Y, gamma, beta = dev(i.y, tt), dev(i.gamma), dev(i.beta)
    mm, mv = torch.zeros(c.C, device='cuda:0'), torch.ones(c.C, device='cuda:0')
    stats = torch.full((4 * c.T * c.C,), SENTINEL, device='cuda:0')
    tmp = torch.empty((c.T * i.Mg, c.C), dtype=tt, device='cuda:0')
    ws = torch.full((c.T * 256 * 2 * c.C,), float('nan'), dtype=torch.float64, device='cuda:0')
    _lib.check(lib.raw.cdrl_bn_train_fwd(P(Y), c.T, i.Mg, c.C, P(gamma), P(beta), P(mm), P(mv), 1, 1, P(tmp), c.C, 0, 0, P(stats), P(ws), i.at, S()))
    sync()
    st = stats.view(4, c.T, c.C).cpu().numpy()
    assert rel_err(st, bn_ref.train_stats(i.y, i.gamma, i.beta, c.T, i.Mg)) < 1e-5
    return st


def run_block_bwd(lib, c, i, at, pl):
    """two runs on one workspace; returns the first run's outputs after holding the second against it"""
    tt = BF if at else torch.float32
    X, Y, St, DPt = dev(i.x), dev(i.y, tt), dev(i.stats), dev(i.dp, tt)
    Am = dev(i.code)
    Pv = dev(i.pv, tt) if c.pooled else None
    keep = [t.clone() for t in (X, Y, St, DPt, Am)]
    nws = int(lib.cdrl_stem_block_bwd_workspace_doubles(c.B, c.T, c.H, c.W, c.C))
    assert nws >= pl['pr_part_doubles'] + pl['part_doubles']
    ws = Flat(nws, torch.float64, fill=float('nan'))
    runs = []
    for _ in range(2):
        dg, dbt, coef = Flat(c.C, torch.float32), Flat(c.C, torch.float32), Flat(3 * c.T * c.C, torch.float32)
        if c.adj:
            wb = Flat(28 * c.C, torch.float32)
            dw, db, outs = wb.t[:27 * c.C], wb.t[27 * c.C:], [wb]
        else:
            wf, bf_ = Flat(27 * c.C, torch.float32), Flat(c.C, torch.float32)
            dw, db, outs = wf.t, bf_.t, [wf, bf_]
        _lib.check(lib.raw.cdrl_stem_block_bwd_pooled(P(X), P(Y), P(St), P(Am), P(DPt), P(Pv), c.B, c.T, c.H, c.W, c.C, P(dg.t), P(dbt.t), P(coef.t), P(dw), P(db),
                                                      P(ws.t), at, S()))
        sync()
        for f, what in [(dg, 'dgamma'), (dbt, 'dbeta'), (coef, 'coef')] + [(o, 'dw / db') for o in outs]:
            f.check(what)
        ws.check('workspace', written=pl['pr_part_doubles'] + pl['nblk'] * 28 * c.C // 2)
        runs.append(SimpleNamespace(dg=dg.np(), dbt=dbt.np(), coef=coef.np(), dw=dw.cpu().numpy().copy(), db=db.cpu().numpy().copy(),
                                    part=ws.np()[:pl['pr_part_doubles']].copy()))
    a, b = runs
    for k in ('dg', 'dbt', 'coef', 'dw', 'db'):
        assert np.array_equal(getattr(a, k).view(np.uint32), getattr(b, k).view(np.uint32)), f'{k}: not reproducible on the dirty workspace'
    assert all(torch.equal(bits(t), bits(k)) for t, k in zip((X, Y, St, DPt, Am), keep)), 'an input was written'
    return a


@pytest.mark.gpu
@pytest.mark.parametrize('c,dt', BWD_PARAMS)
def test_backward(lib, c, dt):
    """cdrl_stem_block_bwd(_pooled): the partial sums, coefficients, dgamma, dbeta, dw and db against stem_ref."""
    at = int(dt == 'bf16')
    pl = plan(lib, c.B, c.T, c.H, c.W, c.C, at, c.pooled, c.adj)
    assert all(pl[k] == v for k, v in c.expect.items()), (pl, c.expect)
    assert pl['ff_form'] == 1 and pl['pr_form'] == 1 and pl['pr_pooled'] == c.pooled and pl['single'] == c.adj and pl['rowstats'] == int(pl['slices_max'] > 2)
    i = bwd_inputs(c, dt)
    if c.real:
        i = bwd_inputs(c, dt, stats=real_statistics(lib, c, i))
    input_conditions(c, dt, i)
    m = margins(c, i)
    print('float32-numpy margins (dgamma, dbeta, dw, db): ' + ' '.join(f'{v:.2e}' for v in m))
    assert m[0] * MARGIN < TOL_BN and m[1] * MARGIN < TOL_BN and m[2] * MARGIN < TOL_DW and (c.real or m[3] * MARGIN < TOL_DW), m
    r = run_block_bwd(lib, c, i, at, pl)
    ref, sums, T, Cc = i.ref, i.sums, c.T, c.C
    nb = pl['pr_nb']
    part = r.part.reshape(T, nb, 2, Cc).sum(axis=1)
    bounds = (2.0 ** -22 * sums.a1, 2.0 ** -22 * sums.a2 + sums.rec)
    for q, s in enumerate((sums.s1, sums.s2)):
        err = np.abs(part[:, q] - s) - bounds[q]
        print(f'partial sums {q}: worst error / bound {float((np.abs(part[:, q] - s) / np.maximum(bounds[q], 1e-300)).max()):.3f}')
        assert err.max() <= 0, f'partial sums {q}: worst excess {err.max():.3e} at (slice, channel) {np.unravel_index(err.argmax(), err.shape)}'
    cf = r.coef.reshape(3, T, Cc)
    assert np.array_equal(cf[0].view(np.uint32), i.stats[2].view(np.uint32)), 'k1 is not the scale'
    for q in (1, 2):
        err = np.abs(cf[q] - ref.k[q]) - (bounds[q - 1] / i.Mg + 2.0 ** -24 * np.abs(ref.k[q]))
        assert err.max() <= 0, f'coef {q}: worst excess {err.max():.3e}'
    e = (rel_err(r.dg, ref.dgamma), rel_err(r.dbt, ref.dbeta), rel_err(r.dw.reshape(27, Cc), ref.dw), rel_err(r.db, ref.db))
    print('rel_err (dgamma, dbeta, dw, db): ' + ' '.join(f'{v:.2e}' for v in e))
    assert e[0] < TOL_BN and e[1] < TOL_BN, e
    assert e[2] < TOL_DW, f'dw: {e[2]:.3e}'
    if c.real:
        assert np.abs(r.db).max() < 1e-4 * np.abs(r.dw).max()
    else:
        assert e[3] < TOL_DW, f'db: {e[3]:.3e}'
    if at and not c.pooled:
        # the float32 run on the same stored inputs: bit-equal (tests/test_gpu_bf16_storage.py::test_stem_block_bf16_storage)
        r0 = run_block_bwd(lib, c, i, 0, plan(lib, c.B, c.T, c.H, c.W, c.C, 0, c.pooled, c.adj))
        for k in ('dg', 'dbt', 'coef', 'dw', 'db'):
            assert np.array_equal(getattr(r, k).view(np.uint32), getattr(r0, k).view(np.uint32)), f'{k}: bf16 storage differs from float32 on the same inputs'


@pytest.mark.gpu
@pytest.mark.parametrize('B,T,H,W,Cc,form', UNFUSED)
def test_unfused_filter(lib, B, T, H, W, Cc, form):
    """cdrl_stem_bwd_filter from a given dy: the MFMA kernel (Cout <= 32, any Cout) and the column reduce."""
    pl = plan(lib, B, T, H, W, Cc)
    assert pl['fg_form'] == form
    rng = np.random.default_rng([13, Cc])
    x = rng.uniform(0.0, 1.0, (B, T, H, W, 3)).astype(F32)
    Pm = stem_ref.patches(x)
    dy = (np.exp(rng.uniform(np.log(0.1), np.log(10.0), Cc)) * (rng.standard_normal((Pm.shape[0], Cc)) + 0.5)).astype(F32)
    dw64, db64 = stem_ref.filter_grad(Pm, dy)
    dw32, db32 = stem_ref.filter_grad(Pm, dy, F32)
    assert rel_err(dw32, dw64) * MARGIN < TOL_DW_UNFUSED and rel_err(db32, db64) * MARGIN < TOL_DW_UNFUSED
    nws = int(lib.cdrl_stem_bwd_workspace_doubles(B, T, H, W, Cc))
    assert nws >= pl['part_doubles']
    ws = Flat(nws, torch.float64, fill=float('nan'))
    X, DY = dev(x), dev(dy)
    res = []
    for _ in range(2):
        dw, db = Flat(27 * Cc, torch.float32), Flat(Cc, torch.float32)
        _lib.check(lib.cdrl_stem_bwd_filter(P(X), P(DY), P(dw.t), P(db.t), B, T, H, W, Cc, P(ws.t), S()))
        sync()
        dw.check('dw')
        db.check('db')
        ws.check('workspace', written=0)
        res.append((dw.np(), db.np()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    e = rel_err(res[0][0].reshape(27, Cc), dw64), rel_err(res[0][1], db64)
    print(f'rel_err dw {e[0]:.2e} db {e[1]:.2e}')
    assert e[0] < TOL_DW_UNFUSED and e[1] < TOL_DW_UNFUSED


@pytest.mark.gpu
def test_generic_pool_reduce(lib):
    """The launch_vcolreduce_t path of pool_bn_bwd_reduce (C % 4 != 0), through cdrl_bn_train_bwd_pooled: sums and dy."""
    B, T, H, W, Cc = 2, 2, 7, 6, 6
    assert plan(lib, B, T, 2 * H + 1, 2 * W + 1, Cc)['pr_form'] == 0
    c = SimpleNamespace(B=B, T=T, C=Cc, thr=0)
    rng = np.random.default_rng(17)
    Mg = B * H * W
    y = (rng.standard_normal((T * Mg, Cc)) * 1.5 + 0.4).astype(F32)
    stats = draw_stats(rng, c, y, Mg)
    _, code, _ = stem_ref.pool_fwd(y, stats, T, B, H, W)
    dp = (rng.standard_normal(code.shape) + 0.5).astype(F32)
    ref = stem_ref.backward(np.zeros((T * Mg, 27), F32), y, stats, code, dp, T, B, H, W)
    r32 = stem_ref.backward(np.zeros((T * Mg, 27), F32), y, stats, code, dp, T, B, H, W, dtype=F32)
    assert bn_ref.channel_err(r32.dy, ref.dy) * MARGIN < TOL_BN
    Y, St, Am, DP = dev(y), dev(stats), dev(code), dev(dp)
    ws = Flat(T * 256 * 3 * Cc, torch.float64, fill=float('nan'))
    dg, dbt, coef, dy = Flat(Cc, torch.float32), Flat(Cc, torch.float32), Flat(3 * T * Cc, torch.float32), Flat(T * Mg * Cc, torch.float32)
    _lib.check(lib.cdrl_bn_train_bwd_pooled(P(Am), P(DP), H, W, P(Y), T, Mg, Cc, P(St), P(dg.t), P(dbt.t), P(dy.t), P(coef.t), P(ws.t), S()))
    sync()
    for f, what in ((dg, 'dgamma'), (dbt, 'dbeta'), (coef, 'coef'), (dy, 'dy')):
        f.check(what)
    ws.check('workspace', written=0)
    assert rel_err(dg.np(), ref.dgamma) < TOL_BN and rel_err(dbt.np(), ref.dbeta) < TOL_BN
    assert bn_ref.channel_err(dy.np().reshape(-1, Cc), ref.dy) < TOL_BN
