"""Fused 1x1-conv backward, float32 kernel (pwb_kernel, csrc/gemm_pw_bwd.hip) on EXACT-INTEGER data: every output must EQUAL an integer
reference, no tolerance.

The kernel reads its filter-product operands out of row-major LDS planes by transposed reads (tr_frag, csrc/mfma_x3.h).  A wrong lane
map, contraction order or plane hand-over between tiles moves an integer here, where a tolerance could hide it behind rounding:

    dz, a in [-4, 4], W in [-2, 2], y in {-1, 1..5, 7} (the ReLU6 mask opens and closes); statistics mean 0 / invstd 1 / scale 1 /
    shift 0 and coefficients k1 = 1, k2 = k3 = 0, so dy = mask dz; with ANORM mean 0 / invstd 1 / gamma 1 / beta 0, so xhat(a) = a.

Small integers are their own first bf16 split term (the other two are 0), every product is an integer and every sum stays below 2^24
in float32 (|Q| <= 16 Mg) and 2^53 in double, so da, dW, db are exact; the BatchNorm sums derived in the reduce kernel are exact
doubles rounded ONCE to float32 (a_dgamma / a_dbeta; k2 / k3 after the division by Mg), which numpy reproduces.

One case per instantiated padding and flag set at G = 8, Mg = 3 * 32 * bm + 5 (32 workgroups per group walking three or four tiles each,
ragged last tile), one per padding at Mg = bm + 1 (one tile per workgroup).  Each runs twice on the dirty workspace and must
reproduce itself bit for bit.  Helpers and the entry are those of tests/test_gpu_pw_bwd_variants.py."""
import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from tests import pw_ref
from tests import test_gpu_pw_bwd_variants as V

pytestmark = pytest.mark.gpu
G = 8


def big(K, N):
    return 3 * 32 * V.bm_of(K, N) + 5


CASES = [
    V.mk(58, 58, G=G, Mg=big(58, 58), tag='exact'),                                                  # 64/64 dense
    V.mk(58, 58, G=G, Mg=big(58, 58), anorm=1, dz='hi', tag='exact'),                                # 64/64 SHUF + ANORM
    V.mk(116, 116, G=G, Mg=big(116, 116), tag='exact'),                                              # 128/128 dense
    V.mk(116, 116, G=G, Mg=big(116, 116), anorm=1, dz='hi', tag='exact'),                            # 128/128 SHUF + ANORM
    V.mk(58, 92, G=G, Mg=big(58, 92), tag='exact'),                                                  # 64 -> 128
    V.mk(24, 58, G=G, Mg=big(24, 58), acc=1, tag='exact'),                                           # ACC
    V.mk(58, 58, G=G, Mg=V.bm_of(58, 58) + 1, tag='exact-one-tile'),
    V.mk(116, 116, G=G, Mg=V.bm_of(116, 116) + 1, tag='exact-one-tile'),
    V.mk(58, 92, G=G, Mg=V.bm_of(58, 92) + 1, tag='exact-one-tile'),
]


def reference(dz, y, a, w, base, c):
    """float64 matrix products of small integers: every partial sum is an integer below 2^53, exact in any order -> int64"""
    Gn, Mg, K, N = c.G, c.Mg, c.K, c.N
    dy = np.where((y >= 1) & (y <= 5), dz, 0).astype(np.float64)
    da = dy @ w.T.astype(np.float64)
    dw = a.astype(np.float64).T @ dy
    r = dict(da=da + base if c.acc else da, dw=dw, db=dy.sum(axis=0))
    if c.anorm:
        s1 = da.reshape(Gn, Mg, K).sum(axis=1)
        s2 = (da * a).reshape(Gn, Mg, K).sum(axis=1)
        r.update(s1=s1, s2=s2)
    for v in r.values():
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() < 2.0 ** 53
    return {k: v.astype(np.int64) for k, v in r.items()}


@pytest.mark.parametrize('c', [pytest.param(c, id=V.case_id(c)) for c in CASES])
def test_exact(lib, c):
    K, N, Mg = c.K, c.N, c.Mg
    M = G * Mg
    f32 = torch.float32
    rng = np.random.default_rng([23, K, N, Mg, c.anorm, c.acc])
    dz = rng.integers(-4, 5, (M, N))
    a = rng.integers(-4, 5, (M, K))
    w = rng.integers(-2, 3, (K, N))
    y = rng.choice(np.array([-1, 1, 2, 3, 4, 5, 7]), (M, N))
    ones, zeros = np.ones((G, N), np.float32), np.zeros((G, N), np.float32)
    yst = np.stack([zeros, ones, ones, zeros])                                  # mean, invstd, scale, shift
    coef = np.stack([ones, zeros, zeros])                                       # k1, k2, k3
    ast = np.stack([np.zeros((G, K), np.float32), np.ones((G, K), np.float32), np.ones((G, K), np.float32), np.zeros((G, K), np.float32)])
    ldz, cdz, ctot = V.dz_view(c)
    lda, ca = V.a_view(c, 'a')
    ldd, cd = V.a_view(c, 'da')
    t = dict(dz=V.Framed(M, ldz, pw_ref.view_cols(cdz, N, ctot), f32, payload=dz), y=V.Framed(M, N, np.arange(N), f32, payload=y),
             a=V.Framed(M, lda, ca + np.arange(K), f32, payload=a), yst=V.dev(yst), ast=V.dev(ast), ga=V.dev(np.ones(K, np.float32)),
             ba=V.dev(np.zeros(K, np.float32)), w=V.dev(w))
    base = rng.integers(-4, 5, (V.GR + M + V.GR, ldd)).astype(np.float32) if c.acc else np.full((V.GR + M + V.GR, ldd), V.SENTINEL, np.float32)
    ref = reference(dz, y, a, w, base[V.GR:V.GR + M, cd:cd + K].astype(np.float64), c)
    assert np.abs(ref['dw']).max() < 2 ** 24 and np.abs(ref['da']).max() < 2 ** 24 and np.abs(ref['db']).max() < 2 ** 24
    out = V.fresh_outputs(c, base, f32)
    p = V.plan_query(lib, c, t['dz'].ptr, t['a'].ptr, out['da'].ptr)
    V.check_plan(p, c)
    assert p['form'] == 0 and p['nbpg'] == min(256 // G, p['tiles']) and p['shuf'] == int(c.dz == 'hi') and p['anorm'] == c.anorm and p['acc'] == c.acc
    t['wp'] = torch.zeros(int(lib.cdrl_pwconv_x3_packed_bytes(N)), dtype=torch.uint8, device=V.DEV)
    _lib.check(lib.cdrl_pwconv_x3_pack(V.P(t['w']), N, K, 1, N, V.P(t['wp']), V.S()))
    t['qpart'] = V.Banded(p['qpart_elems'], f32, float('nan'), band=4096)
    t['dbpart'] = V.Banded(p['dbpart_elems'], torch.float64, float('nan'), band=1024)
    t['fin_tot'] = V.Banded(G * 2 * N, torch.float64, float('nan'))
    for b in (t['qpart'], t['dbpart'], t['fin_tot']):
        b.ref = torch.full_like(b.lo, float('nan'))
    CF = V.dev(coef)
    V.launch(lib, c, t, CF, None, out)

    def guards(o):
        assert o['da'].frame_intact(), 'wrote outside the dA view'
        assert o['dw'].intact() and o['db'].intact(), 'wrote outside dW / db'
        assert t['qpart'].intact() and t['dbpart'].intact() and t['fin_tot'].intact(), 'wrote outside a workspace'
    guards(out)
    got = V.outputs_of(c, out, 0)
    out2 = V.fresh_outputs(c, base, f32)
    V.launch(lib, c, t, CF, None, out2)
    guards(out2)
    for (n, u), v in zip(got.items(), V.outputs_of(c, out2, 0).values()):
        assert torch.equal(V.bits(u), V.bits(v)), f'{n} not reproducible'

    def same(name, g_, r_):
        g_ = g_.cpu().numpy()
        r_ = np.asarray(r_).astype(np.float32).reshape(g_.shape)
        bad = np.argwhere(g_ != r_)
        assert bad.size == 0, f'{V.case_id(c)}: {name} differs in {len(bad)} places, first at {bad[0].tolist()}: {g_[tuple(bad[0])]} != {r_[tuple(bad[0])]}'
    same('da', out['da'].payload(), ref['da'])
    same('dW', out['dw'].t.view(K, N), ref['dw'])
    same('db', out['db'].t, ref['db'])
    if c.anorm:
        f64 = np.float64
        same('a_coef', out['acf'].view(3, G, K), np.stack([ast[2].astype(f64), ref['s1'].astype(f64) / f64(Mg), ref['s2'].astype(f64) / f64(Mg)]))
        same('a_dgamma', out['adg'], ref['s2'].sum(axis=0))
        same('a_dbeta', out['adb'], ref['s1'].sum(axis=0))
