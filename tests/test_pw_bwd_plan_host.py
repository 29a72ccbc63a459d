"""cdrl_pwconv_bwd_plan against an independent restatement of the host decisions of csrc/gemm_pw_bwd.hip (padding, tile height, workgroups
per group, K steps of the weight pack, workspace sizes, LDS bytes), over a sweep of shapes for both storage types, and every refusal
with its code.  Also, on the CPU: the coverage the GPU module asserts, and tests/pw_ref.py against float64 autograd.  The query
launches nothing and reads no memory; no call that is meant to be refused is ever launched.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from tests import pw_ref
from tests import test_gpu_pw_bwd_variants as V

BASE = 1 << 20
SHAPE, ALIGN, PADDING, TWO_GB, GROUPS, FIN, ANORM = 1, 2, 3, 4, 5, 6, 7
WORDS = {SHAPE: 'shape', ALIGN: 'alignment', PADDING: 'equal paddings', TWO_GB: '2 GB', GROUPS: 'groups', FIN: 'finalize', ANORM: 'normalised'}


def cdiv(a, b):
    return -(-a // b)


def pad(c):
    return 64 if c <= 64 else 128


def expected(K, N, G, Mg, at, shuf=0, anorm=0, acc=0, fin=0):
    """the plan of an accepted call, or the refusal code of a call with dense aligned views, no finalize and complete ANORM arguments"""
    if K < 8 or N < 8 or K > 128 or N > 128 or K % 2 or N % 2 or G < 1 or Mg < 1:
        return SHAPE
    if G > 8:
        return GROUPS
    kp, np_ = pad(K), pad(N)
    if at and kp != np_:
        return PADDING
    if kp == 128 and np_ == 64:
        return SHAPE
    bm = 64 if kp == 64 and np_ == 64 else 32
    tiles = cdiv(Mg, bm)
    nb = 256 // G
    if at and tiles >= 6 * (512 // G):          # bf16 storage: two resident workgroups per CU while each still gets six tiles
        nb = 512 // G
    nbpg = min(max(nb, 1), tiles)
    if at:
        lds = (bm * (np_ + 8) + 2 * np_ * (bm + 8)) * 2 + 7 * np_ * 4 + (np_ // 16) * 2 * 128 * 8 * 2
    else:
        lds = (3 * bm * (np_ + 8) + 3 * (np_ + kp) * (bm + 8)) * 2 + 7 * np_ * 4
    return dict(ok=1, refusal=0, form=at, kp=kp, np=np_, bm=bm, tiles=tiles, nbpg=nbpg, wp_ks=2 if N <= 32 else 4 if N <= 64 else 8, shuf=shuf,
                anorm=anorm, acc=acc, fin=int(fin > 0), coef_needed=int(not fin), lds_bytes=lds, qpart_elems=G * nbpg * kp * np_,
                dbpart_elems=G * nbpg * np_ * (3 if at else 1), spart_offset=G * nbpg * np_ if at and anorm else 0)


def query(lib, K, N, G, Mg, at, dz=None, a=None, da=None, shuffle=0, acc=0, anorm=(), fin=(), fin_nb=0):
    """anorm: the six ANORM pointers (a_stats, gamma, beta, dgamma, dbeta, coef) as truth values, () = none; fin: (fin_part, fin_tot,
    o_dgamma, o_dbeta) likewise.  Views: (address, ld, coff), dense and aligned when not given."""
    vz, va, vd = (_lib.View(*(v or (BASE, c, 0))) for v, c in ((dz, N), (a, K), (da, K)))
    pa = [C.c_void_p(BASE) if x else None for x in (anorm or (0,) * 6)]
    pf = [C.c_void_p(BASE) if x else None for x in (fin or (0,) * 4)]
    out = (C.c_int32 * len(V.PLAN_FIELDS))()
    n = lib.cdrl_pwconv_bwd_plan(C.byref(vz), shuffle, C.byref(va), C.byref(vd), acc, G, Mg, N, K, *pa, pf[0], fin_nb, *pf[1:], at, out, len(out))
    assert n == len(V.PLAN_FIELDS)
    return dict(zip(V.PLAN_FIELDS, out))


def check(lib, got, want, what):
    if isinstance(want, int):
        assert got['ok'] == 0 and got['refusal'] == want, (what, got, want)
        assert WORDS[want] in lib.cdrl_last_error().decode(), (what, lib.cdrl_last_error())
    else:
        assert got == want, (what, got, want)
        assert got['lds_bytes'] <= 160 * 1024


def mg_set(G, bm):
    s = {1, 3, bm - 1, bm, bm + 1, 2 * bm + 5}
    for t in (256 // G, 6 * (512 // G)):       # tiles around min(tiles, nb) and around the two-workgroup threshold of bf16 storage
        s |= {(t - 1) * bm, (t - 1) * bm + 1, t * bm, t * bm + 1}
    return sorted(m for m in s if m >= 1)


def test_plan_sweep_channels(lib):
    """every (K, N) in 2..140 for both storage types; G and Mg cycle through 1..9 and the boundary rows along the way"""
    i = 0
    for K in range(2, 141):
        for N in range(2, 141):
            for at in (0, 1):
                i += 1
                G = 1 + i % 9
                ms = mg_set(min(G, 8), 64 if max(K, N) <= 64 else 32)
                Mg = ms[i % len(ms)]
                check(lib, query(lib, K, N, G, Mg, at), expected(K, N, G, Mg, at), (K, N, G, Mg, at))


@pytest.mark.parametrize('K,N', [(8, 8), (58, 58), (64, 64), (58, 92), (64, 66), (66, 66), (116, 116), (128, 128)])
def test_plan_sweep_rows_and_groups(lib, K, N):
    """G in 1..9 x the rows around every tile and threshold boundary x both storage types x the flags"""
    bm = 64 if max(K, N) <= 64 else 32
    for G in range(1, 10):
        for Mg in mg_set(min(G, 8), bm):
            for at in (0, 1):
                for flags in range(8):
                    shuf, anorm, acc = flags & 1, flags >> 1 & 1, flags >> 2 & 1
                    fin = 5 if (flags == 3 and not at) else 0
                    got = query(lib, K, N, G, Mg, at, dz=(BASE, 2 * N, N) if shuf else None, shuffle=2 * N * shuf, acc=acc, anorm=(1,) * 6 * anorm,
                                fin=(1,) * 4 if fin else (), fin_nb=fin)
                    check(lib, got, expected(K, N, G, Mg, at, shuf, anorm, acc, fin), (K, N, G, Mg, at, flags))


def test_the_two_workgroup_threshold(lib):
    """G 8: 384 tiles is the threshold at both paddings (the arithmetic of the GPU module's bf16 cases)"""
    for K, Mg in ((116, 12288), (58, 24576)):
        bm = 32 if K > 64 else 64
        assert query(lib, K, K, 8, Mg, 1)['nbpg'] == 64 and query(lib, K, K, 8, Mg, 1)['tiles'] == 384
        assert query(lib, K, K, 8, Mg - bm, 1)['nbpg'] == 32 and query(lib, K, K, 8, Mg, 0)['nbpg'] == 32


def test_every_refusal_has_its_code_and_words(lib):
    q = lambda *a, **k: query(lib, *a, **k)         # noqa: E731
    ok = q(58, 58, 4, 100, 0)
    assert ok['ok'] == 1
    for K, N in ((57, 58), (58, 57), (6, 58), (58, 6), (130, 58), (58, 130), (116, 58), (128, 64)):      # odd, below 8, above 128, 128 -> 64
        check(lib, q(K, N, 4, 100, 0), SHAPE, (K, N))
    check(lib, q(58, 58, 0, 100, 0), SHAPE, 'G 0')
    check(lib, q(58, 58, 4, 0, 0), SHAPE, 'Mg 0')
    check(lib, q(58, 92, 4, 100, 1), PADDING, 'bf16 64 -> 128')
    check(lib, q(116, 58, 4, 100, 1), PADDING, 'bf16 128 -> 64')
    assert q(58, 92, 4, 100, 0)['ok'] == 1
    check(lib, q(58, 58, 9, 100, 0), GROUPS, 'G 9')
    for at in (0, 1):
        for kw in (dict(a=(BASE, 59, 0)), dict(a=(BASE, 60, 1)), dict(da=(BASE, 59, 0)), dict(da=(BASE, 60, 1)), dict(dz=(BASE, 59, 0)),
                   dict(a=(BASE + 4, 58, 0)), dict(da=(BASE + 4, 58, 0)), dict(dz=(BASE + 4, 58, 0)), dict(a=(BASE + 2, 58, 0))):
            check(lib, q(58, 58, 4, 100, at, **kw), ALIGN, (at, kw))
    check(lib, q(58, 58, 4, 100, 1, dz=(BASE, 60, 1)), ALIGN, 'bf16 odd dz offset')
    assert q(58, 58, 4, 100, 0, dz=(BASE, 60, 1))['ok'] == 1           # (float32 dz: single-element gathers and 4-byte aligned pairs)
    # 2 GB by shape alone: G * Mg * ld * 4 bytes
    rows = (1 << 29) // 116
    assert q(116, 116, 4, rows // 4, 0)['ok'] == 1
    check(lib, q(116, 116, 4, rows // 4 + 1, 0), TWO_GB, 'y / a / dz of 2 GB')
    check(lib, q(58, 58, 4, rows // 4 + 1, 0, da=(BASE, 116, 58)), TWO_GB, 'da view of 2 GB')
    check(lib, q(58, 58, 4, rows // 4 + 1, 0, a=(BASE, 116, 58)), TWO_GB, 'a view of 2 GB')
    # finalize-on-load
    assert q(58, 58, 4, 100, 0, fin=(1, 1, 1, 1), fin_nb=3) == dict(ok, fin=1, coef_needed=0)
    check(lib, q(58, 58, 4, 100, 1, fin=(1, 1, 1, 1), fin_nb=3), FIN, 'bf16')
    check(lib, q(58, 58, 4, 100, 0, fin=(1, 1, 1, 1), fin_nb=0), FIN, 'fin_nb 0')
    check(lib, q(58, 58, 4, 100, 0, fin=(1, 0, 1, 1), fin_nb=3), FIN, 'no fin_tot')
    check(lib, q(58, 58, 4, 100, 0, fin=(1, 1, 0, 1), fin_nb=3), FIN, 'no o_dgamma')
    check(lib, q(58, 58, 4, 100, 0, fin=(1, 1, 1, 0), fin_nb=3), FIN, 'no o_dbeta')
    assert q(58, 58, 4, 100, 0, fin=(0, 1, 1, 1), fin_nb=3) == ok       # no fin_part: the coefficient form
    # ANORM without one of its arguments
    assert q(58, 58, 4, 100, 0, anorm=(1,) * 6) == dict(ok, anorm=1)
    for miss in range(1, 6):
        check(lib, q(58, 58, 4, 100, 0, anorm=tuple(int(j != miss) for j in range(6))), ANORM, miss)
    # the query's own arguments
    v = _lib.View(BASE, 58, 0)
    out = (C.c_int32 * 18)()
    args = (0, 4, 100, 58, 58) + (None,) * 7 + (0,) + (None,) * 3
    assert lib.cdrl_pwconv_bwd_plan(None, 0, C.byref(v), C.byref(v), *args, 0, out, 18) == -1 and lib.cdrl_last_error()
    assert lib.cdrl_pwconv_bwd_plan(C.byref(v), 0, C.byref(v), C.byref(v), *args, 2, out, 18) == -1
    assert lib.cdrl_pwconv_bwd_plan(C.byref(v), 0, C.byref(v), C.byref(v), *args, 0, out, 18) == 18


def test_workspace_query_follows_the_plan(lib):
    for at in (0, 1):
        lib.cdrl_set_op_activation_type(at)
        try:
            for K, N, G, Mg in ((58, 58, 4, 700), (116, 116, 8, 12288), (58, 92, 3, 50), (24, 24, 1, 100000)):
                e = expected(K, N, G, Mg, at)
                if isinstance(e, dict):
                    assert lib.cdrl_pwconv_bwd_fused_workspace(G, Mg, N, K, 0) == e['qpart_elems']
                    assert lib.cdrl_pwconv_bwd_fused_workspace(G, Mg, N, K, 1) == e['dbpart_elems']
        finally:
            lib.cdrl_set_op_activation_type(0)


def test_plan_of_every_gpu_case(lib):
    """the GPU module's cases, their expectations and the restatement agree (the same check_plan the GPU run starts every case with)"""
    for c in V.CASES:
        p = V.plan_query(lib, c)
        V.check_plan(p, c)
        assert p == expected(c.K, c.N, c.G, c.Mg, c.bf16, int(c.dz in ('lo', 'hi')), c.anorm, c.acc, c.fin), V.case_id(c)


def test_coverage_on_the_host(lib):
    """What tests/test_gpu_pw_bwd_variants.py::test_coverage asserts on the GPU (the plan query needs none)."""
    V.test_coverage(lib)


@pytest.mark.parametrize('relu,anorm', [(1, 1), (1, 0), (0, 1)])
def test_reference_against_autograd(relu, anorm):
    """tests/pw_ref.py in its finalize-on-load form (true k2 / k3 from chunk sums) is the float64 autograd gradient of
    [BatchNorm ->] conv 1x1 -> BatchNorm -> [ReLU6] per group, up to the float32 rounding of the statistics blocks it is given."""
    G, Mg, K, N = 2, 37, 10, 12
    rng = np.random.default_rng(5 + relu + 2 * anorm)
    inp = pw_ref.draw(rng, G, Mg, K, N, relu, anorm)
    part = pw_ref.fin_partials(inp, rng, 5)
    ref = pw_ref.evaluate(inp, None, part)
    t = lambda v: torch.tensor(np.asarray(v, np.float64), requires_grad=True)       # noqa: E731
    x, w, ga, ba = t(inp.x.reshape(G, Mg, K)), t(inp.w), t(inp.ga), t(inp.ba)
    bias, gy, by = t(np.zeros(N)), t(np.ones(N)), t(np.zeros(N))
    # gamma / beta of the BatchNorm behind the conv, recovered from its statistics block (scale = gamma invstd, shift = beta - mean scale)
    gy_v = inp.yst[2].astype(np.float64)[0] / inp.yst[1].astype(np.float64)[0]
    by_v = inp.yst[3].astype(np.float64)[0] + inp.yst[0].astype(np.float64)[0] * inp.yst[2].astype(np.float64)[0]
    gy.data, by.data = torch.tensor(gy_v), torch.tensor(by_v)

    def bn(v, g, b):
        m, var = v.mean(dim=1, keepdim=True), v.var(dim=1, unbiased=False, keepdim=True)
        return (v - m) / torch.sqrt(var + pw_ref.EPS) * g + b
    a = bn(x, ga, ba) if anorm else x
    a.retain_grad()
    # the stored y differs from a W + b by its float32 rounding: differentiate at the stored value
    y = a @ w + bias
    y = y + (torch.tensor(inp.y.reshape(G, Mg, N)) - y).detach()
    z = bn(y, gy, by)
    out = torch.clamp(z, 0.0, 6.0) if relu else z
    (out * torch.tensor(inp.dz.reshape(G, Mg, N))).sum().backward()
    err = lambda got, want: float(np.abs(got - want.numpy()).max() / np.abs(want.numpy()).max())      # noqa: E731
    assert err(ref.da, a.grad.reshape(G * Mg, K)) < 1e-5
    assert err(ref.dw, w.grad) < 1e-5
    assert np.abs(ref.db).max() < 1e-5 * np.abs(ref.dw).max() and float(bias.grad.abs().max()) < 1e-9
    assert err(ref.o_dgamma, gy.grad) < 1e-5 and err(ref.o_dbeta, by.grad) < 1e-5
    if anorm:
        assert err(ref.a_dgamma, ga.grad) < 1e-5 and np.abs(ref.a_dbeta - ba.grad.numpy()).max() < 1e-5 * np.abs(ref.a_dgamma).max()


def test_reference_pieces():
    """the reference's own building blocks against hand-computed values"""
    assert pw_ref.view_cols(4, 4, 8).tolist() == [2, 6, 3, 7] and pw_ref.view_cols(58, 4, 116).tolist() == [29, 87, 30, 88]
    assert pw_ref.bf(np.array([1.0, 1.00390625, 1.01171875])).tolist() == [1.0, 1.0, 1.015625]
    inp = pw_ref.draw(np.random.default_rng(0), 1, 4, 8, 8, 0, 0)
    inp.dz[:] = np.arange(32.0).reshape(4, 8)
    inp.y[:] = np.tile(np.array([[0.0], [1.0], [2.0], [3.0]]), (1, 8))
    inp.yst = np.stack([np.full((1, 8), 1.5), np.full((1, 8), 2.0), np.full((1, 8), 3.0), np.zeros((1, 8))]).astype(np.float32)
    part = pw_ref.fin_partials(inp, np.random.default_rng(1), 3)
    assert part.shape == (1, 3, 2, 8) and part[0, :, 0].sum(axis=0).tolist() == [48.0 + 4 * c for c in range(8)]
    xhat = np.array([-3.0, -1.0, 1.0, 3.0])
    assert np.allclose(part[0, :, 1].sum(axis=0), [(xhat * (np.arange(4) * 8.0 + c)).sum() for c in range(8)])
    r = pw_ref.evaluate(inp, None, part)
    k2, k3 = 12.0, 80.0 / 4
    assert np.allclose(r.k[1], k2 + np.arange(8)) and np.allclose(r.k[2], k3)
    dy0 = 3.0 * (np.arange(4) * 8.0 - k2 - xhat * k3)
    assert np.allclose(r.db, dy0.sum()) and np.allclose(r.da, np.outer(dy0, np.ones(8)) @ inp.w.astype(np.float64).T)
