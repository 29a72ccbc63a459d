"""cdrl_traceset_batch at the op level (csrc/traceset.hip) against the numpy restatement tests/traceset_ref.py.
The kernel only copies and decodes, so every comparison is exact equality of BIT PATTERNS (int32 views: NaNs compare); there is no
tolerance.  Every destination sits between canary words that must keep their bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import _lib
from tests import traceset_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY, PAD = 0x5AC3A51E, 64            # 64 words = 256 bytes on each side: the destination stays 16-byte aligned
# per-step traces of 5, 1 and 6 rows and a stacked one of 3: rows 0..4 | 5..7 | 8 | 9..14
LAYOUT = [(5, False), (3, True), (1, False), (6, False)]
ROWS = 15
# the clamp at the start of every trace (rows 0, 1, 2, 9), the stacked trace (5, 7), the one-row trace (8), the last row, a duplicate
EIGHT = [0, 1, 2, 5, 8, 9, 14, 0]


def _up(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(a.dtype)
    return torch.as_tensor(a.view(view) if view else a).to(DEV)


def _source(rng, code, slots, elems):
    """Random coded slots (every bit pattern allowed: NaNs, both zeros, subnormal halves) -> (coded, palette or None, decoded bits)."""
    palette = None
    if code == ref.F32:
        coded = rng.integers(0, 2 ** 32, (slots, elems), dtype=np.uint64).astype(np.uint32)
        coded[0, 0] = 0x80000000
        coded[-1, -1] = 0x7fc00001
        decoded = coded
    elif code == ref.F16:
        coded = rng.integers(0, 2 ** 16, (slots, elems), dtype=np.uint32).astype(np.uint16)
        coded[0, 0], coded[-1, -1] = 0x8000, 0x7e01
        if elems > 2:
            coded[0, 1], coded[0, 2] = 0x0001, 0xfc00                                            # the smallest subnormal, -inf
        decoded = ref.decode(ref.F16, coded)
    else:
        coded = rng.integers(0, 256, (slots, elems), dtype=np.uint16).astype(np.uint8)
        palette = rng.integers(0, 2 ** 32, 256, dtype=np.uint64).astype(np.uint32)
        palette[:3] = (0x00000000, 0x80000000, 0x7fc00001)
        decoded = ref.decode(ref.U8, coded, palette)
    return coded, palette, decoded


class Guarded:
    """A float32 destination of `n` words between two canary bands."""

    def __init__(self, n, shift=0):
        self.n, self.shift = n, shift
        self.buf = torch.full((PAD + shift + n + PAD,), CANARY, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * (PAD + self.shift)

    def bits(self):
        a = self.buf.cpu().numpy().view(np.uint32)
        lo = PAD + self.shift
        assert (a[:lo] == CANARY).all() and (a[lo + self.n:] == CANARY).all(), 'a canary word changed'
        return a[lo:lo + self.n]


def _key(src, palette, dst, elems, code, T, stride=None, direct=0, src_byte_offset=0):
    return _lib.TraceSetKey(src.data_ptr() + src_byte_offset, None if palette is None else palette.data_ptr(), dst.ptr, elems,
                            elems if stride is None else stride, code, T, direct, 0)


def _launch(keys, slot, lo, index, offset, rows, set_rows=ROWS):
    arr = (_lib.TraceSetKey * max(len(keys), 1))(*keys)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.load().cdrl_traceset_batch(arr, len(keys), _lib.ptr(slot), _lib.ptr(lo), _lib.ptr(index), offset, rows, set_rows, stream)


@pytest.fixture(scope='module')
def many():
    """257 rows with duplicates behind three entries that offset = 3 skips."""
    return np.concatenate([[14, 14, 14], np.random.default_rng(77).integers(0, ROWS, 257)]).astype(np.int32)


@pytest.mark.parametrize('T', [1, 4])
@pytest.mark.parametrize('code', [ref.F32, ref.F16, ref.U8], ids=['f32', 'f16', 'u8'])
@pytest.mark.parametrize('elems', [1, 3, 9, 16, 19, 4100, 48 * 64 * 3])
def test_batch_is_the_restatement_bit_for_bit(elems, code, T, many):
    slot, lo, slots = ref.tables(LAYOUT, T)
    coded, palette, decoded = _source(np.random.default_rng(elems * 8 + code * 2 + T), code, slots, elems)
    dslot, dlo, dsrc, dpal = _up(slot), _up(lo), _up(coded), None if palette is None else _up(palette)
    for index, offset, rows in (([14], 0, 1), (EIGHT, 0, 8), (many, 3, 257)):
        index = np.asarray(index, np.int32)
        dst = Guarded(rows * T * elems)
        assert _launch([_key(dsrc, dpal, dst, elems, code, T)], dslot, dlo, _up(index), offset, rows) == 0
        torch.cuda.synchronize()
        want = ref.batch(decoded, slot, lo, index, offset, rows, T)
        assert np.array_equal(dst.bits().reshape(want.shape), want), (rows, offset)
    if T == 4:      # what the formula means: the window of a per-step trace, the own frames of a stacked one
        frames = np.maximum(slot[:, None] - (3 - np.arange(4))[None, :], lo[:, None])
        assert frames[0].tolist() == [0, 0, 0, 0] and frames[2].tolist() == [0, 0, 1, 2] and frames[5].tolist() == [5, 6, 7, 8]
        assert frames[8].tolist() == [17] * 4 and frames[9].tolist() == [18] * 4 and frames[14].tolist() == [20, 21, 22, 23]


@pytest.mark.parametrize('code', [ref.F32, ref.F16, ref.U8], ids=['f32', 'f16', 'u8'])
def test_bases_off_the_16_byte_grid_take_the_element_path(code):
    """16 elements per slot would allow 16-byte accesses; a source or a destination one element off the grid must not use them."""
    T, elems = 4, 16
    slot, lo, slots = ref.tables(LAYOUT, T)
    item = {ref.F32: 4, ref.F16: 2, ref.U8: 1}[code]
    coded, palette, _ = _source(np.random.default_rng(code), code, slots + 1, elems)
    flat = coded.reshape(-1)[1:1 + slots * elems].reshape(slots, elems)                       # the slots start one element in
    dsrc, dpal, index = _up(coded), None if palette is None else _up(palette), np.asarray(EIGHT, np.int32)
    for shift, src_off in ((0, item), (1, 0), (1, item)):
        dst = Guarded(8 * T * elems, shift=shift)
        src = flat if src_off else coded.reshape(-1)[:slots * elems].reshape(slots, elems)
        want = ref.batch(ref.decode(code, src, palette), slot, lo, index, 0, 8, T)
        assert _launch([_key(dsrc, dpal, dst, elems, code, T, src_byte_offset=src_off)], _up(slot), _up(lo), _up(index), 0, 8) == 0
        torch.cuda.synchronize()
        assert np.array_equal(dst.bits().reshape(want.shape), want), (shift, src_off)


def test_four_codes_and_the_column_matrix_in_one_launch(many):
    """An image as bytes, a 9-element byte key (slots at odd addresses), a half key, a float key and three column ranges of one
    (N, W) matrix -- seven keys, one launch."""
    T, rng = 4, np.random.default_rng(3)
    slot, lo, slots = ref.tables(LAYOUT, T)
    specs = [(ref.U8, 48 * 64 * 3), (ref.U8, 9), (ref.F16, 24), (ref.F32, 5)]
    sources = [_source(rng, code, slots, elems) for code, elems in specs]
    W = 6
    matrix = rng.integers(0, 2 ** 32, (ROWS, W), dtype=np.uint64).astype(np.uint32)
    dmat = _up(matrix)
    ranges = [(0, 2), (3, 4), (4, 6)]                                                          # u, one scalar column, returns
    rows, offset = 257, 3
    keep, keys, dsts = [], [], []
    for (code, elems), (coded, palette, _) in zip(specs, sources):
        dsrc, dpal = _up(coded), None if palette is None else _up(palette)
        keep += [dsrc, dpal]
        dsts.append(Guarded(rows * T * elems))
        keys.append(_key(dsrc, dpal, dsts[-1], elems, code, T))
    for c0, c1 in ranges:
        dsts.append(Guarded(rows * (c1 - c0)))
        keys.append(_key(dmat, None, dsts[-1], c1 - c0, ref.F32, 1, stride=W, direct=1, src_byte_offset=4 * c0))
    assert _launch(keys, _up(slot), _up(lo), _up(many), offset, rows) == 0
    torch.cuda.synchronize()
    for (code, elems), (_, _, decoded), dst in zip(specs, sources, dsts):
        want = ref.batch(decoded, slot, lo, many, offset, rows, T)
        assert np.array_equal(dst.bits().reshape(want.shape), want), (code, elems)
    for (c0, c1), dst in zip(ranges, dsts[4:]):
        want = ref.batch(np.ascontiguousarray(matrix[:, c0:c1]), None, None, many, offset, rows, 1, direct=True)
        assert np.array_equal(dst.bits().reshape(want.shape), want), (c0, c1)
    # the whole matrix as ONE direct key, through 16-byte accesses where W allows none (W = 6) and where it does (W = 8)
    for width in (6, 8):
        wide = rng.integers(0, 2 ** 32, (ROWS, width), dtype=np.uint64).astype(np.uint32)
        dst, dwide = Guarded(rows * width), _up(wide)
        assert _launch([_key(dwide, None, dst, width, ref.F32, 1, direct=1)], None, None, _up(many), offset, rows) == 0
        torch.cuda.synchronize()
        assert np.array_equal(dst.bits().reshape(rows, width), wide[many[offset:offset + rows]])


def test_refused_arguments_launch_nothing():
    T, elems = 4, 16
    slot, lo, slots = ref.tables(LAYOUT, T)
    coded, palette, _ = _source(np.random.default_rng(0), ref.U8, slots, elems)
    dsrc, dpal, dslot, dlo, index = _up(coded), _up(palette), _up(slot), _up(lo), _up(np.asarray(EIGHT, np.int32))
    dst = Guarded(8 * T * elems)

    def good(code=ref.U8, T=T, **kw):
        return _key(dsrc, dpal, dst, elems, code, T, **kw)

    lib = _lib.load()
    null_src, null_dst, null_pal = good(), good(), good()
    null_src.src, null_dst.dst, null_pal.palette = None, None, None
    direct = good(direct=1)
    cases = [([null_src], dslot, dlo, index, 8), ([null_dst], dslot, dlo, index, 8), ([null_pal], dslot, dlo, index, 8),
             ([good()], None, dlo, index, 8), ([good()], dslot, None, index, 8), ([good()], dslot, dlo, None, 8),
             ([good()], dslot, dlo, index, 0), ([good()], dslot, dlo, index, 65536), ([good(T=0)], dslot, dlo, index, 8),
             ([good(T=17)], dslot, dlo, index, 8), ([good()] * 9, dslot, dlo, index, 8), ([], dslot, dlo, index, 8),
             ([good(code=3)], dslot, dlo, index, 8), ([good(code=-1)], dslot, dlo, index, 8), ([direct], dslot, dlo, index, 8),
             ([good(stride=elems - 1)], dslot, dlo, index, 8)]
    for keys, s, l, i, rows in cases:
        assert _launch(keys, s, l, i, 0, rows) == -1
        assert lib.cdrl_last_error().decode().startswith('traceset_batch:')
    assert _launch([good()], dslot, dlo, index, -1, 8) == -1 and _launch([good()], dslot, dlo, index, 0, 8, set_rows=0) == -1
    torch.cuda.synchronize()
    assert (dst.bits() == CANARY).all()                                                        # nothing was written
    assert _launch([good()], dslot, dlo, index, 0, 8) == 0                                     # and the same arguments, whole, run
    torch.cuda.synchronize()
    assert not (dst.bits() == CANARY).all()
