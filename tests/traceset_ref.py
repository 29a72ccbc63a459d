"""Numpy restatement of a device-resident trace set: the slot / lo tables, the three codes and the batch that
cdrl_traceset_batch assembles.  Everything works on float32 BIT PATTERNS (uint32), so NaNs and the two zeros compare."""
import numpy as np

F32, F16, U8 = 0, 1, 2


def bits(a) -> np.ndarray:
    """float32 values -> their patterns; an array of patterns (uint32) goes through."""
    a = np.asarray(a)
    return np.ascontiguousarray(a) if a.dtype == np.uint32 else np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tables(layout, T):
    """layout: [(rows, stacked), ...] -> slot, lo (int32 per row of the set), slots in all.  A per-step trace has one slot per row and
    its first slot as lo; a stacked trace has T slots per row and its row's first frame as lo."""
    slot, lo, s0 = [], [], 0
    for n, stacked in layout:
        for j in range(n):
            if stacked:
                slot.append(s0 + j * T + T - 1)
                lo.append(s0 + j * T)
            else:
                slot.append(s0 + j)
                lo.append(s0)
        s0 += n * T if stacked else n
    return np.asarray(slot, np.int32), np.asarray(lo, np.int32), s0


def half_to_float_bits(h) -> np.ndarray:
    """uint16 half patterns -> uint32 float patterns, one element at a time by the definition of the formats."""
    out = np.empty(np.shape(h), np.uint32)
    flat, res = np.asarray(h, np.uint16).reshape(-1), out.reshape(-1)
    for j, x in enumerate(flat):
        x = int(x)
        sign, e, m = (x >> 15) << 31, (x >> 10) & 31, x & 1023
        if e == 31:
            res[j] = sign | 0x7f800000 | (m << 13)
        elif e == 0:
            res[j] = sign | int(np.float32(m * 2.0 ** -24).view(np.uint32))
        else:
            res[j] = sign | ((e + 112) << 23) | (m << 13)
    return out


def decode(code, coded, palette=None) -> np.ndarray:
    """Coded slots [slots][row_elems] -> uint32 patterns."""
    if code == F32:
        return bits(coded)
    if code == F16:
        if not _HALVES:
            _HALVES.append(half_to_float_bits(np.arange(65536, dtype=np.uint32).astype(np.uint16)))       # every half, once
        return _HALVES[0][np.asarray(coded, np.uint16)]
    return np.asarray(palette, np.uint32)[coded]


_HALVES = []


def batch(decoded, slot, lo, index, offset, rows, T, direct=False) -> np.ndarray:
    """decoded [slots][row_elems] uint32 -> [rows][T][row_elems]: frame t of output row i is slot max(slot[r] - (T - 1 - t), lo[r]),
    r = index[offset + i]; direct: slot r itself, T = 1."""
    out = np.empty((rows, T, decoded.shape[1]), np.uint32)
    for i in range(rows):
        r = int(index[offset + i])
        for t in range(T):
            out[i, t] = decoded[r if direct else max(int(slot[r]) - (T - 1 - t), int(lo[r]))]
    return out
