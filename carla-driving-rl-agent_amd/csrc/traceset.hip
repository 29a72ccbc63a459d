// Minibatches from a device-resident trace set, gfx950.
//
//  traceset_batch : ONE launch assembles `rows` output rows of up to 8 keys.  A key is stored as slots -- one slot is one time step's
//                   row of row_elems elements, coded as float32, as IEEE half or as a byte index into a palette of 256 float32 bit
//                   patterns -- and an output row is T decoded slots one behind the other:
//                     frame t of output row i reads slot max(slot[r] - (T - 1 - t), lo[r]),  r = index[offset + i]
//                   (slot[r]: the slot of the row's own, newest step; lo[r]: the lowest slot its window may reach, so the first frame
//                   repeats at the start of a trace and a window never reaches into another trace; a trace stored with its time axis
//                   has lo[r] = slot[r] - (T - 1) and gets its own T frames back).  A `direct` key is indexed by r itself (the matrix
//                   of per-row columns: actions, weights, targets), optionally a column range of it (src_stride > row_elems).
// Grid: x = the keys' chunk blocks one key behind the other (a key gets as many as its slot needs, so a 9-element key costs one
// block per frame, not the image's count), y = output row, z = frame.  The source slot is found once per workgroup.
// Decoding copies bit patterns: the palette is a table lookup from LDS (1 KB), a half is widened by v_cvt_f32_f16 (exact for every
// finite half and for infinities) with the NaN patterns rebuilt from the half's own bits, float32 goes through as 32-bit words.
// Per key the host picks 16-byte accesses (one load; one, two or four 16-byte stores) when row_elems, the slot stride and both base
// addresses allow it, the element loop otherwise (a 9-byte slot sits at an odd address).
#include "cdrl_common.h"
#include "../../include/cdrl.h"

namespace cdrl {

constexpr int TS_THREADS = 256;
constexpr int TS_MAX_KEYS = 8;
constexpr int TS_MAX_T = 16;
constexpr int TS_MAX_CHUNKS = 64;       // chunk blocks per (key, row, frame) at most: they stride over the slot

struct TraceKey {
    const void* src;
    const uint32_t* palette;
    uint32_t* dst;
    int64_t row_elems, src_stride;
    int code, T, direct, vec;
};

struct TraceBatchArgs {
    TraceKey key[TS_MAX_KEYS];
    int xend[TS_MAX_KEYS];              // blockIdx.x below xend[k] (and not below xend[k - 1]) belongs to key k
    const int* slot;
    const int* lo;
    const int* index;
    int64_t offset;
    int set_rows, nkeys;
};

__device__ inline uint32_t half_bits_to_float_bits(uint32_t h) {
    if ((h & 0x7fffu) > 0x7c00u)        // NaN: sign, all-ones exponent, the ten payload bits on top of the mantissa
        return ((h & 0x8000u) << 16) | 0x7f800000u | ((h & 0x3ffu) << 13);
    union { _Float16 f; uint16_t u; } in;
    in.u = (uint16_t)h;
    return __float_as_uint((float)in.f);
}

__global__ void __launch_bounds__(TS_THREADS) traceset_batch_kernel(const TraceBatchArgs a) {
    __shared__ uint32_t pal[256];
    int kz = 0, x0 = 0;
    for (int k = 0; k < TS_MAX_KEYS - 1; ++k)
        if (k + 1 < a.nkeys && (int)blockIdx.x >= a.xend[k]) {
            kz = k + 1;
            x0 = a.xend[k];
        }
    const TraceKey k = a.key[kz];
    const int t = blockIdx.z;
    if (t >= k.T) return;
    const int chunk = (int)blockIdx.x - x0, chunks = a.xend[kz] - x0;
    if (k.code == CDRL_TRACE_U8) {
        pal[threadIdx.x] = k.palette[threadIdx.x];
        __syncthreads();
    }
    const int i = blockIdx.y;
    int r = a.index[a.offset + i];
    r = r < 0 ? 0 : (r >= a.set_rows ? a.set_rows - 1 : r);     // the host layer refuses such an index; the read stays inside the tables
    int64_t s = r;
    if (!k.direct) {
        const int own = a.slot[r] - (k.T - 1 - t), low = a.lo[r];
        s = own > low ? own : low;
    }
    const int64_t n = k.row_elems, first = s * k.src_stride;
    uint32_t* d = k.dst + ((int64_t)i * k.T + t) * n;
    const int64_t start = (int64_t)chunk * TS_THREADS + threadIdx.x, step = (int64_t)chunks * TS_THREADS;
    if (k.code == CDRL_TRACE_F32) {
        const uint32_t* sp = static_cast<const uint32_t*>(k.src) + first;
        if (k.vec) {
            const uint4* s4 = reinterpret_cast<const uint4*>(sp);
            uint4* d4 = reinterpret_cast<uint4*>(d);
            for (int64_t j = start; j < (n >> 2); j += step) d4[j] = s4[j];
        } else {
            for (int64_t j = start; j < n; j += step) d[j] = sp[j];
        }
    } else if (k.code == CDRL_TRACE_F16) {
        const uint16_t* sp = static_cast<const uint16_t*>(k.src) + first;
        if (k.vec) {
            const uint4* s4 = reinterpret_cast<const uint4*>(sp);
            uint4* d4 = reinterpret_cast<uint4*>(d);
            for (int64_t j = start; j < (n >> 3); j += step) {
                const uint4 v = s4[j];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                uint32_t o[8];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    o[2 * q] = half_bits_to_float_bits(w[q] & 0xffffu);
                    o[2 * q + 1] = half_bits_to_float_bits(w[q] >> 16);
                }
                d4[2 * j] = make_uint4(o[0], o[1], o[2], o[3]);
                d4[2 * j + 1] = make_uint4(o[4], o[5], o[6], o[7]);
            }
        } else {
            for (int64_t j = start; j < n; j += step) d[j] = half_bits_to_float_bits(sp[j]);
        }
    } else {
        const uint8_t* sp = static_cast<const uint8_t*>(k.src) + first;
        if (k.vec) {
            const uint4* s4 = reinterpret_cast<const uint4*>(sp);
            uint4* d4 = reinterpret_cast<uint4*>(d);
            for (int64_t j = start; j < (n >> 4); j += step) {
                const uint4 v = s4[j];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    d4[4 * j + q] = make_uint4(pal[w[q] & 0xffu], pal[(w[q] >> 8) & 0xffu], pal[(w[q] >> 16) & 0xffu], pal[w[q] >> 24]);
            }
        } else {
            for (int64_t j = start; j < n; j += step) d[j] = pal[sp[j]];
        }
    }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int traceset_batch(const cdrl_traceset_key* keys, int nkeys, const int* slot, const int* lo, const int* index, int64_t offset,
                   int rows, int set_rows, hipStream_t st) {
    if (!keys || !index) {
        set_error("traceset_batch: null keys / index");
        return -1;
    }
    if (nkeys < 1 || nkeys > TS_MAX_KEYS) {
        set_error("traceset_batch: %d keys (1 .. %d per launch)", nkeys, TS_MAX_KEYS);
        return -1;
    }
    if (rows < 1 || rows > 65535) {
        set_error("traceset_batch: rows = %d (1 .. 65535 per launch)", rows);
        return -1;
    }
    if (set_rows < 1 || offset < 0) {
        set_error("traceset_batch: a set of %d rows, offset %lld: need set_rows >= 1 and offset >= 0", set_rows, (long long)offset);
        return -1;
    }
    TraceBatchArgs a;
    int x = 0, Tmax = 1;
    for (int q = 0; q < TS_MAX_KEYS; ++q) {
        a.key[q] = TraceKey{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0};
        a.xend[q] = 0;
    }
    for (int q = 0; q < nkeys; ++q) {
        const cdrl_traceset_key& in = keys[q];
        if (!in.src || !in.dst || (in.code == CDRL_TRACE_U8 && !in.palette)) {
            set_error("traceset_batch: key %d: null src / dst, or a byte-coded key without a palette", q);
            return -1;
        }
        if (in.code != CDRL_TRACE_F32 && in.code != CDRL_TRACE_F16 && in.code != CDRL_TRACE_U8) {
            set_error("traceset_batch: key %d: code %d (0: float32, 1: half, 2: byte palette)", q, in.code);
            return -1;
        }
        if (in.T < 1 || in.T > TS_MAX_T) {
            set_error("traceset_batch: key %d: T = %d (1 .. %d)", q, in.T, TS_MAX_T);
            return -1;
        }
        if (in.row_elems < 1 || in.src_stride < in.row_elems) {
            set_error("traceset_batch: key %d: row_elems = %lld, src_stride = %lld: need 1 <= row_elems <= src_stride", q,
                      (long long)in.row_elems, (long long)in.src_stride);
            return -1;
        }
        if (!in.direct && (!slot || !lo)) {
            set_error("traceset_batch: key %d is windowed: null slot / lo", q);
            return -1;
        }
        if (in.direct && in.T != 1) {
            set_error("traceset_batch: key %d is indexed by row: T = %d, must be 1", q, in.T);
            return -1;
        }
        // elements per 16 source bytes; 16-byte accesses need whole vectors per slot, slots at 16-byte strides and aligned bases
        const int per = in.code == CDRL_TRACE_F32 ? 4 : (in.code == CDRL_TRACE_F16 ? 8 : 16);
        const int vec = in.row_elems % per == 0 && in.src_stride % per == 0 && aligned16(in.src) && aligned16(in.dst);
        a.key[q] = TraceKey{in.src, reinterpret_cast<const uint32_t*>(in.palette), reinterpret_cast<uint32_t*>(in.dst), in.row_elems,
                            in.src_stride, in.code, in.T, in.direct ? 1 : 0, vec};
        int64_t chunks = cdiv64(vec ? in.row_elems / per : in.row_elems, TS_THREADS * 4);
        chunks = chunks < 1 ? 1 : (chunks > TS_MAX_CHUNKS ? TS_MAX_CHUNKS : chunks);
        x += (int)chunks;
        a.xend[q] = x;
        Tmax = in.T > Tmax ? in.T : Tmax;
    }
    a.slot = slot;
    a.lo = lo;
    a.index = index;
    a.offset = offset;
    a.set_rows = set_rows;
    a.nkeys = nkeys;
    hipLaunchKernelGGL(traceset_batch_kernel, dim3((unsigned)x, (unsigned)rows, (unsigned)Tmax), dim3(TS_THREADS), 0, st, a);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl

extern "C" int cdrl_traceset_batch(const cdrl_traceset_key* keys, int nkeys, const int32_t* slot, const int32_t* lo,
                                   const int32_t* index, int64_t offset, int rows, int set_rows, void* stream) {
    return cdrl::traceset_batch(keys, nkeys, slot, lo, index, offset, rows, set_rows, reinterpret_cast<hipStream_t>(stream));
}
