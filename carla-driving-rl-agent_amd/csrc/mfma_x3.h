// Shared pieces of the MFMA GEMM family (gfx950, v_mfma_f32_32x32x16_bf16): vector types, buffer-descriptor helpers, the 32x32
// accumulator row map, and the float32-on-the-bf16-pipe ("x3") operand split and six-product step.
//
// The x3 accuracy argument, stated once.  A float32 number is the EXACT sum of three bf16 numbers (3 x 8 significand bits):
//     a = a1 + a2 + a3,   b = b1 + b2 + b3            (a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2))
// Both subtractions are exact (Sterbenz-style: the residue of a round-to-nearest fits the remaining bits); only the last
// rounding, to a3, can lose anything, and that is below 2^-24 |a|.  Then
//     a b = a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a2 b2 + a3 b1) + O(2^-24 |a b|)
// so six bf16 products accumulated in float32 carry the product to float32 accuracy; the three dropped terms (a2 b3, a3 b2,
// a3 b3) are below half an ulp of the product.  The products go into the accumulator SMALLEST TERMS FIRST (the three 2^-16
// terms, the two 2^-8 terms, then a1 b1): small terms added to a small running sum keep their low bits, added behind the
// large term they would lose them.  Six K = 16 steps of 32 cycles replace eight K = 2 float32-MFMA steps of 64 cycles.
// The result is not bit-identical to a k-ordered fmaf chain (it is at least as accurate); the ORDER of the six products is part
// of every kernel's result bits, so x3_mfma() below is the one place it is written -- gemm_tn_lds.hip alone keeps another order.
#pragma once
#include "cdrl_kernels.h"

namespace cdrl {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));     // arithmetic on pairs compiles to v_pk_{add,mul,fma}_f32
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// A buffer load at this offset is out of range of every descriptor below (hosts check that operands are < 2 GB): it reads 0, a
// store is dropped.  Masked lanes point here instead of branching.
constexpr uint32_t OOR = 0x80000000u;

// raw buffer descriptor over `bytes` bytes at p (stride 0, dword 3 = 0x00020000: 32-bit raw access, out-of-range checked).
// The count is an int on purpose: callers narrow their 64-bit byte counts at the call, as the descriptor does.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// C/D layout of the 32x32 MFMAs: column = lane & 31, row of accumulator register r = (r & 3) + 8 (r >> 2) + 4 lk, lk = lane >> 5.
// acc_row(r): the register's part alone; acc_row(base, r, lk): the full row on top of a tile's first row (int or int64_t).
__device__ __forceinline__ constexpr int acc_row(int r) { return (r & 3) + 8 * (r >> 2); }
template <class T>
__device__ __forceinline__ T acc_row(T base, int r, int lk) { return base + (r & 3) + 8 * (r >> 2) + 4 * lk; }

// x = h1 + h2 + h3
__device__ __forceinline__ void x3_split(float x, __bf16& h1, __bf16& h2, __bf16& h3) {
    h1 = (__bf16)x;
    const float r1 = x - (float)h1;             // exact
    h2 = (__bf16)r1;
    h3 = (__bf16)(r1 - (float)h2);              // exact difference, final rounding below 2^-24 |x|
}

// a packed bf16 pair {lo = first element, hi = second} <-> two floats: widening by shift / mask, rounding to nearest even
__device__ __forceinline__ f32x2 bf16x2_widen(uint32_t w) { return f32x2{__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)}; }
__device__ __forceinline__ uint32_t bf16x2_pack(f32x2 v) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2)); }

// The same split on a pair, results as packed dwords: the arithmetic compiles to v_pk_add_f32, the three conversions to one
// v_cvt_pk_bf16_f32 each, and the conversion results ARE the packed LDS words (no per-element repacking; DESIGN.md has the
// isolated timing).
__device__ __forceinline__ void x3_split2(f32x2 x, uint32_t& h1, uint32_t& h2, uint32_t& h3) {
    h1 = bf16x2_pack(x);
    const f32x2 r1 = x - bf16x2_widen(h1);      // exact
    h2 = bf16x2_pack(r1);
    h3 = bf16x2_pack(r1 - bf16x2_widen(h2));
}

// Operand fragments of v_mfma_f32_32x32x16_bf16 whose CONTRACTION index runs down the ROWS of a row-major LDS plane [m][ld]
// (ds_read_b64_tr_b16: per 16 lanes a block of 4 rows x 16 columns, delivered column-major).  Both operands have the same shape
// -- lane l owns index l & 31 (row of A / column of B) and contraction elements 8 (l >> 5) + j, j = 0..7 -- so one pair serves both:
//     tr_frag_off(lane, ld):  element offset of the lane's address inside a block of 16 rows x 32 columns:
//                             row 8 (l >> 5) + ((l & 15) >> 2), column 16 ((l >> 4) & 1) + 4 (l & 3)
//     tr_frag(p):             p = plane + (first row) * ld + (first column) + tr_frag_off; element j of the result is row
//                             8 (l >> 5) + j, column l & 31 of the block: two reads, rows +0..3 and +4..7, contraction order as a
//                             16-byte read of the transposed plane would give
// Conditions: every lane of the wave active (the gather crosses lanes), ld a multiple of 4 elements and the block's first column a
// multiple of 4 (8-byte aligned lane addresses).  `ld` is a template argument so that the second read is an offset: immediate.
__device__ __forceinline__ int tr_frag_off(int lane, int ld) { return (8 * (lane >> 5) + ((lane & 15) >> 2)) * ld + 16 * ((lane >> 4) & 1) + 4 * (lane & 3); }
template <int LD>
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* p) {
    static_assert(LD % 4 == 0, "8-byte aligned lane addresses");
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + 4 * LD));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// one K = 16 step of the split product, smallest terms first (see the file header)
__device__ __forceinline__ f32x16 x3_mfma(bf16x8 a1, bf16x8 a2, bf16x8 a3, bf16x8 b1, bf16x8 b2, bf16x8 b3, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
}

}  // namespace cdrl
