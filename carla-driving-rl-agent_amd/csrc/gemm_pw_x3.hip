// Float32 pointwise (1x1) convolution on the bf16 matrix pipe by exact operand splitting (gfx950, v_mfma_f32_32x32x16_bf16).
//
// Reference: core/architectures.py:130,140 (Conv2D(k=1)).  The float32 MFMA (v_mfma_f32_32x32x2_f32) runs at 1/16 of the bf16
// rate, and the persistent float32 kernel of gemm_pw.hip is measurably matrix-bound (MfmaUtil 0.36 at K = N = 116,
// profiles/r02_pmc_mfma.json).  Each operand is split exactly into three bf16 numbers and six bf16 products per K = 16 step carry
// the product to float32 accuracy (mfma_x3.h has the split, the step and the argument): 2.7x less matrix-pipe time for the same
// float32 inputs, outputs and HBM traffic.  Parity is asserted against the float64 reference at 1e-5 (tests/test_gpu_ops.py).
// Same skeleton as gemm_pw.hip: persistent workgroups over the row tiles of one BatchNorm group, W (three bf16 planes, packed
// once per weight version) in registers, A split on its way into LDS, BN-apply prologue, statistics epilogue.
#include <stdlib.h>

#include "cdrl_kernels.h"
#include "pack_bodies.h"

namespace cdrl {

struct PwX3Args {
    View A;
    const float* pro_stats;     // [4][G][K] or null
    const __bf16* Wp;           // [3][KP/16][2][128][8]
    const float* bias;
    View C;
    double* part;               // [G][nbpg][2][N] or null
    int N, K, G, Mg, nbpg;
};

// the three packed planes of one chunk (4 columns = 2 pairs) -> LDS row r (LDA elements per row), columns k4 .. k4 + 3: one 8-byte
// store per plane
template <int LDA, int SZ>
__device__ __forceinline__ void pw_x3_store_planes(__bf16 (&As)[3][SZ], int r, int k4, const uint32_t (&hw)[3][2]) {
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x2_t*>(&As[p][r * LDA + k4]) = u32x2_t{hw[p][0], hw[p][1]};
}

// pair h (columns k4 + 2 h, + 1) of a loaded chunk of A, BatchNorm applied (PRO), ready to be split
template <bool PRO, int KP>
__device__ __forceinline__ f32x2 pw_x3_chunk_pair(u32x4_t ra, int h, int k4, int K, const float (&pc)[2][KP]) {
    f32x2 x = f32x2{__uint_as_float(ra[2 * h]), __uint_as_float(ra[2 * h + 1])};
    // columns beyond K inside the last 4-wide chunk (K = 58: 58, 59) are whatever the neighbouring channels of a wider
    // tensor hold: a non-finite value there would survive the zero weights (0 * NaN); zeroed here
    if (k4 + 2 * h >= K) x[0] = 0.0f;
    if (k4 + 2 * h + 1 >= K) x[1] = 0.0f;
    if (PRO) {
        // (columns beyond K carry scale 0 / shift 0 in pc)
        const f32x2 sc = f32x2{pc[0][k4 + 2 * h], pc[0][k4 + 2 * h + 1]}, sh = f32x2{pc[1][k4 + 2 * h], pc[1][k4 + 2 * h + 1]};
        x = __builtin_elementwise_fma(sc, x, sh);
    }
    return x;
}

template <int KP, int NT, bool PRO, bool EPI>
__global__ void __launch_bounds__(256, 2) pw_x3_kernel(PwX3Args a) {
    constexpr int WC = NT, WR = 4 / WC, BM = 32 * WR, KS = KP / 16;
    constexpr int LDA = KP + 8;
    constexpr int CPR = KP / 4;                      // 16-byte chunks (4 floats) per row
    constexpr int NCH = BM * CPR / 256;
    __shared__ __attribute__((aligned(16))) __bf16 As[3][BM * LDA];
    __shared__ float pc[2][KP];
    __shared__ double red[2][4][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave % WR, wc = wave / WR;
    const int lrow = lane & 31, lk = lane >> 5;
    const int g = blockIdx.x / a.nbpg, b = blockIdx.x % a.nbpg;
    const int K = a.K, N = a.N;
    const int64_t mbeg = (int64_t)g * a.Mg, mend = mbeg + a.Mg;
    const int tiles_g = (a.Mg + BM - 1) / BM;
    const int t0 = (int)((int64_t)b * tiles_g / a.nbpg), t1 = (int)((int64_t)(b + 1) * tiles_g / a.nbpg);
    const int n = wc * 32 + lrow;
    bf16x8 breg[3][KS];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int s = 0; s < KS; ++s)
            breg[p][s] = *reinterpret_cast<const bf16x8*>(a.Wp + (((int64_t)(p * KS + s) * 2 + lk) * 128 + n) * 8);
    const float bv = (a.bias && n < N) ? a.bias[n] : 0.0f;
    if (PRO) {
        const int GK = a.G * K;
        for (int k = tid; k < KP; k += 256) {
            pc[0][k] = k < K ? a.pro_stats[2 * GK + g * K + k] : 0.0f;
            pc[1][k] = k < K ? a.pro_stats[3 * GK + g * K + k] : 0.0f;
        }
        __syncthreads();
    }
    double s1 = 0.0, s2 = 0.0;
    const int64_t Mtot = (int64_t)a.G * a.Mg;
    const __amdgpu_buffer_rsrc_t rsA = buffer_rsrc(a.A.p, (int)(Mtot * a.A.ld * 4));
    u32x4_t ra[NCH];
    auto load_tile = [&](int t) {
        const int64_t m0 = mbeg + (int64_t)t * BM;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = tid + 256 * i, r = c / CPR, k4 = 4 * (c % CPR);
            const bool ok = (m0 + r < mend) && (k4 < K);
            const uint32_t off = (uint32_t)(((m0 + r) * a.A.ld + a.A.coff + k4) * 4);
            ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rsA, ok ? off : OOR, 0, 0);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = tid + 256 * i, r = c / CPR, k4 = 4 * (c % CPR);
            uint32_t hw[3][2];
#pragma unroll
            for (int h = 0; h < 2; ++h) x3_split2(pw_x3_chunk_pair<PRO>(ra[i], h, k4, K, pc), hw[0][h], hw[1][h], hw[2][h]);
            pw_x3_store_planes<LDA>(As, r, k4, hw);
        }
    };
    auto compute_tile = [&](int t) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const int ao = (wr * 32 + lrow) * LDA + 8 * lk;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&As[0][ao + 16 * s]);
            const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(&As[1][ao + 16 * s]);
            const bf16x8 a3 = *reinterpret_cast<const bf16x8*>(&As[2][ao + 16 * s]);
            acc = x3_mfma(a1, a2, a3, breg[0][s], breg[1][s], breg[2][s], acc);
        }
        if (n >= N) return;
        const int64_t m0 = mbeg + (int64_t)t * BM + wr * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = acc_row(m0, r, lk);
            if (m < mend) {
                const float v = acc[r] + bv;
                if (EPI) {
                    s1 += (double)v;
                    s2 += (double)v * (double)v;
                }
                a.C.p[m * a.C.ld + a.C.coff + n] = v;
            }
        }
    };
    if (t0 < t1) load_tile(t0);
    for (int t = t0; t < t1; ++t) {
        store_tile();
        __syncthreads();
        if (t + 1 < t1) load_tile(t + 1);
        compute_tile(t);
        __syncthreads();
    }
    if (EPI && a.part) {
        const double f1 = s1 + __shfl_down(s1, 32), f2 = s2 + __shfl_down(s2, 32);
        if (lk == 0) {
            red[0][wave][lrow] = f1;
            red[1][wave][lrow] = f2;
        }
        __syncthreads();
        if (wr == 0 && lk == 0 && n < N) {
            double u1 = 0.0, u2 = 0.0;
#pragma unroll
            for (int w = 0; w < WR; ++w) {
                u1 += red[0][wc * WR + w][lrow];
                u2 += red[1][wc * WR + w][lrow];
            }
            double* p = a.part + ((int64_t)g * a.nbpg + b) * 2 * N;
            p[n] = u1;
            p[N + n] = u2;
        }
    }
}


// K, N up to 256 (the 232-channel convs of stage 2; M = 12288 rows at B = 256): the product is tiny and the persistent form -- one
// workgroup per CU that walks three tiles with all of W in its registers (gemm_pw.hip <128, 4>: 116 float32-MFMA steps of 64 cycles per
// tile and column tile, one wave per SIMD, 26-36 us per launch for 23 MB) -- is a serial chain of load / MFMA / store phases.  Here a
// workgroup takes ONE 32-row tile and one block of 128 columns: W^(column block) as three bf16 planes in registers (16 K steps x 3 planes
// x 4 VGPRs = 192), the A tile split into three planes in LDS (50 KB), 96 bf16 MFMAs of 32 cycles per wave, two workgroups per CU so
// that one loads / stores while the other multiplies.  Grid = (groups x tiles, column blocks); statistics: one partial row per tile.
//
// The weight stream of the two wide kernels (this one and its backward-data twin below).  A workgroup uses every weight fragment ONCE
// (one tile), so holding all 3 x 16 of them (192 VGPRs) buys nothing but the early issue of their loads -- and spilled next to the
// prologue.  A ring of X3_PF K-steps (3 planes each) is requested ahead instead; pw_x3_wload fetches the three fragments of K-step s
// (wp: the lane's fragment of step 0, plane 0 of its column block).
constexpr int X3_PF = 6;
template <int KS>
__device__ __forceinline__ void pw_x3_wload(const __bf16* wp, int s, bf16x8* dst) {
#pragma unroll
    for (int p = 0; p < 3; ++p) dst[p] = *reinterpret_cast<const bf16x8*>(wp + (int64_t)(p * KS + s) * 2 * 128 * 8);
}

template <bool PRO, bool EPI>
__global__ void __launch_bounds__(256, 2) pw_x3_wide_kernel(PwX3Args a) {
    constexpr int KP = 256, BM = 32, KS = KP / 16, LDA = KP + 8, CPR = KP / 4, NCH = BM * CPR / 256;
    __shared__ __attribute__((aligned(16))) __bf16 As[3][BM * LDA];
    __shared__ float pc[2][KP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, lk = lane >> 5;
    const int g = blockIdx.x / a.nbpg, t = blockIdx.x % a.nbpg;        // nbpg = tiles per group
    const int K = a.K, N = a.N;
    const int64_t mbeg = (int64_t)g * a.Mg, mend = mbeg + a.Mg;
    const int64_t m0 = mbeg + (int64_t)t * BM;
    const int nl = wave * 32 + lrow, n = blockIdx.y * 128 + nl;
    const int64_t Mtot = (int64_t)a.G * a.Mg;
    const __amdgpu_buffer_rsrc_t rsA = buffer_rsrc(a.A.p, (int)(Mtot * a.A.ld * 4));
    // the A tile first (HBM / Infinity Cache), the weight fragments (L2) behind it: both in flight before anything is consumed
    u32x4_t ra[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = tid + 256 * i, r = c / CPR, k4 = 4 * (c % CPR);
        const bool ok = (m0 + r < mend) && (k4 < K);
        const uint32_t off = (uint32_t)(((m0 + r) * a.A.ld + a.A.coff + k4) * 4);
        ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rsA, ok ? off : OOR, 0, 0);
    }
    if (PRO) {
        const int GK = a.G * K;
        for (int k = tid; k < KP; k += 256) {
            pc[0][k] = k < K ? a.pro_stats[2 * GK + g * K + k] : 0.0f;
            pc[1][k] = k < K ? a.pro_stats[3 * GK + g * K + k] : 0.0f;
        }
    }
    const __bf16* wp = a.Wp + (int64_t)blockIdx.y * 3 * KS * 2 * 128 * 8 + ((int64_t)lk * 128 + nl) * 8;
    bf16x8 ring[X3_PF][3];
#pragma unroll
    for (int s = 0; s < X3_PF; ++s) pw_x3_wload<KS>(wp, s, ring[s]);
    const float bv = (a.bias && n < N) ? a.bias[n] : 0.0f;
    if (PRO) __syncthreads();
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = tid + 256 * i, r = c / CPR, k4 = 4 * (c % CPR);
        uint32_t hw[3][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) x3_split2(pw_x3_chunk_pair<PRO>(ra[i], h, k4, K, pc), hw[0][h], hw[1][h], hw[2][h]);
        pw_x3_store_planes<LDA>(As, r, k4, hw);
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int ao = lrow * LDA + 8 * lk;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&As[0][ao + 16 * s]);
        const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(&As[1][ao + 16 * s]);
        const bf16x8 a3 = *reinterpret_cast<const bf16x8*>(&As[2][ao + 16 * s]);
        const bf16x8 b1 = ring[s % X3_PF][0], b2 = ring[s % X3_PF][1], b3 = ring[s % X3_PF][2];
        if (s + X3_PF < KS) pw_x3_wload<KS>(wp, s + X3_PF, ring[s % X3_PF]);
        acc = x3_mfma(a1, a2, a3, b1, b2, b3, acc);
    }
    if (n >= N) return;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t m = acc_row(m0, r, lk);
        if (m < mend) {
            const float v = acc[r] + bv;
            if (EPI) {
                s1 += (double)v;
                s2 += (double)v * (double)v;
            }
            a.C.p[m * a.C.ld + a.C.coff + n] = v;
        }
    }
    if (EPI && a.part) {
        const double f1 = s1 + __shfl_down(s1, 32), f2 = s2 + __shfl_down(s2, 32);
        if (lk == 0) {
            double* p = a.part + ((int64_t)g * a.nbpg + t) * 2 * N;
            p[n] = f1;
            p[N + n] = f2;
        }
    }
}


// Backward-data of the same convs, one tile per workgroup (round 6): C[M, N] (+)= dy[M, K] W^T with the BatchNorm backward of the BatchNorm
// behind the conv applied on load -- dy = k1 (mask dz - k2 - xhat(y) k3), dz optionally gathered through the channel shuffle (destination
// columns c, c + 2 and c + 1, c + 3 are adjacent pairs of the source), column sums of dy (the conv's bias gradient) as one partial row per
// tile -- and optionally the backward sums (sum c, sum c xhat(ey)) of the BatchNorm the OUTPUT feeds (EPI) or accumulation onto the old
// output (ACC).  Same contract as pw_nn_kernel<128, 4, PRO_BNBWD, EPI, 0, ACC> (gemm_pw.hip), which ran these shapes as three serial tiles
// per CU on the float32 matrix pipe (32-53 us per launch at M = 12288).  The weight fragments are requested behind the prologue (its raw
// tiles and the 192 fragment VGPRs do not fit together at two workgroups per CU); the co-resident workgroup covers that latency.
struct PwX3BwdArgs {
    View A;                     // dz
    int a_shuffle, a_act;
    const float* a_y;           // raw input of the BatchNorm behind the conv [M][K] dense
    const float* pro_stats;     // [4][G][K]
    const float* pro_coef;      // [3][G][K]
    double* part2;              // [G][nbpg][K] or null
    const __bf16* Wp;           // pw_x3 packing of B(k, n), column blocks of 128
    View C;
    const float* ey;            // EPI: [M][N] dense
    const float* epi_stats;     // EPI: [4][G][N]
    double* part;               // EPI: [G][nbpg][2][N]
    int N, K, G, Mg, nbpg;
};

template <bool SHUF, bool EPI, bool ACC>
__global__ void __launch_bounds__(256, 2) pw_x3_wide_bwd_kernel(PwX3BwdArgs a) {
    constexpr int KP = 256, BM = 32, KS = KP / 16, LDA = KP + 8, CPR = KP / 4, NCH = BM * CPR / 256;
    __shared__ __attribute__((aligned(16))) __bf16 As[3][BM * LDA];
    __shared__ float qc[7][KP];         // mean, invstd, scale, shift, k1, k2, k3 of the dy columns (0 beyond K)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, lk = lane >> 5;
    const int g = blockIdx.x / a.nbpg, t = blockIdx.x % a.nbpg;
    const int K = a.K, N = a.N;
    const int64_t mbeg = (int64_t)g * a.Mg, mend = mbeg + a.Mg;
    const int64_t m0 = mbeg + (int64_t)t * BM;
    const int nl = wave * 32 + lrow, n = blockIdx.y * 128 + nl;
    const int64_t Mtot = (int64_t)a.G * a.Mg;
    const __amdgpu_buffer_rsrc_t rsA = buffer_rsrc(a.A.p, (int)(Mtot * a.A.ld * 4));
    const __amdgpu_buffer_rsrc_t rsY = buffer_rsrc(a.a_y, (int)(Mtot * K * 4));
    // a thread's chunks: rows r0 + 4 i, ALWAYS the same four columns k4 .. k4 + 3 (256 % CPR == 0)
    const int k4 = 4 * (tid % CPR), r0 = tid / CPR;
    const bool kon = k4 < K;                    // (K % 4 == 0: a chunk is valid or not as a whole)
    uint32_t voD0, voD1;                        // byte offsets inside a row: SHUF -> sources of columns (0, 2) and (1, 3); dense -> one 16-byte chunk
    if (SHUF) {
        voD0 = kon ? (uint32_t)shuffle_dst(a.A.coff + k4, a.a_shuffle) * 4u : OOR;
        voD1 = kon ? (uint32_t)shuffle_dst(a.A.coff + k4 + 1, a.a_shuffle) * 4u : OOR;
    } else {
        voD0 = kon ? (uint32_t)(a.A.coff + k4) * 4u : OOR;
        voD1 = OOR;
    }
    const uint32_t voY = kon ? (uint32_t)k4 * 4u : OOR;
    const uint32_t rowA = (uint32_t)a.A.ld * 4u, rowY = (uint32_t)K * 4u;
    u32x4_t rz[NCH], ry[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int64_t m = m0 + r0 + 4 * i;
        const uint32_t msk = m < mend ? 0u : OOR;
        const uint32_t mu = (uint32_t)m;
        if (SHUF) {
            const u32x2_t p0 = __builtin_amdgcn_raw_buffer_load_b64(rsA, (voD0 + mu * rowA) | msk | (voD0 & OOR), 0, 0);
            const u32x2_t p1 = __builtin_amdgcn_raw_buffer_load_b64(rsA, (voD1 + mu * rowA) | msk | (voD1 & OOR), 0, 0);
            rz[i] = u32x4_t{p0[0], p1[0], p0[1], p1[1]};
        } else {
            rz[i] = __builtin_amdgcn_raw_buffer_load_b128(rsA, (voD0 + mu * rowA) | msk | (voD0 & OOR), 0, 0);
        }
        ry[i] = __builtin_amdgcn_raw_buffer_load_b128(rsY, (voY + mu * rowY) | msk | (voY & OOR), 0, 0);
    }
    {
        const int GK = a.G * K;
        for (int i = tid; i < 7 * KP; i += 256) {
            const int q = i / KP, k = i % KP;
            qc[q][k] = k < K ? (q < 4 ? a.pro_stats[q * GK + g * K + k] : a.pro_coef[(q - 4) * GK + g * K + k]) : 0.0f;
        }
    }
    __syncthreads();
    double cs[4] = {0.0, 0.0, 0.0, 0.0};
    {
        const bool relu6 = a.a_act == ACT_RELU6;
        f32x2 cmean[2], cinv[2], csc[2], csh[2], ck1[2], ck2[2], ck3[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            cmean[h] = f32x2{qc[0][k4 + 2 * h], qc[0][k4 + 2 * h + 1]};
            cinv[h] = f32x2{qc[1][k4 + 2 * h], qc[1][k4 + 2 * h + 1]};
            csc[h] = f32x2{qc[2][k4 + 2 * h], qc[2][k4 + 2 * h + 1]};
            csh[h] = f32x2{qc[3][k4 + 2 * h], qc[3][k4 + 2 * h + 1]};
            ck1[h] = f32x2{qc[4][k4 + 2 * h], qc[4][k4 + 2 * h + 1]};
            ck2[h] = f32x2{qc[5][k4 + 2 * h], qc[5][k4 + 2 * h + 1]};
            ck3[h] = f32x2{qc[6][k4 + 2 * h], qc[6][k4 + 2 * h + 1]};
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int r = r0 + 4 * i;
            const bool rok = m0 + r < mend;
            uint32_t hw[3][2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x2 d = f32x2{__uint_as_float(rz[i][2 * h]), __uint_as_float(rz[i][2 * h + 1])};
                const f32x2 yv = f32x2{__uint_as_float(ry[i][2 * h]), __uint_as_float(ry[i][2 * h + 1])};
                if (relu6) {
                    const f32x2 z = __builtin_elementwise_fma(csc[h], yv, csh[h]);      // = fmaf(scale, y, shift) of the forward
                    if (!relu6_open(z[0])) d[0] = 0.0f;
                    if (!relu6_open(z[1])) d[1] = 0.0f;
                }
                const f32x2 xh = (yv - cmean[h]) * cinv[h];
                f32x2 v = ck1[h] * (d - ck2[h] - xh * ck3[h]);          // columns beyond K: every coefficient 0 -> 0
                if (!rok) v = f32x2{0.0f, 0.0f};
                cs[2 * h] += (double)v[0];
                cs[2 * h + 1] += (double)v[1];
                x3_split2(v, hw[0][h], hw[1][h], hw[2][h]);
            }
            pw_x3_store_planes<LDA>(As, r, k4, hw);
        }
    }
    // weight fragments + the epilogue's operands: requested now, consumed behind the barrier
    const __bf16* wp = a.Wp + (int64_t)blockIdx.y * 3 * KS * 2 * 128 * 8 + ((int64_t)lk * 128 + nl) * 8;
    bf16x8 ring[X3_PF][3];                      // ring of K-steps requested ahead (see pw_x3_wide_kernel)
#pragma unroll
    for (int s = 0; s < X3_PF; ++s) pw_x3_wload<KS>(wp, s, ring[s]);
    const bool non = n < N;
    float ext[(EPI || ACC) ? 16 : 1];           // EPI: raw input of the BatchNorm the output feeds; ACC: old output values
    if (EPI || ACC) {
        const __amdgpu_buffer_rsrc_t rsE = EPI ? buffer_rsrc(a.ey, (int)(Mtot * N * 4)) : buffer_rsrc(a.C.p, (int)(Mtot * a.C.ld * 4));
        const uint32_t rowE = EPI ? (uint32_t)N * 4u : (uint32_t)a.C.ld * 4u;
        const uint32_t voE = non ? (uint32_t)((EPI ? 0 : a.C.coff) + n) * 4u : OOR;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = acc_row(m0, r, lk);
            ext[(EPI || ACC) ? r : 0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsE, (voE + (uint32_t)m * rowE) | (m < mend ? 0u : OOR) | (voE & OOR), 0, 0));
        }
    }
    float emean = 0.0f, einv = 0.0f;
    if (EPI && non) {
        emean = a.epi_stats[0 * a.G * N + g * N + n];
        einv = a.epi_stats[1 * a.G * N + g * N + n];
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int ao = lrow * LDA + 8 * lk;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&As[0][ao + 16 * s]);
        const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(&As[1][ao + 16 * s]);
        const bf16x8 a3 = *reinterpret_cast<const bf16x8*>(&As[2][ao + 16 * s]);
        const bf16x8 b1 = ring[s % X3_PF][0], b2 = ring[s % X3_PF][1], b3 = ring[s % X3_PF][2];
        if (s + X3_PF < KS) pw_x3_wload<KS>(wp, s + X3_PF, ring[s % X3_PF]);
        acc = x3_mfma(a1, a2, a3, b1, b2, b3, acc);
    }
    double s1 = 0.0, s2 = 0.0;
    if (non) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = acc_row(m0, r, lk);
            if (m < mend) {
                float v = acc[r];
                if (EPI) {
                    const float xh = (ext[EPI ? r : 0] - emean) * einv;
                    s1 += (double)v;
                    s2 += (double)v * (double)xh;
                }
                if (ACC) v += ext[ACC ? r : 0];
                a.C.p[m * a.C.ld + a.C.coff + n] = v;
            }
        }
    }
    if (EPI && a.part) {
        const double f1 = s1 + __shfl_down(s1, 32), f2 = s2 + __shfl_down(s2, 32);
        if (lk == 0 && non) {
            double* p = a.part + ((int64_t)g * a.nbpg + t) * 2 * N;
            p[n] = f1;
            p[N + n] = f2;
        }
    }
    if (a.part2 && blockIdx.y == 0) {
        // column sums of dy: the four row groups of a column chunk folded in fixed order (the LDS planes are dead: barrier first)
        __syncthreads();
        double* red = reinterpret_cast<double*>(&As[0][0]);     // [4][KP]
#pragma unroll
        for (int e = 0; e < 4; ++e) red[r0 * KP + k4 + e] = cs[e];
        __syncthreads();
        for (int k = tid; k < K; k += 256) a.part2[((int64_t)g * a.nbpg + t) * K + k] = (red[k] + red[KP + k]) + (red[2 * KP + k] + red[3 * KP + k]);
    }
}

static inline int x3_kp(int K) { return K <= 32 ? 32 : (K <= 64 ? 64 : (K <= 128 ? 128 : 256)); }
static inline bool x3_wide(int N, int K) { return K > 128 || N > 128; }
static inline int x3_nt(int N) { return N <= 32 ? 1 : (N <= 64 ? 2 : 4); }

// B(k, n) = w[k * sbk + n * sbn] -> three bf16 planes of MFMA B fragments [3][KP/16][2][128][8]
__global__ void pw_x3_pack_many_kernel(const PwX3Pack* __restrict__ tab) {
    const PwX3Pack d = tab[blockIdx.y];
    pw_x3_pack_body(d, blockIdx.x, gridDim.x);
}

int64_t pw_x3_packed_bytes(int K) { return (int64_t)3 * (x3_kp(K) / 16) * 2 * 128 * 8 * 2; }      // one column block (N <= 128)
int pw_x3_ksteps(int K) { return x3_kp(K) / 16; }       // K = 16 steps per plane of a pack (K <= 128: 2 | 4 | 8)
// (the wide form always runs with KP = 256: its kernel is instantiated for that padding only)
int64_t pw_x3_packed_bytes_n(int K, int N) { return x3_wide(N, K) ? pw_x3_packed_bytes(256) * ((N + 127) / 128) : pw_x3_packed_bytes(K); }

PwX3Pack pw_x3_pack_entry(const float* w, void* wp, int K, int N, int sbk, int sbn) {
    PwX3Pack e;
    e.w = w;
    e.wp = reinterpret_cast<__bf16*>(wp);
    e.K = K;
    e.N = N;
    e.sbk = sbk;
    e.sbn = sbn;
    e.kp = x3_wide(N, K) ? 256 : x3_kp(K);
    return e;
}

int pw_x3_pack_many(const PwX3Pack* tab_dev, int n, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pw_x3_pack_many_kernel, dim3(8, n), dim3(256), 0, st, tab_dev);
    CDRL_LAUNCH_CHECK();
    return 0;
}

static constexpr int X3_OCC = 2;        // workgroups per CU of the grid: pw_x3_kernel's __launch_bounds__(256, 2)

PwX3Plan pw_x3_plan(View A, View C, int G, int Mg, int N, int K, bool pro, bool epi, bool packed, int nbpg) {
    PwX3Plan p{};
    auto refuse = [&p](int code, const char* fmt, auto... args) -> PwX3Plan {
        p.ok = 0;
        p.refusal = code;
        snprintf(p.why, sizeof(p.why), fmt, args...);
        return p;
    };
    p.form = x3_wide(N, K) ? 1 : 0;
    p.kp = p.form ? 256 : x3_kp(K);             // (the wide form always runs with KP = 256: its kernel is instantiated for that padding only)
    p.nt = p.form ? 4 : x3_nt(N);
    p.pro = pro;
    p.epi = epi;
    p.packed_bytes = pw_x3_packed_bytes_n(K, N);
    if (G < 1 || Mg < 1 || N < 1) return refuse(PWX3_REFUSE_DIMS, "pw_x3: nothing to launch for G=%d Mg=%d N=%d (each at least 1)", G, Mg, N);
    p.bm = p.form ? 32 : 32 * (4 / p.nt);
    p.tiles_g = cdiv(Mg, p.bm);
    if (p.form) {
        p.nbpg = p.tiles_g;                     // one workgroup and one partial row per 32-row tile
    } else {
        p.nbpg = 256 * X3_OCC / G;
        if (p.nbpg < 1) p.nbpg = 1;
        if (p.nbpg > p.tiles_g) p.nbpg = p.tiles_g;
    }
    p.gx = G * p.nbpg;
    p.gy = p.form ? cdiv(N, 128) : 1;
    if (K < 4 || K > 256 || N > 256 || K % (p.form ? 4 : 2) != 0)
        return refuse(PWX3_REFUSE_SHAPE, "pw_x3: unsupported shape / alignment K=%d N=%d (K in 4..256, N <= 256, K even, a multiple of 4 in the wide form)", K, N);
    // K <= 128 (the persistent kernel): its A chunks are 16-byte BUFFER loads, which need dword alignment only, and columns beyond K
    // inside the last chunk are zeroed -- so the 58-channel rows of stage 0 (232-byte pitch, channel offset 58) qualify
    const int al = p.form ? 4 : 2;
    if (A.ld % al != 0 || A.coff % al != 0 || (reinterpret_cast<uintptr_t>(A.p) & 15) != 0)
        return refuse(PWX3_REFUSE_ALIGN, "pw_x3: unsupported shape / alignment K=%d N=%d ld=%d coff=%d (multiples of %d, pointer 16-byte aligned)", K, N, A.ld,
                      A.coff, al);
    if (!packed) return refuse(PWX3_REFUSE_PACKED, "pw_x3: unsupported call K=%d N=%d: no packed weights", K, N);
    if ((int64_t)G * Mg * A.ld * 4 >= (int64_t)1 << 31) return refuse(PWX3_REFUSE_2GB, "pw_x3: operand of 2 GB or more (%lld rows)", (long long)G * Mg);
    if (nbpg > 0) {
        if (p.form && nbpg != p.tiles_g)
            return refuse(PWX3_REFUSE_NBPG, "pw_x3: the wide form writes one partial row per 32-row tile (%d), not %d", p.tiles_g, nbpg);
        if (nbpg > p.tiles_g) return refuse(PWX3_REFUSE_NBPG, "pw_x3: %d workgroups per group for %d tiles: some would own none", nbpg, p.tiles_g);
        p.nbpg = nbpg;
        p.gx = G * nbpg;
    }
    p.ok = 1;
    return p;
}

// the prologue / epilogue level of both forward kernels
#define CDRL_X3_PE(KERNEL, ...)                                                                              \
    do {                                                                                                      \
        if (p.pro && p.epi) hipLaunchKernelGGL((KERNEL<__VA_ARGS__ true, true>), grid, block, 0, st, a);      \
        else if (p.pro) hipLaunchKernelGGL((KERNEL<__VA_ARGS__ true, false>), grid, block, 0, st, a);         \
        else if (p.epi) hipLaunchKernelGGL((KERNEL<__VA_ARGS__ false, true>), grid, block, 0, st, a);         \
        else hipLaunchKernelGGL((KERNEL<__VA_ARGS__ false, false>), grid, block, 0, st, a);                   \
    } while (0)

template <int KP>
static void pw_x3_launch(const PwX3Plan& p, const PwX3Args& a, hipStream_t st) {
    const dim3 grid(p.gx, p.gy), block(256);
    if (p.nt == 1) CDRL_X3_PE(pw_x3_kernel, KP, 1, );
    else if (p.nt == 2) CDRL_X3_PE(pw_x3_kernel, KP, 2, );
    else CDRL_X3_PE(pw_x3_kernel, KP, 4, );
}

int pw_x3(View A, const float* pro_stats, const void* Wp, const float* bias, View C, int G, int Mg, int N, int K, double* part,
          hipStream_t st, int nbpg) {
    const PwX3Plan p = pw_x3_plan(A, C, G, Mg, N, K, pro_stats != nullptr, part != nullptr, Wp != nullptr, nbpg);
    if (!p.ok) {
        set_error("%s", p.why);
        return -1;
    }
    PwX3Args a{A, pro_stats, reinterpret_cast<const __bf16*>(Wp), bias, C, part, N, K, G, Mg, p.nbpg};
    if (p.form) {
        const dim3 grid(p.gx, p.gy), block(256);
        CDRL_X3_PE(pw_x3_wide_kernel, );
    } else if (p.kp == 32) {
        pw_x3_launch<32>(p, a, st);
    } else if (p.kp == 64) {
        pw_x3_launch<64>(p, a, st);
    } else {
        pw_x3_launch<128>(p, a, st);
    }
    CDRL_LAUNCH_CHECK();
    return 0;
}
#undef CDRL_X3_PE

PwX3BwdPlan pw_x3_wide_bwd_plan(View dz, View C, int G, int Mg, int N, int K, int shuffle_ctot, bool epi, int accumulate, bool operands) {
    PwX3BwdPlan p{};
    auto refuse = [&p](int code, const char* fmt, auto... args) -> PwX3BwdPlan {
        p.ok = 0;
        p.refusal = code;
        snprintf(p.why, sizeof(p.why), fmt, args...);
        return p;
    };
    p.sh = shuffle_ctot != 0;
    p.epi = epi;
    p.acc = accumulate != 0;
    p.rows = cdiv(Mg, 32);
    if (G < 1 || Mg < 1) return refuse(PWX3B_REFUSE_DIMS, "pw_x3_wide_bwd: nothing to launch for G=%d Mg=%d (each at least 1)", G, Mg);
    p.gx = G * p.rows;
    p.gy = cdiv(N, 128);
    if (!x3_wide(N, K) || K > 256 || N > 256 || (K & 3))
        return refuse(PWX3B_REFUSE_SHAPE, "pw_x3_wide_bwd: unsupported shape / alignment K=%d N=%d (one above 128, both at most 256, K a multiple of 4)", K, N);
    const bool al = shuffle_ctot ? ((dz.coff & 1) == 0 && ((shuffle_ctot >> 1) & 1) == 0) : ((dz.ld & 3) == 0 && (dz.coff & 3) == 0);
    if ((reinterpret_cast<uintptr_t>(dz.p) & 15) || (dz.ld & 1) || !al)
        return refuse(PWX3B_REFUSE_ALIGN, "pw_x3_wide_bwd: unsupported shape / alignment K=%d N=%d ld=%d coff=%d shuffle=%d", K, N, dz.ld, dz.coff, shuffle_ctot);
    if (!operands) return refuse(PWX3B_REFUSE_OPERANDS, "pw_x3_wide_bwd: unsupported call K=%d N=%d: packed weights, y, stats and coef are required", K, N);
    if (p.epi && p.acc) return refuse(PWX3B_REFUSE_EPI_ACC, "pw_x3_wide_bwd: the BatchNorm-sum epilogue and accumulation are not instantiated together (K=%d N=%d)", K, N);
    const int64_t Mtot = (int64_t)G * Mg, lim = (int64_t)1 << 31;
    if (Mtot * dz.ld * 4 >= lim || Mtot * K * 4 >= lim || Mtot * C.ld * 4 >= lim) return refuse(PWX3B_REFUSE_2GB, "pw_x3_wide_bwd: operand of 2 GB or more (%lld rows)", (long long)Mtot);
    p.ok = 1;
    return p;
}

template <bool SH>
static void pw_x3_wide_bwd_launch(const PwX3BwdPlan& p, const PwX3BwdArgs& a, hipStream_t st) {
    const dim3 grid(p.gx, p.gy), block(256);
    if (p.epi) hipLaunchKernelGGL((pw_x3_wide_bwd_kernel<SH, true, false>), grid, block, 0, st, a);
    else if (p.acc) hipLaunchKernelGGL((pw_x3_wide_bwd_kernel<SH, false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((pw_x3_wide_bwd_kernel<SH, false, false>), grid, block, 0, st, a);
}

int pw_x3_wide_bwd(View dz, const PwBnBwd& bb, const void* Wp, View C, int accumulate, int G, int Mg, int N, int K, const float* ey,
                   const float* epi_stats, double* part, hipStream_t st) {
    const PwX3BwdPlan p = pw_x3_wide_bwd_plan(dz, C, G, Mg, N, K, bb.shuffle_ctot, ey != nullptr, accumulate, Wp && bb.y && bb.stats && bb.coef);
    if (!p.ok) {
        set_error("%s", p.why);
        return -1;
    }
    PwX3BwdArgs a;
    a.A = dz;
    a.a_shuffle = bb.shuffle_ctot;
    a.a_act = bb.act;
    a.a_y = bb.y;
    a.pro_stats = bb.stats;
    a.pro_coef = bb.coef;
    a.part2 = bb.part2;
    a.Wp = reinterpret_cast<const __bf16*>(Wp);
    a.C = C;
    a.ey = ey;
    a.epi_stats = epi_stats;
    a.part = part;
    a.N = N;
    a.K = K;
    a.G = G;
    a.Mg = Mg;
    a.nbpg = p.rows;
    if (p.sh) pw_x3_wide_bwd_launch<true>(p, a, st);
    else pw_x3_wide_bwd_launch<false>(p, a, st);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
