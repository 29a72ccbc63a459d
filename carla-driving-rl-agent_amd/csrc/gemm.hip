// fp32 MFMA GEMMs for gfx950 (CDNA4): v_mfma_f32_32x32x2_f32, 64-lane wavefronts.
//
// Used for every GEMM-shaped op of the learner (K4 pointwise convs, K8 dense layers, K10 GRU
// projections).  The f32-input MFMA is an exact k-ordered fmaf chain, so the
// results carry plain fp32 rounding (needed for the 1e-4 parity bar) at the matrix-core rate.
//
//   gemm_nn : C[M,N] (+)= A[M,K] * B(k,n) + bias     (forward, backward-data via strided B)
//   gemm_tn : W[K,N]  = sum_m A[m,K]^T D[m,N]        (backward-filter: gemm_tn_direct.hip; split over M, two-stage
//                                                      deterministic reduction, no atomics)
//
// Tiling: 256-thread workgroups = 4 wavefronts.  gemm_nn: 128 x (32*NT) output tile, every
// wave owns 32 rows x NT 32x32 accumulators; A/B staged through LDS in BK=32 slices (A tile
// padded to 33 floats per row -> conflict-free ds_read_b32 for the MFMA A fragment, B fragment
// reads are lane-consecutive).  Awkward channel counts (24/58/92/116/232/464) are zero-padded in
// LDS only; HBM tensors stay dense NHWC.
#include <stdlib.h>

#include "cdrl_kernels.h"
#include "pack_bodies.h"

namespace cdrl {


#define BK 32

// Software-pipelined K loop: the global loads of slice k+1 are issued into registers before the
// MFMAs of slice k run out of the other LDS buffer (one barrier per slice).  BT selects the lane
// order of the B staging so that the global reads stay coalesced for both W (sbn == 1, forward)
// and W^T (sbk == 1, backward-data); the B tile is padded to BN+1 floats per row so that both
// store orders are bank-conflict free.
// WR = wave rows: 4 -> 128-row tile, every wave owns 32 rows x all NT column tiles;
//                 2 -> 64-row tile, 2x2 wave grid, every wave owns 32 rows x NT/2 column tiles (more,
//                      smaller workgroups: balances the late, small-M layers over 256 CUs).
template <int NT, bool BT, bool VEC, int WR>
__global__ void __launch_bounds__(256, 2) gemm_nn_kernel(View A, const float* __restrict__ Bp, int sbk, int sbn,
                                                         const float* __restrict__ bias, View C, int M, int N, int Kfull,
                                                         int accumulate, int kchunk, int64_t cz_stride) {
    // split-K: blockIdx.z owns the K range [kb, kb + K) and writes its own dense partial slab (C.p + z * cz_stride)
    const int kb = blockIdx.z * kchunk;
    const int K = min(kchunk, Kfull - kb);
    A.coff += kb;
    Bp += (int64_t)kb * sbk;
    C.p += (int64_t)blockIdx.z * cz_stride;
    constexpr int BM = 32 * WR;
    constexpr int WC = 4 / WR;                   // wave columns
    constexpr int NTW = NT / WC;                 // column tiles per wave
    constexpr int BN = 32 * NT;
    constexpr int NA = (BM * BK) / 256;          // A elements per thread per slice
    constexpr int NB = (BK * BN) / 256;          // 4*NT B elements per thread per slice
    __shared__ float As[2][BM][BK + 1];
    __shared__ float Bs[2][BK][BN + 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave % WR, wc = wave / WR;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    f32x16 acc[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    const int lrow = lane & 31, lk = lane >> 5;
    float ra[NA], rb[NB];

    auto load_slice = [&](int k0) {
        if (VEC) {
#pragma unroll
            for (int i = 0; i < NA / 2; ++i) {
                const int idx = tid + 256 * i;
                const int r = idx >> 4, kk = (idx & 15) * 2;
                const int64_t m = m0 + r;
                float2 v = make_float2(0.0f, 0.0f);
                if (m < M && (k0 + kk) < K) v = *reinterpret_cast<const float2*>(&A.p[m * A.ld + A.coff + k0 + kk]);
                ra[2 * i] = v.x;
                ra[2 * i + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int idx = tid + 256 * i;
                const int r = idx >> 5, kk = idx & 31;
                const int64_t m = m0 + r;
                ra[i] = (m < M && (k0 + kk) < K) ? A.p[m * A.ld + A.coff + k0 + kk] : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + 256 * i;
            const int kk = BT ? (idx & (BK - 1)) : (idx / BN);
            const int nn = BT ? (idx / BK) : (idx % BN);
            rb[i] = ((k0 + kk) < K && (n0 + nn) < N) ? Bp[(int64_t)(k0 + kk) * sbk + (int64_t)(n0 + nn) * sbn] : 0.0f;
        }
    };
    auto store_slice = [&](int buf) {
        if (VEC) {
#pragma unroll
            for (int i = 0; i < NA / 2; ++i) {
                const int idx = tid + 256 * i;
                const int r = idx >> 4, kk = (idx & 15) * 2;
                As[buf][r][kk] = ra[2 * i];
                As[buf][r][kk + 1] = ra[2 * i + 1];
            }
        } else {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int idx = tid + 256 * i;
                As[buf][idx >> 5][idx & 31] = ra[i];
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + 256 * i;
            const int kk = BT ? (idx & (BK - 1)) : (idx / BN);
            const int nn = BT ? (idx / BK) : (idx % BN);
            Bs[buf][kk][nn] = rb[i];
        }
    };

    load_slice(0);
    store_slice(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < K; k0 += BK) {
        const bool more = (k0 + BK) < K;
        if (more) load_slice(k0 + BK);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float a = As[buf][wr * 32 + lrow][kk + lk];
#pragma unroll
            for (int j = 0; j < NTW; ++j) {
                const float b = Bs[buf][kk + lk][(wc + j * WC) * 32 + lrow];
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[j], 0, 0, 0);
            }
        }
        if (more) store_slice(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    // epilogue: C/D layout col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int n = n0 + (wc + j * WC) * 32 + lrow;
        if (n >= N) continue;
        const float bv = bias ? bias[n] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = acc_row(m0 + wr * 32, r, lk);
            if (m < M) {
                float* c = &C.p[m * C.ld + C.coff + n];
                float v = acc[j][r] + bv;
                if (accumulate) v += *c;
                *c = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// Row-stacked variant for the wide late layers (stage-3 units K = N = 232, head conv 464 -> 768): a (32*RT) x 128
// tile, wave w owns column tile w and RT row tiles, so one B fragment feeds RT MFMAs (LDS reads per MFMA: (RT+1)/RT
// instead of 3/2) and M = 12288 splits into exactly 256 workgroups at RT = 3 (the 64 x 128 tiling gave 384 = 1.5
// rounds over 256 CUs: 33 us for 8.4 us of MFMA time).  A and B slices are fetched with 16-byte loads (the generic
// kernel issues 16 scalar B loads per thread and slice), the K tail (232 = 7*32 + 8) runs only the k-steps that exist.
// Requires K % 4 == 0, 16-byte aligned A rows and weight rows (N % 4 == 0 forward, K % 4 == 0 transposed).
// ------------------------------------------------------------------------------------------
template <int RT, bool BT>
__global__ void __launch_bounds__(256, 2) gemm_nn_rt_kernel(View A, const float* __restrict__ Bp, int sbk, int sbn,
                                                            const float* __restrict__ bias, View C, int M, int N, int K,
                                                            int accumulate) {
    constexpr int BM = 32 * RT, BN = 128;
    constexpr int NA4 = (BM * BK / 4) / 256;     // float4 loads of A per thread and slice (RT)
    constexpr int NB4 = (BK * BN / 4) / 256;     // 4
    __shared__ float As[2][BM][BK + 1];
    __shared__ float Bs[2][BK][BN + 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, lk = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    f32x16 acc[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    // Three-stage pipeline: slice s is multiplied out of LDS while slice s+1 waits in one register set and the global
    // loads of slice s+2 are issued into the other.  With the loads issued only one slice ahead (1.3 us of MFMA work) every
    // slice waited ~1 us for HBM at one workgroup per CU: 29 us for the 12288 x 232 x 232 GEMM whose MFMA time is 9 us.
    float4 ra[2][NA4], rb[2][NB4];
    const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    auto load_slice = [&](int k0, float4* qa, float4* qb) {
#pragma unroll
        for (int i = 0; i < NA4; ++i) {
            const int idx = tid + 256 * i;
            const int r = idx >> 3, kk = (idx & 7) * 4;
            const int64_t m = m0 + r;
            qa[i] = (m < M && (k0 + kk) < K) ? *reinterpret_cast<const float4*>(&A.p[m * A.ld + A.coff + k0 + kk]) : z4;
        }
#pragma unroll
        for (int i = 0; i < NB4; ++i) {
            const int idx = tid + 256 * i;
            if (BT) {       // W^T: contiguous along k
                const int kk = (idx & 7) * 4, nn = idx >> 3;
                qb[i] = ((k0 + kk) < K && (n0 + nn) < N)
                            ? *reinterpret_cast<const float4*>(&Bp[(int64_t)(k0 + kk) * sbk + (int64_t)(n0 + nn) * sbn]) : z4;
            } else {        // W: contiguous along n
                const int kk = idx >> 5, nn = (idx & 31) * 4;
                qb[i] = ((k0 + kk) < K && (n0 + nn) < N)
                            ? *reinterpret_cast<const float4*>(&Bp[(int64_t)(k0 + kk) * sbk + (int64_t)(n0 + nn) * sbn]) : z4;
            }
        }
    };
    auto store_slice = [&](int buf, const float4* qa, const float4* qb) {
#pragma unroll
        for (int i = 0; i < NA4; ++i) {
            const int idx = tid + 256 * i;
            const int r = idx >> 3, kk = (idx & 7) * 4;
            As[buf][r][kk] = qa[i].x;
            As[buf][r][kk + 1] = qa[i].y;
            As[buf][r][kk + 2] = qa[i].z;
            As[buf][r][kk + 3] = qa[i].w;
        }
#pragma unroll
        for (int i = 0; i < NB4; ++i) {
            const int idx = tid + 256 * i;
            if (BT) {
                const int kk = (idx & 7) * 4, nn = idx >> 3;
                Bs[buf][kk][nn] = qb[i].x;
                Bs[buf][kk + 1][nn] = qb[i].y;
                Bs[buf][kk + 2][nn] = qb[i].z;
                Bs[buf][kk + 3][nn] = qb[i].w;
            } else {
                const int kk = idx >> 5, nn = (idx & 31) * 4;
                Bs[buf][kk][nn] = qb[i].x;
                Bs[buf][kk][nn + 1] = qb[i].y;
                Bs[buf][kk][nn + 2] = qb[i].z;
                Bs[buf][kk][nn + 3] = qb[i].w;
            }
        }
    };
    auto mma_slice = [&](int buf, int k0) {
        const int kmax = min(BK, K - k0);        // K % 4 == 0 -> even
        if (kmax == BK) {
#pragma unroll
            for (int h = 0; h < BK; h += 16) {
                float bf[8], af[8][RT];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    bf[q] = Bs[buf][h + 2 * q + lk][wave * 32 + lrow];
#pragma unroll
                    for (int i = 0; i < RT; ++i) af[q][i] = As[buf][i * 32 + lrow][h + 2 * q + lk];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q)
#pragma unroll
                    for (int i = 0; i < RT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q][i], bf[q], acc[i], 0, 0, 0);
            }
        } else {
            for (int kk = 0; kk < kmax; kk += 2) {
                const float b = Bs[buf][kk + lk][wave * 32 + lrow];
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    const float a = As[buf][i * 32 + lrow][kk + lk];
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
                }
            }
        }
    };

    load_slice(0, ra[0], rb[0]);
    if (BK < K) load_slice(BK, ra[1], rb[1]);
    store_slice(0, ra[0], rb[0]);
    __syncthreads();
    // invariant at the top of step s (k0 = s*BK): LDS[s & 1] holds slice s, register set (s+1) & 1 holds slice s+1
    for (int k0 = 0; k0 < K; k0 += 2 * BK) {
        // even step: LDS 0, next slice in set 1, fetch slice s+2 into set 0
        if (k0 + 2 * BK < K) load_slice(k0 + 2 * BK, ra[0], rb[0]);
        mma_slice(0, k0);
        if (k0 + BK < K) store_slice(1, ra[1], rb[1]);
        __syncthreads();
        if (k0 + BK >= K) break;
        // odd step: LDS 1, next slice in set 0, fetch slice s+2 into set 1
        if (k0 + 3 * BK < K) load_slice(k0 + 3 * BK, ra[1], rb[1]);
        mma_slice(1, k0 + BK);
        if (k0 + 2 * BK < K) store_slice(0, ra[0], rb[0]);
        __syncthreads();
    }
    const int n = n0 + wave * 32 + lrow;
    if (n >= N) return;
    const float bv = bias ? bias[n] : 0.0f;
#pragma unroll
    for (int i = 0; i < RT; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = acc_row(m0 + i * 32, r, lk);
            if (m < M) {
                float* c = &C.p[m * C.ld + C.coff + n];
                float v = acc[i][r] + bv;
                if (accumulate) v += *c;
                *c = v;
            }
        }
    }
}

template <int RT>
static void launch_nn_rt(bool bt, hipStream_t st, View A, const float* Bp, int sbk, int sbn, const float* bias, View C, int M,
                         int N, int K, int acc) {
    dim3 grid(cdiv(M, 32 * RT), cdiv(N, 128));
    if (bt) hipLaunchKernelGGL((gemm_nn_rt_kernel<RT, true>), grid, dim3(256), 0, st, A, Bp, sbk, sbn, bias, C, M, N, K, acc);
    else hipLaunchKernelGGL((gemm_nn_rt_kernel<RT, false>), grid, dim3(256), 0, st, A, Bp, sbk, sbn, bias, C, M, N, K, acc);
}

template <int NT, int WR>
static void launch_nn(bool bt, bool vec, dim3 grid, hipStream_t st, View A, const float* Bp, int sbk, int sbn,
                      const float* bias, View C, int M, int N, int K, int acc, int kchunk, int64_t czs) {
    if (bt) {
        if (vec) hipLaunchKernelGGL((gemm_nn_kernel<NT, true, true, WR>), grid, dim3(256), 0, st, A, Bp, sbk, sbn, bias, C, M, N, K, acc, kchunk, czs);
        else hipLaunchKernelGGL((gemm_nn_kernel<NT, true, false, WR>), grid, dim3(256), 0, st, A, Bp, sbk, sbn, bias, C, M, N, K, acc, kchunk, czs);
    } else {
        if (vec) hipLaunchKernelGGL((gemm_nn_kernel<NT, false, true, WR>), grid, dim3(256), 0, st, A, Bp, sbk, sbn, bias, C, M, N, K, acc, kchunk, czs);
        else hipLaunchKernelGGL((gemm_nn_kernel<NT, false, false, WR>), grid, dim3(256), 0, st, A, Bp, sbk, sbn, bias, C, M, N, K, acc, kchunk, czs);
    }
}

// C(view) (+)= bias + sum_z part[z]  (fixed order)
// act_out (dense [M][N], optional): the layer's activation of the reduced value as well -- act_value (cdrl_common.h), the function
// act_fwd_kernel (bn.hip) applies, which was a launch of its own behind every split-K Dense layer
__global__ void splitk_reduce_kernel(const float* __restrict__ part, int nsplit, int M, int N, const float* __restrict__ bias,
                                     View C, int accumulate, float* __restrict__ act_out, int act) {
    const int64_t n = (int64_t)M * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / N;
        const int c = (int)(i - m * N);
        float s = bias ? bias[c] : 0.0f;
        for (int z = 0; z < nsplit; ++z) s += part[(int64_t)z * n + i];
        float* o = &C.p[m * C.ld + C.coff + c];
        const float x = accumulate ? *o + s : s;
        *o = x;
        if (act_out) act_out[i] = act_value(x, act);
    }
}

// split-K is for few output tiles and a long reduction (GRU projections: M = B or T*B, K = 256 / 768), in at most NN_MAX_SPLIT slabs
static constexpr int NN_MAX_SPLIT = 8;
static inline bool nn_splitk_shape(int M, int K) { return M <= 2048 && K >= 256; }

int64_t gemm_nn_splitk_elems(int M, int N, int K) {
    if (!nn_splitk_shape(M, K)) return 0;
    return (int64_t)NN_MAX_SPLIT * M * N;
}

NnPlan gemm_nn_plan(View A, const float* Bp, int sbk, int sbn, int M, int N, int K, bool has_workspace) {
    NnPlan p{};
    p.kernel = -1;
    if (M <= 0 || N <= 0) return p;
    int nt = cdiv(N, 32);
    if (nt > 4) nt = 4;
    // balance column blocks: e.g. N=232 -> 2 blocks of 4 tiles; N=92 -> 1 block of 3 tiles
    const int ncb = cdiv(N, 32 * nt);
    nt = cdiv(cdiv(N, ncb), 32);
    const uintptr_t pa = reinterpret_cast<uintptr_t>(A.p), pb = reinterpret_cast<uintptr_t>(Bp);
    p.NT = nt;
    p.gy = cdiv(N, 32 * nt);
    p.gz = 1;
    p.kchunk = 1 << 30;
    p.BT = sbn != 1;
    p.VEC = (K % 2 == 0) && (A.ld % 2 == 0) && (A.coff % 2 == 0) && ((pa & 7) == 0);
    p.a16 = (K % 4 == 0) && (A.ld % 4 == 0) && (A.coff % 4 == 0) && ((pa & 15) == 0);
    p.b16 = ((pb & 15) == 0) && (p.BT ? (sbk == 1 && sbn % 4 == 0) : (sbn == 1 && sbk % 4 == 0 && N % 4 == 0));
    // 64-row tiles (2 x 2 waves) whenever the column-tile count is even: measured, they win at every learner shape
    p.WR = nt % 2 == 0 ? 2 : 4;
    p.gx = cdiv(M, 32 * p.WR);
    if (has_workspace && nn_splitk_shape(M, K) && nt % 2 == 0) {
        // partial slabs + fixed-order reduction, enough slabs to fill the chip (the 4x2-workgroup launch took 60 us for 0.1 GFLOP)
        int nsplit = cdiv(512, p.gx * p.gy);
        if (nsplit > NN_MAX_SPLIT) nsplit = NN_MAX_SPLIT;
        const int kchunk = cdiv(cdiv(K, nsplit), 32) * 32;
        nsplit = cdiv(K, kchunk);
        if (nsplit > 1) {
            const int64_t n = (int64_t)M * N;
            p.kernel = 2;
            p.gz = nsplit;
            p.kchunk = kchunk;
            p.ws_elems = nsplit * n;
            p.reduce_grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
            p.act_fused = 1;
            return p;
        }
    }
    // row-stacked tiles for the wide late layers
    if (N >= 129 && K >= 64 && M >= 2048 && p.a16 && p.b16) {
        p.kernel = 1;
        p.NT = 3;           // RT
        p.WR = 0;
        p.VEC = 0;
        p.gx = cdiv(M, 96);
        p.gy = cdiv(N, 128);
        return p;
    }
    p.kernel = 0;
    return p;
}

int gemm_nn(View A, const float* Bp, int sbk, int sbn, const float* bias, View C, int M, int N, int K,
            int accumulate, hipStream_t st, float* splitk_ws, float* act_out, int act, bool* act_done) {
    if (act_done) *act_done = false;
    const NnPlan p = gemm_nn_plan(A, Bp, sbk, sbn, M, N, K, splitk_ws != nullptr);
    if (p.kernel < 0) return 0;
    if (p.kernel == 1) {
        launch_nn_rt<3>(p.BT, st, A, Bp, sbk, sbn, bias, C, M, N, K, accumulate);
        CDRL_LAUNCH_CHECK();
        return 0;
    }
    // kernel 2: every slab is a plain product into its own dense [M][N] piece of the workspace
    const bool split = p.kernel == 2;
    const View out = split ? make_view(splitk_ws, N) : C;
    const float* kb = split ? nullptr : bias;
    const int kacc = split ? 0 : accumulate;
    const int64_t czs = split ? (int64_t)M * N : 0;
    const dim3 grid(p.gx, p.gy, p.gz);
    if (p.WR == 2) {
        if (p.NT == 2) launch_nn<2, 2>(p.BT, p.VEC, grid, st, A, Bp, sbk, sbn, kb, out, M, N, K, kacc, p.kchunk, czs);
        else launch_nn<4, 2>(p.BT, p.VEC, grid, st, A, Bp, sbk, sbn, kb, out, M, N, K, kacc, p.kchunk, czs);
    } else {
        if (p.NT == 1) launch_nn<1, 4>(p.BT, p.VEC, grid, st, A, Bp, sbk, sbn, kb, out, M, N, K, kacc, p.kchunk, czs);
        else launch_nn<3, 4>(p.BT, p.VEC, grid, st, A, Bp, sbk, sbn, kb, out, M, N, K, kacc, p.kchunk, czs);
    }
    CDRL_LAUNCH_CHECK();
    if (split) {
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)p.reduce_grid), dim3(256), 0, st, splitk_ws, p.gz, M, N, bias, C, accumulate,
                           act_done ? act_out : nullptr, act);
        CDRL_LAUNCH_CHECK();
        if (act_done && act_out) *act_done = true;
    }
    return 0;
}

// (the filter-gradient GEMM lives in gemm_tn_direct.hip; its split-M partials are reduced here)
// (CX output lanes) x (1024/CX split lanes) per block: the split partials are summed in parallel and combined in a
// fixed order (deterministic).  CX = 4 when there are few outputs (see reduce_partials_kernel in bn.hip).
template <int CX>
__global__ void __launch_bounds__(1024) tn_reduce_kernel(const float* __restrict__ part, int nsplit, int64_t n,
                                                         int64_t stride, float* __restrict__ out, int accumulate) {
    constexpr int PY = 1024 / CX;
    __shared__ double sm[PY][CX];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int64_t i = (int64_t)blockIdx.x * CX + tx;
    double s = 0.0;
    if (i < n) {
        for (int p0 = ty; p0 < nsplit; p0 += PY * 8) {       // 8 independent loads in flight per thread
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int p = p0 + u * PY;
                v[u] = p < nsplit ? part[(int64_t)p * stride + i] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (double)v[u];
        }
    }
    sm[ty][tx] = s;
    __syncthreads();
    if (PY > 64) {
        if (ty < 64) {
            double a = 0.0;
            for (int y = ty; y < PY; y += 64) a += sm[y][tx];
            sm[ty][tx] = a;
        }
        __syncthreads();
    }
    if (i < n && ty == 0) {
        s = 0.0;
#pragma unroll
        for (int y = 0; y < 64; ++y) s += sm[y][tx];
        out[i] = accumulate ? out[i] + (float)s : (float)s;
    }
}

// float4 variant: TX lanes x 4 consecutive outputs (16-byte loads, 256-byte row segments at TX = 16) x 256/TX split
// lanes, 8 independent 16-byte loads in flight per thread.  The CX = 16 scalar kernel above read 64-byte segments with
// 1024-thread blocks: 31 us for the 384 x 116 x 116 partials of a stage-1 filter gradient (0.66 TB/s).
template <int TX>
__global__ void __launch_bounds__(256) tn_reduce_v4_kernel(const float* __restrict__ part, int nsplit, int64_t n,
                                                           int64_t stride, float* __restrict__ out, int accumulate) {
    constexpr int TY = 256 / TX;
    __shared__ double sm[TY][TX][4];
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int64_t i = ((int64_t)blockIdx.x * TX + tx) * 4;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (i < n) {
        const float* src = part + i;
        for (int p0 = ty; p0 < nsplit; p0 += TY * 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                // clamped address + select AFTER the load: a conditional load becomes a branch with its own s_waitcnt
                // (the 8 loads were issued one at a time)
                const int p = p0 + u * TY;
                v[u] = *reinterpret_cast<const float4*>(src + (int64_t)min(p, nsplit - 1) * stride);
                if (p >= nsplit) v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s0 += (double)v[u].x;
                s1 += (double)v[u].y;
                s2 += (double)v[u].z;
                s3 += (double)v[u].w;
            }
        }
    }
    sm[ty][tx][0] = s0;
    sm[ty][tx][1] = s1;
    sm[ty][tx][2] = s2;
    sm[ty][tx][3] = s3;
    __syncthreads();
    // fixed-order fold over the TY split lanes: thread (c, tx) of the first 4*TX threads owns output i + c
    if (threadIdx.x < 4 * TX) {
        const int c = threadIdx.x % 4, x = threadIdx.x / 4;
        const int64_t o = ((int64_t)blockIdx.x * TX + x) * 4 + c;
        if (o < n) {
            double s = 0.0;
#pragma unroll 8
            for (int y = 0; y < TY; ++y) s += sm[y][x][c];
            out[o] = accumulate ? out[o] + (float)s : (float)s;
        }
    }
}

// few partials (batch-sized GEMMs: GRU / dense weight gradients with 1-8 row splits): one thread per 4 outputs walks
// the partials in order.  The lane-parallel kernels above spend 1024 threads per 16 outputs on 4 partials: 97 us for
// the 768 x 768 GRU kernel gradient.
__global__ void __launch_bounds__(256) tn_reduce_few_kernel(const float* __restrict__ part, int nsplit, int64_t n,
                                                            int64_t stride, float* __restrict__ out, int accumulate) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int p0 = 0; p0 < nsplit; p0 += 4) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
        {
            v[u] = *reinterpret_cast<const float4*>(part + (int64_t)min(p0 + u, nsplit - 1) * stride + i);
            if (p0 + u >= nsplit) v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s0 += (double)v[u].x;
            s1 += (double)v[u].y;
            s2 += (double)v[u].z;
            s3 += (double)v[u].w;
        }
    }
    float4 o = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
    if (accumulate) {
        o.x += out[i];
        o.y += out[i + 1];
        o.z += out[i + 2];
        o.w += out[i + 3];
    }
    out[i] = o.x;
    out[i + 1] = o.y;
    out[i + 2] = o.z;
    out[i + 3] = o.w;
}

ReduceF32Plan reduce_partials_f32_plan(uintptr_t part_addr, int nparts, int64_t n, int64_t stride) {
    const bool v4 = n % 4 == 0 && stride % 4 == 0 && (part_addr & 15) == 0;
    if (v4 && nparts < 16 && n >= 4096) return {0, (unsigned)cdiv64(n, 1024), 256, 1};
    if (v4 && nparts >= 16) {
        if (cdiv64(n, 64) >= 160) return {1, (unsigned)cdiv64(n, 64), 256, 1};
        if (cdiv64(n, 16) >= 128 || nparts < 128) return {2, (unsigned)cdiv64(n, 16), 256, 1};
        return {3, (unsigned)cdiv64(n, 4), 256, 1};
    }
    if (cdiv64(n, 16) >= 128 || nparts <= 64) return {4, (unsigned)cdiv64(n, 16), 16, 64};
    return {5, (unsigned)cdiv64(n, 4), 4, 256};
}

int reduce_partials_f32(const float* part, int nparts, int64_t n, int64_t stride, float* out, int accumulate,
                        hipStream_t st) {
    const ReduceF32Plan p = reduce_partials_f32_plan(reinterpret_cast<uintptr_t>(part), nparts, n, stride);
    const dim3 grid(p.grid), blk(p.bx, p.by);
    switch (p.form) {
        case 0: hipLaunchKernelGGL(tn_reduce_few_kernel, grid, blk, 0, st, part, nparts, n, stride, out, accumulate); break;
        case 1: hipLaunchKernelGGL(tn_reduce_v4_kernel<16>, grid, blk, 0, st, part, nparts, n, stride, out, accumulate); break;
        case 2: hipLaunchKernelGGL(tn_reduce_v4_kernel<4>, grid, blk, 0, st, part, nparts, n, stride, out, accumulate); break;
        case 3: hipLaunchKernelGGL(tn_reduce_v4_kernel<1>, grid, blk, 0, st, part, nparts, n, stride, out, accumulate); break;
        case 4: hipLaunchKernelGGL(tn_reduce_kernel<16>, grid, blk, 0, st, part, nparts, n, stride, out, accumulate); break;
        default: hipLaunchKernelGGL(tn_reduce_kernel<4>, grid, blk, 0, st, part, nparts, n, stride, out, accumulate); break;
    }
    CDRL_LAUNCH_CHECK();
    return 0;
}

// one 32 x 32 tile per block through LDS; grid = (tiles of the largest matrix, matrices)
__global__ void __launch_bounds__(256) transpose_many_kernel(const PwTranspose* __restrict__ tab) {
    __shared__ float t[32][33];
    const PwTranspose d = tab[blockIdx.y];
    transpose_body(d, blockIdx.x, t);
}

int transpose_many(const PwTranspose* tab_dev, int n, int tiles, hipStream_t st) {
    if (n <= 0 || tiles <= 0) return 0;
    hipLaunchKernelGGL(transpose_many_kernel, dim3(tiles, n), dim3(256), 0, st, tab_dev);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
