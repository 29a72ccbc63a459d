// NT-Xent (SimCLR) loss on a batch of embeddings, forward + analytic backward (gfx950; include/cdrl.h).
//
//   zn_i = z_i / max(||z_i||, 1e-12);  s_ij = zn_i . zn_j / temperature;  l_i = log sum_{j != i} exp(s_ij) - s_{i,pair(i)};
//   L = mean_i l_i;  pair(i) = (i + B/2) mod B.
//
// The B x B similarity matrix is never stored.  Five launches, every reduction in a fixed order, no atomics:
//   1. ntxent_normalize_kernel  one wave per row: ||z_i|| (double sum), zn
//   2. ntxent_tile_stats_kernel one workgroup per 64 x 64 tile of S: per row of the tile (max, sum exp, sum of negative cosines,
//                               largest negative logit) over the tile's columns, and the positive's cosine where the tile holds it
//   3. ntxent_rows_kernel       one workgroup: per row the column tiles folded in order -> lse_i; the metrics, row sums in double
//   4. ntxent_grad_tile_kernel  one workgroup per (row tile, group of column tiles): the tile of S again, its coefficients
//                               c_ij = (p_ij + p_ji - 2 [j == pair(i)]) / (B temperature) (S is symmetric: p_ji = exp(s_ij - lse_j)),
//                               then the partial dL/dzn_i = sum_j c_ij zn_j over the group's columns
//   5. ntxent_dz_kernel         one wave per row: the groups' partials added in order, the normalisation's backward, grad_scale
// Plain float32 FMA through LDS-staged tiles (K = D): exact float32 products keep the 1e-5 bound with room (measured figures:
// DESIGN.md 6.11); at B = 2048 the three GEMM-shaped phases are ~13 GFLOP, small next to the trunk pass of that batch.
#include "cdrl_kernels.h"

namespace cdrl {

namespace {
constexpr int NX_TILE = 64;       // rows and columns of one tile of S
constexpr int NX_KC = 32;         // K chunk staged in LDS
constexpr int NX_LD = 68;         // LDS row stride of a staged chunk (floats; keeps 16-byte alignment)
constexpr int NX_DC = 512;        // columns of dL/dzn one workgroup of the gradient kernel accumulates
constexpr int NX_MAXB = 2048;

struct NtxentPlan {
    int nct;        // column (= row) tiles
    int tpb;        // column tiles per workgroup of the gradient kernel
    int js;         // column groups = partial planes of dL/dzn
    int64_t o_zn, o_norm, o_lse, o_pos, o_part, o_dpart, total;     // float offsets inside the workspace
};

inline int64_t up4(int64_t n) { return (n + 3) / 4 * 4; }

NtxentPlan ntxent_plan(int B, int D) {
    NtxentPlan p;
    p.nct = cdiv(B, NX_TILE);
    p.tpb = p.nct / 8 > 0 ? p.nct / 8 : 1;
    p.js = cdiv(p.nct, p.tpb);
    int64_t o = 0;
    p.o_zn = o;     o += up4((int64_t)B * D);
    p.o_norm = o;   o += up4(B);
    p.o_lse = o;    o += up4(B);
    p.o_pos = o;    o += up4(B);
    p.o_part = o;   o += (int64_t)p.nct * B * 4;
    p.o_dpart = o;  o += up4((int64_t)p.js * B * D);
    p.total = o;
    return p;
}
}  // namespace

__global__ void __launch_bounds__(256) ntxent_normalize_kernel(const float* __restrict__ z, int B, int D, float* __restrict__ zn,
                                                               float* __restrict__ norm) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    const float* zi = z + (int64_t)i * D;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = (double)zi[d];
        acc += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    const float n = (float)sqrt(acc);
    const float den = fmaxf(n, 1e-12f);
    for (int d = lane; d < D; d += 64) zn[(int64_t)i * D + d] = zi[d] / den;
    if (lane == 0) norm[i] = n;
}

// acc[a][b] = zn_{i0 + ty*4 + a} . zn_{j0 + tx*4 + b} (ty = tid >> 4, tx = tid & 15); rows at or behind B and columns of zn at or
// behind D read as 0.  As / Bs: [NX_KC][NX_LD], chunk element k of row r at [k][r].
__device__ __forceinline__ void ntxent_dot_tile(const float* __restrict__ zn, int B, int D, int i0, int j0, float (*As)[NX_LD],
                                                float (*Bs)[NX_LD], float acc[4][4]) {
    const int tid = threadIdx.x;
    const int ty = tid >> 4, tx = tid & 15;
    const int kk = tid & 31, rb = tid >> 5;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
    for (int k0 = 0; k0 < D; k0 += NX_KC) {
        const bool kin = k0 + kk < D;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int r = rb + 8 * e;
            As[kk][r] = (kin && i0 + r < B) ? zn[(int64_t)(i0 + r) * D + k0 + kk] : 0.0f;
            Bs[kk][r] = (kin && j0 + r < B) ? zn[(int64_t)(j0 + r) * D + k0 + kk] : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < NX_KC; ++k) {
            const float4 av = *reinterpret_cast<const float4*>(&As[k][ty * 4]);
            const float4 bv = *reinterpret_cast<const float4*>(&Bs[k][tx * 4]);
            const float a4[4] = {av.x, av.y, av.z, av.w}, b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(a4[a], b4[b], acc[a][b]);
        }
        __syncthreads();
    }
}

// part[(jt * B + i) * 4 + 0..3] = over the columns j of tile jt: max_{j != i} s_ij, sum_{j != i} exp(s_ij - max), sum of the cosines
// of the negatives (j != i, pair(i)), max of the negatives' logits; pos[i] = cosine of the pair (written by the one tile holding it)
__global__ void __launch_bounds__(256) ntxent_tile_stats_kernel(const float* __restrict__ zn, int B, int D, float inv_t,
                                                                float* __restrict__ part, float* __restrict__ pos) {
    __shared__ __align__(16) float As[NX_KC][NX_LD];
    __shared__ __align__(16) float Bs[NX_KC][NX_LD];
    __shared__ float Ss[NX_TILE][NX_TILE + 1];
    const int it = blockIdx.x, jt = blockIdx.y;
    const int i0 = it * NX_TILE, j0 = jt * NX_TILE;
    float acc[4][4];
    ntxent_dot_tile(zn, B, D, i0, j0, As, Bs, acc);
    const int tid = threadIdx.x;
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) Ss[ty * 4 + a][tx * 4 + b] = acc[a][b];
    __syncthreads();
    // four lanes per row, 16 columns each, folded in lane order
    const int r = tid >> 2, q = tid & 3;
    const int i = i0 + r;
    const int N = B >> 1;
    const int pi = i < N ? i + N : i - N;
    float m = -INFINITY, l = 0.0f, cs = 0.0f, mo = -INFINITY;
    for (int c = 0; c < 16; ++c) {
        const int j = j0 + q * 16 + c;
        if (i >= B || j >= B || j == i) continue;
        const float dot = Ss[r][q * 16 + c];
        const float s = dot * inv_t;
        if (s > m) {
            l = l * expf(m - s) + 1.0f;       // (m = -inf: l is 0 and expf gives 0)
            m = s;
        } else {
            l += expf(s - m);
        }
        if (j == pi) {
            pos[i] = dot;
        } else {
            cs += dot;
            mo = fmaxf(mo, s);
        }
    }
    // lanes q = 1, 2, 3 into lane q = 0, in that order (all four lanes of a row sit in one wave)
    float M = m, L = l, CS = cs, MO = mo;
#pragma unroll
    for (int o = 1; o < 4; ++o) {
        const float m2 = __shfl(m, (tid & 60) + o, 64), l2 = __shfl(l, (tid & 60) + o, 64);
        const float c2 = __shfl(cs, (tid & 60) + o, 64), o2 = __shfl(mo, (tid & 60) + o, 64);
        const float Mn = fmaxf(M, m2);
        const float w1 = M == -INFINITY ? 0.0f : expf(M - Mn), w2 = m2 == -INFINITY ? 0.0f : expf(m2 - Mn);
        L = L * w1 + l2 * w2;
        M = Mn;
        CS += c2;
        MO = fmaxf(MO, o2);
    }
    if (q == 0 && i < B) {
        float4 o4;
        o4.x = M; o4.y = L; o4.z = CS; o4.w = MO;
        *reinterpret_cast<float4*>(part + ((int64_t)jt * B + i) * 4) = o4;
    }
}

__global__ void __launch_bounds__(256) ntxent_rows_kernel(const float* __restrict__ part, const float* __restrict__ pos,
                                                          const float* __restrict__ norm, int B, int nct, float temperature,
                                                          float* __restrict__ lse, float* __restrict__ metrics) {
    __shared__ double sm[5 * 256];
    const int tid = threadIdx.x;
    const float inv_t = 1.0f / temperature;
    double acc[5] = {0, 0, 0, 0, 0};    // loss, top-1 hits, pair cosine, negative cosines, norm
    for (int i = tid; i < B; i += 256) {
        float M = -INFINITY, L = 0.0f, MO = -INFINITY;
        double cs = 0.0;
        for (int jt = 0; jt < nct; ++jt) {
            const float4 p = *reinterpret_cast<const float4*>(part + ((int64_t)jt * B + i) * 4);
            const float Mn = fmaxf(M, p.x);
            const float w1 = M == -INFINITY ? 0.0f : expf(M - Mn), w2 = p.x == -INFINITY ? 0.0f : expf(p.x - Mn);
            L = L * w1 + p.y * w2;
            M = Mn;
            cs += (double)p.z;
            MO = fmaxf(MO, p.w);
        }
        const float ls = M + logf(L);
        lse[i] = ls;
        const float sp = pos[i] * inv_t;
        acc[0] += (double)ls - (double)sp;
        acc[1] += sp > MO ? 1.0 : 0.0;
        acc[2] += (double)pos[i];
        acc[3] += cs;
        acc[4] += (double)norm[i];
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) sm[q * 256 + tid] = acc[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < 5; ++q) sm[q * 256 + tid] += sm[q * 256 + tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double invB = 1.0 / (double)B;
        metrics[0] = (float)(sm[0] * invB);
        metrics[1] = (float)(sm[256] * invB);
        metrics[2] = (float)(sm[512] * invB);
        metrics[3] = B > 2 ? (float)(sm[768] / ((double)B * (double)(B - 2))) : 0.0f;
        metrics[4] = (float)(sm[1024] * invB);
        metrics[5] = temperature;
        for (int k = 6; k < 16; ++k) metrics[k] = 0.0f;
    }
}

// dpart[(js * B + i) * D + d] = sum over the columns j of group js of c_ij zn_j[d], d in this workgroup's chunk of NX_DC columns.
// Thread (ty = tid >> 5, tx = tid & 31) owns rows ty*8 .. +7 and columns tx + 32 c, c = 0 .. 15, of the chunk.
__global__ void __launch_bounds__(256) ntxent_grad_tile_kernel(const float* __restrict__ zn, const float* __restrict__ lse, int B, int D,
                                                               float inv_t, float coef, int nct, int tpb,
                                                               float* __restrict__ dpart) {
    __shared__ __align__(16) float As[NX_KC][NX_LD];
    __shared__ __align__(16) float Bs[NX_KC][NX_LD];
    __shared__ float Cs[NX_TILE][NX_TILE + 1];
    const int it = blockIdx.x, js = blockIdx.y, d0 = blockIdx.z * NX_DC;
    const int i0 = it * NX_TILE;
    const int tid = threadIdx.x;
    const int N = B >> 1;
    float out[8][16];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int c = 0; c < 16; ++c) out[a][c] = 0.0f;
    const int jt_end = (js + 1) * tpb < nct ? (js + 1) * tpb : nct;
    for (int jt = js * tpb; jt < jt_end; ++jt) {
        const int j0 = jt * NX_TILE;
        float acc[4][4];
        ntxent_dot_tile(zn, B, D, i0, j0, As, Bs, acc);
        {
            const int ty = tid >> 4, tx = tid & 15;
            float lj[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) lj[b] = j0 + tx * 4 + b < B ? lse[j0 + tx * 4 + b] : 0.0f;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int i = i0 + ty * 4 + a;
                const float li = i < B ? lse[i] : 0.0f;
                const int pi = i < N ? i + N : i - N;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int j = j0 + tx * 4 + b;
                    float c = 0.0f;
                    if (i < B && j < B && j != i) {
                        const float s = acc[a][b] * inv_t;
                        c = (expf(s - li) + expf(s - lj[b]) - (j == pi ? 2.0f : 0.0f)) * coef;
                    }
                    Cs[ty * 4 + a][tx * 4 + b] = c;
                }
            }
        }
        __syncthreads();
        {
            const int ty = tid >> 5, tx = tid & 31;
            for (int k = 0; k < NX_TILE; ++k) {
                const int j = j0 + k;
                if (j >= B) break;          // (uniform over the workgroup)
                const float* zj = zn + (int64_t)j * D + d0 + tx;
                float bv[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) bv[c] = d0 + tx + 32 * c < D ? zj[32 * c] : 0.0f;
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    const float av = Cs[ty * 8 + a][k];
#pragma unroll
                    for (int c = 0; c < 16; ++c) out[a][c] = fmaf(av, bv[c], out[a][c]);
                }
            }
        }
        __syncthreads();        // Cs (and As / Bs) are rewritten by the next tile
    }
    const int ty = tid >> 5, tx = tid & 31;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int i = i0 + ty * 8 + a;
        if (i >= B) continue;
        float* o = dpart + ((int64_t)js * B + i) * D + d0 + tx;
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (d0 + tx + 32 * c < D) o[32 * c] = out[a][c];
    }
}

// g = sum_js dpart[js][i] (in order) = dL/dzn_i;  dz_i = grad_scale * (g - zn_i (zn_i . g)) / ||z_i||, or grad_scale * g / 1e-12
// where the norm was clamped (zn = z / 1e-12 there: a constant divisor)
__global__ void __launch_bounds__(256) ntxent_dz_kernel(const float* __restrict__ dpart, const float* __restrict__ zn,
                                                        const float* __restrict__ norm, int B, int D, int njs, float grad_scale,
                                                        float* __restrict__ dz) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    const float* zi = zn + (int64_t)i * D;
    const float n = norm[i];
    const bool clamped = !(n >= 1e-12f);
    float dot = 0.0f;
    for (int d = lane; d < D; d += 64) {
        float g = 0.0f;
        for (int js = 0; js < njs; ++js) g += dpart[((int64_t)js * B + i) * D + d];
        dot = fmaf(g, zi[d], dot);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    const float inv = clamped ? 1e12f : 1.0f / n;
    if (clamped) dot = 0.0f;
    for (int d = lane; d < D; d += 64) {
        float g = 0.0f;
        for (int js = 0; js < njs; ++js) g += dpart[((int64_t)js * B + i) * D + d];
        dz[(int64_t)i * D + d] = grad_scale * ((g - zi[d] * dot) * inv);
    }
}

static int ntxent_check(const char* who, int B, int D) {
    if (B < 2) {
        set_error("%s: B = %d rows: at least one pair (B >= 2) is needed", who, B);
        return -1;
    }
    if (B & 1) {
        set_error("%s: B = %d is odd: rows i and i + B/2 are the two views of one observation", who, B);
        return -1;
    }
    if (B > NX_MAXB) {
        set_error("%s: B = %d rows above the limit of %d", who, B, NX_MAXB);
        return -1;
    }
    if (D < 1) {
        set_error("%s: D = %d columns: at least one is needed", who, D);
        return -1;
    }
    return 0;
}

int64_t ntxent_workspace_floats(int B, int D) {
    if (ntxent_check("ntxent_workspace_floats", B, D) != 0) return -1;
    return ntxent_plan(B, D).total;
}

int ntxent_loss(const NtxentArgs& a, hipStream_t st) {
    CDRL_TRY(ntxent_check("ntxent_loss", a.B, a.D));
    if (!(a.temperature > 0.0f)) {
        set_error("ntxent_loss: temperature = %g must be positive", (double)a.temperature);
        return -1;
    }
    if (!a.z || !a.dz || !a.metrics || !a.workspace) {
        set_error("ntxent_loss: a null z / dz / metrics / workspace");
        return -1;
    }
    if (a.z == a.dz) {
        set_error("ntxent_loss: dz may not alias z");
        return -1;
    }
    const int B = a.B, D = a.D;
    const NtxentPlan p = ntxent_plan(B, D);
    float* ws = a.workspace;
    float *zn = ws + p.o_zn, *norm = ws + p.o_norm, *lse = ws + p.o_lse, *pos = ws + p.o_pos, *part = ws + p.o_part,
          *dpart = ws + p.o_dpart;
    const float inv_t = 1.0f / a.temperature;
    const float coef = (float)(1.0 / ((double)B * (double)a.temperature));
    hipLaunchKernelGGL(ntxent_normalize_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, a.z, B, D, zn, norm);
    CDRL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ntxent_tile_stats_kernel, dim3(p.nct, p.nct), dim3(256), 0, st, (const float*)zn, B, D, inv_t, part, pos);
    CDRL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ntxent_rows_kernel, dim3(1), dim3(256), 0, st, (const float*)part, (const float*)pos, (const float*)norm, B,
                       p.nct, a.temperature, lse, a.metrics);
    CDRL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ntxent_grad_tile_kernel, dim3(p.nct, p.js, cdiv(D, NX_DC)), dim3(256), 0, st, (const float*)zn,
                       (const float*)lse, B, D, inv_t, coef, p.nct, p.tpb, dpart);
    CDRL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ntxent_dz_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, (const float*)dpart, (const float*)zn,
                       (const float*)norm, B, D, p.js, a.grad_scale, a.dz);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
