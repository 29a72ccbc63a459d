// Spatial kernels of the image tower (gfx950): 3x3/s2 stem conv, depthwise 3x3, max-pool, GAP.
//
// Layout: NHWC dense, frames ordered f = t*B + b.  All kernels are HBM-bound streams with
// channel-fastest lane mapping (coalesced along C); reductions (filter gradients) reuse the
// column-mapped skeleton with double partials (deterministic, no atomics).
// TF 'SAME' padding is asymmetric for stride 2 on even sizes:
// pad_before = floor(total/2).
#include "colreduce.h"

namespace cdrl {

// ------------------------------------------------------------------------------------------
// stem: Conv2D(24, 3, strides=2, 'valid') on the (B,T,H,W,3) observation tensor
// (reference core/architectures.py:159).  Output frame index = t*B + b.
// ------------------------------------------------------------------------------------------
// each thread computes 4 consecutive output channels of one pixel: the 27 input taps are loaded once
// per 4 outputs, weights come from LDS as float4, the store is one 16-byte access.
__global__ void __launch_bounds__(256) stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ y, int B,
                                                       int T, int H, int W, int Ho, int Wo, int Cout) {
    extern __shared__ float ws[];      // [27][Cout] + [Cout]
    for (int i = threadIdx.x; i < 27 * Cout; i += blockDim.x) ws[i] = w[i];
    for (int i = threadIdx.x; i < Cout; i += blockDim.x) ws[27 * Cout + i] = bias[i];
    __syncthreads();
    const int C4 = Cout >> 2;
    const int64_t total = (int64_t)B * T * Ho * Wo * C4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % C4) * 4;
        int64_t pix = i / C4;
        const int ox = (int)(pix % Wo);
        pix /= Wo;
        const int oy = (int)(pix % Ho);
        const int f = (int)(pix / Ho);
        const int t = f / B, b = f % B;
        const float* xp = x + ((((int64_t)b * T + t) * H + 2 * oy) * W + 2 * ox) * 3;
        float4 acc = *reinterpret_cast<const float4*>(&ws[27 * Cout + co]);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int j = 0; j < 9; ++j) {          // 3 pixels x 3 channels are contiguous in the input row
                const float xv = xp[(int64_t)ky * W * 3 + j];
                const float4 wv = *reinterpret_cast<const float4*>(&ws[(ky * 9 + j) * Cout + co]);
                acc.x = fmaf(xv, wv.x, acc.x);
                acc.y = fmaf(xv, wv.y, acc.y);
                acc.z = fmaf(xv, wv.z, acc.z);
                acc.w = fmaf(xv, wv.w, acc.w);
            }
        *reinterpret_cast<float4*>(&y[(i / C4) * Cout + co]) = acc;
    }
}

__global__ void __launch_bounds__(256) stem_fwd_scalar_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ y,
                                                              int B, int T, int H, int W, int Ho, int Wo, int Cout) {
    extern __shared__ float ws[];
    for (int i = threadIdx.x; i < 27 * Cout; i += blockDim.x) ws[i] = w[i];
    for (int i = threadIdx.x; i < Cout; i += blockDim.x) ws[27 * Cout + i] = bias[i];
    __syncthreads();
    const int64_t total = (int64_t)B * T * Ho * Wo * Cout;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % Cout);
        int64_t pix = i / Cout;
        const int ox = (int)(pix % Wo);
        pix /= Wo;
        const int oy = (int)(pix % Ho);
        const int f = (int)(pix / Ho);
        const int t = f / B, b = f % B;
        const float* xp = x + ((((int64_t)b * T + t) * H + 2 * oy) * W + 2 * ox) * 3;
        float acc = ws[27 * Cout + co];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int j = 0; j < 9; ++j) acc = fmaf(xp[(int64_t)ky * W * 3 + j], ws[(ky * 9 + j) * Cout + co], acc);
        y[i] = acc;
    }
}

// Stem conv with the following BatchNorm's statistics in the epilogue: one workgroup = a contiguous pixel range of ONE
// time slice, block = (Cout/4 channel lanes, pixel lanes); per-thread (sum, sum of squares) in double, LDS fold over the
// pixel lanes, one partial row per workgroup in bn_finalize's [T][nb][2][Cout] layout (no second pass over the 255 MB y).
template <int NP, class AT>
__global__ void __launch_bounds__(256) stem_fwd_stats_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, AT* __restrict__ y,
                                                             double* __restrict__ part, int B, int T, int H, int W, int Ho,
                                                             int Wo, int Cout, int rb) {
    extern __shared__ __attribute__((aligned(16))) float ws[];      // [27][Cout] + [Cout], then the reduction scratch
    const int CX = blockDim.x, CY = blockDim.y, tx = threadIdx.x, ty = threadIdx.y;
    const int tid = ty * CX + tx, nthr = CX * CY;
    for (int i = tid; i < 27 * Cout; i += nthr) ws[i] = w[i];
    for (int i = tid; i < Cout; i += nthr) ws[27 * Cout + i] = bias[i];
    __syncthreads();
    const int g = blockIdx.y, nb = gridDim.x;
    const int Mg = B * Ho * Wo;
    const int r0 = blockIdx.x * rb, r1 = min(r0 + rb, Mg);
    const int co = tx * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    // NP output pixels per thread and iteration: their 27-float input windows (3 rows x 9 contiguous floats, 8-byte
    // aligned -> 4 x 8 B + 4 B per row) are all requested before the first FMA, and every filter tap read from LDS feeds
    // NP pixels.  One pixel per iteration exposed one memory round trip per pixel (62 per thread) and spent as much
    // LDS bandwidth on the taps (27 ds_read_b128 per pixel) as the kernel needs HBM time.
    const float4 bq = *reinterpret_cast<const float4*>(&ws[27 * Cout + co]);
    const bool x8 = (reinterpret_cast<uintptr_t>(x) & 7) == 0 && ((W * 3) % 2) == 0;
    for (int rr = r0 + ty; rr < r1; rr += CY * NP) {
        float xv[NP][27];
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int r = min(rr + u * CY, r1 - 1);                  // clamped: unconditional loads
            const int ox = r % Wo;
            const int t2 = r / Wo;
            const int oy = t2 % Ho;
            const int b = t2 / Ho;                                 // frame inside the time slice g: f = g*B + b
            const float* xp = x + ((((int64_t)b * T + g) * H + 2 * oy) * W + 2 * ox) * 3;
            if (x8) {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const float* xr = xp + (int64_t)ky * W * 3;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float2 t = *reinterpret_cast<const float2*>(xr + 2 * j);
                        xv[u][ky * 9 + 2 * j] = t.x;
                        xv[u][ky * 9 + 2 * j + 1] = t.y;
                    }
                    xv[u][ky * 9 + 8] = xr[8];
                }
            } else {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int j = 0; j < 9; ++j) xv[u][ky * 9 + j] = xp[(int64_t)ky * W * 3 + j];
            }
        }
        float4 acc[NP];
#pragma unroll
        for (int u = 0; u < NP; ++u) acc[u] = bq;
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const float4 wv = *reinterpret_cast<const float4*>(&ws[k * Cout + co]);
#pragma unroll
            for (int u = 0; u < NP; ++u) {
                acc[u].x = fmaf(xv[u][k], wv.x, acc[u].x);
                acc[u].y = fmaf(xv[u][k], wv.y, acc[u].y);
                acc[u].z = fmaf(xv[u][k], wv.z, acc[u].z);
                acc[u].w = fmaf(xv[u][k], wv.w, acc[u].w);
            }
        }
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int r = rr + u * CY;
            if (r >= r1) continue;
            VecF<4> o4;
            o4.v[0] = acc[u].x; o4.v[1] = acc[u].y; o4.v[2] = acc[u].z; o4.v[3] = acc[u].w;
            vstore<4>(y + ((int64_t)g * Mg + r) * Cout + co, o4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // bf16 storage: statistics of the values the consumers will read (the rounded ones)
                const double a = sizeof(AT) == 2 ? (double)(float)(bf16_t)o4.v[i] : (double)o4.v[i];
                s[i] += a;
                q[i] += a * a;
            }
        }
    }
    __syncthreads();
    double* sm = reinterpret_cast<double*>(ws);                     // [2][4][CY][CX]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sm[((0 * 4 + i) * CY + ty) * CX + tx] = s[i];
        sm[((1 * 4 + i) * CY + ty) * CX + tx] = q[i];
    }
    __syncthreads();
    for (int j = ty; j < 8; j += CY) {                              // 8 (quantity, channel-in-group) columns per channel lane
        double a = 0.0;
        for (int yy = 0; yy < CY; ++yy) a += sm[(j * CY + yy) * CX + tx];
        const int qq = j >> 2, i = j & 3;
        part[(((int64_t)g * nb + blockIdx.x) * 2 + qq) * Cout + co + i] = a;
    }
}

// Band-staged form of the same kernel (round 5; float32 and bf16 storage): a workgroup walks (frame, band of R output rows) units of one
// time slice; the band's 2 R + 1 image rows are contiguous and go to LDS with 16-byte lanes, the next band waits in registers while the
// current one is convolved (the form above has every thread fetch its pixels' 27-float windows from global memory, 8 bytes per lane and
// load, six channel lanes asking for the same bytes: 160 us for 50 us of traffic).  Per output element the SAME fmaf chain (bias, then taps
// 0..26), so y is bit-identical; the statistics are per-thread doubles folded in a fixed order -- another order than above, i.e. the double
// sums differ in their last bits and the float statistics derived from them do not (checked: tools/iso_stem_fwd.py).
#ifndef STEM_FWD_NP
#define STEM_FWD_NP 2        // pixels per thread and iteration (4: 256 VGPRs, one wave per SIMD)
#endif
// (StemFwdGeom: cdrl_kernels.h)

template <int NP, int PX, class AT>
__global__ void __launch_bounds__(256) stem_fwd_band_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                            AT* __restrict__ y, double* __restrict__ part, int B, int T, int H, int W, int Ho,
                                                            int Wo, int Cout, StemFwdGeom gm) {
    extern __shared__ __attribute__((aligned(16))) float fsm[];
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    float* xs = fsm;
    float* ws = fsm + gm.xs_floats;             // [27][Cout] + [Cout]
    const int tid = threadIdx.x;
    const int CX = Cout / 4, CY = 256 / CX;     // channel lanes x pixel lanes (252 threads busy at 24 channels)
    const int tx = tid % CX, ty = tid / CX;
    const bool active = ty < CY;
    for (int i = tid; i < 27 * Cout; i += 256) ws[i] = w[i];
    for (int i = tid; i < Cout; i += 256) ws[27 * Cout + i] = bias[i];
    const int g = blockIdx.x / gm.nbpg, bg = blockIdx.x % gm.nbpg;
    const int R = gm.R, NB = gm.NB, units = B * NB, W3 = W * 3;
    const int co = tx * 4;
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)((int64_t)B * T * H * W3 * 4), 0x00020000);
    const uint32_t OOR = 0x80000000u;
    u32x4_t px[PX];
    auto prefetch = [&](int u) {
        const int b = u / NB, k = u - b * NB;
        const int oy0 = k * R, Rb = min(R, Ho - oy0);
        const uint32_t b0 = (uint32_t)(((((int64_t)b * T + g) * H + 2 * oy0) * W3) * 4);
        const int nx = (2 * Rb + 1) * W3;
#pragma unroll
        for (int q = 0; q < PX; ++q) {
            const int i = (q * 256 + tid) * 4;
            px[q] = __builtin_amdgcn_raw_buffer_load_b128(rsX, i < nx ? b0 + (uint32_t)i * 4u : OOR, 0, 0);
        }
    };
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q2[4] = {0.0, 0.0, 0.0, 0.0};
    if (bg < units) prefetch(bg);
    __syncthreads();                            // weights / bias in place
    const float4 bq = *reinterpret_cast<const float4*>(&ws[27 * Cout + co]);
    for (int u = bg; u < units; u += gm.nbpg) {
        const int b = u / NB, k = u - b * NB;
        const int oy0 = k * R, Rb = min(R, Ho - oy0), npix = Rb * Wo;
        __syncthreads();                        // the previous band's reads are done
        {
            const int nx = (2 * Rb + 1) * W3;
#pragma unroll
            for (int q = 0; q < PX; ++q) {
                const int i = (q * 256 + tid) * 4;
                if (i < nx) *reinterpret_cast<u32x4_t*>(xs + i) = px[q];
            }
        }
        __syncthreads();
        if (u + gm.nbpg < units) prefetch(u + gm.nbpg);
        if (!active) continue;
        const int64_t row0 = ((int64_t)(g * B + b) * Ho + oy0) * Wo;       // first output row of the band in y
        for (int p0 = ty; p0 < npix; p0 += CY * NP) {
            float xv[NP][27];
#pragma unroll
            for (int uu = 0; uu < NP; ++uu) {
                const int p = min(p0 + uu * CY, npix - 1);
                const int oyl = p / Wo, ox = p - oyl * Wo;
                const float* xp = xs + (2 * oyl * W + 2 * ox) * 3;          // 8-byte aligned
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const float* xr = xp + ky * W3;
                    if ((W3 & 1) == 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float2 t = *reinterpret_cast<const float2*>(xr + 2 * j);
                            xv[uu][ky * 9 + 2 * j] = t.x;
                            xv[uu][ky * 9 + 2 * j + 1] = t.y;
                        }
                        xv[uu][ky * 9 + 8] = xr[8];
                    } else {
#pragma unroll
                        for (int j = 0; j < 9; ++j) xv[uu][ky * 9 + j] = xr[j];
                    }
                }
            }
            float4 acc[NP];
#pragma unroll
            for (int uu = 0; uu < NP; ++uu) acc[uu] = bq;
#pragma unroll
            for (int kk = 0; kk < 27; ++kk) {
                const float4 wv = *reinterpret_cast<const float4*>(&ws[kk * Cout + co]);
#pragma unroll
                for (int uu = 0; uu < NP; ++uu) {
                    acc[uu].x = fmaf(xv[uu][kk], wv.x, acc[uu].x);
                    acc[uu].y = fmaf(xv[uu][kk], wv.y, acc[uu].y);
                    acc[uu].z = fmaf(xv[uu][kk], wv.z, acc[uu].z);
                    acc[uu].w = fmaf(xv[uu][kk], wv.w, acc[uu].w);
                }
            }
#pragma unroll
            for (int uu = 0; uu < NP; ++uu) {
                const int p = p0 + uu * CY;
                if (p >= npix) continue;
                VecF<4> o4;
                o4.v[0] = acc[uu].x; o4.v[1] = acc[uu].y; o4.v[2] = acc[uu].z; o4.v[3] = acc[uu].w;
                vstore<4>(y + (row0 + p) * Cout + co, o4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double a = sizeof(AT) == 2 ? (double)(float)(bf16_t)o4.v[i] : (double)o4.v[i];
                    s[i] += a;
                    q2[i] += a * a;
                }
            }
        }
    }
    __syncthreads();
    double* sm = reinterpret_cast<double*>(fsm);                    // [2][4][CY][CX]; the band and the weights are dead
    if (active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sm[((0 * 4 + i) * CY + ty) * CX + tx] = s[i];
            sm[((1 * 4 + i) * CY + ty) * CX + tx] = q2[i];
        }
    }
    __syncthreads();
    if (active)
        for (int j = ty; j < 8; j += CY) {
            double a = 0.0;
            for (int yy = 0; yy < CY; ++yy) a += sm[(j * CY + yy) * CX + tx];
            const int qq = j >> 2, i = j & 3;
            part[(((int64_t)g * gm.nbpg + bg) * 2 + qq) * Cout + co + i] = a;
        }
}

static StemFwdGeom stem_fwd_geom(int B, int T, int H, int W, int Cout) {
    const int Ho = (H - 3) / 2 + 1;
    StemFwdGeom g{};
    static const bool on = !(cdrl_getenv("CDRL_STEM_FWD_BAND") && atoi(cdrl_getenv("CDRL_STEM_FWD_BAND")) == 0);
    if (!on || Cout % 4 || Cout > 64 || Cout < 4) return g;
    // the band kernel addresses the images through a 32-bit buffer descriptor: planner (stem_fwd_stats_nb) and launcher must agree
    // on the form, so the size test lives here
    if ((int64_t)B * T * H * W * 3 * 4 >= (1ll << 31)) return g;
    const int CX = Cout / 4, CY = 256 / CX;
    const size_t red = (size_t)8 * CY * CX * sizeof(double);
    const int cand[] = {8, 6, 4, 3, 2, 1};
    static const int rmax = 8;
    for (int R : cand) {
        const int nx = (2 * R + 1) * W * 3;
        const int px = cdiv(nx, 1024);
        if (px > 6 || (R > rmax && R != 1)) continue;
        g.R = R;
        g.NB = cdiv(Ho, R);
        g.xs_floats = (nx + 3) / 4 * 4 + 4;
        g.px = px <= 2 ? 2 : px <= 4 ? 4 : 6;
        g.lds = std::max((size_t)(g.xs_floats + 28 * Cout) * sizeof(float), red);
        g.ok = true;
        break;
    }
    if (!g.ok) return g;
    static const int wgs_env = 512;     // two workgroups per CU are resident (196-216 VGPRs)
    g.nbpg = std::max(1, std::min(wgs_env / std::max(T, 1), B * g.NB));
    return g;
}

bool stem_fwd_stats_supported(int Cout) { return (Cout % 4) == 0 && Cout <= 64; }
bool stem_bwd_fused_supported(int Cout) { return Cout <= 32 && (Cout % 4) == 0; }

#define STEM_NBLK_MAX 2048                          // capacity of the partial buffer of the MFMA filter gradient
static int stem_nblk() {
    static const int n = 1024;
    return n < 64 ? 64 : (n > STEM_NBLK_MAX ? STEM_NBLK_MAX : n);
}

// time slices (Mg rows each) that the rows [k * rows_per, (k + 1) * rows_per) of one workgroup can come from, the largest over k
static int stem_slices_max(int rows, int rows_per, int Mg, int T) {
    if (rows <= 0 || Mg <= 0 || rows_per <= 0) return 0;
    int m = 1;
    if (rows_per <= Mg) {                           // at most one slice boundary per workgroup: is one of them inside a workgroup?
        for (int g = 1; g < T && m == 1; ++g)
            if (((int64_t)g * Mg) % rows_per) m = 2;
        return m;
    }
    for (int r0 = 0; r0 < rows; r0 += rows_per) {
        const int r1 = std::min(r0 + rows_per, rows);
        m = std::max(m, (r1 - 1) / Mg - r0 / Mg + 1);
    }
    return m;
}

StemPlan stem_plan(int B, int T, int H, int W, int Cout, int at, bool pooled, bool db_adjacent, bool y_aligned) {
    StemPlan p{};
    p.Ho = (H - 3) / 2 + 1;
    p.Wo = (W - 3) / 2 + 1;
    p.Hp = same_out(p.Ho, 2);
    p.Wp = same_out(p.Wo, 2);
    const int Mg = B * p.Ho * p.Wo;
    // plain forward
    p.fwd_vec = (Cout % 4 == 0) && y_aligned;
    // forward with statistics
    p.st_refusal = !stem_fwd_stats_supported(Cout) ? STEM_REFUSE_COUT : !y_aligned ? STEM_REFUSE_ALIGN : 0;
    p.geom = stem_fwd_geom(B, T, H, W, Cout);
    if (p.geom.ok) {
        static const int npx = STEM_FWD_NP;
        p.st_form = 0;
        p.R = p.geom.R;
        p.NB = p.geom.NB;
        p.nbpg = p.geom.nbpg;
        p.px = p.geom.px;
        p.NP = npx >= 4 ? 4 : npx == 3 ? 3 : 2;
        p.lds = (int)p.geom.lds;
        p.units_max = cdiv(B * p.geom.NB, p.geom.nbpg);
        p.part_rows = p.geom.nbpg;
    } else {
        p.st_form = 1;
        p.st_rb = std::max(1, cdiv(Mg, NB_STATS));
        p.part_rows = cdiv(Mg, p.st_rb);
        p.nbpg = p.part_rows;
        p.NP = 4;
        p.units_max = 1;
        if (Cout >= 4 && Cout % 4 == 0 && Cout <= 1024) {
            const int cx = Cout / 4, cy = 256 / cx;
            p.lds = (int)std::max((size_t)(27 * Cout + Cout) * sizeof(float), (size_t)8 * cy * cx * sizeof(double));
        }
    }
    // pool forward, scatter-form BatchNorm sums over the pooled gradient
    p.pf = stem_pool_fwd_geom(B * T * p.Hp * p.Wp, Cout);
    p.pr = pool_bn_reduce_plan(B * p.Hp * p.Wp, Cout, pooled);
    p.pr_part_doubles = (int64_t)T * p.pr.g.nb * 2 * Cout;
    // filter gradient
    const int64_t rows64 = (int64_t)B * T * p.Ho * p.Wo;
    const int rows = (int)rows64;
    p.NCH = 1;
    if (Cout <= 32) {
        p.fg_form = 0;
        p.rows_per = std::max(128, cdiv(cdiv(rows, stem_nblk()), 128) * 128);
        p.nblk = cdiv(rows, p.rows_per);
        p.slices_max = stem_slices_max(rows, p.rows_per, Mg, T);
        p.part_doubles = ((int64_t)p.nblk * 28 * Cout + 1) / 2;                 // float partials inside a double buffer
        p.ws_doubles = ((int64_t)STEM_NBLK_MAX * 28 * Cout + 1) / 2;
    } else {
        const ColGeom g = col_geom(rows, Cout, NB_FILTER);
        p.fg_form = 2;
        p.rows_per = g.rb;
        p.nblk = g.nb;
        p.slices_max = stem_slices_max(rows, g.rb, Mg, T);
        p.part_doubles = p.ws_doubles = (int64_t)g.nb * 28 * Cout;
    }
    p.ff_refusal = !stem_bwd_fused_supported(Cout) ? STEM_REFUSE_COUT : rows64 * Cout * 4 >= (1ll << 31) ? STEM_REFUSE_2GB : 0;
    p.ff_form = p.ff_refusal ? -1 : 1;
    if (!p.ff_refusal) {
        p.NCH = ((Cout >> 2) + 1) / 2 <= 3 ? 3 : 4;
        // the kernel stages the statistics of two time slices; a workgroup whose rows come from more reads them row by row
        p.ff_rowstats = p.slices_max > 2;
        p.single_reduce = db_adjacent;
    }
    (void)at;                                       // both storage types take the same decisions; the launchers pick the element type
    return p;
}

int stem_fwd_stats_nb(int B, int T, int H, int W, int Cout) { return stem_plan(B, T, H, W, Cout, 0, false, false, true).part_rows; }

int stem_fwd_stats(const float* x, const float* w, const float* bias, float* y, double* part, int B, int T, int H, int W, int Cout,
                   hipStream_t st, int at) {
    const StemPlan sp = stem_plan(B, T, H, W, Cout, at, false, false, (reinterpret_cast<uintptr_t>(y) & 15) == 0);
    if (sp.st_refusal) {
        set_error("stem_fwd_stats: Cout=%d / alignment not supported", Cout);
        return -1;
    }
    const int Ho = sp.Ho, Wo = sp.Wo;
    if (sp.st_form == 0) {
        const StemFwdGeom& bg = sp.geom;
#define CDRL_STEM_FWD_BAND_LAUNCH(NPN, PXN)                                                                                                 \
    do {                                                                                                                                    \
        if (at) hipLaunchKernelGGL((stem_fwd_band_kernel<NPN, PXN, bf16_t>), dim3(T * bg.nbpg), dim3(256), bg.lds, st, x, w, bias,          \
                                   reinterpret_cast<bf16_t*>(y), part, B, T, H, W, Ho, Wo, Cout, bg);                                       \
        else hipLaunchKernelGGL((stem_fwd_band_kernel<NPN, PXN, float>), dim3(T * bg.nbpg), dim3(256), bg.lds, st, x, w, bias, y, part, B,  \
                                T, H, W, Ho, Wo, Cout, bg);                                                                                 \
    } while (0)
        if (sp.NP == 4) {
            if (bg.px == 2) CDRL_STEM_FWD_BAND_LAUNCH(4, 2);
            else if (bg.px == 4) CDRL_STEM_FWD_BAND_LAUNCH(4, 4);
            else CDRL_STEM_FWD_BAND_LAUNCH(4, 6);
        } else if (sp.NP == 3) {
            if (bg.px == 2) CDRL_STEM_FWD_BAND_LAUNCH(3, 2);
            else if (bg.px == 4) CDRL_STEM_FWD_BAND_LAUNCH(3, 4);
            else CDRL_STEM_FWD_BAND_LAUNCH(3, 6);
        } else {
            if (bg.px == 2) CDRL_STEM_FWD_BAND_LAUNCH(2, 2);
            else if (bg.px == 4) CDRL_STEM_FWD_BAND_LAUNCH(2, 4);
            else CDRL_STEM_FWD_BAND_LAUNCH(2, 6);
        }
#undef CDRL_STEM_FWD_BAND_LAUNCH
        CDRL_LAUNCH_CHECK();
        return 0;
    }
    const int rb = sp.st_rb, nb = sp.part_rows;
    const int cx = Cout / 4, cy = 256 / cx;
    const size_t lds = (size_t)sp.lds;
    if (at) hipLaunchKernelGGL((stem_fwd_stats_kernel<4, bf16_t>), dim3(nb, T), dim3(cx, cy), lds, st, x, w, bias, reinterpret_cast<bf16_t*>(y), part, B, T, H, W, Ho, Wo, Cout, rb);
    else hipLaunchKernelGGL((stem_fwd_stats_kernel<4, float>), dim3(nb, T), dim3(cx, cy), lds, st, x, w, bias, y, part, B, T, H, W, Ho, Wo, Cout, rb);
    CDRL_LAUNCH_CHECK();
    return 0;
}

int stem_fwd(const float* x, const float* w, const float* bias, float* y, int B, int T, int H, int W, int Cout,
             hipStream_t st) {
    const StemPlan sp = stem_plan(B, T, H, W, Cout, 0, false, false, (reinterpret_cast<uintptr_t>(y) & 15) == 0);
    const int Ho = sp.Ho, Wo = sp.Wo;
    const bool v4 = sp.fwd_vec != 0;
    const int64_t total = (int64_t)B * T * Ho * Wo * (v4 ? Cout / 4 : Cout);
    int64_t nb = cdiv64(total, 256 * 2);
    if (nb > 16384) nb = 16384;
    if (nb < 1) nb = 1;
    const size_t lds = (27 * Cout + Cout) * sizeof(float);
    if (v4)
        hipLaunchKernelGGL(stem_fwd_kernel, dim3((unsigned)nb), dim3(256), lds, st, x, w, bias, y, B, T, H, W, Ho, Wo, Cout);
    else
        hipLaunchKernelGGL(stem_fwd_scalar_kernel, dim3((unsigned)nb), dim3(256), lds, st, x, w, bias, y, B, T, H, W, Ho, Wo,
                           Cout);
    CDRL_LAUNCH_CHECK();
    return 0;
}

struct StemBwdF {
    const float* x;
    const float* dy;
    int B, T, H, W, Ho, Wo, Cout;
    __device__ void operator()(int, int64_t row, int c, double* acc) const {
        const int ox = (int)(row % Wo);
        int64_t r = row / Wo;
        const int oy = (int)(r % Ho);
        const int f = (int)(r / Ho);
        const int t = f / B, b = f % B;
        const float* xp = x + ((((int64_t)b * T + t) * H + 2 * oy) * W + 2 * ox) * 3;
        const double d = (double)dy[row * Cout + c];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int ci = 0; ci < 3; ++ci)
                    acc[(ky * 3 + kx) * 3 + ci] += (double)xp[((int64_t)ky * W + kx) * 3 + ci] * d;
        acc[27] += d;
    }
};

// MFMA form of the stem filter gradient: dW[27][Cout] (+ db as a 28th "ones" patch column) is a
// TN GEMM  P^T dY  over M = B*T*Ho*Wo pixel rows with the im2col patch tile P (32 rows x 27+1)
// gathered on the fly into LDS.  Each of the 4 waves owns 32 rows of a 128-row slice and its own
// 32x32 accumulator; the 4 accumulators are summed through LDS at the end and written as one
// float partial per workgroup (deterministic two-stage reduction, no atomics).
typedef float f32x16_c __attribute__((ext_vector_type(16)));
// (STEM_NBLK_MAX, stem_nblk: next to stem_plan above)

// FUSED: dy is not read but computed on the fly, dy = k1*(dz - k2 - xhat*k3) with dz gathered from the pooled gradient
// through the max-pool argmax (pool_gather) and masked by ReLU6: the stem BatchNorm's backward "apply" and the 255 MB
// dy tensor disappear from the critical stream (this kernel runs on the side stream).
struct StemBnBwd {
    PoolSrc ps;
    const float* y;         // raw stem conv output [rows][Cout]
    const float* stats;     // [4][T][Cout]
    const float* coef;      // [3][T][Cout]
};

// wave-private LDS tiles: ordering between a wave's own ds_write / ds_read needs no workgroup barrier
__device__ __forceinline__ void stem_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#ifndef STEM_BWD_WGS
#define STEM_BWD_WGS 3      // waves per SIMD the register allocation aims at (153 + 16 registers sat one above the three-wave step: 180 -> 173 us)
#endif
// AT: element type of the pooled gradient and of the raw conv output y in the FUSED form (bf16 activation storage)
// ROWSTATS (FUSED only): a workgroup's rows may come from more than the two time slices CF holds (few rows per slice: B * Ho * Wo below
// rows_per / 2), so every row reads the seven values of ITS slice from global memory -- slow, and only selected at such tiny shapes
// (StemPlan::ff_rowstats); the other instantiations are what they were.
template <bool FUSED, int NCH, class AT = float, bool ROWSTATS = false>
__global__ void __launch_bounds__(256, STEM_BWD_WGS) stem_bwd_mfma_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            float* __restrict__ part, int B, int T, int H, int W, int Ho,
                                                            int Wo, int Cout, int rows, int rows_per, StemBnBwd bb) {
    __shared__ float P[4][32][33];
    __shared__ float D[4][32][33];
    __shared__ float CF[2][7][32];      // FUSED: BatchNorm statistics / coefficients of the (at most two) time slices of this block
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lcol = lane & 31, lk = lane >> 5;
    const int r0 = blockIdx.x * rows_per;
    const int r1 = min(r0 + rows_per, rows);
    const int rows_per_group = B * Ho * Wo;
    const int g0 = r0 / rows_per_group;
    f32x16_c acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int i = lane; i < 32 * 33; i += 64) {       // zero the padding columns once
        (&P[wave][0][0])[i] = 0.0f;
        (&D[wave][0][0])[i] = 0.0f;
    }
    if (FUSED && !ROWSTATS) {
        const int GC = T * Cout;
        for (int i = tid; i < 2 * 7 * 32; i += 256) {
            const int gg = i / (7 * 32), q = (i / 32) % 7, c = i % 32;
            const int g = min(g0 + gg, T - 1);
            float v = 0.0f;
            if (c < Cout) v = q < 4 ? bb.stats[q * GC + g * Cout + c] : bb.coef[(q - 4) * GC + g * Cout + c];
            CF[gg][q][c] = v;
        }
        __syncthreads();
    }
    constexpr int nch = NCH;                         // 16-byte channel chunks per half-wave lane (3 for 24 channels)
    __amdgpu_buffer_rsrc_t rsDP, rsAM, rsY;
    if (FUSED) {
        const int64_t pel = (int64_t)B * T * bb.ps.Ho * bb.ps.Wo * Cout;
        rsDP = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bb.ps.dp), 0, (int)(pel * sizeof(AT)), 0x00020000);
        rsAM = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(bb.ps.argmax), 0, (int)pel, 0x00020000);
        rsY = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bb.y), 0, (int)((int64_t)rows * Cout * sizeof(AT)), 0x00020000);
    }
    for (int base = r0; base < r1; base += 128) {
        const int wrow0 = base + wave * 32;
        stem_wave_sync();
        // Lane l owns row (l & 31); ONE row decode per lane and slice (32-bit), shared by the patch tile and the gradient tile.
        const int r = lane & 31, half = lane >> 5;
        const int row = wrow0 + r;
        const bool ok = row < r1;
        int ox = 0, oy = 0, f = 0, t = 0;
        const float* xp = x;
        if (ok) {
            ox = row % Wo;
            const int q = row / Wo;
            oy = q % Ho;
            f = q / Ho;
            t = f / B;
            const int b = f - t * B;
            xp = x + ((((int64_t)b * T + t) * H + 2 * oy) * W + 2 * ox) * 3;
        }
        // patch tile: 32 rows x 28 (27 taps + ones column); the lane's 14 columns [14*half, 14*half+14), tap offsets are
        // compile-time constants
        // (unconditional loads, select afterwards: with the loads inside `if (ok)` they were issued pair by pair, each pair
        //  with its own s_waitcnt -- 7 round trips per slice; rows that do not exist read the first pixel of the image)
        float pv[14];
#pragma unroll
        for (int jj = 0; jj < 14; ++jj) {
            const int j1 = jj == 13 ? 12 : 14 + jj;        // column 27 is the ones column: no load (tap 26 is loaded twice)
            const int o0 = (jj / 9) * W * 3 + (jj % 9);
            const int o1 = (j1 / 9) * W * 3 + (j1 % 9);
            pv[jj] = xp[half ? o1 : o0];
        }
#pragma unroll
        for (int jj = 0; jj < 14; ++jj) {
            float val = pv[jj];
            if (jj == 13 && half) val = 1.0f;
            if (!ok) val = 0.0f;
            P[wave][r][half * 14 + jj] = val;
        }
        if (FUSED) {
            // gradient tile: the lane's nch chunks of 4 channels of its row.  dz is gathered from the pooled gradient through
            // the argmax (<= 4 candidate windows), masked by ReLU6, then dy = k1*(dz - k2 - xhat*k3).
            // The 3x3 / stride-2 pool reaches a pre-pool pixel from at most 2 x 2 windows: ky = parity(oy + pt) and, for an
            // even parity, ky + 2 (one pooled row up); same along x.  All candidate loads are issued unconditionally through
            // buffer descriptors -- a window that does not exist gets an out-of-range offset and returns 0 -- so that the
            // whole slice is ONE batch of independent loads (the branchy gather serialised up to 27 load/wait rounds per
            // slice: 450 us for 470 MB).
            const PoolSrc& ps = bb.ps;
            const int gs = min(max(t - g0, 0), 1);
            const uint32_t OOR = 0x80000000u;
            const int kyA = (oy + ps.pt) & 1, kxA = (ox + ps.pl) & 1;
            const int pyA = (oy + ps.pt - kyA) >> 1, pxA = (ox + ps.pl - kxA) >> 1;
            const bool vyA = ok && pyA < ps.Ho, vyB = ok && kyA == 0 && pyA >= 1 && (pyA - 1) < ps.Ho;
            const bool vxA = pxA < ps.Wo, vxB = kxA == 0 && pxA >= 1 && (pxA - 1) < ps.Wo;
            const int pbase = ((f * ps.Ho + pyA) * ps.Wo + pxA) * Cout;          // window (A, A); (B, .) is one pooled row up
            const int dyB = -ps.Wo * Cout, dxB = -Cout;
            uint32_t wo[4];         // element offsets of the 4 candidate windows (or OOR)
            uint32_t wk[4];         // their argmax codes ky*3 + kx
            wo[0] = (vyA && vxA) ? (uint32_t)pbase : OOR;
            wo[1] = (vyA && vxB) ? (uint32_t)(pbase + dxB) : OOR;
            wo[2] = (vyB && vxA) ? (uint32_t)(pbase + dyB) : OOR;
            wo[3] = (vyB && vxB) ? (uint32_t)(pbase + dyB + dxB) : OOR;
            wk[0] = kyA * 3 + kxA;
            wk[1] = kyA * 3 + kxA + 2;
            wk[2] = (kyA + 2) * 3 + kxA;
            wk[3] = (kyA + 2) * 3 + kxA + 2;
            const uint32_t yo = ok ? (uint32_t)row * (uint32_t)Cout : OOR;
            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
            typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
            u32x4_t gd[NCH][4], gy[NCH];
            uint32_t ga[NCH][4];
            // 4 channels of the pooled gradient / of y as float bit patterns (bf16 storage: 8-byte loads, widened here)
            auto load4 = [&](const __amdgpu_buffer_rsrc_t& rs, uint32_t eo) -> u32x4_t {
                if (sizeof(AT) == 2) {
                    const u32x2_t h = __builtin_amdgcn_raw_buffer_load_b64(rs, eo == OOR ? OOR : eo * 2u, 0, 0);
                    u32x4_t o;
                    o[0] = h[0] << 16; o[1] = h[0] & 0xffff0000u; o[2] = h[1] << 16; o[3] = h[1] & 0xffff0000u;
                    return o;
                }
                return __builtin_amdgcn_raw_buffer_load_b128(rs, eo == OOR ? OOR : eo * 4u, 0, 0);
            };
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int c0 = (half * nch + j) * 4;
                const bool on = c0 < Cout;
#pragma unroll
                for (int w4 = 0; w4 < 4; ++w4) {
                    const uint32_t eo = (on && wo[w4] != OOR) ? wo[w4] + c0 : OOR;
                    gd[j][w4] = load4(rsDP, eo);
                    ga[j][w4] = __builtin_amdgcn_raw_buffer_load_b32(rsAM, eo, 0, 0);
                }
                gy[j] = load4(rsY, (on && yo != OOR) ? yo + c0 : OOR);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int c0 = (half * nch + j) * 4;
                if (c0 >= Cout) continue;
                float o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float d = 0.0f;
#pragma unroll
                    for (int w4 = 0; w4 < 4; ++w4)
                        if (((ga[j][w4] >> (8 * i)) & 0x7fu) == wk[w4]) d += __uint_as_float(gd[j][w4][i]);
                    const float v = __uint_as_float(gy[j][i]);
                    float mean, inv, sc, sh, k1, k2, k3;
                    if (ROWSTATS) {         // t is the row's own slice (0 for a row that does not exist: its result is dropped)
                        const int GC = T * Cout, o = t * Cout + c0 + i;
                        mean = bb.stats[o]; inv = bb.stats[GC + o]; sc = bb.stats[2 * GC + o]; sh = bb.stats[3 * GC + o];
                        k1 = bb.coef[o]; k2 = bb.coef[GC + o]; k3 = bb.coef[2 * GC + o];
                    } else {
                        mean = CF[gs][0][c0 + i]; inv = CF[gs][1][c0 + i]; sc = CF[gs][2][c0 + i]; sh = CF[gs][3][c0 + i];
                        k1 = CF[gs][4][c0 + i]; k2 = CF[gs][5][c0 + i]; k3 = CF[gs][6][c0 + i];
                    }
                    const float z = fmaf(sc, v, sh);
                    if (!relu6_open(z)) d = 0.0f;
                    const float xh = (v - mean) * inv;
                    o[i] = ok ? k1 * (d - k2 - xh * k3) : 0.0f;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) D[wave][r][c0 + i] = o[i];
            }
        } else {
            for (int idx = lane; idx < 32 * Cout; idx += 64) {
                const int rr = idx / Cout, c = idx - rr * Cout;
                const int row2 = wrow0 + rr;
                D[wave][rr][c] = row2 < r1 ? dy[(int64_t)row2 * Cout + c] : 0.0f;
            }
        }
        stem_wave_sync();
#pragma unroll
        for (int mm = 0; mm < 32; mm += 2) {
            const float a = P[wave][mm + lk][lcol];
            const float bq = D[wave][mm + lk][lcol];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq, acc, 0, 0, 0);
        }
    }
    __syncthreads();
    // sum the 4 wave accumulators: reuse P as [4][32][33]
#pragma unroll
    for (int r = 0; r < 16; ++r) P[wave][(r & 3) + 8 * (r >> 2) + 4 * lk][lcol] = acc[r];
    __syncthreads();
    float* out = part + (int64_t)blockIdx.x * 28 * Cout;
    for (int idx = tid; idx < 28 * Cout; idx += 256) {
        const int k = idx / Cout, n = idx - k * Cout;
        out[idx] = (P[0][k][n] + P[1][k][n]) + (P[2][k][n] + P[3][k][n]);
    }
}

int64_t stem_bwd_part_elems(int B, int T, int H, int W, int Cout) { return stem_plan(B, T, H, W, Cout, 0, false, false, true).ws_doubles; }

int stem_bwd_filter(const float* x, const float* dy, float* dw, float* db, int B, int T, int H, int W, int Cout,
                    double* part, hipStream_t st) {
    const StemPlan sp = stem_plan(B, T, H, W, Cout, 0, false, false, true);
    const int Ho = sp.Ho, Wo = sp.Wo;
    const int rows = B * T * Ho * Wo;
    if (sp.fg_form == 0) {
        float* pf = reinterpret_cast<float*>(part);
        const int rows_per = sp.rows_per, nblk = sp.nblk;
        hipLaunchKernelGGL((stem_bwd_mfma_kernel<false, 1>), dim3(nblk), dim3(256), 0, st, x, dy, pf, B, T, H, W, Ho, Wo, Cout, rows,
                           rows_per, StemBnBwd{});
        CDRL_LAUNCH_CHECK();
        CDRL_TRY(reduce_partials_f32(pf, nblk, (int64_t)27 * Cout, (int64_t)28 * Cout, dw, 0, st));
        return reduce_partials_f32(pf + 27 * Cout, nblk, Cout, (int64_t)28 * Cout, db, 0, st);
    }
    StemBwdF f{x, dy, B, T, H, W, Ho, Wo, Cout};
    CDRL_TRY(launch_colreduce<28>(f, 1, rows, Cout, part, st, NB_FILTER));
    CDRL_TRY(reduce_partials(part, sp.nblk, 27 * Cout, (int64_t)28 * Cout, dw, 0, st));
    CDRL_TRY(reduce_partials(part + 27 * Cout, sp.nblk, Cout, (int64_t)28 * Cout, db, 0, st));
    return 0;
}

int stem_bwd_filter_fused(const float* x, const PoolSrc& ps, const float* y, const float* stats, const float* coef, float* dw,
                          float* db, int B, int T, int H, int W, int Cout, double* part, hipStream_t st, int at) {
    const StemPlan sp = stem_plan(B, T, H, W, Cout, at, ps.pa != nullptr, db == dw + 27 * Cout, true);
    if (sp.ff_refusal == STEM_REFUSE_COUT) {
        set_error("stem_bwd_filter_fused: Cout=%d not supported", Cout);
        return -1;
    }
    const int Ho = sp.Ho, Wo = sp.Wo;
    const int rows = B * T * Ho * Wo;
    if (sp.ff_refusal) {                                 // 32-bit buffer-descriptor offsets
        set_error("stem_bwd_filter_fused: conv output of 2 GB or more is not supported (rows=%d)", rows);
        return -1;
    }
    float* pf = reinterpret_cast<float*>(part);
    const int rows_per = sp.rows_per, nblk = sp.nblk;
    StemBnBwd bb{ps, y, stats, coef};
    const bool n3 = sp.NCH == 3;
    if (sp.ff_rowstats) {
        // rows of more than two time slices in one workgroup (a few rows per slice): the per-row form
        if (at && n3)
            hipLaunchKernelGGL((stem_bwd_mfma_kernel<true, 3, bf16_t, true>), dim3(nblk), dim3(256), 0, st, x, nullptr, pf, B, T, H, W, Ho, Wo, Cout,
                               rows, rows_per, bb);
        else if (at)
            hipLaunchKernelGGL((stem_bwd_mfma_kernel<true, 4, bf16_t, true>), dim3(nblk), dim3(256), 0, st, x, nullptr, pf, B, T, H, W, Ho, Wo, Cout,
                               rows, rows_per, bb);
        else if (n3)
            hipLaunchKernelGGL((stem_bwd_mfma_kernel<true, 3, float, true>), dim3(nblk), dim3(256), 0, st, x, nullptr, pf, B, T, H, W, Ho, Wo, Cout,
                               rows, rows_per, bb);
        else
            hipLaunchKernelGGL((stem_bwd_mfma_kernel<true, 4, float, true>), dim3(nblk), dim3(256), 0, st, x, nullptr, pf, B, T, H, W, Ho, Wo, Cout,
                               rows, rows_per, bb);
    } else if (at && n3)
        hipLaunchKernelGGL((stem_bwd_mfma_kernel<true, 3, bf16_t>), dim3(nblk), dim3(256), 0, st, x, nullptr, pf, B, T, H, W, Ho, Wo, Cout, rows,
                           rows_per, bb);
    else if (at)
        hipLaunchKernelGGL((stem_bwd_mfma_kernel<true, 4, bf16_t>), dim3(nblk), dim3(256), 0, st, x, nullptr, pf, B, T, H, W, Ho, Wo, Cout, rows,
                           rows_per, bb);
    else if (n3)
        hipLaunchKernelGGL((stem_bwd_mfma_kernel<true, 3>), dim3(nblk), dim3(256), 0, st, x, nullptr, pf, B, T, H, W, Ho, Wo, Cout, rows,
                           rows_per, bb);
    else
        hipLaunchKernelGGL((stem_bwd_mfma_kernel<true, 4>), dim3(nblk), dim3(256), 0, st, x, nullptr, pf, B, T, H, W, Ho, Wo, Cout, rows,
                           rows_per, bb);
    CDRL_LAUNCH_CHECK();
    // (the engine's arena holds the bias gradient right behind the filter gradient: one reduce over the 28 * Cout columns of a partial)
    if (sp.single_reduce) return reduce_partials_f32(pf, nblk, (int64_t)28 * Cout, (int64_t)28 * Cout, dw, 0, st);
    CDRL_TRY(reduce_partials_f32(pf, nblk, (int64_t)27 * Cout, (int64_t)28 * Cout, dw, 0, st));
    return reduce_partials_f32(pf + 27 * Cout, nblk, Cout, (int64_t)28 * Cout, db, 0, st);
}

// ------------------------------------------------------------------------------------------
// depthwise 3x3 (reference core/architectures.py:132,138); kernel layout (3,3,C,1) -> [9][C]
// ------------------------------------------------------------------------------------------
template <int s, int VEC>
__global__ void __launch_bounds__(256) dw_fwd_kernel(View a, const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ y, int rows, int H, int W, int Ho, int Wo, int C,
                                                     int pt, int pl, int rb, int nloop, bool al) {
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int CX = blockDim.x, CY = blockDim.y;
    const int r0 = blockIdx.x * rb;
    const int r1 = min(r0 + rb, rows);
    for (int l = 0; l < nloop; ++l) {
        const int c0 = (l * CX + tx) * VEC;
        if (c0 >= C) continue;
        VecF<VEC> wk[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wk[k] = vload<VEC>(w + k * C + c0);
        const VecF<VEC> bv = vload<VEC>(bias + c0);
        for (int r = r0 + ty; r < r1; r += CY) {
            const int ox = r % Wo;
            const int q = r / Wo;
            const int oy = q % Ho;
            const int n = q / Ho;
            VecF<VEC> acc = bv;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = oy * s + ky - pt;
                if (iy < 0 || iy >= H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = ox * s + kx - pl;
                    if (ix < 0 || ix >= W) continue;
                    const int64_t irow = ((int64_t)n * H + iy) * W + ix;
                    const VecF<VEC> x = vload_view<VEC>(a, irow, c0, 0, al);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc.v[i] = fmaf(x.v[i], wk[ky * 3 + kx].v[i], acc.v[i]);
                }
            }
            vstore<VEC>(y + (int64_t)r * C + c0, acc);
        }
    }
}

template <int s>
static void launch_dw_fwd(const VColGeom& g, hipStream_t st, View a, const float* w, const float* bias, float* y, int rows,
                          int H, int W, int Ho, int Wo, int C) {
    dim3 grid(g.nb), block(g.cx, g.cy);
    const bool al = view_aligned(a, g.vec);
    const int pt = same_pad_before(H, s), pl = same_pad_before(W, s);
    if (g.vec == 4) hipLaunchKernelGGL((dw_fwd_kernel<s, 4>), grid, block, 0, st, a, w, bias, y, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop, al);
    else if (g.vec == 2) hipLaunchKernelGGL((dw_fwd_kernel<s, 2>), grid, block, 0, st, a, w, bias, y, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop, al);
    else hipLaunchKernelGGL((dw_fwd_kernel<s, 1>), grid, block, 0, st, a, w, bias, y, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop, al);
}

int dw_fwd(View a, const float* w, const float* bias, float* y, int N, int H, int W, int C, int stride,
           hipStream_t st) {
    const int Ho = same_out(H, stride), Wo = same_out(W, stride);
    const int rows = N * Ho * Wo;
    VColGeom g = vcol_geom(rows, C, 4096);
    if (stride == 1) launch_dw_fwd<1>(g, st, a, w, bias, y, rows, H, W, Ho, Wo, C);
    else launch_dw_fwd<2>(g, st, a, w, bias, y, rows, H, W, Ho, Wo, C);
    CDRL_LAUNCH_CHECK();
    return 0;
}

template <int s, int VEC>
__global__ void __launch_bounds__(256) dw_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                          View da, int rows, int H, int W, int Ho, int Wo, int C,
                                                          int pt, int pl, int rb, int nloop, int accumulate, bool al) {
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int CX = blockDim.x, CY = blockDim.y;
    const int r0 = blockIdx.x * rb;
    const int r1 = min(r0 + rb, rows);
    for (int l = 0; l < nloop; ++l) {
        const int c0 = (l * CX + tx) * VEC;
        if (c0 >= C) continue;
        VecF<VEC> wk[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wk[k] = vload<VEC>(w + k * C + c0);
        for (int r = r0 + ty; r < r1; r += CY) {
            const int ix = r % W;
            const int q = r / W;
            const int iy = q % H;
            const int n = q / H;
            VecF<VEC> acc;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc.v[i] = 0.0f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int ny = iy + pt - ky;
                if (ny < 0 || (ny % s) != 0) continue;
                const int oy = ny / s;
                if (oy >= Ho) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int nx = ix + pl - kx;
                    if (nx < 0 || (nx % s) != 0) continue;
                    const int ox = nx / s;
                    if (ox >= Wo) continue;
                    const VecF<VEC> d = vload<VEC>(dy + (((int64_t)n * Ho + oy) * Wo + ox) * C + c0);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc.v[i] = fmaf(d.v[i], wk[ky * 3 + kx].v[i], acc.v[i]);
                }
            }
            if (accumulate) {
                const VecF<VEC> old = vload_view<VEC>(da, r, c0, 0, al);
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc.v[i] += old.v[i];
            }
            vstore_view<VEC>(da, r, c0, 0, al, acc);
        }
    }
}

template <int s>
static void launch_dw_bwd_data(const VColGeom& g, hipStream_t st, const float* dy, const float* w, View da, int rows, int H,
                               int W, int Ho, int Wo, int C, int accumulate) {
    dim3 grid(g.nb), block(g.cx, g.cy);
    const bool al = view_aligned(da, g.vec);
    const int pt = same_pad_before(H, s), pl = same_pad_before(W, s);
    if (g.vec == 4) hipLaunchKernelGGL((dw_bwd_data_kernel<s, 4>), grid, block, 0, st, dy, w, da, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop, accumulate, al);
    else if (g.vec == 2) hipLaunchKernelGGL((dw_bwd_data_kernel<s, 2>), grid, block, 0, st, dy, w, da, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop, accumulate, al);
    else hipLaunchKernelGGL((dw_bwd_data_kernel<s, 1>), grid, block, 0, st, dy, w, da, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop, accumulate, al);
}

int dw_bwd_data(const float* dy, const float* w, View da, int N, int H, int W, int C, int stride, int accumulate,
                hipStream_t st) {
    const int Ho = same_out(H, stride), Wo = same_out(W, stride);
    const int rows = N * H * W;
    VColGeom g = vcol_geom(rows, C, 4096);
    if (stride == 1) launch_dw_bwd_data<1>(g, st, dy, w, da, rows, H, W, Ho, Wo, C, accumulate);
    else launch_dw_bwd_data<2>(g, st, dy, w, da, rows, H, W, Ho, Wo, C, accumulate);
    CDRL_LAUNCH_CHECK();
    return 0;
}

template <int VEC>
struct DwBwdDataBnF {
    const float* dy;
    const float* w;
    View da;
    int H, W, Ho, Wo, C, s, pt, pl;
    const float* ypre;
    const float* stats;
    int GC, act;
    bool al;
    __device__ void operator()(int g, int64_t row, int c0, double (*acc)[VEC]) const {
        const int ix = (int)(row % W);
        const int64_t q = row / W;
        const int iy = (int)(q % H);
        const int64_t n = q / H;
        VecF<VEC> d;
#pragma unroll
        for (int i = 0; i < VEC; ++i) d.v[i] = 0.0f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ny = iy + pt - ky;
            if (ny < 0 || (ny % s) != 0) continue;
            const int oy = ny / s;
            if (oy >= Ho) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int nx = ix + pl - kx;
                if (nx < 0 || (nx % s) != 0) continue;
                const int ox = nx / s;
                if (ox >= Wo) continue;
                const VecF<VEC> g2 = vload<VEC>(dy + ((n * Ho + oy) * Wo + ox) * C + c0);
                const VecF<VEC> wk = vload<VEC>(w + (ky * 3 + kx) * C + c0);
#pragma unroll
                for (int i = 0; i < VEC; ++i) d.v[i] = fmaf(g2.v[i], wk.v[i], d.v[i]);
            }
        }
        vstore_view<VEC>(da, row, c0, 0, al, d);
        // BatchNorm-backward sums of the producing layer
        const VecF<VEC> v = vload<VEC>(ypre + row * C + c0);
        const VecF<VEC> mean = vload<VEC>(stats + 0 * GC + g * C + c0), invstd = vload<VEC>(stats + 1 * GC + g * C + c0);
        if (act == ACT_RELU6) {
            const VecF<VEC> sc = vload<VEC>(stats + 2 * GC + g * C + c0), sh = vload<VEC>(stats + 3 * GC + g * C + c0);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float z = fmaf(sc.v[i], v.v[i], sh.v[i]);
                if (!relu6_open(z)) d.v[i] = 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float xh = (v.v[i] - mean.v[i]) * invstd.v[i];
            acc[0][i] += (double)d.v[i];
            acc[1][i] += (double)d.v[i] * (double)xh;
        }
    }
};

int dw_bwd_data_bnreduce(const float* dy, const float* w, View da, int N, int H, int W, int C, int stride, int G,
                         const float* y_pre, const float* stats_pre, int act_pre, double* part, hipStream_t st) {
    const int Ho = same_out(H, stride), Wo = same_out(W, stride);
    const int Mg = (N / G) * H * W;
    const int vec = vcol_geom(Mg, C).vec;
    return launch_vcolreduce<2, DwBwdDataBnF>(G, Mg, C, part, st, NB_STATS, dy, w, da, H, W, Ho, Wo, C, stride,
                                              same_pad_before(H, stride), same_pad_before(W, stride), y_pre, stats_pre, G * C,
                                              act_pre, view_aligned(da, vec));
}

template <int VEC>
struct DwBwdFilterF {
    View a;
    const float* dy;
    int H, W, Ho, Wo, C, s, pt, pl;
    bool al;
    __device__ void operator()(int, int64_t row, int c0, double (*acc)[VEC]) const {
        const int ox = (int)(row % Wo);
        const int64_t q = row / Wo;
        const int oy = (int)(q % Ho);
        const int n = (int)(q / Ho);
        const VecF<VEC> d = vload<VEC>(dy + row * C + c0);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * s + ky - pt;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * s + kx - pl;
                if (ix < 0 || ix >= W) continue;
                const int64_t irow = ((int64_t)n * H + iy) * W + ix;
                const VecF<VEC> x = vload_view<VEC>(a, irow, c0, 0, al);
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[ky * 3 + kx][i] += (double)(x.v[i] * d.v[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[9][i] += (double)d.v[i];
    }
};

int64_t dw_bwd_part_elems(int N, int H, int W, int C, int stride) {
    const int Ho = same_out(H, stride), Wo = same_out(W, stride);
    VColGeom g = vcol_geom(N * Ho * Wo, C, NB_FILTER);
    return (int64_t)g.nb * 10 * C;
}

int dw_bwd_filter(View a, const float* dy, float* dw, float* db, int N, int H, int W, int C, int stride,
                  double* part, hipStream_t st) {
    const int Ho = same_out(H, stride), Wo = same_out(W, stride);
    const int rows = N * Ho * Wo;
    VColGeom g = vcol_geom(rows, C, NB_FILTER);
    CDRL_TRY((launch_vcolreduce<10, DwBwdFilterF>(1, rows, C, part, st, NB_FILTER, a, dy, H, W, Ho, Wo, C, stride,
                                                  same_pad_before(H, stride), same_pad_before(W, stride),
                                                  view_aligned(a, g.vec))));
    CDRL_TRY(reduce_partials(part, g.nb, 9 * C, (int64_t)10 * C, dw, 0, st));
    CDRL_TRY(reduce_partials(part + 9 * C, g.nb, C, (int64_t)10 * C, db, 0, st));
    return 0;
}

// ------------------------------------------------------------------------------------------
// MaxPooling2D(3, 2, 'same') (reference core/architectures.py:161); padding never wins.
// argmax (first maximum in (ky,kx) scan order) is saved as one byte per output element.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) maxpool_fwd_kernel(const float* __restrict__ a, float* __restrict__ p,
                                                          uint8_t* __restrict__ argmax, int rows, int H, int W, int Ho,
                                                          int Wo, int C, int pt, int pl, int rb) {
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int CX = blockDim.x, CY = blockDim.y;
    const int r0 = blockIdx.x * rb;
    const int r1 = min(r0 + rb, rows);
    for (int c = tx; c < C; c += CX) {
        for (int r = r0 + ty; r < r1; r += CY) {
            const int ox = r % Wo;
            const int q = r / Wo;
            const int oy = q % Ho;
            const int n = q / Ho;
            float best = -INFINITY;
            int bi = 0;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = oy * 2 + ky - pt;
                if (iy < 0 || iy >= H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = ox * 2 + kx - pl;
                    if (ix < 0 || ix >= W) continue;
                    const float v = a[(((int64_t)n * H + iy) * W + ix) * C + c];
                    if (v > best) {
                        best = v;
                        bi = ky * 3 + kx;
                    }
                }
            }
            p[(int64_t)r * C + c] = best;
            if (argmax) argmax[(int64_t)r * C + c] = (uint8_t)bi;
        }
    }
}

int maxpool_fwd(const float* a, float* p, uint8_t* argmax, int N, int H, int W, int C, hipStream_t st) {
    const int Ho = same_out(H, 2), Wo = same_out(W, 2);
    const int rows = N * Ho * Wo;
    ColGeom g = col_geom(rows, C, 2048);
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(g.nb), dim3(g.cx, g.cy), 0, st, a, p, argmax, rows, H, W, Ho, Wo, C,
                       same_pad_before(H, 2), same_pad_before(W, 2), g.rb);
    CDRL_LAUNCH_CHECK();
    return 0;
}

__global__ void __launch_bounds__(256) maxpool_bwd_kernel(const uint8_t* __restrict__ argmax, const float* __restrict__ dp,
                                                          float* __restrict__ da, int rows, int H, int W, int Ho, int Wo,
                                                          int C, int pt, int pl, int rb) {
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int CX = blockDim.x, CY = blockDim.y;
    const int r0 = blockIdx.x * rb;
    const int r1 = min(r0 + rb, rows);
    for (int c = tx; c < C; c += CX) {
        for (int r = r0 + ty; r < r1; r += CY) {
            const int ix = r % W;
            const int q = r / W;
            const int iy = q % H;
            const int n = q / H;
            float acc = 0.0f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int ny = iy + pt - ky;
                if (ny < 0 || (ny & 1)) continue;
                const int oy = ny >> 1;
                if (oy >= Ho) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int nx = ix + pl - kx;
                    if (nx < 0 || (nx & 1)) continue;
                    const int ox = nx >> 1;
                    if (ox >= Wo) continue;
                    const int64_t o = (((int64_t)n * Ho + oy) * Wo + ox) * C + c;
                    if ((argmax[o] & 0x7f) == (uint8_t)(ky * 3 + kx)) acc += dp[o];
                }
            }
            da[(int64_t)r * C + c] = acc;
        }
    }
}

int maxpool_bwd(const uint8_t* argmax, const float* dp, float* da, int N, int H, int W, int C, hipStream_t st) {
    const int Ho = same_out(H, 2), Wo = same_out(W, 2);
    const int rows = N * H * W;
    ColGeom g = col_geom(rows, C, 2048);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(g.nb), dim3(g.cx, g.cy), 0, st, argmax, dp, da, rows, H, W, Ho, Wo, C,
                       same_pad_before(H, 2), same_pad_before(W, 2), g.rb);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// fused BN-apply + ReLU6 + max-pool: reads the RAW stem conv output, so the 255 MB activated tensor
// is never materialised (the backward needs only y, the statistics and the argmax).
template <int VEC, class T>
__global__ void __launch_bounds__(256) maxpool_bn_fwd_kernel(const T* __restrict__ y, const float* __restrict__ stats,
                                                             int GC, int fpg, T* __restrict__ p,
                                                             uint8_t* __restrict__ argmax, int rows, int H, int W, int Ho,
                                                             int Wo, int C, int pt, int pl, int rb, int nloop) {
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int CX = blockDim.x, CY = blockDim.y;
    const int r0 = blockIdx.x * rb;
    const int r1 = min(r0 + rb, rows);
    for (int l = 0; l < nloop; ++l) {
        const int c0 = (l * CX + tx) * VEC;
        if (c0 >= C) continue;
        for (int r = r0 + ty; r < r1; r += CY) {
            const int ox = r % Wo;
            const int q = r / Wo;
            const int oy = q % Ho;
            const int n = q / Ho;
            const int g = n / fpg;
            const VecF<VEC> sc = vload<VEC>(stats + 2 * GC + g * C + c0), sh = vload<VEC>(stats + 3 * GC + g * C + c0);
            VecF<VEC> best;
            int bi[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                best.v[i] = -INFINITY;
                bi[i] = 0;
            }
            // all 9 window loads first, at clamped (always valid) addresses; validity is applied afterwards.  With the
            // bounds tests around the loads every load sat in its own branch with its own s_waitcnt: 9 round trips per row.
            VecF<VEC> xw[9];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = min(max(oy * 2 + ky - pt, 0), H - 1);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = min(max(ox * 2 + kx - pl, 0), W - 1);
                    xw[ky * 3 + kx] = vload<VEC>(y + (((int64_t)n * H + iy) * W + ix) * C + c0);
                }
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = oy * 2 + ky - pt;
                const bool vy = iy >= 0 && iy < H;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = ox * 2 + kx - pl;
                    const bool v = vy && ix >= 0 && ix < W;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const float a = fminf(fmaxf(fmaf(sc.v[i], xw[ky * 3 + kx].v[i], sh.v[i]), 0.0f), 6.0f);
                        if (v && a > best.v[i]) {
                            best.v[i] = a;
                            bi[i] = ky * 3 + kx;
                        }
                    }
                }
            }
            vstore<VEC>(p + (int64_t)r * C + c0, best);
            // bit 7 of the code: the winning activation is clamped (ReLU6 closed) -- a backward mask for kernels that do not read y
            // (round 5's coefficient-free stem gradient used it); every decoder masks the bit away
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (!relu6_open(best.v[i])) bi[i] |= 0x80;
            if (VEC == 4) {
                *reinterpret_cast<uint32_t*>(argmax + (int64_t)r * C + c0) =
                    (uint32_t)bi[0] | ((uint32_t)bi[1 % VEC] << 8) | ((uint32_t)bi[2 % VEC] << 16) | ((uint32_t)bi[3 % VEC] << 24);
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i) argmax[(int64_t)r * C + c0 + i] = (uint8_t)bi[i];
            }
        }
    }
}

int maxpool_bn_fwd(const float* y, const float* stats, int G, int frames_per_group, float* p, uint8_t* argmax, int N,
                   int H, int W, int C, hipStream_t st, int at) {
    const int Ho = same_out(H, 2), Wo = same_out(W, 2);
    const int rows = N * Ho * Wo;
    const VColGeom g = stem_pool_fwd_geom(rows, C);
    dim3 grid(g.nb), block(g.cx, g.cy);
    const int pt = same_pad_before(H, 2), pl = same_pad_before(W, 2);
    if (at) {
        const bf16_t* yb = reinterpret_cast<const bf16_t*>(y);
        bf16_t* pb = reinterpret_cast<bf16_t*>(p);
        if (g.vec == 4) hipLaunchKernelGGL((maxpool_bn_fwd_kernel<4, bf16_t>), grid, block, 0, st, yb, stats, G * C, frames_per_group, pb, argmax, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop);
        else if (g.vec == 2) hipLaunchKernelGGL((maxpool_bn_fwd_kernel<2, bf16_t>), grid, block, 0, st, yb, stats, G * C, frames_per_group, pb, argmax, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop);
        else hipLaunchKernelGGL((maxpool_bn_fwd_kernel<1, bf16_t>), grid, block, 0, st, yb, stats, G * C, frames_per_group, pb, argmax, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop);
    } else if (g.vec == 4) hipLaunchKernelGGL((maxpool_bn_fwd_kernel<4, float>), grid, block, 0, st, y, stats, G * C, frames_per_group, p, argmax, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop);
    else if (g.vec == 2) hipLaunchKernelGGL((maxpool_bn_fwd_kernel<2, float>), grid, block, 0, st, y, stats, G * C, frames_per_group, p, argmax, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop);
    else hipLaunchKernelGGL((maxpool_bn_fwd_kernel<1, float>), grid, block, 0, st, y, stats, G * C, frames_per_group, p, argmax, rows, H, W, Ho, Wo, C, pt, pl, g.rb, g.nloop);
    CDRL_LAUNCH_CHECK();
    return 0;
}

PoolSrc make_pool_src(const uint8_t* argmax, const float* dp, int H, int W) {
    PoolSrc ps;
    ps.argmax = argmax;
    ps.dp = dp;
    ps.H = H;
    ps.W = W;
    ps.Ho = same_out(H, 2);
    ps.Wo = same_out(W, 2);
    ps.pt = same_pad_before(H, 2);
    ps.pl = same_pad_before(W, 2);
    return ps;
}

}  // namespace cdrl
