// Occlusion saliency of one decision, gfx950: which cell of which frame moves the Beta policy and the value when it
// is replaced by a neutral baseline.  Forward only: the acting network runs on N = 1 + F*gh*gw (+ 4) variants of ONE observation.
//
//     occlusion_baseline   image -> baseline stack (zeros, or the per-frame channel mean)            one launch
//     occlusion_rows       rows [first, first + count) of the N variants -> one chunk of engine inputs one launch per chunk
//     occlusion_scores     alpha / beta / value of the N rows -> float64 scores of rows 1..N-1 vs row 0 one launch
//     occlusion_maps       cell scores -> (K, F, H, W) float32 maps, nearest or bilinear, normalised     one launch
//
// Row r of the N rows: 0 the observation; 1 + (f*gh + cy)*gw + cx the cell (cy, cx) of frame f (of every frame when F = 1) replaced
// by the baseline; then, with modalities, the whole image replaced, road zeroed, vehicle zeroed, navigation zeroed.  Cell (cy, cx)
// covers rows [(cy*H)/gh, ((cy+1)*H)/gh) and columns [(cx*W)/gw, ((cx+1)*W)/gw).  A row index >= N is a copy of row 0.
// The N-row tensor never exists: occlusion_rows reads one stack and its baseline and writes `count` stacks, the row being the grid's
// y dimension and its rectangle a handful of workgroup-uniform integers.
#include "aug_bodies.h"
#include "loss_bodies.h"
#include "resize_bodies.h"

namespace cdrl {

constexpr int OCC_THREADS = 256;
constexpr int OCC_SPAN = 4096;                  // floats of one row per workgroup: four 16-byte accesses per thread
constexpr int OCC_MAX_SIDE = 1 << 14;           // H, W (the cell arithmetic is 32-bit)

enum { OCC_COPY = 0, OCC_CELL, OCC_IMAGE, OCC_ROAD, OCC_VEHICLE, OCC_NAVIGATION };

struct OccRect {            // what a row occludes; workgroup-uniform
    int kind;
    int f;                  // frame of a cell, -1: every frame
    int y0, y1, x0, x1;
};

__host__ __device__ inline int occlusion_row_count(int T, int gh, int gw, int per_frame, int modalities) {
    return 1 + (per_frame ? T : 1) * gh * gw + (modalities ? 4 : 0);
}

__device__ __forceinline__ OccRect occ_decode(const OcclusionRowsArgs& p, int r) {
    OccRect o = {OCC_COPY, -1, 0, 0, 0, 0};
    const int F = p.per_frame ? p.T : 1, cells = F * p.gh * p.gw;
    if (r < 1 || r >= occlusion_row_count(p.T, p.gh, p.gw, p.per_frame, p.modalities)) return o;
    if (r > cells) {
        o.kind = OCC_IMAGE + (r - 1 - cells);
        return o;
    }
    const int c = r - 1, cx = c % p.gw, cy = (c / p.gw) % p.gh;
    o.kind = OCC_CELL;
    o.f = p.per_frame ? c / (p.gw * p.gh) : -1;
    o.y0 = (cy * p.H) / p.gh;
    o.y1 = ((cy + 1) * p.H) / p.gh;
    o.x0 = (cx * p.W) / p.gw;
    o.x1 = ((cx + 1) * p.W) / p.gw;
    return o;
}

__device__ __forceinline__ bool occ_inside(const OccRect& o, unsigned t, unsigned y, unsigned x) {
    return (o.f < 0 || (int)t == o.f) && (int)y >= o.y0 && (int)y < o.y1 && (int)x >= o.x0 && (int)x < o.x1;
}

// does any image line of the floats [e0, e1) of a stack cross the rectangle's rows?  (uniform; a few frames at most)
__device__ __forceinline__ bool occ_touches(const OccRect& o, unsigned e0, unsigned e1, int H, int W) {
    const int l0 = (int)(e0 / (3u * W)), l1 = (int)((e1 - 1) / (3u * W));
    for (int t = l0 / H; t <= l1 / H; ++t) {
        if (o.f >= 0 && t != o.f) continue;
        if (t * H + o.y0 <= l1 && t * H + o.y1 - 1 >= l0) return true;
    }
    return false;
}

// grid (spans of a row, rows of the chunk).  VEC: 16-byte accesses (the row length a multiple of 4 floats, all three bases aligned)
template <bool VEC>
__global__ void __launch_bounds__(OCC_THREADS) occlusion_rows_kernel(OcclusionRowsArgs p) {
    const int j = blockIdx.y;
    const OccRect o = occ_decode(p, p.first + j);
    const unsigned n = (unsigned)p.T * p.H * p.W * 3u;
    const unsigned e0 = blockIdx.x * (unsigned)OCC_SPAN, e1 = min(n, e0 + (unsigned)OCC_SPAN);
    const unsigned H = p.H, W = p.W;
    // a span the rectangle does not reach is a plain copy that never reads the baseline; the image row is the baseline itself
    const bool mix = o.kind == OCC_CELL && occ_touches(o, e0, e1, p.H, p.W);
    const float* __restrict__ src = o.kind == OCC_IMAGE ? p.baseline : p.image;
    const float* __restrict__ base = p.baseline;
    float* __restrict__ dst = p.out_image + (int64_t)j * n;
    if (VEC) {
        const float4* __restrict__ src4 = reinterpret_cast<const float4*>(src);
        const float4* __restrict__ base4 = reinterpret_cast<const float4*>(base);
        float4* __restrict__ dst4 = reinterpret_cast<float4*>(dst);
        for (unsigned q = e0 / 4u + threadIdx.x; q < e1 / 4u; q += OCC_THREADS) {
            float4 v = src4[q];
            if (mix) {
                // floats 4q .. 4q+3 belong to pixel px (those of channel phase k .. 2) and to pixel px + 1
                const unsigned e = 4u * q, px = e / 3u, k = e - 3u * px;
                const unsigned line = px / W, x = px - line * W, t = line / H, y = line - t * H;
                unsigned xn = x + 1u, yn = y, tn = t;
                if (xn == W) {
                    xn = 0u;
                    if (++yn == H) {
                        yn = 0u;
                        ++tn;
                    }
                }
                const bool in0 = occ_inside(o, t, y, x), in1 = occ_inside(o, tn, yn, xn);
                if (in0 || in1) {
                    const float4 b = base4[q];
                    v.x = in0 ? b.x : v.x;
                    v.y = (k + 1u < 3u ? in0 : in1) ? b.y : v.y;
                    v.z = (k + 2u < 3u ? in0 : in1) ? b.z : v.z;
                    v.w = in1 ? b.w : v.w;
                }
            }
            dst4[q] = v;
        }
    } else {
        for (unsigned e = e0 + threadIdx.x; e < e1; e += OCC_THREADS) {
            float v = src[e];
            if (mix) {
                const unsigned px = e / 3u, line = px / W, x = px - line * W, t = line / H, y = line - t * H;
                if (occ_inside(o, t, y, x)) v = base[e];
            }
            dst[e] = v;
        }
    }
    if (blockIdx.x != 0) return;
    // the three vector inputs of the row: a few dozen floats
    const int nr = p.T * p.Dr, nv = p.T * p.Dv, nn = p.T * p.Dn;
    for (int i = threadIdx.x; i < nr + nv + nn; i += OCC_THREADS) {
        if (i < nr)
            p.out_road[(int64_t)j * nr + i] = o.kind == OCC_ROAD ? 0.0f : p.road[i];
        else if (i < nr + nv)
            p.out_vehicle[(int64_t)j * nv + i - nr] = o.kind == OCC_VEHICLE ? 0.0f : p.vehicle[i - nr];
        else
            p.out_navigation[(int64_t)j * nn + i - nr - nv] = o.kind == OCC_NAVIGATION ? 0.0f : p.navigation[i - nr - nv];
    }
}

static bool occ_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb;
    return a0 < b1 && b0 < a1;
}

static int occ_check_shape(const char* what, int T, int H, int W) {
    if (T < 1 || H < 1 || W < 1 || H > OCC_MAX_SIDE || W > OCC_MAX_SIDE || (int64_t)T * H * W * 3 >= ((int64_t)1 << 31)) {
        set_error("%s: bad shape %dx%dx%d (at least one frame of 1 x 1, sides up to 16384, fewer than 2^31 floats)", what, T, H, W);
        return -1;
    }
    return 0;
}

int occlusion_rows(const OcclusionRowsArgs& a, hipStream_t st) {
    if (!a.image || !a.baseline || !a.road || !a.vehicle || !a.navigation || !a.out_image || !a.out_road || !a.out_vehicle ||
        !a.out_navigation) {
        set_error("occlusion_rows: null pointer");
        return -1;
    }
    CDRL_TRY(occ_check_shape("occlusion_rows", a.T, a.H, a.W));
    if (a.gh < 1 || a.gh > a.H || a.gw < 1 || a.gw > a.W) {
        set_error("occlusion_rows: grid %d x %d outside 1..%d x 1..%d", a.gh, a.gw, a.H, a.W);
        return -1;
    }
    if (a.Dr < 1 || a.Dv < 1 || a.Dn < 1 || a.Dr > 4096 || a.Dv > 4096 || a.Dn > 4096) {
        set_error("occlusion_rows: vector widths %d / %d / %d outside 1..4096", a.Dr, a.Dv, a.Dn);
        return -1;
    }
    if ((int64_t)a.T * a.gh * a.gw + 5 >= ((int64_t)1 << 30)) {
        set_error("occlusion_rows: %d frames of %d x %d cells are too many rows", a.T, a.gh, a.gw);
        return -1;
    }
    if (a.first < 0 || a.count < 1 || a.count > 65535 || (int64_t)a.first + a.count >= ((int64_t)1 << 31)) {
        set_error("occlusion_rows: rows [%d, %d + %d): first >= 0 and 1 <= count <= 65535", a.first, a.first, a.count);
        return -1;
    }
    const int64_t n = (int64_t)a.T * a.H * a.W * 3, bytes = n * (int64_t)sizeof(float);
    if (occ_overlap(a.out_image, bytes * a.count, a.image, bytes) || occ_overlap(a.out_image, bytes * a.count, a.baseline, bytes)) {
        set_error("occlusion_rows: the chunk overlaps the image or the baseline");
        return -1;
    }
    const bool vec = n % 4 == 0 && ((uintptr_t)a.image | (uintptr_t)a.baseline | (uintptr_t)a.out_image) % 16 == 0;
    const dim3 grid((unsigned)cdiv64(n, OCC_SPAN), (unsigned)a.count);
    if (vec)
        hipLaunchKernelGGL(occlusion_rows_kernel<true>, grid, dim3(OCC_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(occlusion_rows_kernel<false>, grid, dim3(OCC_THREADS), 0, st, a);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// grid (T): one workgroup per frame; the mean as channel_mean_body forms it (fixed-order double sums), then the frame is filled
__global__ void __launch_bounds__(1024) occlusion_baseline_kernel(const float* __restrict__ image, float* __restrict__ baseline, int P,
                                                                  int mode) {
    __shared__ float m3[3];
    const int64_t off = (int64_t)blockIdx.x * P * 3;
    if (mode == 1)
        channel_mean_body(image + off, P, 0.0f, m3);
    else if (threadIdx.x < 3)
        m3[threadIdx.x] = 0.0f;
    __syncthreads();
    const float m[3] = {m3[0], m3[1], m3[2]};
    for (int q = threadIdx.x; q < P; q += blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) baseline[off + (int64_t)q * 3 + c] = m[c];
    }
}

int occlusion_baseline(const float* image, float* baseline, int T, int H, int W, int mode, hipStream_t st) {
    if (!image || !baseline) {
        set_error("occlusion_baseline: null pointer");
        return -1;
    }
    CDRL_TRY(occ_check_shape("occlusion_baseline", T, H, W));
    if (T > 65535) {
        set_error("occlusion_baseline: %d frames (at most 65535)", T);
        return -1;
    }
    if (mode != 0 && mode != 1) {
        set_error("occlusion_baseline: mode %d (0: zeros, 1: per-frame channel mean)", mode);
        return -1;
    }
    const int64_t bytes = (int64_t)T * H * W * 3 * (int64_t)sizeof(float);
    if (occ_overlap(image, bytes, baseline, bytes)) {
        set_error("occlusion_baseline: the baseline overlaps the image");
        return -1;
    }
    hipLaunchKernelGGL(occlusion_baseline_kernel, dim3(T), dim3(1024), 0, st, image, baseline, H * W, mode);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// one thread per row g = 1 .. N-1 against row 0, everything in double: [0] KL(Beta(row 0) || Beta(row g)) summed over the actions
// (the analytic form of beta_kl_kernel, the anchor first), [1] the value difference, [2 + a] the signed shift of the Beta mean
__global__ void __launch_bounds__(256) occlusion_scores_kernel(const float* __restrict__ alpha, const float* __restrict__ beta,
                                                               const float* __restrict__ value, int N, int A,
                                                               double* __restrict__ scores) {
    const int g = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    double* s = scores + (int64_t)(g - 1) * (2 + A);
    double kl = 0.0;
    for (int a = 0; a < A; ++a) {
        const double a0 = (double)alpha[a], b0 = (double)beta[a];
        const double al = (double)alpha[(int64_t)g * A + a], be = (double)beta[(int64_t)g * A + a];
        const double lnB = lgamma(al) + lgamma(be) - lgamma(al + be);
        const double lnB0 = lgamma(a0) + lgamma(b0) - lgamma(a0 + b0);
        kl += lnB - lnB0 + (a0 - al) * digamma_d(a0) + (b0 - be) * digamma_d(b0) + (al - a0 + be - b0) * digamma_d(a0 + b0);
        s[2 + a] = al / (al + be) - a0 / (a0 + b0);
    }
    s[0] = kl;
    s[1] = (double)value[2 * (int64_t)g] * pow(10.0, (double)value[2 * (int64_t)g + 1]) - (double)value[0] * pow(10.0, (double)value[1]);
}

int occlusion_scores(const float* alpha, const float* beta, const float* value, int N, int A, double* scores, hipStream_t st) {
    if (!alpha || !beta || !value || !scores) {
        set_error("occlusion_scores: null pointer");
        return -1;
    }
    if (N < 2 || N > (1 << 24) || A < 1 || A > 8) {
        set_error("occlusion_scores: N = %d rows (2 .. 2^24), A = %d actions (1 .. 8)", N, A);
        return -1;
    }
    hipLaunchKernelGGL(occlusion_scores_kernel, dim3(cdiv(N - 1, 256)), dim3(256), 0, st, alpha, beta, value, N, A, scores);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// grid (blocks over F*H*W, K): every workgroup finds its column's largest |score| over the F*gh*gw cells itself (strided maxima,
// then a tree: a fixed order), then writes pixels.  nearest: the score of the cell that holds the pixel; bilinear: resize_src's taps
// on the gh x gw grid of a frame, x first, then y, in double.
__global__ void __launch_bounds__(256) occlusion_maps_kernel(const double* __restrict__ scores, int K, int F, int gh, int gw, int H, int W,
                                                             int bilinear, int normalize, float* __restrict__ maps) {
    __shared__ double sm[256];
    const int k = blockIdx.y, cells = F * gh * gw, tid = threadIdx.x;
    double m = 0.0;
    if (normalize) {
        for (int c = tid; c < cells; c += 256) {
            const double x = fabs(scores[(int64_t)c * K + k]);
            m = x > m ? x : m;
        }
        sm[tid] = m;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) sm[tid] = sm[tid + s] > sm[tid] ? sm[tid + s] : sm[tid];
            __syncthreads();
        }
        m = sm[0];
    }
    const bool zero = normalize && !(m > 0.0);          // an all-zero column: zeros, never 0 / 0
    const int64_t npix = (int64_t)F * H * W;
    float* out = maps + (int64_t)k * npix;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < npix; i += (int64_t)gridDim.x * 256) {
        int64_t q = i;
        const int x = (int)(q % W);
        q /= W;
        const int y = (int)(q % H);
        const int f = (int)(q / H);
        const double* sf = scores + (int64_t)f * gh * gw * K + k;
        double v = 0.0;
        if (zero) {
        } else if (!bilinear) {
            // the last cell whose first row (column) is not beyond the pixel
            const int cy = ((y + 1) * gh - 1) / H, cx = ((x + 1) * gw - 1) / W;
            const double s = sf[(int64_t)(cy * gw + cx) * K];
            v = normalize ? s / m : s;
        } else {
            int x0, x1, y0, y1;
            float fx, fy;
            resize_src(x, gw, W, x0, x1, fx);
            resize_src(y, gh, H, y0, y1, fy);
            double s00 = sf[(int64_t)(y0 * gw + x0) * K], s01 = sf[(int64_t)(y0 * gw + x1) * K];
            double s10 = sf[(int64_t)(y1 * gw + x0) * K], s11 = sf[(int64_t)(y1 * gw + x1) * K];
            if (normalize) {
                s00 /= m;
                s01 /= m;
                s10 /= m;
                s11 /= m;
            }
            const double top = s00 + (s01 - s00) * (double)fx, bot = s10 + (s11 - s10) * (double)fx;
            v = top + (bot - top) * (double)fy;
        }
        out[i] = (float)v;
    }
}

int occlusion_maps(const double* scores, int K, int F, int gh, int gw, int H, int W, int upsample, int normalize, float* maps,
                   hipStream_t st) {
    if (!scores || !maps) {
        set_error("occlusion_maps: null pointer");
        return -1;
    }
    CDRL_TRY(occ_check_shape("occlusion_maps", F, H, W));
    if (K < 1 || K > 10 || gh < 1 || gh > H || gw < 1 || gw > W) {
        set_error("occlusion_maps: K = %d columns (1 .. 10), grid %d x %d outside 1..%d x 1..%d", K, gh, gw, H, W);
        return -1;
    }
    if (upsample != 0 && upsample != 1) {
        set_error("occlusion_maps: upsample %d (0: nearest, 1: bilinear)", upsample);
        return -1;
    }
    const int64_t npix = (int64_t)F * H * W;
    const int gx = (int)(cdiv64(npix, 256) < 1024 ? cdiv64(npix, 256) : 1024);
    hipLaunchKernelGGL(occlusion_maps_kernel, dim3(gx, K), dim3(256), 0, st, scores, K, F, gh, gw, H, W, upsample, normalize != 0, maps);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
