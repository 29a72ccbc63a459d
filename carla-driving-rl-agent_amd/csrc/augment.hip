// Rollout-time image augmentation on the device (reference core/carla_agent.py:545-577: color jitter -> random-kernel
// "blur" -> salt & pepper -> gaussian noise -> per-image min-max normalisation -> cutout -> coarse dropout; ops from
// rl/augmentations/augmentations.py and rl/augmentations/simclr.py:49-63).
//
// The host draws the plan (which ops fire and their scalar parameters: tf_chance / tf.image.random_* in the reference);
// the per-pixel random fields (salt & pepper masks, gaussian noise, dropout grid) come from Philox streams keyed by
// (seed, offset*8 + stream id, element index) so that a plan + seed determines the output exactly (oracle/augment.py
// reproduces the streams bit for bit).  One stack is tiny (T x 90 x 120 x 3 floats): kernels are simple grid-stride
// loops, reductions use one workgroup per image.  Nothing here is on the learner's timed path, but with aug_intensity > 0 it IS on
// the rollout path, once per environment step: augment_images serves one stack with up to six launches and a copy, and
// augment_images_batch serves a whole environment shard (E stacks, E plans in device memory) with five launches whatever E is,
// writing for every environment the bytes augment_images writes (both are built from the __device__ bodies below).
#include "aug_bodies.h"
#include "cdrl_kernels.h"
#include "philox.h"

namespace cdrl {

enum { AUG_SP_SELECT = 1, AUG_SP_NOISE = 2, AUG_GN_SELECT = 3, AUG_GN_NOISE = 4, AUG_DROPOUT = 5 };

// ---- per-pixel / per-image bodies, shared by the single-stack and the batched kernels so that both are compiled from the same
// expressions (the batched form must write the single-stack form's bytes); the HSV conversions, the jitter of one pixel and the
// channel mean live in aug_bodies.h, which views.hip shares

// color jitter of pixel i of a stack (x, y: the stack's base; mean: its [T][3] channel means)
__device__ __forceinline__ void jitter_pixel(const float* __restrict__ x, float* __restrict__ y, int64_t i, int P,
                                             const float* __restrict__ mean, float brightness, float contrast, float saturation,
                                             float hue) {
    const int t = (int)(i / P);
    float c[3] = {x[i * 3], x[i * 3 + 1], x[i * 3 + 2]};
    jitter_rgb(c, mean + t * 3, brightness, contrast, saturation, hue);
#pragma unroll
    for (int k = 0; k < 3; ++k) y[i * 3 + k] = c[k];
}

// k x k cross-correlation of channel c at (t, yy, xx), zero padding; w: [k][k][3]
__device__ __forceinline__ float blur_tap(const float* __restrict__ x, int t, int yy, int xx, int c, int H, int W, int k,
                                          const float* __restrict__ w) {
    const int r = k / 2;
    float acc = 0.0f;
    for (int ky = 0; ky < k; ++ky) {
        const int iy = yy + ky - r;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < k; ++kx) {
            const int ix = xx + kx - r;
            if (ix < 0 || ix >= W) continue;
            acc = fmaf(x[(((int64_t)t * H + iy) * W + ix) * 3 + c], w[(ky * k + kx) * 3 + c], acc);
        }
    }
    return acc;
}

// salt & pepper, then gaussian noise, on the three channels of pixel i of a stack (i keys the Philox streams)
__device__ __forceinline__ void noise_pixel(float (&c)[3], int64_t i, int salt_pepper, float sp_p, float sp_prob, int gauss,
                                            float gn_amount, float gn_std, uint64_t seed, uint64_t offset) {
    if (salt_pepper) {
        Philox a(seed, offset * 8 + AUG_SP_SELECT, (uint64_t)i), b(seed, offset * 8 + AUG_SP_NOISE, (uint64_t)i);
        const float sel = a.uniform() < (double)sp_p ? 1.0f : 0.0f;
        const float nz = b.uniform() < (double)sp_prob ? 1.0f : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = c[k] * (1.0f - sel) + nz * sel;
    }
    if (gauss) {
        Philox a(seed, offset * 8 + AUG_GN_SELECT, (uint64_t)i);
        const float sel = a.uniform() < (double)gn_amount ? 1.0f : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            Philox g(seed, offset * 8 + AUG_GN_NOISE, (uint64_t)(i * 3 + k));
            const float nz = (float)(g.normal() * (double)gn_std);
            c[k] += fminf(fmaxf(sel * nz, 0.0f), 1.0f);
        }
    }
}

// per-image (min, max - min) over n_per_image floats: the whole 1024-thread workgroup
__device__ __forceinline__ void minmax_body(const float* __restrict__ xp, int n_per_image, float* __restrict__ mm2) {
    __shared__ float smin[1024], smax[1024];
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < n_per_image; i += blockDim.x) {
        lo = fminf(lo, xp[i]);
        hi = fmaxf(hi, xp[i]);
    }
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int st = blockDim.x / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + st]);
            smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + st]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mm2[0] = smin[0];
        mm2[1] = smax[0] - smin[0];
    }
}

__device__ __forceinline__ int nearest_src(int dst, int out, int in) {
    int s = (int)floorf(((float)dst + 0.5f) * (float)in / (float)out);
    return s < in - 1 ? s : in - 1;
}

// min-max normalisation, cutout and coarse dropout of pixel i of a stack (mm: the stack's [T][2], read only if normalize)
__device__ __forceinline__ void final_pixel(const float* __restrict__ x, float* __restrict__ y, int64_t i, int H, int W, int normalize,
                                            const float* __restrict__ mm, float eps, int cutout_size, int cutout_cell,
                                            int dropout_size, float dropout_keep, uint64_t seed, uint64_t offset) {
    int64_t p = i;
    const int xx = (int)(p % W);
    p /= W;
    const int yy = (int)(p % H);
    const int t = (int)(p / H);
    float mask = 1.0f;
    if (cutout_size > 0) {
        const int cy = nearest_src(yy, H, cutout_size), cx = nearest_src(xx, W, cutout_size);
        if (cy * cutout_size + cx == cutout_cell) mask = 0.0f;
    }
    if (dropout_size > 0) {
        const int cy = nearest_src(yy, H, dropout_size), cx = nearest_src(xx, W, dropout_size);
        Philox d(seed, offset * 8 + AUG_DROPOUT, (uint64_t)(cy * dropout_size + cx));
        if (!(d.uniform() < (double)dropout_keep)) mask = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = x[i * 3 + k];
        if (normalize) v = (v - mm[t * 2]) / (mm[t * 2 + 1] + eps);
        y[i * 3 + k] = v * mask;
    }
}

constexpr float AUG_EPS = 1.1920929e-07f;

// ---- one stack: the plan's scalars are kernel arguments, the host launches only the stages that fire

// one workgroup per image
__global__ void __launch_bounds__(1024) aug_channel_mean_kernel(const float* __restrict__ x, int P, float add, float* __restrict__ mean) {
    channel_mean_body(x + (int64_t)blockIdx.x * P * 3, P, add, mean + blockIdx.x * 3);
}

__global__ void aug_jitter_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t npix, int P,
                                  const float* __restrict__ mean, float brightness, float contrast, float saturation, float hue) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x)
        jitter_pixel(x, y, i, P, mean, brightness, contrast, saturation, hue);
}

struct BlurK {
    float w[75];
};

__global__ void aug_blur_kernel(const float* __restrict__ x, float* __restrict__ y, int T, int H, int W, int k, BlurK bk) {
    const int64_t n = (int64_t)T * H * W * 3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3);
        int64_t p = i / 3;
        const int xx = (int)(p % W);
        p /= W;
        const int yy = (int)(p % H);
        const int t = (int)(p / H);
        y[i] = blur_tap(x, t, yy, xx, c, H, W, k, bk.w);
    }
}

__global__ void aug_noise_kernel(float* __restrict__ x, int64_t npix, int salt_pepper, float sp_p, float sp_prob, int gauss, float gn_amount,
                                 float gn_std, uint64_t seed, uint64_t offset) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        float c[3] = {x[i * 3], x[i * 3 + 1], x[i * 3 + 2]};
        noise_pixel(c, i, salt_pepper, sp_p, sp_prob, gauss, gn_amount, gn_std, seed, offset);
#pragma unroll
        for (int k = 0; k < 3; ++k) x[i * 3 + k] = c[k];
    }
}

// one workgroup per image
__global__ void __launch_bounds__(1024) aug_minmax_kernel(const float* __restrict__ x, int n_per_image, float* __restrict__ mm) {
    minmax_body(x + (int64_t)blockIdx.x * n_per_image, n_per_image, mm + blockIdx.x * 2);
}

__global__ void aug_final_kernel(const float* __restrict__ x, float* __restrict__ y, int T, int H, int W, int normalize,
                                 const float* __restrict__ mm, float eps, int cutout_size, int cutout_cell, int dropout_size,
                                 float dropout_keep, uint64_t seed, uint64_t offset) {
    const int64_t npix = (int64_t)T * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x)
        final_pixel(x, y, i, H, W, normalize, mm, eps, cutout_size, cutout_cell, dropout_size, dropout_keep, seed, offset);
}

int augment_images(const float* in, float* out, int T, int H, int W, const AugPlan& p, float* workspace, hipStream_t st) {
    if (T <= 0 || H <= 0 || W <= 0) {
        set_error("augment_images: bad shape %dx%dx%d", T, H, W);
        return -1;
    }
    if (p.blur_size != 0 && p.blur_size != 3 && p.blur_size != 5) {
        set_error("augment_images: blur_size must be 0, 3 or 5");
        return -1;
    }
    const int P = H * W;
    const int64_t npix = (int64_t)T * P, n = npix * 3;
    float* bufA = workspace;                // [n]
    float* bufB = workspace + n;            // [n]
    float* small = workspace + 2 * n;       // means [T][3] | minmax [T][2]
    const int grid = (int)((npix + 255) / 256 < 1024 ? (npix + 255) / 256 : 1024);
    const float* cur = in;
    if (p.jitter) {
        hipLaunchKernelGGL(aug_channel_mean_kernel, dim3(T), dim3(1024), 0, st, cur, P, p.brightness, small);
        hipLaunchKernelGGL(aug_jitter_kernel, dim3(grid), dim3(256), 0, st, cur, bufA, npix, P, small, p.brightness, p.contrast,
                           p.saturation, p.hue);
        cur = bufA;
    }
    if (p.blur_size) {
        BlurK bk;
        for (int i = 0; i < 75; ++i) bk.w[i] = p.blur_kernel[i];
        float* dst = cur == bufA ? bufB : bufA;
        hipLaunchKernelGGL(aug_blur_kernel, dim3(grid * 3 < 1024 ? grid * 3 : 1024), dim3(256), 0, st, cur, dst, T, H, W, p.blur_size, bk);
        cur = dst;
    }
    if (p.salt_pepper || p.gauss_noise) {
        float* buf = const_cast<float*>(cur);
        if (cur == in) {        // never write into the caller's input
            CDRL_HIP(hipMemcpyAsync(bufA, in, n * sizeof(float), hipMemcpyDeviceToDevice, st));
            buf = bufA;
        }
        hipLaunchKernelGGL(aug_noise_kernel, dim3(grid), dim3(256), 0, st, buf, npix, p.salt_pepper, p.sp_amount / 10.0f, p.sp_prob,
                           p.gauss_noise, p.gn_amount, p.gn_std, p.seed, p.offset);
        cur = buf;
    }
    if (p.normalize) hipLaunchKernelGGL(aug_minmax_kernel, dim3(T), dim3(1024), 0, st, cur, P * 3, small + 3 * T);
    hipLaunchKernelGGL(aug_final_kernel, dim3(grid), dim3(256), 0, st, cur, out, T, H, W, p.normalize, small + 3 * T, AUG_EPS,
                       p.cutout_size, p.cutout_cell, p.dropout_size, 1.0f - p.dropout_amount, p.seed, p.offset);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// ---- a shard of E stacks: the environment is the grid's y dimension and every plan field is a wave-uniform load from plans[e].
// Five launches whatever E is and whatever the plans say.  No stage copies a stack it does not change: each kernel works out from
// the plan where environment e's current data lives, as the single-stack host code does with `cur`:
//     after the jitter stage      cur1 = jitter ? A[e] : in[e]
//     after the blur/noise stage  cur2 = (blur | salt&pepper | gauss) ? B[e] : cur1
// so the caller's input is only ever read (noise without blur reads cur1 and writes B[e], where the single-stack code copies
// the input and works in place: the same values), and a workgroup of a stage that does not fire for e exits at once.
struct AugShard {
    const float* in;        // [E][n]
    float* bufA;            // [E][n]   jitter output
    float* bufB;            // [E][n]   blur / noise output
    float* mean;            // [E][T][3]
    float* mm;              // [E][T][2]
    int64_t n;              // floats per stack
};

__device__ __forceinline__ int blur_size_of(const AugPlan& p) { return p.blur_size == 3 || p.blur_size == 5 ? p.blur_size : 0; }
__device__ __forceinline__ const float* shard_cur1(const AugShard& s, const AugPlan& p, int64_t e) {
    return p.jitter ? s.bufA + e * s.n : s.in + e * s.n;
}
__device__ __forceinline__ const float* shard_cur2(const AugShard& s, const AugPlan& p, int64_t e) {
    return (blur_size_of(p) || p.salt_pepper || p.gauss_noise) ? s.bufB + e * s.n : shard_cur1(s, p, e);
}

// grid (T, E)
__global__ void __launch_bounds__(1024) aug_batch_channel_mean_kernel(AugShard s, const AugPlan* __restrict__ plans, int T, int P) {
    const int64_t e = blockIdx.y;
    const AugPlan& p = plans[e];
    if (!p.jitter) return;
    channel_mean_body(s.in + e * s.n + (int64_t)blockIdx.x * P * 3, P, p.brightness, s.mean + (e * T + blockIdx.x) * 3);
}

// grid (blocks per stack, E)
__global__ void aug_batch_jitter_kernel(AugShard s, const AugPlan* __restrict__ plans, int T, int P) {
    const int64_t e = blockIdx.y;
    const AugPlan& p = plans[e];
    if (!p.jitter) return;
    const int64_t npix = (int64_t)T * P;
    const float* x = s.in + e * s.n;
    float* y = s.bufA + e * s.n;
    const float* mean = s.mean + e * T * 3;
    const float brightness = p.brightness, contrast = p.contrast, saturation = p.saturation, hue = p.hue;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x)
        jitter_pixel(x, y, i, P, mean, brightness, contrast, saturation, hue);
}

// grid (blocks per stack, E): blur (or pass-through) of the pixel's three channels, then the noise stages, into B[e]
__global__ void aug_batch_blur_noise_kernel(AugShard s, const AugPlan* __restrict__ plans, int T, int H, int W) {
    const int64_t e = blockIdx.y;
    const AugPlan& p = plans[e];
    const int k = blur_size_of(p);
    const int salt_pepper = p.salt_pepper, gauss = p.gauss_noise;
    if (!k && !salt_pepper && !gauss) return;
    const int64_t npix = (int64_t)T * H * W;
    const float* x = shard_cur1(s, p, e);
    float* y = s.bufB + e * s.n;
    const float sp_p = p.sp_amount / 10.0f, sp_prob = p.sp_prob, gn_amount = p.gn_amount, gn_std = p.gn_std;
    const uint64_t seed = p.seed, offset = p.offset;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        float c[3];
        if (k) {
            int64_t q = i;
            const int xx = (int)(q % W);
            q /= W;
            const int yy = (int)(q % H);
            const int t = (int)(q / H);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = blur_tap(x, t, yy, xx, ch, H, W, k, p.blur_kernel);
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = x[i * 3 + ch];
        }
        noise_pixel(c, i, salt_pepper, sp_p, sp_prob, gauss, gn_amount, gn_std, seed, offset);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) y[i * 3 + ch] = c[ch];
    }
}

// grid (T, E)
__global__ void __launch_bounds__(1024) aug_batch_minmax_kernel(AugShard s, const AugPlan* __restrict__ plans, int T, int P) {
    const int64_t e = blockIdx.y;
    const AugPlan& p = plans[e];
    if (!p.normalize) return;
    minmax_body(shard_cur2(s, p, e) + (int64_t)blockIdx.x * P * 3, P * 3, s.mm + (e * T + blockIdx.x) * 2);
}

// grid (blocks per stack, E)
__global__ void aug_batch_final_kernel(AugShard s, const AugPlan* __restrict__ plans, float* __restrict__ out, int T, int H, int W) {
    const int64_t e = blockIdx.y;
    const AugPlan& p = plans[e];
    const int64_t npix = (int64_t)T * H * W;
    const float* x = shard_cur2(s, p, e);
    float* y = out + e * s.n;
    const float* mm = s.mm + e * T * 2;
    const int normalize = p.normalize, cutout_size = p.cutout_size, cutout_cell = p.cutout_cell, dropout_size = p.dropout_size;
    const float dropout_keep = 1.0f - p.dropout_amount;
    const uint64_t seed = p.seed, offset = p.offset;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x)
        final_pixel(x, y, i, H, W, normalize, mm, AUG_EPS, cutout_size, cutout_cell, dropout_size, dropout_keep, seed, offset);
}

int64_t augment_batch_workspace_floats(int E, int T, int H, int W) {
    if (E <= 0 || T <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)E * (2 * (int64_t)T * H * W * 3 + 5 * (int64_t)T);
}

int augment_images_batch(const float* in, float* out, int E, int T, int H, int W, const AugPlan* plans_dev, float* workspace,
                         hipStream_t st) {
    if (!in || !out || !plans_dev || !workspace || in == out) {
        set_error("augment_images_batch: null pointer or aliased in/out");
        return -1;
    }
    if (E <= 0 || E > AUG_BATCH_MAX_ENVS) {
        set_error("augment_images_batch: E = %d outside 1..%d", E, AUG_BATCH_MAX_ENVS);
        return -1;
    }
    if (T <= 0 || H <= 0 || W <= 0 || (int64_t)H * W * 3 > INT32_MAX) {     // the per-image index arithmetic is 32-bit
        set_error("augment_images_batch: bad shape %dx%dx%d", T, H, W);
        return -1;
    }
    const int P = H * W;
    const int64_t npix = (int64_t)T * P, n = npix * 3;
    // Philox contract (philox.h): the element index is that of ONE stack (< 3 * npix <= 2^31), far below 2^48
    AugShard s;
    s.in = in;
    s.bufA = workspace;
    s.bufB = workspace + (int64_t)E * n;
    s.mean = workspace + 2 * (int64_t)E * n;
    s.mm = s.mean + (int64_t)E * T * 3;
    s.n = n;
    const int gx = (int)((npix + 255) / 256 < 1024 ? (npix + 255) / 256 : 1024);
    const dim3 per_image(T, E), per_pixel(gx, E);
    hipLaunchKernelGGL(aug_batch_channel_mean_kernel, per_image, dim3(1024), 0, st, s, plans_dev, T, P);
    hipLaunchKernelGGL(aug_batch_jitter_kernel, per_pixel, dim3(256), 0, st, s, plans_dev, T, P);
    hipLaunchKernelGGL(aug_batch_blur_noise_kernel, per_pixel, dim3(256), 0, st, s, plans_dev, T, H, W);
    hipLaunchKernelGGL(aug_batch_minmax_kernel, per_image, dim3(1024), 0, st, s, plans_dev, T, P);
    hipLaunchKernelGGL(aug_batch_final_kernel, per_pixel, dim3(256), 0, st, s, plans_dev, out, T, H, W);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
