// __device__ bodies shared by the rollout augmentation (augment.hip) and the contrastive view pipeline (views.hip): the HSV
// conversions, the colour jitter of one pixel and the per-(frame, channel) mean.  Both translation units are compiled from these
// expressions, so a jitter plan gives the same values in either.
#pragma once
#include "cdrl_common.h"

namespace cdrl {

__device__ __forceinline__ void rgb_to_hsv(float r, float g, float b, float& h, float& s, float& v) {
    v = fmaxf(fmaxf(r, g), b);
    const float mn = fminf(fminf(r, g), b);
    const float d = v - mn;
    s = v > 0.0f ? d / v : 0.0f;
    if (d > 0.0f) {
        float hh;
        if (v == r) hh = (g - b) / d;
        else if (v == g) hh = 2.0f + (b - r) / d;
        else hh = 4.0f + (r - g) / d;
        hh /= 6.0f;
        h = hh - floorf(hh);
    } else {
        h = 0.0f;
    }
}

__device__ __forceinline__ float hsv_f(float n, float h6, float s, float v) {
    const float k = fmodf(n + h6, 6.0f);
    return v - v * s * fmaxf(0.0f, fminf(fminf(k, 4.0f - k), 1.0f));
}

__device__ __forceinline__ void hsv_to_rgb(float h, float s, float v, float& r, float& g, float& b) {
    const float h6 = h * 6.0f;
    r = hsv_f(5.0f, h6, s, v);
    g = hsv_f(3.0f, h6, s, v);
    b = hsv_f(1.0f, h6, s, v);
}

// per-(image, channel) mean over H*W of x + add: the whole 1024-thread workgroup, strided partial sums in double, then a tree
__device__ __forceinline__ void channel_mean_body(const float* __restrict__ xp, int P, float add, float* __restrict__ mean3) {
    __shared__ double sm[3][1024];
    double s[3] = {0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < P; p += blockDim.x)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += (double)(xp[p * 3 + c] + add);
#pragma unroll
    for (int c = 0; c < 3; ++c) sm[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int st = blockDim.x / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
#pragma unroll
            for (int c = 0; c < 3; ++c) sm[c][threadIdx.x] += sm[c][threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x < 3) mean3[threadIdx.x] = (float)(sm[threadIdx.x][0] / (double)P);
}

// color jitter of one pixel's three channels (m3: the channel means of its frame): brightness -> contrast about the mean ->
// saturation -> hue -> clip to [0, 1]
__device__ __forceinline__ void jitter_rgb(float (&c)[3], const float* __restrict__ m3, float brightness, float contrast,
                                           float saturation, float hue) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float m = m3[k];
        c[k] = (c[k] + brightness - m) * contrast + m;
    }
    float h, s, v;
    rgb_to_hsv(c[0], c[1], c[2], h, s, v);
    s = fminf(fmaxf(s * saturation, 0.0f), 1.0f);
    hsv_to_rgb(h, s, v, c[0], c[1], c[2]);
    rgb_to_hsv(c[0], c[1], c[2], h, s, v);
    h = h + hue;
    h = h - floorf(h);
    hsv_to_rgb(h, s, v, c[0], c[1], c[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = fminf(fmaxf(c[k], 0.0f), 1.0f);
}

}  // namespace cdrl
