// Device bodies shared by the trajectory kernels: gae.hip (GAE(lambda) + rewards-to-go) and vtrace.hip (their off-policy extension).
#pragma once
#include "cdrl_kernels.h"

namespace cdrl {

// The tail of a trajectory, shared by the GAE and the V-trace kernels (vtrace.hip): adv64 [N] / ret64 [N] hold the finished float64
// advantages and returns; adv_raw = (float) advantage, returns = (float) return and its decompose_number, adv = tf_sp_norm over the
// trajectory's own max / min times `scale`.  Called by the whole 256-thread workgroup behind a barrier; its barriers are block-uniform.
__device__ __forceinline__ void trajectory_tail(const double* __restrict__ adv64, const double* __restrict__ ret64, int N, float scale,
                                                float* __restrict__ returns, float* __restrict__ returns_be,
                                                float* __restrict__ adv_raw, float* __restrict__ adv) {
    __shared__ float smax[256], smin[256];
    const int tid = threadIdx.x;
    float mx = -INFINITY, mn = INFINITY;
    for (int i = tid; i < N; i += 256) {
        const float a = (float)adv64[i];
        adv_raw[i] = a;
        mx = fmaxf(mx, a);
        mn = fminf(mn, a);
        // decompose_number: while |x| > 1: x /= 10 (float32 division)
        float x = (float)ret64[i];
        returns[i] = x;
        int e = 0;
        while (fabsf(x) > 1.0f) {
            x = __fdiv_rn(x, 10.0f);
            ++e;
        }
        returns_be[2 * i] = x;
        returns_be[2 * i + 1] = (float)e;
    }
    smax[tid] = mx;
    smin[tid] = mn;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
            smax[tid] = fmaxf(smax[tid], smax[tid + k]);
            smin[tid] = fminf(smin[tid], smin[tid + k]);
        }
        __syncthreads();
    }
    // tf_sp_norm: positives / (max + eps) + negatives / -(min - eps), then * scale
    const float pden = __fadd_rn(smax[0], 1e-3f);
    const float nden = -__fsub_rn(smin[0], 1e-3f);
    for (int i = tid; i < N; i += 256) {
        const float a = adv_raw[i];
        const float pos = a > 0.0f ? a : __fmul_rn(a, 0.0f);
        const float neg = a < 0.0f ? a : __fmul_rn(a, 0.0f);
        adv[i] = __fmul_rn(__fadd_rn(__fdiv_rn(pos, pden), __fdiv_rn(neg, nden)), scale);
    }
}

}  // namespace cdrl
