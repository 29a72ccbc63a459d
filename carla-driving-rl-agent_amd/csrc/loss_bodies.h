// Device bodies shared by the one-workgroup loss kernels: loss.hip (policy / clone / value losses) and trust.hip (Beta KL).
// Everything transcendental runs in double; the reductions are double LDS trees in a fixed order.
#pragma once
#include "cdrl_kernels.h"

namespace cdrl {

__device__ inline double digamma_d(double x) {
    double r = 0.0;
    while (x < 10.0) {
        r -= 1.0 / x;
        x += 1.0;
    }
    const double f = 1.0 / (x * x);
    const double t = f * (-1.0 / 12.0 + f * (1.0 / 120.0 + f * (-1.0 / 252.0 + f * (1.0 / 240.0 + f * (-1.0 / 132.0)))));
    return r + log(x) - 0.5 / x + t;
}

__device__ __forceinline__ double softplus_d(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double sigmoid_d(double x) { return 1.0 / (1.0 + exp(-x)); }

template <int NQ>
__device__ void block_reduce(double* acc, double* sm) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NQ; ++q) sm[q * blockDim.x + tid] = acc[q];
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) sm[q * blockDim.x + tid] += sm[q * blockDim.x + tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = sm[q * blockDim.x];
    __syncthreads();
}

}  // namespace cdrl
