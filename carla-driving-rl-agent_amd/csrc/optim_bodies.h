// __device__ bodies shared by the optimizer step (optim.hip) and the update diagnostics (train_stats.hip): the bounds of a chunk, the
// 256-thread sum of squares of a chunk, the wave fold of a tensor's chunk partials, the step-counter tick and the per-optimizer
// fields of DevHP.  Every kernel that needs one of them is compiled from these expressions, so the clip path, the gradient gate and
// the train-stats rows get the same float64 bits from the same gradient.
// (stats_chunk_sqnorm_kernel, train_stats.hip, is not a caller of chunk_sqsum: one wave per chunk, no LDS, another summation order.)
#pragma once
#include "cdrl_kernels.h"

namespace cdrl {

constexpr int CHUNK = 1024;

// DevHP fields of optimizer `which` (WHICH_*).  The trunk has no per-tensor threshold: it is never clipped by tensor.
__device__ __forceinline__ float hp_lr(const DevHP* hp, int which) {
    return which == WHICH_POLICY ? hp->lr_policy : (which == WHICH_VALUE ? hp->lr_value : hp->lr_dynamics);
}
__device__ __forceinline__ int hp_t(const DevHP* hp, int which) {
    return which == WHICH_POLICY ? hp->t_policy : (which == WHICH_VALUE ? hp->t_value : hp->t_dynamics);
}
__device__ __forceinline__ float hp_m_cache(const DevHP* hp, int which) {
    return which == WHICH_POLICY ? hp->m_cache_policy : (which == WHICH_VALUE ? hp->m_cache_value : hp->m_cache_dynamics);
}
__device__ __forceinline__ float hp_clip_norm(const DevHP* hp, int which) {
    return which == WHICH_POLICY ? hp->clip_norm_policy : (which == WHICH_VALUE ? hp->clip_norm_value : 0.0f);
}

// Keras Nadam's momentum schedule (schedule decay 0.004), float32 as TensorFlow computes it: mu_t = beta1 (1 - 0.5 * 0.96^(0.004 t)).
// S_t = m_cache * mu_t is formed by an update that runs ahead of its tick and stored by the tick: one function, so both produce
// the same bits.
__device__ __forceinline__ float nadam_mu(float b1, int t) { return b1 * (1.0f - 0.5f * powf(0.96f, 0.004f * (float)t)); }

// Step counters advanced by `tick` (TickMask bits; TICK_NADAM: each ticked optimizer's m_cache also becomes S_t of its new count).
// One thread.
__device__ __forceinline__ void tick_counters(DevHP* hp, int tick) {
    if (tick & TICK_POLICY) hp->t_policy += 1;
    if (tick & TICK_VALUE) hp->t_value += 1;
    if (tick & TICK_TRUNK) hp->t_dynamics += 1;
    if (tick & TICK_NADAM) {
        if (tick & TICK_POLICY) hp->m_cache_policy = hp->m_cache_policy * nadam_mu(hp->beta1, hp->t_policy);
        if (tick & TICK_VALUE) hp->m_cache_value = hp->m_cache_value * nadam_mu(hp->beta1, hp->t_value);
        if (tick & TICK_TRUNK) hp->m_cache_dynamics = hp->m_cache_dynamics * nadam_mu(hp->beta1, hp->t_dynamics);
    }
}

// chunk c of a table: its tensor, and its elements [beg, end) of the arena (the tensor's last chunk may be partial)
__device__ __forceinline__ TensorSeg chunk_bounds(const ChunkTable& tab, int c, int64_t& beg, int64_t& end) {
    const TensorSeg s = tab.segs[tab.chunk_tensor[c]];
    beg = tab.chunk_off[c];
    end = beg + CHUNK;
    if (end > s.off + s.n) end = s.off + s.n;
    return s;
}

// sum of g[i]^2 over [beg, end) by one 256-thread workgroup: thread i takes elements i, i + 256, ... in order, each converted to
// double and squared, then a fixed LDS tree (sm: 256 doubles).  Every thread returns the same bits.
__device__ __forceinline__ double chunk_sqsum(const float* __restrict__ g, int64_t beg, int64_t end, double* sm) {
    double acc = 0.0;
    for (int64_t i = beg + threadIdx.x; i < end; i += 256) {
        const double v = (double)g[i];
        acc += v * v;
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) sm[threadIdx.x] += sm[threadIdx.x + k];
        __syncthreads();
    }
    return sm[0];
}

// a tensor's squared norm from its chunk partials by one wave: lane l takes the chunks l, l + 64, ... in order, then a fixed shuffle
// tree; every lane returns lane 0's sum, so every wave of every block that folds the tensor has the same bits.  (One thread per
// tensor would walk up to 768 partials one dependent load at a time: 17 us.)
__device__ __forceinline__ double fold_chunk_parts(const double* __restrict__ chunk_part, const TensorSeg& s) {
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int c = lane; c < s.nchunks; c += 64) acc += chunk_part[s.first_chunk + c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    return __shfl(acc, 0, 64);
}

}  // namespace cdrl
