// Update diagnostics of the apply steps (gfx950): per-tensor gradient norms and the row writer of the train-stats ring.
//
// Reference: the TensorBoard scalars PPOAgent.update / CARLAgent.update log per minibatch (rl/agents/ppo.py:209-225,
// core/carla_agent.py:382,423-426,461,483-484): tf.norm of every gradient tensor as get_*_gradients returned it (unclipped), the loss
// terms, the mean auxiliary predictions, the DynamicParameter values in force.  Here they are produced on the device at the tail of
// policy_apply / value_apply and appended to a ring the host reads once per update(); the row index is a device-side counter, so a
// replayed hipGraph of the apply step writes successive rows.
// Norms: float64 accumulation in two deterministic stages (1024-element chunk partials, then one wave per tensor), no atomics.  The
// heads' chunk partials are the clip path's (sqnorm_chunk_kernel, optim.hip); every tensor is folded by the body the update kernel
// clips with (fold_chunk_parts, optim_bodies.h).
#include "optim_bodies.h"

namespace cdrl {

// one wave per chunk: lane l takes elements l, l + 64, ... of the chunk (coalesced 256-byte rows), fixed shuffle tree.  Not
// chunk_sqsum (optim_bodies.h): that one sums 256 threads through LDS, in another order, so the trunk norms of a row would get other
// float64 bits.
__global__ void __launch_bounds__(256) stats_chunk_sqnorm_kernel(const float* __restrict__ g, ChunkTable tab) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= tab.nchunks) return;
    int64_t beg, end;
    chunk_bounds(tab, c, beg, end);
    double acc = 0.0;
#pragma unroll 4
    for (int64_t i = beg + lane; i < end; i += 64) {
        const double v = (double)g[i];
        acc += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) tab.chunk_part[c] = acc;
}

int stats_chunk_sqnorms(const float* g, const ChunkTable& tab, hipStream_t st) {
    if (tab.nchunks <= 0) return 0;
    hipLaunchKernelGGL(stats_chunk_sqnorm_kernel, dim3(cdiv(tab.nchunks, 4)), dim3(256), 0, st, g, tab);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// one wave per tensor: the tensors of table a, then those of table b
__global__ void __launch_bounds__(256) stats_fold_norms_kernel(float* __restrict__ ring, int header, int rows, int width,
                                                               ChunkTable tab_a, int off_a, ChunkTable tab_b, int off_b) {
    int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= tab_a.ntensors + tab_b.ntensors) return;
    const bool second = t >= tab_a.ntensors;
    if (second) t -= tab_a.ntensors;
    const double sum = second ? fold_chunk_parts(tab_b.chunk_part, tab_b.segs[t]) : fold_chunk_parts(tab_a.chunk_part, tab_a.segs[t]);
    if ((threadIdx.x & 63) == 0) {
        const unsigned count = reinterpret_cast<const unsigned*>(ring)[0];
        float* row = ring + header + (size_t)(count % (unsigned)rows) * width;
        row[(second ? off_b : off_a) + t] = (float)sqrt(sum);
    }
}

int stats_fold_norms(float* ring, int header, int rows, int width, const ChunkTable& tab_a, int off_a, const ChunkTable& tab_b,
                     int off_b, hipStream_t st) {
    const int na = tab_a.ntensors, nb = tab_b.ntensors;
    if (na + nb <= 0) return 0;
    if (rows <= 0 || off_a + na > width || off_b + nb > width) {
        set_error("stats_fold_norms: %d + %d / %d + %d tensors do not fit a row of %d floats", off_a, na, off_b, nb, width);
        return -1;
    }
    hipLaunchKernelGGL(stats_fold_norms_kernel, dim3(cdiv(na + nb, 4)), dim3(256), 0, st, ring, header, rows, width, tab_a, off_a,
                       tab_b, off_b);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// One workgroup: metrics block verbatim, hyper-parameters and step counts from DevHP, the means of the two auxiliary heads over the
// B rows (float64, fixed tree), zeros in the norm slots this kind of row does not use; thread 0 then advances the counters.  Every
// thread reads the row counter before the barrier in front of that store.
__global__ void __launch_bounds__(256) stats_row_kernel(StatsRowArgs a) {
    __shared__ double sm[2][256];
    unsigned* head = reinterpret_cast<unsigned*>(a.ring);
    const unsigned count = head[0];
    float* row = a.ring + a.header + (size_t)(count % (unsigned)a.rows) * a.width;
    const int tid = threadIdx.x;
    double sp = 0.0, si = 0.0;
    for (int b = tid; b < a.B; b += 256) {
        const double ls = (double)a.lin[(int64_t)b * a.ld + a.col_speed], lm = (double)a.lin[(int64_t)b * a.ld + a.col_similarity];
        sp += 2.0 / (1.0 + exp(-ls));
        si += tanh(lm);
    }
    sm[0][tid] = sp;
    sm[1][tid] = si;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
            sm[0][tid] += sm[0][tid + k];
            sm[1][tid] += sm[1][tid + k];
        }
        __syncthreads();
    }
    if (tid < STATS_NSCALARS) {
        const DevHP* hp = a.hp;
        float v = 0.0f;
        switch (tid) {
            case STATS_KIND: v = __int_as_float(a.kind); break;
            case STATS_T_HEAD: v = __int_as_float(hp_t(hp, a.kind)); break;
            case STATS_T_DYNAMICS: v = __int_as_float(hp->t_dynamics); break;
            case STATS_LR: v = hp_lr(hp, a.kind); break;
            case STATS_LR_DYNAMICS: v = hp->lr_dynamics; break;
            case STATS_CLIP_RATIO: v = hp->clip_ratio; break;
            case STATS_ENTROPY_COEF: v = hp->entropy_coef; break;
            case STATS_SPEED: v = (float)(sm[0][0] / (double)a.B); break;
            case STATS_SIMILARITY: v = (float)(sm[1][0] / (double)a.B); break;
            default: break;
        }
        row[a.off_scalars + tid] = v;
    } else if (tid < STATS_NSCALARS + 16) {
        row[a.off_metrics + tid - STATS_NSCALARS] = a.metrics[tid - STATS_NSCALARS];
    }
    for (int i = a.off_norms + a.n_head + tid; i < a.off_trunk; i += 256) row[i] = 0.0f;
    for (int i = a.off_trunk + a.n_trunk + tid; i < a.width; i += 256) row[i] = 0.0f;
    __syncthreads();
    if (tid == 0) {
        head[0] = count + 1u;
        if (count >= (unsigned)a.rows) head[1] += 1u;
    }
}

int stats_write_row(const StatsRowArgs& a, hipStream_t st) {
    if (!a.ring || a.rows <= 0 || a.off_norms + a.n_head > a.off_trunk || a.off_trunk + a.n_trunk > a.width ||
        a.off_scalars + STATS_NSCALARS > a.width || a.off_metrics + 16 > a.width) {
        set_error("stats_write_row: bad row layout");
        return -1;
    }
    hipLaunchKernelGGL(stats_row_kernel, dim3(1), dim3(256), 0, st, a);
    CDRL_LAUNCH_CHECK();
    return 0;
}

__global__ void stats_reset_kernel(unsigned* head) {
    head[0] = 0u;
    head[1] = 0u;
}

int stats_reset_ring(float* ring, hipStream_t st) {
    hipLaunchKernelGGL(stats_reset_kernel, dim3(1), dim3(1), 0, st, reinterpret_cast<unsigned*>(ring));
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
