// Update diagnostics of the apply steps (gfx950): per-tensor gradient norms and the row writer of the train-stats ring.
//
// Reference: the TensorBoard scalars PPOAgent.update / CARLAgent.update log per minibatch (rl/agents/ppo.py:209-225,
// core/carla_agent.py:382,423-426,461,483-484): tf.norm of every gradient tensor as get_*_gradients returned it (unclipped), the loss
// terms, the mean auxiliary predictions, the DynamicParameter values in force.  Here they are produced on the device at the tail of
// policy_apply / value_apply and appended to a ring the host reads once per update(); the row index is a device-side counter, so a
// replayed hipGraph of the apply step writes successive rows.
// Norms: float64 accumulation in two deterministic stages (1024-element chunk partials, then one wave per tensor), no atomics.  The
// heads' chunk partials are the clip path's (sqnorm_chunk_kernel, optim.hip), folded in sqnorm_final_kernel's order.
#include "cdrl_kernels.h"

namespace cdrl {

#define CHUNK 1024

// one wave per chunk: lane l takes elements l, l + 64, ... of the chunk (coalesced 256-byte rows), fixed shuffle tree
__global__ void __launch_bounds__(256) stats_chunk_sqnorm_kernel(const float* __restrict__ g, const TensorSeg* __restrict__ segs,
                                                                 const int* __restrict__ chunk_tensor,
                                                                 const int64_t* __restrict__ chunk_off, int nchunks,
                                                                 double* __restrict__ chunk_part) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= nchunks) return;
    const TensorSeg s = segs[chunk_tensor[c]];
    const int64_t beg = chunk_off[c];
    int64_t end = beg + CHUNK;
    if (end > s.off + s.n) end = s.off + s.n;
    double acc = 0.0;
#pragma unroll 4
    for (int64_t i = beg + lane; i < end; i += 64) {
        const double v = (double)g[i];
        acc += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) chunk_part[c] = acc;
}

int stats_chunk_sqnorms(const float* g, const TensorSeg* segs_dev, const int* chunk_tensor_dev, const int64_t* chunk_off_dev,
                        int nchunks, double* chunk_part, hipStream_t st) {
    if (nchunks <= 0) return 0;
    hipLaunchKernelGGL(stats_chunk_sqnorm_kernel, dim3(cdiv(nchunks, 4)), dim3(256), 0, st, g, segs_dev, chunk_tensor_dev,
                       chunk_off_dev, nchunks, chunk_part);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// one wave per tensor (sqnorm_final_kernel's fold: a thread per tensor would walk up to 768 partials one dependent load at a time);
// tensors [0, na) of table a, then [0, nb) of table b
__global__ void __launch_bounds__(256) stats_fold_norms_kernel(float* __restrict__ ring, int header, int rows, int width,
                                                               const TensorSeg* __restrict__ segs_a, int na,
                                                               const double* __restrict__ part_a, int off_a,
                                                               const TensorSeg* __restrict__ segs_b, int nb,
                                                               const double* __restrict__ part_b, int off_b) {
    const int lane = threadIdx.x & 63;
    int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= na + nb) return;
    const bool second = t >= na;
    if (second) t -= na;
    const TensorSeg s = second ? segs_b[t] : segs_a[t];
    const double* part = second ? part_b : part_a;
    double acc = 0.0;
    for (int c = lane; c < s.nchunks; c += 64) acc += part[s.first_chunk + c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) {
        const unsigned count = reinterpret_cast<const unsigned*>(ring)[0];
        float* row = ring + header + (size_t)(count % (unsigned)rows) * width;
        row[(second ? off_b : off_a) + t] = (float)sqrt(acc);
    }
}

int stats_fold_norms(float* ring, int header, int rows, int width, const TensorSeg* segs_a, int na, const double* part_a, int off_a,
                     const TensorSeg* segs_b, int nb, const double* part_b, int off_b, hipStream_t st) {
    if (na + nb <= 0) return 0;
    if (rows <= 0 || off_a + na > width || off_b + nb > width) {
        set_error("stats_fold_norms: %d + %d / %d + %d tensors do not fit a row of %d floats", off_a, na, off_b, nb, width);
        return -1;
    }
    hipLaunchKernelGGL(stats_fold_norms_kernel, dim3(cdiv(na + nb, 4)), dim3(256), 0, st, ring, header, rows, width, segs_a, na,
                       part_a, off_a, segs_b, nb, part_b, off_b);
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
            case STATS_T_HEAD: v = __int_as_float(a.kind == 0 ? hp->t_policy : hp->t_value); break;
            case STATS_T_DYNAMICS: v = __int_as_float(hp->t_dynamics); break;
            case STATS_LR: v = a.kind == 0 ? hp->lr_policy : hp->lr_value; break;
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
