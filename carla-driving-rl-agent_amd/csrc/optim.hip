// Per-tensor clip-by-norm + the optimizer step over flat parameter arenas (gfx950).
//
// Reference: utils.clip_gradients -> tf.clip_by_norm per tensor (rl/utils.py:120-121), applied to
// the policy / value heads only (F9); Keras Adam (beta1 .9, beta2 .999, eps 1e-7) in the fused
// `ResourceApplyAdam` form:
//     alpha = lr * sqrt(1 - b2^t) / (1 - b1^t);  m += (g - m)(1 - b1);  v += (g*g - v)(1 - b2)
//     theta -= m * alpha / (sqrt(v) + eps)
// Hyper-parameters and the step counters live in a device block (DevHP) so that a captured
// hipGraph of the whole update step can be replayed while learning rates change between steps.
// One workgroup handles one 1024-element chunk of one tensor: HBM-bound streaming, no atomics,
// norms reduced in two deterministic stages (bodies: optim_bodies.h).
// One update kernel, clip_update_kernel<OPT, GATE>, serves Adam, the seven other Keras optimizers of cdrl_config.optimizer (table in
// include/cdrl.h), polyak averaging and the gated forms.
#include "optim_bodies.h"
#include "../../include/cdrl.h"

namespace cdrl {

// the tick without a norm (the trunk-only apply: its update ran in front, nothing runs behind)
__global__ void tick_kernel(DevHP* hp, int tick) {
    if (blockIdx.x == 0 && threadIdx.x == 0) tick_counters(hp, tick);
}

int tick_steps(DevHP* hp, int tick_mask, hipStream_t st) {
    if (!hp || tick_mask <= 0) {
        set_error("tick_steps: null hyper-parameter block or empty mask");
        return -1;
    }
    hipLaunchKernelGGL(tick_kernel, dim3(1), dim3(64), 0, st, hp, tick_mask);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// Step counters advanced here instead of by a launch of their own: the trunk's (its update ran in FRONT of this kernel) and the head's,
// whose update runs BEHIND it and is told so (clip_update's `ticked`).
__global__ void __launch_bounds__(256) sqnorm_chunk_kernel(const float* __restrict__ g, ChunkTable tab, DevHP* hp, int tick) {
    __shared__ double sm[256];
    const int c = blockIdx.x;
    if (tick > 0 && c == 0 && threadIdx.x == 0) tick_counters(hp, tick);
    int64_t beg, end;
    chunk_bounds(tab, c, beg, end);
    const double sum = chunk_sqsum(g, beg, end, sm);
    if (threadIdx.x == 0) tab.chunk_part[c] = sum;
}

int chunk_sqnorms_tick(const float* g, const ChunkTable& tab, DevHP* hp, int tick_mask, hipStream_t st) {
    hipLaunchKernelGGL(sqnorm_chunk_kernel, dim3(tab.nchunks), dim3(256), 0, st, g, tab, hp, tick_mask);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// clip + one step of the optimizer OPT (include/cdrl.h table) + optional polyak averaging.  Per element one streaming pass over p, g
// and the slots the optimizer uses (none for SGD; never the others).
// chunk_tensor (or null: plain chunks of [0, n), no clip): the chunk table; with a positive threshold every block folds the chunk
// partials of its tensor into the norm the tensor is clipped by.
// GATE (GATE_MODE_*): the gated forms.  Both return before touching anything when the gate block says skip; GATE_MODE_GLOBAL takes
// the list's scale s from the block in place of the per-tensor clip (cn = s, denom = 1: the loop's g * cn / denom is g * s).
template <int OPT, int GATE>
__global__ void __launch_bounds__(256) clip_update_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                          const int* __restrict__ chunk_tensor,
                                                          const int64_t* __restrict__ chunk_off,
                                                          const TensorSeg* __restrict__ segs, const DevHP* __restrict__ hp,
                                                          int which, const double* __restrict__ chunk_part, int ticked,
                                                          int blend, float pa, float pc, const GateBlock* __restrict__ gate) {
    if (GATE != GATE_MODE_OFF && gate->skip) return;
    int64_t beg, end;
    float cn = 0.0f, denom = 1.0f;
    const float clip_norm = hp_clip_norm(hp, which);
    if (chunk_tensor) {
        const int c = blockIdx.x;
        const TensorSeg s = segs[chunk_tensor[c]];
        beg = chunk_off[c];
        end = beg + CHUNK;
        if (end > s.off + s.n) end = s.off + s.n;
        if (GATE != GATE_MODE_GLOBAL && clip_norm > 0.0f) {
            const float l2 = (float)fold_chunk_parts(chunk_part, s);
            const float norm = l2 > 0.0f ? sqrtf(l2) : l2;
            cn = clip_norm;
            denom = fmaxf(norm, clip_norm);
        }
    } else {
        beg = (int64_t)blockIdx.x * CHUNK;
        end = beg + CHUNK;
        if (end > n) end = n;
    }
    if (GATE == GATE_MODE_GLOBAL) cn = which == WHICH_TRUNK ? gate->scale_trunk : gate->scale_head;
    const float lr = hp_lr(hp, which);
    const int t1 = hp_t(hp, which) + (ticked ? 0 : 1);
    const float b1 = hp->beta1, b2 = hp->beta2, eps = hp->eps;
    // per-step scalars, float32 (Keras _prepare_local / the training ops' scalar operands)
    float k0 = 0.0f, k1 = 0.0f, k2 = 0.0f, k3 = 0.0f, k4 = 0.0f;
    if (OPT == CDRL_OPT_ADAM) {
        k0 = lr * sqrtf(1.0f - powf(b2, (float)t1)) / (1.0f - powf(b1, (float)t1));
    } else if (OPT == CDRL_OPT_RMSPROP) {
        k0 = 0.9f;
        k1 = 1.0f - k0;
    } else if (OPT == CDRL_OPT_ADADELTA) {
        k0 = 0.95f;
        k1 = 1.0f - k0;
    } else if (OPT == CDRL_OPT_ADAMAX) {
        k0 = lr / (1.0f - powf(b1, (float)t1));
    } else if (OPT == CDRL_OPT_NADAM) {
        const float mc = hp_m_cache(hp, which);
        const float mu = nadam_mu(b1, t1), mu1 = nadam_mu(b1, t1 + 1);
        const float st = ticked ? mc : mc * mu;      // S_t (ticked: the tick stored it already)
        k0 = 1.0f - mu;                              // one_minus_m_t
        k1 = 1.0f - st;                              // one_minus_m_schedule_new
        k2 = 1.0f - st * mu1;                        // one_minus_m_schedule_next
        k3 = mu1;                                    // m_t_1
        k4 = 1.0f - powf(b2, (float)t1);             // v_t_prime_denominator
    }
    for (int64_t i = beg + threadIdx.x; i < end; i += 256) {
        float gi = g[i];
        if (cn > 0.0f) gi = (gi * cn) / denom;
        const float po = p[i];
        float pn;
        if (OPT == CDRL_OPT_ADAM) {
            float mi = m[i], vi = v[i];
            mi += (gi - mi) * (1.0f - b1);
            vi += (gi * gi - vi) * (1.0f - b2);
            m[i] = mi;
            v[i] = vi;
            pn = po - (mi * k0) / (sqrtf(vi) + eps);
        } else if (OPT == CDRL_OPT_SGD) {
            pn = po - gi * lr;
        } else if (OPT == CDRL_OPT_RMSPROP) {
            const float r = k0 * v[i] + k1 * (gi * gi);
            v[i] = r;
            pn = po - lr * gi / (sqrtf(r) + eps);
        } else if (OPT == CDRL_OPT_ADAGRAD) {
            const float a = v[i] + gi * gi;
            v[i] = a;
            pn = po - gi * lr / (sqrtf(a) + eps);
        } else if (OPT == CDRL_OPT_ADADELTA) {
            const float a = v[i] * k0 + (gi * gi) * k1;           // accum_grad
            const float d = m[i];                                 // accum_var
            const float u = sqrtf(d + eps) * (1.0f / sqrtf(a + eps)) * gi;
            v[i] = a;
            m[i] = d * k0 + (u * u) * k1;
            pn = po - u * lr;
        } else if (OPT == CDRL_OPT_ADAMAX) {
            float mi = m[i];
            mi += (gi - mi) * (1.0f - b1);
            const float vi = fmaxf(b2 * v[i], fabsf(gi));
            m[i] = mi;
            v[i] = vi;
            pn = po - k0 * (mi / (vi + eps));
        } else if (OPT == CDRL_OPT_NADAM) {
            const float gp = gi / k1;
            const float mi = b1 * m[i] + (1.0f - b1) * gi;
            const float vi = b2 * v[i] + (1.0f - b2) * (gi * gi);
            m[i] = mi;
            v[i] = vi;
            const float mbar = k0 * gp + k3 * (mi / k2);
            pn = po - lr * mbar / (sqrtf(vi / k4) + eps);
        } else {      // CDRL_OPT_FTRL
            const float nn = v[i], n1 = nn + gi * gi;
            const float z = m[i] + (gi - (sqrtf(n1) - sqrtf(nn)) / lr * po);
            m[i] = z;
            v[i] = n1;
            pn = fabsf(z) > 0.0f ? -z / (sqrtf(n1) / lr) : 0.0f;
        }
        if (blend) pn = pa * pn + pc * po;      // polyak: two float32 products, one float32 sum (numpy's order)
        p[i] = pn;
    }
}

int clip_update(int opt, float polyak, const ArenaSlice& a, const ChunkTable& tab, DevHP* hp, int which, hipStream_t st, int ticked,
                const GateBlock* gate, int gate_mode) {
    const int blend = polyak < 1.0f;
    if (gate_mode != GATE_MODE_OFF && !gate) {
        set_error("clip_update: gated form without a gate block");
        return -1;
    }
    const float pa = polyak, pc = (float)(1.0 - (double)polyak);
    const int grid = tab.chunk_tensor ? tab.nchunks : (int)cdiv64(a.n, CHUNK);
#define CDRL_CLIP_UPDATE_G(O, G)                                                                                                 \
    hipLaunchKernelGGL((clip_update_kernel<O, G>), dim3(grid), dim3(256), 0, st, a.p, a.g, a.m, a.v, a.n, tab.chunk_tensor,       \
                       tab.chunk_off, tab.segs, hp, which, tab.chunk_part, ticked, blend, pa, pc, gate)
#define CDRL_CLIP_UPDATE(O)                                                                                                      \
    do {                                                                                                                         \
        if (gate_mode == GATE_MODE_OFF) CDRL_CLIP_UPDATE_G(O, GATE_MODE_OFF);                                                    \
        else if (gate_mode == GATE_MODE_TENSOR) CDRL_CLIP_UPDATE_G(O, GATE_MODE_TENSOR);                                         \
        else CDRL_CLIP_UPDATE_G(O, GATE_MODE_GLOBAL);                                                                            \
    } while (0)
    switch (opt) {
        case CDRL_OPT_ADAM: CDRL_CLIP_UPDATE(CDRL_OPT_ADAM); break;
        case CDRL_OPT_SGD: CDRL_CLIP_UPDATE(CDRL_OPT_SGD); break;
        case CDRL_OPT_RMSPROP: CDRL_CLIP_UPDATE(CDRL_OPT_RMSPROP); break;
        case CDRL_OPT_ADAGRAD: CDRL_CLIP_UPDATE(CDRL_OPT_ADAGRAD); break;
        case CDRL_OPT_ADADELTA: CDRL_CLIP_UPDATE(CDRL_OPT_ADADELTA); break;
        case CDRL_OPT_ADAMAX: CDRL_CLIP_UPDATE(CDRL_OPT_ADAMAX); break;
        case CDRL_OPT_NADAM: CDRL_CLIP_UPDATE(CDRL_OPT_NADAM); break;
        case CDRL_OPT_FTRL: CDRL_CLIP_UPDATE(CDRL_OPT_FTRL); break;
        default: set_error("clip_update: unknown optimizer %d", opt); return -1;
    }
#undef CDRL_CLIP_UPDATE
#undef CDRL_CLIP_UPDATE_G
    CDRL_LAUNCH_CHECK();
    return 0;
}

__global__ void reset_steps_kernel(DevHP* hp) {
    hp->t_policy = 0;
    hp->t_value = 0;
    hp->t_dynamics = 0;
    hp->m_cache_policy = 1.0f;
    hp->m_cache_value = 1.0f;
    hp->m_cache_dynamics = 1.0f;
}

int reset_steps(DevHP* hp, hipStream_t st) {
    hipLaunchKernelGGL(reset_steps_kernel, dim3(1), dim3(1), 0, st, hp);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// the six values travel by value (the caller's struct may be gone when the kernel runs); nothing in front of t_policy is written
__global__ void set_steps_kernel(DevHP* hp, int t_policy, int t_value, int t_dynamics, float mc_policy, float mc_value,
                                 float mc_dynamics) {
    hp->t_policy = t_policy;
    hp->t_value = t_value;
    hp->t_dynamics = t_dynamics;
    hp->m_cache_policy = mc_policy;
    hp->m_cache_value = mc_value;
    hp->m_cache_dynamics = mc_dynamics;
}

int set_steps(DevHP* hp, const int t[3], const float m_cache[3], hipStream_t st) {
    hipLaunchKernelGGL(set_steps_kernel, dim3(1), dim3(1), 0, st, hp, t[0], t[1], t[2], m_cache[0], m_cache[1], m_cache[2]);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// two device-to-device copies as ONE launch of the library's own (old_policy <- policy: trainable and state slices): hipMemcpyAsync ran
// two blit kernels of the runtime with their own fences in the middle of the apply.  gate (or null): the gated apply's form, which
// copies nothing when the gate block says skip.
__global__ void __launch_bounds__(256) copy_two_kernel(float* __restrict__ d0, const float* __restrict__ s0, int64_t n0,
                                                       float* __restrict__ d1, const float* __restrict__ s1, int64_t n1,
                                                       const GateBlock* __restrict__ gate) {
    if (gate && gate->skip) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n0) d0[i] = s0[i];
    else if (i < n0 + n1) d1[i - n0] = s1[i - n0];
}

int copy_two(float* d0, const float* s0, int64_t n0, float* d1, const float* s1, int64_t n1, hipStream_t st, const GateBlock* gate) {
    if (n0 + n1 <= 0) return 0;
    hipLaunchKernelGGL(copy_two_kernel, dim3((unsigned)cdiv64(n0 + n1, 256)), dim3(256), 0, st, d0, s0, n0, d1, s1, n1, gate);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// ---- gradient gate (cdrl_config.clip_mode / skip_nonfinite; include/cdrl.h) ----------------------------------------------------
// Whether the apply of `head` needs the squared norm of list 0 (the head's) or 1 (the trunk's): the guard needs every list the
// step consumes, global mode the lists with a positive threshold.  One function for the chunk kernel and the gate.
__device__ __forceinline__ bool gate_needs(const DevHP* hp, const GateBlock* gate, int head, int list, int flags) {
    if (list == 1 && !(flags & GATE_TRUNK)) return false;
    if (flags & GATE_GUARD) return true;
    if (!(flags & GATE_GLOBAL)) return false;
    return (list == 1 ? gate->clip_norm_dynamics : hp_clip_norm(hp, head)) > 0.0f;
}

// blocks [0, tab_h.nchunks): the head's chunk table, the blocks behind them: the trunk's.  sqnorm_chunk_kernel's partials, no tick.
__global__ void __launch_bounds__(256) gate_chunk_kernel(const float* __restrict__ g_head, ChunkTable tab_h,
                                                         const float* __restrict__ g_trunk, ChunkTable tab_t,
                                                         const DevHP* __restrict__ hp, const GateBlock* __restrict__ gate, int head,
                                                         int flags) {
    __shared__ double sm[256];
    const int list = (int)blockIdx.x < tab_h.nchunks ? 0 : 1;
    if (!gate_needs(hp, gate, head, list, flags) && !(list == 0 && (flags & GATE_HEAD_PARTS))) return;      // (uniform per block)
    const int c = list == 0 ? (int)blockIdx.x : (int)blockIdx.x - tab_h.nchunks;
    const ChunkTable& tab = list == 0 ? tab_h : tab_t;
    int64_t beg, end;
    chunk_bounds(tab, c, beg, end);
    const double sum = chunk_sqsum(list == 0 ? g_head : g_trunk, beg, end, sm);
    if (threadIdx.x == 0) tab.chunk_part[c] = sum;
}

int gate_chunk_sqnorms(const float* g_head, const ChunkTable& tab_h, const float* g_trunk, const ChunkTable& tab_t, const DevHP* hp,
                       const GateBlock* gate, int head, int flags, hipStream_t st) {
    const int nchunks_t = (flags & GATE_TRUNK) ? tab_t.nchunks : 0;
    if (tab_h.nchunks + nchunks_t <= 0) return 0;
    hipLaunchKernelGGL(gate_chunk_kernel, dim3(tab_h.nchunks + nchunks_t), dim3(256), 0, st, g_head, tab_h, g_trunk, tab_t, hp, gate,
                       head, flags);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// sum of n chunk partials by one 256-thread workgroup: thread i adds the partials i, i + 256, ... in order, then a fixed LDS tree;
// every thread returns the same bits
__device__ __forceinline__ double gate_fold(const double* __restrict__ part, int n, double* sm) {
    double acc = 0.0;
    for (int c = threadIdx.x; c < n; c += 256) acc += part[c];
    __syncthreads();        // (sm may still be read from the fold in front)
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) sm[threadIdx.x] += sm[threadIdx.x + k];
        __syncthreads();
    }
    return sm[0];
}

// NaN and +-Inf elements are ordinary data: their squares make the double sum NaN or +Inf, which is all the guard asks about.  A
// finite float32 squared is below 1.2e77, so no finite list overflows the sum.
__device__ __forceinline__ bool gate_finite(double s) { return s <= 1.7976931348623157e308; }      // (false for NaN)

__global__ void __launch_bounds__(256) gate_kernel(const double* __restrict__ part_h, int nchunks_h,
                                                   const double* __restrict__ part_t, int nchunks_t, DevHP* hp, GateBlock* gate,
                                                   int head, int flags, TrustBlock* trust) {
    __shared__ double sm[256];
    const bool need_h = gate_needs(hp, gate, head, 0, flags), need_t = gate_needs(hp, gate, head, 1, flags);
    const double S_h = need_h ? gate_fold(part_h, nchunks_h, sm) : 0.0;
    const double S_t = need_t ? gate_fold(part_t, nchunks_t, sm) : 0.0;
    if (threadIdx.x != 0) return;
    int skip = (flags & GATE_GUARD) && !(gate_finite(S_h) && gate_finite(S_t)) ? 1 : 0;
    // trust-region latch: the pass in front of this apply measured a KL (armed) and the run has left the region
    if (trust && trust->armed && trust->stop) {
        skip = 1;
        trust->skipped += 1;
    }
    const double n_h = sqrt(S_h), n_t = sqrt(S_t);
    float s_h = 1.0f, s_t = 1.0f;
    if (flags & GATE_GLOBAL) {      // s = (float)(c / max(sqrt(S), c)) in double, rounded once; at or below the threshold exactly 1
        const double c_h = (double)hp_clip_norm(hp, head), c_t = (double)gate->clip_norm_dynamics;
        if (need_h && c_h > 0.0) s_h = (float)(c_h / fmax(n_h, c_h));
        if (need_t && c_t > 0.0) s_t = (float)(c_t / fmax(n_t, c_t));
    }
    gate->scale_head = s_h;
    gate->scale_trunk = s_t;
    gate->skip = skip;
    gate->last_norm[head][0] = (float)n_h;
    gate->last_norm[head][1] = (float)n_t;
    gate->last_scale[head][0] = s_h;
    gate->last_scale[head][1] = s_t;
    if (skip) {
        gate->skipped[head] += 1;
        return;
    }
    gate->applied[head] += 1;
    // the ticks of sqnorm_chunk_kernel, in front of BOTH updates of the step (they run TICKED)
    tick_counters(hp, (head == 0 ? TICK_POLICY : TICK_VALUE) | ((flags & GATE_TRUNK) ? TICK_TRUNK : 0) |
                          ((flags & GATE_NADAM) ? TICK_NADAM : 0));
}

int gate_decide(const ChunkTable& tab_h, const ChunkTable& tab_t, DevHP* hp, GateBlock* gate, int head, int flags, hipStream_t st,
                TrustBlock* trust) {
    if (head != 0 && head != 1) {
        set_error("gate_decide: head %d", head);
        return -1;
    }
    hipLaunchKernelGGL(gate_kernel, dim3(1), dim3(256), 0, st, tab_h.chunk_part, tab_h.nchunks, tab_t.chunk_part,
                       (flags & GATE_TRUNK) ? tab_t.nchunks : 0, hp, gate, head, flags, trust);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
