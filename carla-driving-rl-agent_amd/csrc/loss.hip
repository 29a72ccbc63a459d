// Fused loss kernels (forward + analytic backward w.r.t. the linear head outputs), gfx950.
//
//  policy_loss : CARLAgent.policy_objective (reference core/carla_agent.py:394-428) on top of
//                PolicyNetwork.call (core/networks.py:96-110): Beta(alpha,beta) log-prob of the
//                clipped sample, entropy, mean-over-actions ratio, spinning-up style clipping,
//                0.5*MSE aux speed / similarity heads.  The Beta sample u and (optionally) its
//                pathwise Jacobians are inputs (F8 / Appendix C-1).
//  value_loss  : CARLAgent.value_objective (core/carla_agent.py:469-486).
//  clone_loss  : behaviour cloning (no reference counterpart): weighted negative Beta log-likelihood of an expert
//                action, with the entropy and auxiliary terms of policy_loss.
// One workgroup, wavefront/LDS reductions in double: B is a few hundred rows, the kernels are
// latency-bound, so everything transcendental (lgamma / digamma / trigamma) runs in double.
#include "loss_bodies.h"      // the Beta action / row bodies, block_reduce (shared with trust.hip and demo.hip)

namespace cdrl {

__global__ void __launch_bounds__(256) policy_loss_kernel(PolicyLossArgs p) {
    __shared__ double sm[6 * 256];
    const DevHP* hp = reinterpret_cast<const DevHP*>(p.hp);
    const double clip = (double)hp->clip_ratio, cent = (double)hp->entropy_coef;
    const int B = p.B, A = p.A, L = 2 * A + 2;
    const double invB = 1.0 / (double)B, invA = 1.0 / (double)A;
    const double gs = (double)p.inv_world;
    double acc[6] = {0, 0, 0, 0, 0, 0};   // policy term, entropy, speed sq, sim sq, ratio, logp
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        ppo_row(p, b, clip, cent, invB, invB, invA, gs, acc[0], acc[1], acc[4], acc[5]);
        aux_heads_row(p.lin + (int64_t)b * L, p.dlin + (int64_t)b * L, A, (double)p.speed[b], (double)p.similarity[b], gs * invB, acc[2],
                      acc[3]);
    }
    block_reduce<6>(acc, sm);
    if (threadIdx.x == 0) {
        const double policy_loss = -acc[0] * invB;
        const double entropy = acc[1] * invB * invA;
        const double speed_loss = 0.5 * acc[2] * invB, sim_loss = 0.5 * acc[3] * invB;
        p.metrics[0] = (float)(policy_loss - cent * entropy + speed_loss + sim_loss);
        p.metrics[1] = (float)policy_loss;
        p.metrics[2] = (float)entropy;
        p.metrics[3] = (float)speed_loss;
        p.metrics[4] = (float)sim_loss;
        p.metrics[5] = (float)(acc[4] * invB);
        p.metrics[6] = (float)(acc[5] * invB * invA);
    }
}

int policy_loss(const PolicyLossArgs& a, hipStream_t st) {
    if (a.A > 8) {
        set_error("policy_loss: num_actions %d > 8 unsupported", a.A);
        return -1;
    }
    hipLaunchKernelGGL(policy_loss_kernel, dim3(1), dim3(256), 0, st, a);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// Behaviour cloning: weighted negative log-likelihood of the expert action under Beta(alpha, beta), the entropy
// bonus and the auxiliary heads of the policy objective.  Same structure as policy_loss_kernel: one workgroup, row loop, double
// transcendentals, one double block reduction, one float rounding per output.  No gradient flows through the clipped action.
__global__ void __launch_bounds__(256) clone_loss_kernel(CloneLossArgs p) {
    __shared__ double sm[7 * 256];
    const double cent = p.hp ? (double)reinterpret_cast<const DevHP*>(p.hp)->entropy_coef : (double)p.entropy_coef;
    const double aw = (double)p.aux_weight;
    const int B = p.B, A = p.A, L = 2 * A + 2;
    const double invB = 1.0 / (double)B, invA = 1.0 / (double)A;
    const double gs = (double)p.grad_scale;
    const bool targets = p.speed && p.similarity;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};   // weighted nll, entropy, speed sq, sim sq, weight, logp, mode error
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* lin = p.lin + (int64_t)b * L;
        float* dlin = p.dlin + (int64_t)b * L;
        const double w = p.weight ? (double)p.weight[b] : 1.0;
        clone_row(lin, dlin, p.u, p.aux, b, A, w, cent, invB, invB, invA, gs, acc[0], acc[1], acc[5], acc[6]);
        acc[4] += w;
        if (targets) {
            aux_heads_row(lin, dlin, A, (double)p.speed[b], (double)p.similarity[b], gs * aw * invB, acc[2], acc[3]);
        } else {
            dlin[2 * A] = 0.0f;
            dlin[2 * A + 1] = 0.0f;
        }
    }
    block_reduce<7>(acc, sm);
    if (threadIdx.x == 0) {
        const double clone = acc[0] * invB;
        const double entropy = acc[1] * invB * invA;
        const double speed_loss = 0.5 * acc[2] * invB, sim_loss = 0.5 * acc[3] * invB;
        p.metrics[0] = (float)(clone - cent * entropy + aw * (speed_loss + sim_loss));
        p.metrics[1] = (float)clone;
        p.metrics[2] = (float)entropy;
        p.metrics[3] = (float)speed_loss;
        p.metrics[4] = (float)sim_loss;
        p.metrics[5] = (float)(acc[4] * invB);
        p.metrics[6] = (float)(acc[5] * invB * invA);
        p.metrics[7] = (float)(acc[6] * invB * invA);
    }
}

int clone_loss(const CloneLossArgs& a, hipStream_t st) {
    if (a.A < 1 || a.A > 8) {
        set_error("clone_loss: num_actions %d outside 1..8 unsupported", a.A);
        return -1;
    }
    if (a.B < 1 || !a.lin || !a.u || !a.dlin || !a.metrics) {
        set_error("clone_loss: B = %d rows or a null lin / u / dlin / metrics", a.B);
        return -1;
    }
    if (!a.speed != !a.similarity) {
        set_error("clone_loss: speed and similarity targets come together (both, or both null)");
        return -1;
    }
    hipLaunchKernelGGL(clone_loss_kernel, dim3(1), dim3(256), 0, st, a);
    CDRL_LAUNCH_CHECK();
    return 0;
}

__global__ void __launch_bounds__(256) value_loss_kernel(ValueLossArgs p) {
    __shared__ double sm[4 * 256];
    const int B = p.B;
    const double invB = 1.0 / (double)B, es = (double)p.exp_scale, gs = (double)p.inv_world;
    double acc[4] = {0, 0, 0, 0};
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* lin = p.lin + (int64_t)b * 4;
        float* dlin = p.dlin + (int64_t)b * 4;
        const double base = tanh((double)lin[0]);
        const double se = sigmoid_d((double)lin[1]), ex = es * se;
        const double ss = sigmoid_d((double)lin[2]), spd = 2.0 * ss;
        const double sim = tanh((double)lin[3]);
        const double d0 = base - (double)p.returns[2 * b], d1 = ex - (double)p.returns[2 * b + 1];
        const double d2 = spd - (double)p.speed[b], d3 = sim - (double)p.similarity[b];
        acc[0] += d0 * d0;
        acc[1] += d1 * d1;
        acc[2] += d2 * d2;
        acc[3] += d3 * d3;
        // total = 0.25 * (0.25*mean d0^2 + mean d1^2 / es^2 + mean d2^2 + mean d3^2)
        dlin[0] = (float)(gs * 0.25 * 0.25 * 2.0 * d0 * invB * (1.0 - base * base));
        dlin[1] = (float)(gs * 0.25 * 2.0 * d1 * invB / (es * es) * es * se * (1.0 - se));
        dlin[2] = (float)(gs * 0.25 * 2.0 * d2 * invB * 2.0 * ss * (1.0 - ss));
        dlin[3] = (float)(gs * 0.25 * 2.0 * d3 * invB * (1.0 - sim * sim));
        if (p.values) {
            p.values[2 * b] = (float)base;
            p.values[2 * b + 1] = (float)ex;
        }
    }
    block_reduce<4>(acc, sm);
    if (threadIdx.x == 0) {
        const double value_loss = 0.25 * acc[0] * invB + acc[1] * invB / (es * es);
        const double speed_loss = acc[2] * invB, sim_loss = acc[3] * invB;
        p.metrics[0] = (float)(0.25 * (value_loss + speed_loss + sim_loss));
        p.metrics[1] = (float)value_loss;
        p.metrics[2] = (float)speed_loss;
        p.metrics[3] = (float)sim_loss;
    }
}

int value_loss(const ValueLossArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(value_loss_kernel, dim3(1), dim3(256), 0, st, a);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// inference-side head activations (reference core/networks.py:96-110, 267-275)
__global__ void policy_dist_kernel(const float* __restrict__ lin, float* __restrict__ out, int B, int A) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * A) return;
    const int b = i / A, a = i % A, L = 2 * A + 2;
    const double al = softplus_d((double)lin[(int64_t)b * L + a]) + 1.01;
    const double be = softplus_d((double)lin[(int64_t)b * L + A + a]) + 1.01;
    float* o = out + (int64_t)b * 4 * A;
    o[a] = (float)al;
    o[A + a] = (float)be;
    o[2 * A + a] = (float)(al / (al + be));
    o[3 * A + a] = (float)sqrt(al * be / ((al + be) * (al + be) * (al + be + 1.0)));
}

int policy_dist(const float* lin, float* out, int B, int A, hipStream_t st) {
    hipLaunchKernelGGL(policy_dist_kernel, dim3(cdiv(B * A, 256)), dim3(256), 0, st, lin, out, B, A);
    CDRL_LAUNCH_CHECK();
    return 0;
}

__global__ void value_act_kernel(const float* __restrict__ lin, float* __restrict__ out, int B, float exp_scale) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    out[4 * b + 0] = (float)tanh((double)lin[4 * b + 0]);
    out[4 * b + 1] = (float)((double)exp_scale * sigmoid_d((double)lin[4 * b + 1]));
    out[4 * b + 2] = (float)(2.0 * sigmoid_d((double)lin[4 * b + 2]));
    out[4 * b + 3] = (float)tanh((double)lin[4 * b + 3]);
}

int value_act(const float* lin, float* out, int B, float exp_scale, hipStream_t st) {
    hipLaunchKernelGGL(value_act_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, lin, out, B, exp_scale);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
