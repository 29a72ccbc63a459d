// Mixed policy loss, gfx950: one minibatch of fresh rows and demonstration rows through one launch.
//
//  mixed_policy_loss : row b is a demonstration row iff demo_w[b] > 0, a PPO row otherwise.  PPO rows take the clipped surrogate of
//                      policy_loss_kernel (ppo_row, averaged over the NP PPO rows); demonstration rows the weighted negative Beta
//                      log-likelihood of clone_loss_kernel on demo_u (clone_row, averaged over the ND demonstration rows), and their
//                      adv / old_logp / u / du_da / du_db are never read.  Entropy bonus and the two auxiliary heads: all B rows.
// Same structure as its two neighbours in loss.hip: one workgroup, row loop, double transcendentals, double block reductions in a
// fixed order, one float rounding per output.  The row bodies are the ones those two kernels call (loss_bodies.h), so with
// demo_w == 0 everywhere the launch writes the bits of policy_loss_kernel.
#include "loss_bodies.h"

namespace cdrl {

__global__ void __launch_bounds__(256) mixed_policy_loss_kernel(MixedPolicyLossArgs m) {
    __shared__ double sm[9 * 256];
    const PolicyLossArgs& p = m.ppo;
    const DevHP* hp = reinterpret_cast<const DevHP*>(p.hp);
    const double clip = (double)hp->clip_ratio, cent = (double)hp->entropy_coef;
    const int B = p.B, A = p.A, L = 2 * A + 2;
    const double invB = 1.0 / (double)B, invA = 1.0 / (double)A;
    const double gs = (double)p.inv_world;
    // the row counts first: both normalisers are needed inside the row loop
    double cnt[1] = {0.0};
    for (int b = threadIdx.x; b < B; b += blockDim.x) cnt[0] += m.demo_w[b] > 0.0f ? 1.0 : 0.0;
    block_reduce<1>(cnt, sm);
    const double ND = cnt[0], NP = (double)B - ND;
    const double invND = ND > 0.0 ? 1.0 / ND : 0.0, invNP = NP > 0.0 ? 1.0 / NP : 0.0;
    // policy term, entropy, speed sq, sim sq, ratio, logp (PPO rows) | weighted nll, logp, mode error (demonstration rows)
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* lin = p.lin + (int64_t)b * L;
        float* dlin = p.dlin + (int64_t)b * L;
        const float wf = m.demo_w[b];
        if (wf > 0.0f)
            clone_row(lin, dlin, m.demo_u, p.aux, b, A, (double)wf, cent, invND, invB, invA, gs, acc[6], acc[1], acc[7], acc[8]);
        else
            ppo_row(p, b, clip, cent, invNP, invB, invA, gs, acc[0], acc[1], acc[4], acc[5]);
        aux_heads_row(lin, dlin, A, (double)p.speed[b], (double)p.similarity[b], gs * invB, acc[2], acc[3]);
    }
    block_reduce<9>(acc, sm);
    if (threadIdx.x != 0) return;
    const double policy_loss = -acc[0] * invNP;
    const double entropy = acc[1] * invB * invA;
    const double speed_loss = 0.5 * acc[2] * invB, sim_loss = 0.5 * acc[3] * invB;
    const double demo = acc[6] * invND;
    const float m7 = (float)demo, m8 = (float)(acc[7] * invND * invA), m9 = (float)(acc[8] * invND * invA), m10 = (float)ND;
    p.metrics[0] = (float)(policy_loss - cent * entropy + speed_loss + sim_loss + demo);
    p.metrics[1] = (float)policy_loss;
    p.metrics[2] = (float)entropy;
    p.metrics[3] = (float)speed_loss;
    p.metrics[4] = (float)sim_loss;
    p.metrics[5] = (float)(acc[4] * invNP);
    p.metrics[6] = (float)(acc[5] * invNP * invA);
    p.metrics[7] = m7;
    p.metrics[8] = m8;
    p.metrics[9] = m9;
    p.metrics[10] = m10;
    // launches of one stream run in order: one thread, plain read-modify-write
    if (DemoBlock* d = m.block) {
        d->loss_sum += (double)m7;
        d->logp_sum += (double)m8;
        d->mode_sum += (double)m9;
        d->rows_sum += (double)m10;
        d->passes += 1;
    }
}

int mixed_policy_loss(const MixedPolicyLossArgs& a, hipStream_t st) {
    const PolicyLossArgs& p = a.ppo;
    if (p.A < 1 || p.A > 8) {
        set_error("mixed_policy_loss: num_actions %d outside 1..8 unsupported", p.A);
        return -1;
    }
    if (p.B < 1 || !p.lin || !p.u || !a.demo_u || !a.demo_w || !p.dlin || !p.metrics) {
        set_error("mixed_policy_loss: B = %d rows or a null lin / u / demo_u / demo_w / dlin / metrics", p.B);
        return -1;
    }
    hipLaunchKernelGGL(mixed_policy_loss_kernel, dim3(1), dim3(256), 0, st, a);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
