// Trust-region guard of the policy steps, gfx950.
//
//  beta_kl : the analytic KL between the anchor policy (the acting network at the start of an update, alpha0 / beta0 as float32
//            inputs) and the policy of the pass in flight (alpha, beta from the head's linear outputs, as policy_loss_kernel forms
//            them), per row the sum over its actions (the KL of the joint distribution), averaged over the rows:
//                KL(Beta(a0,b0) || Beta(a,b)) = lnB(a,b) - lnB(a0,b0) + (a0-a) psi(a0) + (b0-b) psi(b0) + (a-a0+b-b0) psi(a0+b0)
//                dKL/da = psi(a) - psi(a+b) - psi(a0) + psi(a0+b0)     (b alike), times sigmoid(lin) through the softplus
//            Works for the stored-action and the re-sampled loss alike: it needs no action and no stored log-probability.
// Same structure as policy_loss_kernel: one workgroup, row loop, double transcendentals, one double block reduction, one float
// rounding per output.  Thread 0 keeps the statistics and the latch of the device TrustBlock; the gated policy_apply reads the latch
// (gate_decide), so no host read stands between a pass that left the trust region and the apply that has to be left out.
#include "loss_bodies.h"

namespace cdrl {

// sum of acc[0] and NaN-propagating maximum of acc[1] over the workgroup, one LDS tree for both
__device__ __forceinline__ void block_sum_max(double* acc, double* sm) {
    const int tid = threadIdx.x;
    sm[tid] = acc[0];
    sm[256 + tid] = acc[1];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            sm[tid] += sm[tid + s];
            const double x = sm[256 + tid], y = sm[256 + tid + s];
            sm[256 + tid] = (x > y || x != x) ? x : y;
        }
        __syncthreads();
    }
    acc[0] = sm[0];
    acc[1] = sm[256];
}

__global__ void __launch_bounds__(256) beta_kl_kernel(BetaKlArgs p) {
    __shared__ double sm[2 * 256];
    const int B = p.B, A = p.A, L = 2 * A + 2;
    const double invB = 1.0 / (double)B;
    const double coef = (double)(p.trust ? p.trust->kl_coef : p.kl_coef);
    const bool grad = coef > 0.0;               // (block-uniform; false for NaN: a broken coefficient writes no gradient)
    const double gs = (double)p.inv_world * coef * invB;
    double acc[2] = {0.0, -INFINITY};           // sum of the rows' KL, their maximum
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* lin = p.lin + (int64_t)b * L;
        const float* anc = p.anchor + (int64_t)b * 2 * A;
        double row = 0.0;
        for (int a = 0; a < A; ++a) {
            const double la = (double)lin[a], lb = (double)lin[A + a];
            const double al = softplus_d(la) + 1.01, be = softplus_d(lb) + 1.01;
            const double a0 = (double)anc[a], b0 = (double)anc[A + a];
            const double lnB = lgamma(al) + lgamma(be) - lgamma(al + be);
            const double lnB0 = lgamma(a0) + lgamma(b0) - lgamma(a0 + b0);
            const double pa0 = digamma_d(a0), pb0 = digamma_d(b0), pab0 = digamma_d(a0 + b0);
            row += lnB - lnB0 + (a0 - al) * pa0 + (b0 - be) * pb0 + (al - a0 + be - b0) * pab0;
            if (grad) {
                float* dlin = p.dlin + (int64_t)b * L;
                const double pab = digamma_d(al + be);
                const double dk_da = digamma_d(al) - pab - pa0 + pab0, dk_db = digamma_d(be) - pab - pb0 + pab0;
                dlin[a] = (float)((double)dlin[a] + gs * dk_da * sigmoid_d(la));
                dlin[A + a] = (float)((double)dlin[A + a] + gs * dk_db * sigmoid_d(lb));
            }
        }
        acc[0] += row;
        acc[1] = (row > acc[1] || row != row) ? row : acc[1];
    }
    block_sum_max(acc, sm);
    if (threadIdx.x != 0) return;
    const double mean = acc[0] * invB;
    const double kl = mean < 0.0 ? 0.0 : mean;          // rounding can put a true zero slightly negative; NaN stays NaN
    if (p.metrics) {
        p.metrics[0] = (float)kl;
        p.metrics[1] = (float)acc[1];
        p.metrics[2] = (float)(kl / (double)A);
    }
    TrustBlock* t = p.trust;
    if (!t) return;
    const float klf = (float)kl;
    t->kl_last = klf;
    t->kl_max = (klf > t->kl_max || klf != klf) ? klf : t->kl_max;
    t->kl_sum += kl;
    const int pass = t->passes;
    t->passes = pass + 1;
    t->armed = 1;
    // !(kl <= bound): a NaN KL (a broken anchor) stops the run instead of passing
    if (t->target_kl > 0.0f && !t->stop && !(kl <= (double)t->kl_stop_factor * (double)t->target_kl)) {
        t->stop = 1;
        t->stop_pass = pass;
    }
}

int beta_kl(const BetaKlArgs& a, hipStream_t st) {
    if (a.A < 1 || a.A > 8) {
        set_error("beta_kl: num_actions %d outside 1..8 unsupported", a.A);
        return -1;
    }
    if (a.B < 1 || !a.lin || !a.anchor) {
        set_error("beta_kl: B = %d rows or a null lin / anchor", a.B);
        return -1;
    }
    if (!a.dlin && (a.trust || a.kl_coef > 0.0f)) {
        set_error("beta_kl: a null dlin with a coefficient that may be positive");
        return -1;
    }
    if (!a.trust && !a.metrics) {
        set_error("beta_kl: neither a trust block nor metrics: nothing to write");
        return -1;
    }
    hipLaunchKernelGGL(beta_kl_kernel, dim3(1), dim3(256), 0, st, a);
    CDRL_LAUNCH_CHECK();
    return 0;
}

__global__ void trust_disarm_kernel(TrustBlock* t) { t->armed = 0; }

int trust_disarm(TrustBlock* trust, hipStream_t st) {
    hipLaunchKernelGGL(trust_disarm_kernel, dim3(1), dim3(1), 0, st, trust);
    CDRL_LAUNCH_CHECK();
    return 0;
}

__global__ void trust_set_params_kernel(TrustBlock* t, float target_kl, float kl_stop_factor, float kl_coef) {
    t->target_kl = target_kl;
    t->kl_stop_factor = kl_stop_factor;
    t->kl_coef = kl_coef;
}

int trust_set_params(TrustBlock* trust, float target_kl, float kl_stop_factor, float kl_coef, hipStream_t st) {
    hipLaunchKernelGGL(trust_set_params_kernel, dim3(1), dim3(1), 0, st, trust, target_kl, kl_stop_factor, kl_coef);
    CDRL_LAUNCH_CHECK();
    return 0;
}

// the host-written head stays
__global__ void trust_reset_kernel(TrustBlock* t) {
    t->kl_last = 0.0f;
    t->kl_max = 0.0f;
    t->passes = 0;
    t->stop = 0;
    t->stop_pass = -1;
    t->armed = 0;
    t->skipped = 0;
    t->kl_sum = 0.0;
}

int trust_reset(TrustBlock* trust, hipStream_t st) {
    hipLaunchKernelGGL(trust_reset_kernel, dim3(1), dim3(1), 0, st, trust);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
