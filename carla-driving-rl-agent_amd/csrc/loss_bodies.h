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

__device__ inline double trigamma_d(double x) {
    double r = 0.0;
    while (x < 10.0) {
        r += 1.0 / (x * x);
        x += 1.0;
    }
    const double f = 1.0 / (x * x);
    const double t = 1.0 / x + 0.5 * f +
                     (1.0 / x) * f * (1.0 / 6.0 + f * (-1.0 / 30.0 + f * (1.0 / 42.0 + f * (-1.0 / 30.0 + f * (5.0 / 66.0)))));
    return r + t;
}

__device__ __forceinline__ double softplus_d(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double sigmoid_d(double x) { return 1.0 / (1.0 + exp(-x)); }

#define F32_EPS 1.1920929e-07f

// One action of the Beta head: alpha = softplus(la) + 1.01 (beta likewise), the clipped action x, log Beta(x; alpha, beta), the
// entropy, their derivatives with respect to alpha / beta at fixed x, and the softplus chain.  dlx = d logp / d x where the
// unclipped action lies inside the clip band, 0 outside it (the pathwise term of a re-sampled action).
struct BetaAction {
    double al, be, x, lx, l1x, logp, ent;
    double dlp_da, dlp_db;      // d logp / d alpha, d beta (x fixed)
    double dlx;
    double dH_da, dH_db;
    double sg_a, sg_b;          // d alpha / d la, d beta / d lb
};

__device__ __forceinline__ BetaAction beta_action(double la, double lb, float uf) {
    BetaAction t;
    t.al = softplus_d(la) + 1.01;
    t.be = softplus_d(lb) + 1.01;
    const double al = t.al, be = t.be;
    const float xf = fminf(fmaxf(uf, F32_EPS), 1.0f - F32_EPS);      // _clip_actions
    const bool inside = (uf >= F32_EPS) && (uf <= 1.0f - F32_EPS);
    const double x = (double)xf;
    t.x = x;
    t.lx = log(x);
    t.l1x = log1p(-x);
    const double lnB = lgamma(al) + lgamma(be) - lgamma(al + be);
    const double pa = digamma_d(al), pb = digamma_d(be), pab = digamma_d(al + be);
    t.logp = (al - 1.0) * t.lx + (be - 1.0) * t.l1x - lnB;
    t.ent = lnB - (al - 1.0) * pa - (be - 1.0) * pb + (al + be - 2.0) * pab;
    t.dlx = inside ? ((al - 1.0) / x - (be - 1.0) / (1.0 - x)) : 0.0;
    t.dlp_da = t.lx - pa + pab;
    t.dlp_db = t.l1x - pb + pab;
    const double tab = trigamma_d(al + be);
    t.dH_da = -(al - 1.0) * trigamma_d(al) + (al + be - 2.0) * tab;
    t.dH_db = -(be - 1.0) * trigamma_d(be) + (al + be - 2.0) * tab;
    t.sg_a = sigmoid_d(la);
    t.sg_b = sigmoid_d(lb);
    return t;
}

__device__ __forceinline__ void beta_aux_store(float* aux, int b, int A, int a, const BetaAction& t) {
    if (!aux) return;
    float* ax = aux + (int64_t)b * 4 * A;
    ax[a] = (float)t.al;
    ax[A + a] = (float)t.be;
    ax[2 * A + a] = (float)t.logp;
    ax[3 * A + a] = (float)t.ent;
}

// The distribution columns of one PPO row (policy_objective): clipped surrogate on the mean-over-actions ratio, `pass` routing,
// pathwise Jacobians, entropy bonus.  inv_n: one over the number of rows the surrogate is averaged over; the entropy bonus is a
// mean over all B rows.  Adds the row's surrogate, entropy sum, ratio and logp sum to the four accumulators.
__device__ __forceinline__ void ppo_row(const PolicyLossArgs& p, int b, double clip, double cent, double inv_n, double invB, double invA,
                                        double gs, double& acc_term, double& acc_ent, double& acc_ratio, double& acc_logp) {
    const int A = p.A, L = 2 * A + 2;
    const float* lin = p.lin + (int64_t)b * L;
    float* dlin = p.dlin + (int64_t)b * L;
    double ea[8], dlp_da[8], dlp_db[8], dH_da[8], dH_db[8], sg_a[8], sg_b[8];
    double ratio = 0.0;
    for (int a = 0; a < A; ++a) {
        const BetaAction t = beta_action((double)lin[a], (double)lin[A + a], p.u[(int64_t)b * A + a]);
        const double e = exp(t.logp - (double)p.old_logp[(int64_t)b * A + a]);
        ea[a] = e;
        ratio += e;
        const double ja = p.du_da ? (double)p.du_da[(int64_t)b * A + a] : 0.0;
        const double jb = p.du_db ? (double)p.du_db[(int64_t)b * A + a] : 0.0;
        dlp_da[a] = t.dlp_da + t.dlx * ja;
        dlp_db[a] = t.dlp_db + t.dlx * jb;
        dH_da[a] = t.dH_da;
        dH_db[a] = t.dH_db;
        sg_a[a] = t.sg_a;
        sg_b[a] = t.sg_b;
        acc_ent += t.ent;
        acc_logp += t.logp;
        beta_aux_store(p.aux, b, A, a, t);
    }
    ratio *= invA;
    const double adv = (double)p.adv[b];
    const double minadv = adv > 0.0 ? (1.0 + clip) * adv : (1.0 - clip) * adv;
    const double s = ratio * adv;
    const bool pass = s <= minadv;                 // tf.minimum routes the gradient to x where x <= y
    acc_term += pass ? s : minadv;
    acc_ratio += ratio;
    for (int a = 0; a < A; ++a) {
        const double dL_dlogp = pass ? (-inv_n * adv * invA * ea[a]) : 0.0;
        const double dL_dH = -cent * invB * invA;
        dlin[a] = (float)(gs * (dL_dlogp * dlp_da[a] + dL_dH * dH_da[a]) * sg_a[a]);
        dlin[A + a] = (float)(gs * (dL_dlogp * dlp_db[a] + dL_dH * dH_db[a]) * sg_b[a]);
    }
}

// The distribution columns of one maximum-likelihood row (behaviour cloning, demonstrations): weight w on -mean_a logp of the
// clipped expert action, no gradient through the action, entropy bonus as above.  inv_n: one over the number of rows the
// likelihood term is averaged over.
__device__ __forceinline__ void clone_row(const float* lin, float* dlin, const float* u, float* aux, int b, int A, double w, double cent,
                                          double inv_n, double invB, double invA, double gs, double& acc_nll, double& acc_ent,
                                          double& acc_logp, double& acc_mode) {
    const double dL_dlogp = -inv_n * w * invA, dL_dH = -cent * invB * invA;
    double nll = 0.0;
    for (int a = 0; a < A; ++a) {
        const BetaAction t = beta_action((double)lin[a], (double)lin[A + a], u[(int64_t)b * A + a]);
        dlin[a] = (float)(gs * (dL_dlogp * t.dlp_da + dL_dH * t.dH_da) * t.sg_a);
        dlin[A + a] = (float)(gs * (dL_dlogp * t.dlp_db + dL_dH * t.dH_db) * t.sg_b);
        nll -= t.logp;
        acc_ent += t.ent;
        acc_logp += t.logp;
        acc_mode += fabs((t.al - 1.0) / (t.al + t.be - 2.0) - t.x);       // alpha, beta >= 1.01: the mode exists
        beta_aux_store(aux, b, A, a, t);
    }
    acc_nll += w * nll * invA;
}

// The two auxiliary columns of a row: 0.5 * (tanh(lin_sim) - similarity)^2 and 0.5 * (2 sigmoid(lin_speed) - speed)^2, their dlin
// scaled by `scale` (gradient scale x auxiliary weight / B); adds the squared errors to the two accumulators.
__device__ __forceinline__ void aux_heads_row(const float* lin, float* dlin, int A, double speed, double similarity, double scale,
                                              double& acc_speed, double& acc_sim) {
    const double sim = tanh((double)lin[2 * A]);
    const double sgs = sigmoid_d((double)lin[2 * A + 1]);
    const double spd = 2.0 * sgs;
    const double dsim = sim - similarity, dspd = spd - speed;
    acc_sim += dsim * dsim;
    acc_speed += dspd * dspd;
    dlin[2 * A] = (float)(scale * dsim * (1.0 - sim * sim));
    dlin[2 * A + 1] = (float)(scale * dspd * 2.0 * sgs * (1.0 - sgs));
}

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
