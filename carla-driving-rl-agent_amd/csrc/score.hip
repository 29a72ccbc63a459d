// Scoring the acting policy on held-out expert rows, gfx950.
//
//  beta_score : the head outputs of one inference chunk (alpha, beta as float32; base, exp, speed, similarity) against the recorded
//               rows of a trace -- expert actions in the unit interval, optionally returns (base, exp) and speed / similarity -- added
//               to a block of double sums (score_block.h): per action log-likelihood, mode error, bias, squared error, predicted
//               variance, entropy and the histogram of the probability integral transform F = I_x(alpha, beta), the Beta CDF at the
//               expert action; for the value head the sums behind bias, RMSE and explained variance.
// The regularised incomplete beta function is the continued fraction of the Beta CDF taken with modified Lentz steps, directly for
// x < (a + 1) / (a + b + 2) and as 1 - I_{1-x}(b, a) beyond, with a FIXED cap on the steps: a launch ends whatever it is given.
// Same structure as beta_kl_kernel: one workgroup, row loop, double transcendentals, double LDS trees in a fixed order -- per action
// one tree over the group of that action, then one over the value and auxiliary sums.  Thread 0 adds the totals to the block, so a
// sweep over a trace is one launch per chunk into one block and the same rows in the same chunks give the same bits.
#include "loss_bodies.h"
#include "score_block.h"

namespace cdrl {

constexpr int SCORE_THREADS = 256;
constexpr int SCORE_PIT_CAP = 256;                      // continued-fraction steps at most (93 needed up to 5000)
constexpr int SCORE_NQ = SCORE_PER_ACTION + 2;          // a thread's sums of one action: its group, non-finite, unconverged

// h of I_x(a, b) = front * h / a by modified Lentz steps (two terms of the fraction per step); stops when a step's factor is within
// 1e-15 of one or at the cap.  Every operand finite or not, the loop runs SCORE_PIT_CAP times at most.
__device__ inline double betacf_d(double a, double b, double x, bool& converged) {
    const double tiny = 1e-300;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    converged = false;
    for (int m = 1; m <= SCORE_PIT_CAP; ++m) {
        const double dm = (double)m, m2 = 2.0 * dm;
        double aa = dm * (b - dm) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1e-15) {
            converged = true;
            break;
        }
    }
    return h;
}

// lnB = ln B(a, b), lx = log x, l1x = log1p(-x) as the caller has them for the log-density
__device__ inline double betainc_d(double a, double b, double x, double lnB, double lx, double l1x, bool& converged) {
    const double front = exp(a * lx + b * l1x - lnB);
    if (x < (a + 1.0) / (a + b + 2.0)) return front * betacf_d(a, b, x, converged) / a;
    return 1.0 - front * betacf_d(b, a, 1.0 - x, converged) / b;
}

__global__ void __launch_bounds__(SCORE_THREADS) beta_score_kernel(BetaScoreArgs p) {
    __shared__ double sm[SCORE_NQ * SCORE_THREADS];
    const int A = p.A, tid = threadIdx.x;
    double nonfinite = 0.0, unconverged = 0.0;          // (thread 0: totals over the actions)
    for (int a = 0; a < A; ++a) {
        double acc[SCORE_NQ];
#pragma unroll
        for (int q = 0; q < SCORE_NQ; ++q) acc[q] = 0.0;
        for (int b = tid; b < p.count; b += SCORE_THREADS) {
            const float* d = p.dist + (int64_t)b * 4 * A;
            const double al = (double)d[a], be = (double)d[A + a];
            double* pit = p.pit ? p.pit + (int64_t)b * A + a : nullptr;
            if (!isfinite(al) || !isfinite(be)) {
                acc[SCORE_PER_ACTION] += 1.0;
                if (pit) *pit = NAN;
                continue;
            }
            const float uf = p.u[(int64_t)b * A + a];
            const double x = (double)fminf(fmaxf(uf, F32_EPS), 1.0f - F32_EPS);      // _clip_actions, as beta_action
            const double lx = log(x), l1x = log1p(-x);
            const double ab = al + be;
            const double lnB = lgamma(al) + lgamma(be) - lgamma(ab);
            const double mean = al / ab, err = mean - x;
            acc[SCORE_A_COUNT] += 1.0;
            acc[SCORE_A_LOGP] += (al - 1.0) * lx + (be - 1.0) * l1x - lnB;
            acc[SCORE_A_MODE_ERR] += fabs((al - 1.0) / (ab - 2.0) - x);
            acc[SCORE_A_ERR] += err;
            acc[SCORE_A_ERR2] += err * err;
            acc[SCORE_A_VAR] += al * be / (ab * ab * (ab + 1.0));
            acc[SCORE_A_ENTROPY] += lnB - (al - 1.0) * digamma_d(al) - (be - 1.0) * digamma_d(be) + (ab - 2.0) * digamma_d(ab);
            bool converged;
            const double F = betainc_d(al, be, x, lnB, lx, l1x, converged);
            if (!converged) {
                acc[SCORE_PER_ACTION + 1] += 1.0;
                if (pit) *pit = NAN;
                continue;
            }
            if (pit) *pit = F;
            const int bin = min(SCORE_BINS - 1, (int)floor(F * (double)SCORE_BINS));
#pragma unroll
            for (int k = 0; k < SCORE_BINS; ++k) acc[SCORE_A_HIST + k] += (k == bin) ? 1.0 : 0.0;
            acc[SCORE_A_COVER50] += (F >= 0.25 && F <= 0.75) ? 1.0 : 0.0;
            acc[SCORE_A_COVER90] += (F >= 0.05 && F <= 0.95) ? 1.0 : 0.0;
        }
        block_reduce<SCORE_NQ>(acc, sm);
        if (tid == 0) {
            double* g = p.block + SCORE_HEAD + a * SCORE_PER_ACTION;
#pragma unroll
            for (int q = 0; q < SCORE_PER_ACTION; ++q) g[q] += acc[q];
            nonfinite += acc[SCORE_PER_ACTION];
            unconverged += acc[SCORE_PER_ACTION + 1];
        }
    }
    const bool with_returns = p.returns_be != nullptr, with_aux = p.speed != nullptr;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (with_returns || with_aux) {                     // (block-uniform)
        for (int b = tid; b < p.count; b += SCORE_THREADS) {
            const float* val = p.value + (int64_t)b * 4;
            if (with_returns) {
                const double V = (double)val[0] * pow(10.0, (double)val[1]);
                const double R = (double)p.returns_be[2 * (int64_t)b] * pow(10.0, (double)p.returns_be[2 * (int64_t)b + 1]);
                const double e = V - R;
                v[0] += e;
                v[1] += e * e;
                v[2] += R;
                v[3] += R * R;
            }
            if (with_aux) {
                const double ds = (double)val[2] - (double)p.speed[b], dm = (double)val[3] - (double)p.similarity[b];
                v[4] += ds * ds;
                v[5] += dm * dm;
            }
        }
        block_reduce<6>(v, sm);
    }
    if (tid != 0) return;
    double* h = p.block;
    h[SCORE_ROWS] += (double)p.count;
    h[SCORE_NONFINITE] += nonfinite;
    h[SCORE_UNCONVERGED] += unconverged;
    if (with_returns) {
        h[SCORE_ROWS_RETURNS] += (double)p.count;
        h[SCORE_V_ERR] += v[0];
        h[SCORE_V_ERR2] += v[1];
        h[SCORE_V_RET] += v[2];
        h[SCORE_V_RET2] += v[3];
    }
    if (with_aux) {
        h[SCORE_ROWS_AUX] += (double)p.count;
        h[SCORE_SPEED_ERR2] += v[4];
        h[SCORE_SIM_ERR2] += v[5];
    }
}

int beta_score(const BetaScoreArgs& a, hipStream_t st) {
    if (!a.dist || !a.value || !a.u || !a.block) {
        set_error("beta_score: a null dist / value / u / block");
        return -1;
    }
    if (a.rows < 1 || a.count < 1 || a.count > a.rows) {
        set_error("beta_score: rows = %d, count = %d: need 1 <= count <= rows", a.rows, a.count);
        return -1;
    }
    if (a.A < 1 || a.A > 8) {
        set_error("beta_score: num_actions %d outside 1..8 unsupported", a.A);
        return -1;
    }
    if ((a.speed == nullptr) != (a.similarity == nullptr)) {
        set_error("beta_score: speed and similarity go together: both or neither");
        return -1;
    }
    hipLaunchKernelGGL(beta_score_kernel, dim3(1), dim3(SCORE_THREADS), 0, st, a);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
