// V-trace targets for replayed (off-policy) trajectories (gfx950): the extension of gae.hip by truncated importance weights
// (Espeholt et al. 2018, IMPALA).  With every ratio clipped to 1 the two recurrences below are GAE(lambda) over the TD errors and the
// bootstrapped rewards-to-go of gae.hip, in float64 throughout (gae.hip rounds its deltas to float32, as the reference does).
//
// Per row i of a trajectory of n steps (entry n of rewards / values_be is the bootstrap entry):
//   V_i     = base * 10^exp                                      float32, the three ops of gae_trajectory
//   log pi  = sum_a (alpha-1) ln u + (beta-1) ln(1-u) - lnB      float64, u clipped as cdrl_beta_sample_logp clips it
//   ratio   = exp(log pi - sum_a log_prob_old),  rho = min(rho_bar, ratio),  c = min(c_bar, ratio)
//   td_i    = r_i + gamma * V_{i+1} - V_i
//   x_i     = rho_i td_i + gamma lambda c_i x_{i+1}              A_i  = td_i + gamma lambda x_{i+1}   (policy advantage)
//   y_i     = rho_i td_i + gamma c_i y_{i+1}                     vs_i = V_i + y_i                     (value target, lambda = 1)
// One workgroup per trajectory: everything but the two recurrences is a wavefront-parallel map; the recurrences are latency-bound
// chains, staged through LDS with their per-row coefficient and run side by side on two waves, as the GAE scans are.
#include "cdrl_kernels.h"
#include "gae_bodies.h"

namespace cdrl {

// x[j] = a[j] + (k * c[j]) * x[j + 1] over a[0 .. n) in place, from the top down, `acc` = x[n].  The eight LDS reads of the terms and
// of the coefficients, and the products k * c[j], are issued ahead of each group of eight dependent (multiply, add) steps.
__device__ __forceinline__ double vtrace_scan(double* a, const double* c, int n, double k, double acc) {
    int j = n - 1;
    for (; j >= 7; j -= 8) {
        double x[8], m[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            x[u] = a[j - u];
            m[u] = k * c[j - u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            acc = x[u] + m[u] * acc;
            x[u] = acc;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) a[j - u] = x[u];
    }
    for (; j >= 0; --j) {
        acc = a[j] + (k * c[j]) * acc;
        a[j] = acc;
    }
    return acc;
}

// One trajectory of n steps by one 256-thread workgroup: rewards [n + 1] / values_be [n + 1][2] incl. the bootstrap entry, alpha / beta /
// actions / log_prob_old [n][A], outputs [n], scratch 4 * n doubles (td -> A, x, y -> vs, c).  Every barrier is block-uniform: all loop
// bounds derive from n.
__device__ __forceinline__ void vtrace_trajectory(const float* __restrict__ rewards, const float* __restrict__ values_be,
                                                  const float* __restrict__ alpha, const float* __restrict__ beta,
                                                  const float* __restrict__ actions, const float* __restrict__ log_prob_old,
                                                  int n, int A, double gamma, double lambda, double rho_bar, double c_bar, float scale,
                                                  float* __restrict__ returns, float* __restrict__ returns_be,
                                                  float* __restrict__ adv_raw, float* __restrict__ adv, float* __restrict__ rho_out,
                                                  double* __restrict__ scratch) {
    const int tid = threadIdx.x;
    double* td = scratch;                   // [n] TD errors, then the advantages A
    double* x = scratch + n;                // [n] rho * td, then the lambda-scan
    double* y = scratch + 2 * (int64_t)n;   // [n] the lambda = 1 scan, then the value targets vs
    double* cc = scratch + 3 * (int64_t)n;  // [n] c
    const double gl = gamma * lambda;
    for (int i = tid; i < n; i += 256) {
        const float v0 = __fmul_rn(values_be[2 * i], (float)pow(10.0, (double)values_be[2 * i + 1]));
        const float v1 = __fmul_rn(values_be[2 * i + 2], (float)pow(10.0, (double)values_be[2 * i + 3]));
        const double d = (double)rewards[i] + gamma * (double)v1 - (double)v0;
        double lp = 0.0, lp_old = 0.0;
        for (int k = 0; k < A; ++k) {
            const int64_t e = (int64_t)i * A + k;
            const double a = (double)alpha[e], b = (double)beta[e];
            const float eps = 1.1920929e-07f;
            const double u = (double)fminf(fmaxf(actions[e], eps), 1.0f - eps);
            lp += (a - 1.0) * log(u) + (b - 1.0) * log1p(-u) - (lgamma(a) + lgamma(b) - lgamma(a + b));
            lp_old += (double)log_prob_old[e];
        }
        const double ratio = exp(lp - lp_old);              // may overflow to inf: the comparisons below clip it, no inf * 0 arises
        const double rho = ratio < rho_bar ? ratio : rho_bar;
        const double c = ratio < c_bar ? ratio : c_bar;
        rho_out[i] = (float)ratio;
        td[i] = d;
        x[i] = rho * d;
        cc[i] = c;
    }
    __syncthreads();
    {
        __shared__ double sx[VTRACE_CH], sy[VTRACE_CH], sc[VTRACE_CH];     // 48 KB of the 64 KB a workgroup may always take
        double accx = 0.0, accy = 0.0;              // carries (live in tid 0 / tid 64 only)
        for (int hi = n; hi > 0; hi -= VTRACE_CH) { // chunk = rows [lo, hi)
            const int lo = hi > VTRACE_CH ? hi - VTRACE_CH : 0;
            for (int j = tid; j < hi - lo; j += 256) {
                const double t = x[lo + j];
                sx[j] = t;
                sy[j] = t;
                sc[j] = cc[lo + j];
            }
            __syncthreads();
            if (tid == 0) accx = vtrace_scan(sx, sc, hi - lo, gl, accx);
            if (tid == 64) accy = vtrace_scan(sy, sc, hi - lo, gamma, accy);
            __syncthreads();
            for (int j = tid; j < hi - lo; j += 256) {
                x[lo + j] = sx[j];
                y[lo + j] = sy[j];
            }
            __syncthreads();
        }
    }
    // A_i = td_i + gamma lambda x_{i+1} (into td: only x is read across rows), vs_i = V_i + y_i (into y)
    for (int i = tid; i < n; i += 256) {
        const float v0 = __fmul_rn(values_be[2 * i], (float)pow(10.0, (double)values_be[2 * i + 1]));
        td[i] = td[i] + gl * (i + 1 < n ? x[i + 1] : 0.0);
        y[i] = (double)v0 + y[i];
    }
    __syncthreads();
    trajectory_tail(td, y, n, scale, returns, returns_be, adv_raw, adv);
}

// Workgroup s = segment s: rows [seg_off[s], seg_off[s + 1]) of the dense inputs and packed outputs, entries [seg_off[s] + s,
// seg_off[s + 1] + s] of rewards / values_be, 4 * n_s doubles of scratch from 4 * seg_off[s].  A malformed segment (empty, or outside
// [0, N]) leaves before the first barrier -- the whole block takes the same branch -- and writes nothing; with 0 <= seg_off[s] <
// seg_off[s + 1] <= N every access stays inside the N + S padded entries, the N rows and the 4 * N doubles of scratch.
__global__ void __launch_bounds__(256) vtrace_segments_kernel(const float* __restrict__ rewards, const float* __restrict__ values_be,
                                                              const float* __restrict__ alpha, const float* __restrict__ beta,
                                                              const float* __restrict__ actions, const float* __restrict__ log_prob_old,
                                                              const int32_t* __restrict__ seg_off, int S, int N, int A,
                                                              double gamma, double lambda, double rho_bar, double c_bar, float scale,
                                                              float* __restrict__ returns, float* __restrict__ returns_be,
                                                              float* __restrict__ adv_raw, float* __restrict__ adv,
                                                              float* __restrict__ rho, double* __restrict__ scratch) {
    const int s = blockIdx.x;
    if (s >= S) return;
    const int lo = seg_off[s], hi = seg_off[s + 1];
    if (lo < 0 || hi <= lo || hi > N) return;
    const int64_t in = (int64_t)lo + s;         // first padded input entry of the segment
    const int64_t row = (int64_t)lo * A;
    vtrace_trajectory(rewards + in, values_be + 2 * in, alpha + row, beta + row, actions + row, log_prob_old + row, hi - lo, A, gamma,
                      lambda, rho_bar, c_bar, scale, returns + lo, returns_be + 2 * (int64_t)lo, adv_raw + lo, adv + lo, rho + lo,
                      scratch + 4 * (int64_t)lo);
}

int vtrace_segments(const float* rewards, const float* values_be, const float* alpha, const float* beta, const float* actions,
                    const float* log_prob_old, const int32_t* seg_off, int S, int N, int A, double gamma, double lambda, double rho_bar,
                    double c_bar, float scale, float* returns, float* returns_be, float* adv_raw, float* adv, float* rho, double* scratch,
                    hipStream_t st) {
    hipLaunchKernelGGL(vtrace_segments_kernel, dim3(S), dim3(256), 0, st, rewards, values_be, alpha, beta, actions, log_prob_old, seg_off,
                       S, N, A, gamma, lambda, rho_bar, c_bar, scale, returns, returns_be, adv_raw, adv, rho, scratch);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
