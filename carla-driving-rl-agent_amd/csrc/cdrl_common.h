// Common device/host helpers for libcdrl_hip.so (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "cdrl_host.h"

namespace cdrl {

// Channels-last 2-D view: element (row r, channel c) lives at p[r*ld + coff + c].
// A "row" is one pixel of one frame; frames are ordered f = t*B + b so that the rows of
// one BatchNorm statistics group (one time slice) are contiguous.
struct View {
    float* p;
    int ld;
    int coff;
};

__host__ __device__ inline View make_view(float* p, int ld, int coff = 0) {
    View v;
    v.p = p;
    v.ld = ld;
    v.coff = coff;
    return v;
}

enum Act : int { ACT_NONE = 0, ACT_RELU6 = 1, ACT_SWISH6 = 2, ACT_TANH = 3, ACT_SIGMOID = 4 };

// De-interleaving channel shuffle of the reference (core/architectures.py:109-118, F7):
// concat index i -> output channel (i & 1) * (C/2) + (i >> 1).
// ReLU6 pass-through test 0 < z < 6 as ONE vector compare.  min(z, 6 - z) > 0 is exactly that predicate (6 - z is exact near 6 and
// never rounds to 0 unless z == 6; NaN -> false like the two-sided form).  The two-sided form compiles to two v_cmp into scalar
// register pairs combined by s_and_b64 right in front of the v_cndmask that consumes it; see DESIGN.md ("What round 3 found"):
// with another kernel's waves on the same SIMD the top lanes of that mask were occasionally stale.
__device__ __forceinline__ bool relu6_open(float z) { return fminf(z, 6.0f - z) > 0.0f; }

// The dense activations (relu6 for the feature nets, swish6 for the control branches, tanh / sigmoid for the gates), stated once:
// act_fwd_kernel (bn.hip) and the split-K reduce of gemm_nn (gemm.hip) both call act_value, act_bwd_kernel calls act_grad.
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float act_value(float x, int act) {
    float o = x;
    if (act == ACT_RELU6) o = fminf(fmaxf(x, 0.0f), 6.0f);
    else if (act == ACT_SWISH6) o = fminf(x * sigmoidf_(x), 6.0f);      // rl/utils.py:420-421
    else if (act == ACT_TANH) o = tanhf(x);
    else if (act == ACT_SIGMOID) o = sigmoidf_(x);
    return o;
}

#define SWISH6_CLOSED 6.01465654f      // 0x1.80f022p+2

// d = dL/da -> dL/dz at pre-activation x
__device__ __forceinline__ float act_grad(float x, float d, int act) {
    if (act == ACT_RELU6) {
        if (!relu6_open(x)) d = 0.0f;
    } else if (act == ACT_SWISH6) {
        // SURVEY.md Appendix E.  The gate x sigmoid(x) < 6 is decided on x: the product is increasing for x > 0 and crosses 6 at
        // x* = 6.014656129..., and SWISH6_CLOSED is the smallest float32 above x*.  The rounded float32 product reaches 6.0f one float32
        // below x* already (x = 6.01465607), where the true product is still below 6: the gate was closed one input early.
        const float s = sigmoidf_(x);
        d = (x < SWISH6_CLOSED) ? d * (s * (1.0f + x * (1.0f - s))) : 0.0f;
    } else if (act == ACT_TANH) {
        const float t = tanhf(x);
        d *= (1.0f - t * t);
    } else if (act == ACT_SIGMOID) {
        const float s = sigmoidf_(x);
        d *= s * (1.0f - s);
    }
    return d;
}

__host__ __device__ inline int shuffle_dst(int i, int ctot) { return (i & 1) * (ctot >> 1) + (i >> 1); }

int diag_active();                          // number of active CDRL_DIAG_* switches (0 unless CDRL_DIAG=1)
int env_overrides(char* buf, int cap);      // "NAME=VALUE ..." of every CDRL_* variable in the environment; returns their count

#define CDRL_LAUNCH_CHECK() CDRL_HIP(hipGetLastError())

// Every kernel launch of the library: with the stop event the tail-event bookkeeping asks for (TailEvents, cdrl_host.h), or plain
template <typename... Args, typename... Act>
inline void launch_tracked(void (*kernel)(Args...), dim3 grid, dim3 block, uint32_t lds, hipStream_t st, Act&&... args) {
    if (hipEvent_t ev = tail_note_launch(st)) {
        hipExtLaunchKernelGGL(kernel, grid, block, lds, st, nullptr, ev, 0, static_cast<Args>(args)...);
        return;
    }
    kernel<<<grid, block, lds, st>>>(static_cast<Args>(args)...);
}

// "Set the dynamic-LDS attribute of this kernel once" guards: once PER DEVICE (a second engine on another device of the same process, or
// the optional second enqueue thread racing the first launch, must not launch without it -- ADVICE r4): one flag per device and guard
// site, set after the attribute call returned; the call is idempotent, so two threads doing it at once is harmless.
struct LdsAttrOnce {
    volatile unsigned char done[64] = {};
    bool need() const {
        int d = 0;
        (void)hipGetDevice(&d);
        return !done[d & 63];
    }
    void mark() {
        int d = 0;
        (void)hipGetDevice(&d);
        done[d & 63] = 1;
    }
};

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline int pow2ceil(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// Geometry of the "column-mapped" kernels: blockDim = (CX channel lanes, CY row lanes), 256 threads.
struct ColGeom {
    int cx, cy;     // block dims
    int rb;         // rows per block
    int nb;         // blocks per group
};

// blocks per BatchNorm group for the statistics / backward reductions (x G groups), and for the
// single-group filter-gradient reductions (depthwise / stem): enough workgroups to fill 256 CUs.
// (128 since round 5 -- 256 before: the step is indifferent to it alone, 14.33 vs 14.32 ms, 64 costs +0.48 ms; with 128 rows the finalize
//  folded into the consumer's prologue (CDRL_FIN_ON_LOAD) reads half as much per workgroup: 14.15 vs 14.31 ms same box)
constexpr int NB_STATS = 128;
constexpr int NB_FILTER = 1024;

inline ColGeom col_geom(int rows_per_group, int C, int max_blocks_per_group = NB_STATS) {
    ColGeom g;
    g.cx = pow2ceil(C);
    if (g.cx < 32) g.cx = 32;
    if (g.cx > 256) g.cx = 256;
    g.cy = 256 / g.cx;
    int rb = cdiv(rows_per_group, max_blocks_per_group);
    // many small workgroups: the streaming kernels need >= 1024 resident workgroups to cover HBM
    // latency (measured: 64 elements/thread minimum made the late stages 2-3x slower); the finalize
    // kernels cope with the larger partial counts by summing them with 64 lanes per channel
    int minrb = g.cy * 4;
    if (rb < minrb) rb = minrb;
    rb = cdiv(rb, g.cy) * g.cy;
    g.rb = rb;
    g.nb = cdiv(rows_per_group, rb);
    return g;
}

// Geometry of the VECTORISED column-mapped kernels (BatchNorm family, column sums): every thread
// owns `vec` consecutive channels (16-byte accesses when C % 4 == 0, 8-byte when C is even), the
// block is (cx = C/vec channel lanes) x (cy row lanes) -- not a power of two in general (C = 116:
// 29 x 8 = 232 threads).  A function of (rows, C) only, so producers and consumers of the partial
// sums agree on `nb` without talking to each other.
// TF 'SAME' geometry of a 3x3 window (asymmetric padding for stride 2 on even sizes)
__host__ __device__ inline int same_out(int n, int s) { return (n + s - 1) / s; }
__host__ __device__ inline int same_pad_before(int n, int s) {
    const int out = (n + s - 1) / s;
    int tot = (out - 1) * s + 3 - n;
    if (tot < 0) tot = 0;
    return tot / 2;
}

struct VColGeom {
    int vec, cx, cy, nloop;   // nloop: channel-lane passes when C/vec > 256
    int rb, nb;
};

inline VColGeom vcol_geom(int rows_per_group, int C, int max_blocks_per_group = NB_STATS) {
    VColGeom g;
    g.vec = (C % 4 == 0) ? 4 : ((C % 2 == 0) ? 2 : 1);
    const int lanes = C / g.vec;
    g.cx = lanes > 256 ? 256 : lanes;
    g.nloop = cdiv(lanes, g.cx);
    g.cy = 256 / g.cx;
    if (g.cy < 1) g.cy = 1;
    int rb = cdiv(rows_per_group, max_blocks_per_group);
    int minrb = g.cy * 2;
    if (rb < minrb) rb = minrb;
    rb = cdiv(rb, g.cy) * g.cy;
    g.rb = rb;
    g.nb = cdiv(rows_per_group, rb);
    return g;
}

}  // namespace cdrl

// every launch of the library goes through launch_tracked
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) ::cdrl::launch_tracked(kernel, dim3(grid), dim3(block), (uint32_t)(lds), stream, __VA_ARGS__)
