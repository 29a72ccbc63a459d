// Contrastive views on the device (the view pipeline of SimCLR, rl/augmentations/simclr.py:pipeline of the reference): random crop
// resized back to H x W, horizontal flip, colour jitter, colour drop, separable Gaussian blur.  One plan per view, shared by the T
// frames of its stack; the plan holds scalars only (the host draws them), so nothing here needs a random stream.
//
// V views of N rows in four launches whatever V is and whatever the plans say (view v reads row v % N: no doubled copy of the rows):
//     1  crop -> bilinear resize -> flip              rows -> A       per pixel, a gather of four taps inside the crop window
//     2  per-(view, frame, channel) mean of A + brightness  -> mean   one workgroup per frame, fixed-order double sums (jitter only)
//     3  jitter -> colour drop -> horizontal blur     A -> B          one workgroup per image row, the row staged in LDS
//     4  vertical blur                                B -> out        per pixel
// A stage that does not fire for a view passes the view's data through inside its launch (every launch writes its whole output),
// so no launch depends on which buffer an earlier one chose.  The work is bandwidth-shaped: three writes and four reads of the views.
#include "aug_bodies.h"
#include "cdrl_kernels.h"
#include "resize_bodies.h"              // resize_src: the source taps of the crop resize

namespace cdrl {

constexpr int VIEW_ROW_TILE = 128;              // pixels of a row staged per pass of launch 3
constexpr int VIEW_MAX_RADIUS = VIEW_MAX_TAPS / 2;

__device__ __forceinline__ int view_taps_of(const ViewPlan& p) {
    return (p.blur_taps >= 3 && p.blur_taps <= VIEW_MAX_TAPS && (p.blur_taps & 1)) ? p.blur_taps : 0;
}

// launch 1, grid (blocks per view, views): crop window of row v % N -> bilinear resize to H x W -> flip, into A[v]
__global__ void views_resize_kernel(const float* __restrict__ rows, int N, float* __restrict__ A, int V, int T, int H, int W,
                                    const ViewPlan* __restrict__ plans) {
    const int64_t npix = (int64_t)T * H * W;
    for (int64_t v = blockIdx.y; v < V; v += gridDim.y) {
        const ViewPlan& p = plans[v];
        // the window is validated on the host; clamped here as well so that no plan can make the gather leave the row
        const int ch = min(max(p.crop_h, 1), H), cw = min(max(p.crop_w, 1), W), flip = p.flip;
        const int cy = min(max(p.crop_y, 0), H - ch), cx = min(max(p.crop_x, 0), W - cw);
        const float* x = rows + (v % N) * npix * 3;
        float* y = A + v * npix * 3;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
            int64_t q = i;
            const int xx = (int)(q % W);
            q /= W;
            const int yy = (int)(q % H);
            const int t = (int)(q / H);
            int x0, x1, y0, y1;
            float fx, fy;
            resize_src(flip ? W - 1 - xx : xx, cw, W, x0, x1, fx);
            resize_src(yy, ch, H, y0, y1, fy);
            const float* r0 = x + ((int64_t)t * H + cy + y0) * W * 3;
            const float* r1 = x + ((int64_t)t * H + cy + y1) * W * 3;
            const int a = (cx + x0) * 3, b = (cx + x1) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float top = r0[a + c] + (r0[b + c] - r0[a + c]) * fx;
                const float bot = r1[a + c] + (r1[b + c] - r1[a + c]) * fx;
                y[i * 3 + c] = top + (bot - top) * fy;
            }
        }
    }
}

// launch 2, grid (T, views): the contrast mean of every frame of a view that jitters
__global__ void __launch_bounds__(1024) views_mean_kernel(const float* __restrict__ A, float* __restrict__ mean, int V, int T, int P,
                                                          const ViewPlan* __restrict__ plans) {
    for (int64_t v = blockIdx.y; v < V; v += gridDim.y) {
        const ViewPlan& p = plans[v];
        if (!p.jitter) continue;
        channel_mean_body(A + (v * T + blockIdx.x) * (int64_t)P * 3, P, p.brightness, mean + (v * T + blockIdx.x) * 3);
        __syncthreads();            // the body's shared sums are free again before the next view's frame
    }
}

// launch 3, grid (image rows of a view, views): jitter and colour drop of a row tile (and its blur halo) into LDS, then the horizontal
// blur out of LDS with the index clamped to the row (replicate edge)
__global__ void __launch_bounds__(VIEW_ROW_TILE) views_colour_hblur_kernel(const float* __restrict__ A, const float* __restrict__ mean,
                                                                           float* __restrict__ B, int V, int T, int H, int W,
                                                                           const ViewPlan* __restrict__ plans) {
    __shared__ float tile[(VIEW_ROW_TILE + 2 * VIEW_MAX_RADIUS) * 3];
    const int nrows = T * H;
    for (int64_t v = blockIdx.y; v < V; v += gridDim.y) {
        const ViewPlan& p = plans[v];
        const int jitter = p.jitter, drop = p.drop, taps = view_taps_of(p), r = taps / 2;
        const float brightness = p.brightness, contrast = p.contrast, saturation = p.saturation, hue = p.hue;
        for (int row = blockIdx.x; row < nrows; row += gridDim.x) {
            const float* x = A + (v * nrows + row) * (int64_t)W * 3;
            float* y = B + (v * nrows + row) * (int64_t)W * 3;
            const float* m3 = mean + (v * T + row / H) * 3;
            for (int x0 = 0; x0 < W; x0 += VIEW_ROW_TILE) {
                const int lo = x0 - r > 0 ? x0 - r : 0;                                    // staged pixels: [lo, hi)
                const int hi = x0 + VIEW_ROW_TILE + r < W ? x0 + VIEW_ROW_TILE + r : W;
                for (int px = lo + (int)threadIdx.x; px < hi; px += blockDim.x) {
                    float c[3] = {x[px * 3], x[px * 3 + 1], x[px * 3 + 2]};
                    if (jitter) jitter_rgb(c, m3, brightness, contrast, saturation, hue);
                    if (drop) {
                        const float g = 0.2989f * c[0] + 0.5870f * c[1] + 0.1140f * c[2];
                        c[0] = c[1] = c[2] = g;
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) tile[(px - lo) * 3 + k] = c[k];
                }
                __syncthreads();
                const int px = x0 + (int)threadIdx.x;
                if (px < W) {
                    float acc[3] = {0.0f, 0.0f, 0.0f};
                    if (taps) {
                        for (int k = 0; k < taps; ++k) {
                            int s = px + k - r;
                            s = s < 0 ? 0 : (s > W - 1 ? W - 1 : s);
                            const float w = p.blur_w[k];
#pragma unroll
                            for (int c = 0; c < 3; ++c) acc[c] += w * tile[(s - lo) * 3 + c];
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[c] = tile[(px - lo) * 3 + c];
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) y[px * 3 + c] = acc[c];
                }
                __syncthreads();        // the tile is rewritten by the next pass
            }
        }
    }
}

// launch 4, grid (blocks per view, views): vertical blur, row index clamped to the frame (replicate edge); one float per thread
__global__ void views_vblur_kernel(const float* __restrict__ B, float* __restrict__ out, int V, int T, int H, int W,
                                   const ViewPlan* __restrict__ plans) {
    const int64_t n = (int64_t)T * H * W * 3;
    const int rowf = W * 3;
    for (int64_t v = blockIdx.y; v < V; v += gridDim.y) {
        const ViewPlan& p = plans[v];
        const int taps = view_taps_of(p), r = taps / 2;
        const float* x = B + v * n;
        float* y = out + v * n;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
            if (!taps) {
                y[i] = x[i];
                continue;
            }
            const int64_t line = i / rowf;                  // t * H + yy
            const int col = (int)(i - line * rowf);
            const int yy = (int)(line % H);
            const float* frame = x + (line - yy) * rowf;
            float acc = 0.0f;
            for (int k = 0; k < taps; ++k) {
                int s = yy + k - r;
                s = s < 0 ? 0 : (s > H - 1 ? H - 1 : s);
                acc += p.blur_w[k] * frame[(int64_t)s * rowf + col];
            }
            y[i] = acc;
        }
    }
}

int64_t views_workspace_floats(int V, int T, int H, int W) {
    if (V <= 0 || T <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)V * (2 * (int64_t)T * H * W * 3 + 3 * (int64_t)T);
}

static bool ranges_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * sizeof(float), b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * sizeof(float);
    return a0 < b1 && b0 < a1;
}

int views_batch(const float* rows, int N, float* out, int V, int T, int H, int W, const ViewPlan* plans_dev, float* workspace,
                hipStream_t st) {
    if (!rows || !out || !plans_dev || !workspace) {
        set_error("views_batch: null pointer");
        return -1;
    }
    if (V < 1 || N < 1 || N > V) {
        set_error("views_batch: V = %d views of N = %d rows: need V >= 1 and 1 <= N <= V", V, N);
        return -1;
    }
    // the per-frame index arithmetic and the resize numerators are 32-bit
    if (T < 1 || T > 65535 || H < 2 || W < 2 || H > (1 << 14) || W > (1 << 14)) {
        set_error("views_batch: bad shape %dx%dx%d (1..65535 frames of at least 2 x 2 and at most 16384 x 16384 pixels)", T, H, W);
        return -1;
    }
    const int P = H * W;
    const int64_t npix = (int64_t)T * P, n = npix * 3, ws = views_workspace_floats(V, T, H, W);
    if (ranges_overlap(workspace, ws, rows, (int64_t)N * n) || ranges_overlap(workspace, ws, out, (int64_t)V * n)) {
        set_error("views_batch: the workspace overlaps rows or out");
        return -1;
    }
    float* A = workspace;
    float* B = workspace + (int64_t)V * n;
    float* mean = workspace + 2 * (int64_t)V * n;
    const int gy = V < 65535 ? V : 65535;
    const int gpix = (int)((npix + 255) / 256 < 1024 ? (npix + 255) / 256 : 1024);
    const int gflt = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    const int grow = T * H < 65535 ? T * H : 65535;
    hipLaunchKernelGGL(views_resize_kernel, dim3(gpix, gy), dim3(256), 0, st, rows, N, A, V, T, H, W, plans_dev);
    hipLaunchKernelGGL(views_mean_kernel, dim3(T, gy), dim3(1024), 0, st, A, mean, V, T, P, plans_dev);
    hipLaunchKernelGGL(views_colour_hblur_kernel, dim3(grow, gy), dim3(VIEW_ROW_TILE), 0, st, A, mean, B, V, T, H, W, plans_dev);
    hipLaunchKernelGGL(views_vblur_kernel, dim3(gflt, gy), dim3(256), 0, st, B, out, V, T, H, W, plans_dev);
    CDRL_LAUNCH_CHECK();
    return 0;
}

}  // namespace cdrl
