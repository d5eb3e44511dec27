// s360_metrics.hip — mean SSIM per image: the evaluation step's `compute_ssim` (the reference's
// src/evaluation/metrics.py:38-54), i.e. skimage.metrics.structural_similarity(gt, hat, win_size=11,
// gaussian_weights=True, channel_axis=0, data_range=1.0) per image, on the GPU.  gfx950 only.
//
// Algorithm (skimage's, restated; tests/ssim_reference.py is the numpy statement the tests compare against):
//   window   normalised Gaussian, sigma 1.5, truncate 3.5 -> radius 5, 11 taps, applied separably (scipy gaussian_filter)
//   moments  mx, my, <x^2>, <y^2>, <xy> filtered; vx = cn (<x^2> - mx^2), vy, vxy likewise, cn = 121 / 120
//   S        (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)), C1 = 0.01^2, C2 = 0.03^2
//   score    mean of S over the interior [5, H-5) x [5, W-5) per channel (float64), then the mean over channels.
// Every interior pixel's 11 x 11 window lies inside the image, so skimage's reflect padding never reaches the score: the
// kernel evaluates interior pixels only and has no boundary rule.  Values are not clipped.
//
// Precision: the moments are accumulated in float32 (skimage's type) about a shift per tile — the value of the tile's first
// halo pixel, subtracted from x (and y's from y) as the tile is staged.  Variance is shift-invariant, so the score is the same
// algorithm; the shift removes the cancellation of <x^2> - mx^2 on near-flat images (against C2 = 9e-4), which unshifted
// float32 leaves at a few 1e-7 of the float64 score.
//
// Determinism: each workgroup writes the double sum of S over its tile (block_sum: fixed lane / wave order) to its own
// workspace slot; k_ssim_reduce sums the slots of an image in a fixed order (block_tree_sum).  No atomics: the result is
// bit-identical from call to call and independent of the other images of the batch.
#include "s360_device.h"

namespace s360 {

constexpr int SS_R = 5, SS_TAPS = 2 * SS_R + 1;
constexpr int SS_TW = 64, SS_TH = 16;                        // interior pixels per workgroup: one wave per row of 64
constexpr int SS_HW = SS_TW + 2 * SS_R, SS_HH = SS_TH + 2 * SS_R;  // staged halo: 74 x 26
constexpr int SS_NQ = 5;                                     // x, y, x^2, y^2, xy

struct SsimWeights {
    float w[SS_TAPS];
};

// Horizontal 11-tap pass of the five quantities for all 26 halo rows, then the vertical pass and S for the 16 x 64 interior
// pixels of the tile; one double partial sum per workgroup.  LDS: 2 x 26 x 74 + 5 x 26 x 64 floats = 47.5 KB.
__global__ __launch_bounds__(S360_BLOCK) void k_ssim_tiles(const float* __restrict__ x, const float* __restrict__ y, int H, int W,
                                                           int tiles_x, int tiles_per_plane, SsimWeights wt, double* __restrict__ partials) {
    __shared__ float sx[SS_HH * SS_HW], sy[SS_HH * SS_HW];
    __shared__ float hq[SS_NQ][SS_HH * SS_TW];
    __shared__ double wsum[1][BLOCK_WAVES];

    const int tid = threadIdx.x;
    const int plane = blockIdx.x / tiles_per_plane, tile = blockIdx.x - plane * tiles_per_plane;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int hy0 = ty * SS_TH, hx0 = tx * SS_TW;            // halo origin; interior pixel (r, c) of the tile is (hy0+5+r, hx0+5+c)
    const size_t pofs = (size_t)plane * H * W;
    const float* xp = x + pofs;
    const float* yp = y + pofs;
    // hy0 <= H - 11 and hx0 <= W - 11 for every tile, so the shift pixel is inside the plane
    const float shx = xp[(size_t)hy0 * W + hx0], shy = yp[(size_t)hy0 * W + hx0];

    for (int i = tid; i < SS_HH * SS_HW; i += S360_BLOCK) {
        const int r = i / SS_HW, c = i - r * SS_HW;
        const int gy = hy0 + r, gx = hx0 + c;
        float vx = 0.f, vy = 0.f;                            // outside the plane: feeds only pixels outside the interior
        if (gy < H && gx < W) {
            const size_t o = (size_t)gy * W + gx;
            vx = xp[o] - shx;
            vy = yp[o] - shy;
        }
        sx[i] = vx;
        sy[i] = vy;
    }
    __syncthreads();

    for (int i = tid; i < SS_HH * SS_TW; i += S360_BLOCK) {
        const int r = i / SS_TW, c = i - r * SS_TW;
        const float* rx = sx + r * SS_HW + c;
        const float* ry = sy + r * SS_HW + c;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < SS_TAPS; ++k) {
            const float u = rx[k], v = ry[k], w = wt.w[k];
            a += w * u;
            b += w * v;
            aa += w * (u * u);
            bb += w * (v * v);
            ab += w * (u * v);
        }
        hq[0][i] = a;
        hq[1][i] = b;
        hq[2][i] = aa;
        hq[3][i] = bb;
        hq[4][i] = ab;
    }
    __syncthreads();

    const float cov_norm = 121.0f / 120.0f, C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    double acc[1] = {0.0};
    for (int i = tid; i < SS_TH * SS_TW; i += S360_BLOCK) {
        const int r = i / SS_TW, c = i - r * SS_TW;
        if (hy0 + SS_R + r >= H - SS_R || hx0 + SS_R + c >= W - SS_R) continue;
        float q[SS_NQ] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SS_TAPS; ++k) {
            const int o = (r + k) * SS_TW + c;
            const float w = wt.w[k];
#pragma unroll
            for (int j = 0; j < SS_NQ; ++j) q[j] += w * hq[j][o];
        }
        // q[0], q[1]: filtered shifted means; the true means are shx + q[0], shy + q[1]
        const float vx = cov_norm * (q[2] - q[0] * q[0]);
        const float vy = cov_norm * (q[3] - q[1] * q[1]);
        const float vxy = cov_norm * (q[4] - q[0] * q[1]);
        const float mx = shx + q[0], my = shy + q[1];
        const float d = (shx - shy) + (q[0] - q[1]);         // mx - my without the rounding of mx and my
        const float b1 = mx * mx + my * my + C1;
        const float a1 = b1 - d * d;                         // == 2 mx my + C1
        const float s = (a1 * (2.0f * vxy + C2)) / (b1 * (vx + vy + C2));
        acc[0] += (double)s;
    }
    block_sum<false>(acc, wsum);
    if (tid == 0) partials[blockIdx.x] = acc[0];
}

// One workgroup per image: per channel, thread t sums slots t, t + 256, ... in order, then a fixed tree; the channel mean
// (float64, as skimage's crop(S).mean(dtype=float64)) and the mean over channels.
__global__ __launch_bounds__(S360_BLOCK) void k_ssim_reduce(const double* __restrict__ partials, int channels, int tiles_per_plane,
                                                            double count, float* __restrict__ out) {
    __shared__ double red[1][S360_BLOCK];
    const int tid = threadIdx.x, img = blockIdx.x;
    double total = 0.0;
    for (int c = 0; c < channels; ++c) {
        const double* p = partials + ((size_t)img * channels + c) * tiles_per_plane;
        double t[1] = {0.0};
        for (int j = tid; j < tiles_per_plane; j += S360_BLOCK) t[0] += p[j];
        block_tree_sum(t, red);
        total += red[0][0] / count;
        __syncthreads();                                     // red[0][0] read by every thread before the next channel overwrites it
    }
    if (tid == 0) out[img] = (float)(total / channels);
}

static SsimWeights ssim_weights() {
    // scipy.ndimage._gaussian_kernel1d(sigma=1.5, order=0, radius=int(3.5 * 1.5 + 0.5) = 5), normalised in double
    SsimWeights w;
    double e[SS_TAPS], sum = 0.0;
    for (int k = 0; k < SS_TAPS; ++k) {
        const double t = k - SS_R;
        e[k] = exp(-0.5 / (1.5 * 1.5) * t * t);
        sum += e[k];
    }
    for (int k = 0; k < SS_TAPS; ++k) w.w[k] = (float)(e[k] / sum);
    return w;
}

}  // namespace s360

using namespace s360;

extern "C" int s360_ssim(const float* pred, const float* gt, int32_t n_images, int32_t channels, int32_t height, int32_t width,
                         float* ssim_out, void* workspace, size_t* workspace_bytes, void* stream) {
    if (!workspace_bytes || n_images < 1 || channels < 1 || height < SS_TAPS || width < SS_TAPS) return S360_E_BADARG;
    const int tiles_x = (width - 2 * SS_R + SS_TW - 1) / SS_TW, tiles_y = (height - 2 * SS_R + SS_TH - 1) / SS_TH;
    const long long tiles_per_plane = (long long)tiles_x * tiles_y;
    const long long blocks = (long long)n_images * channels * tiles_per_plane;
    if (!s360_grid_fits(blocks)) return S360_E_BADARG;
    const int ws = s360_workspace(workspace, workspace_bytes, (size_t)blocks * sizeof(double), 8, pred && gt && ssim_out);
    if (ws != S360_WS_READY) return ws;
    double* partials = (double*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ssim_tiles, dim3((unsigned)blocks), dim3(S360_BLOCK), 0, st, pred, gt, (int)height, (int)width, tiles_x,
                       (int)tiles_per_plane, ssim_weights(), partials);
    S360_CHECK_LAUNCH();
    const double count = (double)(height - 2 * SS_R) * (double)(width - 2 * SS_R);
    hipLaunchKernelGGL(k_ssim_reduce, dim3((unsigned)n_images), dim3(S360_BLOCK), 0, st, (const double*)partials, (int)channels,
                       (int)tiles_per_plane, count, ssim_out);
    return s360_launch_status();
}
