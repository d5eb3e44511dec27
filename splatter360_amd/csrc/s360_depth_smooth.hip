// s360_depth_smooth.hip — the training step's edge-aware depth-smoothness loss (the reference's LossDepth,
// src/loss/loss_depth.py:26-60), forward and backward.  gfx950 only.
//
//   n        = (max(min(d, lf), ln) - ln) / (lf - ln) per pixel, lf = log(far), ln = log(near) of the pixel's view (inputs: the
//              Python layer takes the logs with torch), min / max as torch's minimum / maximum (a NaN stays a NaN)
//   dx, dy   first differences of n along W and H; second derivative: the difference of two adjacent first differences
//   bilateral  e = exp(-c sigma), c = max over channels of the SIGNED image difference of the same two pixels (second
//              derivative: the larger of the two adjacent c), t = dx e
//   loss     = sum |tx| / Nx + sum |ty| / Ny, Nx and Ny the two numbers of terms
//   backward grad_d = g (Sx / Nx + Sy / Ny) gate / (lf - ln), S = sum over the terms that hold the pixel of coef sgn(t) e with
//              coef (+1, -1) or (+1, -2, +1), sgn(0) = sgn(NaN) = 0, gate = torch's halves at the ties of minimum / maximum
// Every operation is float64 on the float32 inputs (the library is compiled with -ffp-contract=off: no FMA); the loss and each
// gradient are rounded to float32 once.
//
// Forward: one workgroup per 32 x 64 tile of one [H, W] plane; the thread of pixel (y, x) forms the x-term that starts at x and
// the y-term that starts at y.  Sums: block_sum (lanes by a fixed shuffle tree, the four waves through LDS in wave order), one
// double pair per tile in its own workspace slot; k_ds_finish adds the slots in index order.  No atomics, no memset, no host read.
// Backward: a gather, one thread per pixel, lanes along W; a pixel recomputes the n and e of its own plus-shaped stencil from
// plain loads (its x-neighbours lie in the cache lines the wave's own row load fetched; the y-neighbours need loads anyway,
// and a lane exchange would leave the lanes at the wave's edges with a special case for no saved HBM traffic).
#include "s360_device.h"

namespace s360 {

constexpr int DS_TW = S360_WAVE, DS_TH = 32;                  // tile: 32 rows x 64 columns; a lane is a column
constexpr int DS_WAVES = S360_BLOCK / S360_WAVE, DS_ROWS = DS_TH / DS_WAVES;

struct DSArgs {
    const float* depth;
    const float* ln;                                          // [B, Vn]
    const float* lf;
    const float* image;                                       // [B, V, C, H, W] or null
    int V, vdiv, C, H, W;                                     // vdiv = V / Vn: view v of a batch element uses bound v / vdiv
    int tiles_x, tiles_per_plane;
    float sigma;
};

// torch's minimum / maximum: a NaN on either side gives NaN
__device__ __forceinline__ double ds_min(double a, double b) { return a <= b ? a : (a != a ? a : b); }
__device__ __forceinline__ double ds_max(double a, double b) { return a >= b ? a : (a != a ? a : b); }

__device__ __forceinline__ double ds_norm(float d, double ln, double lf, double span) {
    return (ds_max(ds_min((double)d, lf), ln) - ln) / span;
}

// max over channels of image[c][q + step] - image[c][q] (signed), ip -> channel 0 at q
__device__ __forceinline__ double ds_colour(const float* __restrict__ ip, size_t step, size_t cstride, int C) {
    double m = (double)ip[step] - (double)ip[0];
    for (int c = 1; c < C; ++c) m = ds_max((double)ip[c * cstride + step] - (double)ip[c * cstride], m);
    return m;
}

__device__ __forceinline__ double ds_sgn(double t) { return (double)((0.0 < t) - (t < 0.0)); }

// The term of one axis that STARTS at the pixel dp / ip point to (stride = 1 along W, W along H); the caller has checked that
// the term's 2 (3) pixels are inside.
template <bool SECOND, bool BILATERAL>
__device__ __forceinline__ double ds_term(const float* __restrict__ dp, const float* __restrict__ ip, size_t stride, size_t cstride, int C,
                                          double ln, double lf, double span, double sigma) {
    const double n0 = ds_norm(dp[0], ln, lf, span), n1 = ds_norm(dp[stride], ln, lf, span);
    double t = n1 - n0;
    if constexpr (SECOND) t = (ds_norm(dp[2 * stride], ln, lf, span) - n1) - t;
    if constexpr (BILATERAL) {
        double c = ds_colour(ip, stride, cstride, C);
        if constexpr (SECOND) c = ds_max(ds_colour(ip + stride, stride, cstride, C), c);
        t = t * exp(-c * sigma);
    }
    return t;
}

template <bool SECOND, bool BILATERAL>
__global__ __launch_bounds__(S360_BLOCK) void k_ds_forward(DSArgs a, double2* __restrict__ partials) {
    __shared__ double wsum[2][DS_WAVES];
    constexpr int ORD = SECOND ? 2 : 1;
    const int tid = threadIdx.x, lane = tid & (S360_WAVE - 1), wave = tid / S360_WAVE;
    const int plane = blockIdx.x / a.tiles_per_plane, tile = blockIdx.x - plane * a.tiles_per_plane;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x = tx * DS_TW + lane, y0 = ty * DS_TH;
    const int H = a.H, W = a.W;
    const int b = plane / a.V, v = plane - b * a.V, bound = b * (a.V / a.vdiv) + v / a.vdiv;
    const double ln = (double)a.ln[bound], lf = (double)a.lf[bound], span = lf - ln, sigma = (double)a.sigma;
    const size_t hw = (size_t)H * W;
    const float* dplane = a.depth + (size_t)plane * hw;
    const float* iplane = BILATERAL ? a.image + (size_t)plane * a.C * hw : nullptr;
    double sx = 0.0, sy = 0.0;
    if (x < W) {
#pragma unroll 2
        for (int j = 0; j < DS_ROWS; ++j) {
            const int y = y0 + wave + DS_WAVES * j;
            if (y >= H) break;
            const size_t o = (size_t)y * W + x;
            if (x + ORD < W) sx += fabs(ds_term<SECOND, BILATERAL>(dplane + o, iplane + o, 1, hw, a.C, ln, lf, span, sigma));
            if (y + ORD < H) sy += fabs(ds_term<SECOND, BILATERAL>(dplane + o, iplane + o, (size_t)W, hw, a.C, ln, lf, span, sigma));
        }
    }
    double s[2] = {sx, sy};
    block_sum<false>(s, wsum);
    if (tid == 0) partials[blockIdx.x] = make_double2(s[0], s[1]);
}

// One workgroup: the slots are staged through LDS 256 at a time and thread 0 adds them in index order.
__global__ __launch_bounds__(S360_BLOCK) void k_ds_finish(const double2* __restrict__ partials, long long slots, double nx, double ny,
                                                          float* __restrict__ loss) {
    __shared__ double2 s[S360_BLOCK];
    const int tid = threadIdx.x;
    double p = 0.0, q = 0.0;
    for (long long base = 0; base < slots; base += S360_BLOCK) {
        if (base + tid < slots) s[tid] = partials[base + tid];
        __syncthreads();
        if (tid == 0) {
            const int n = (int)(slots - base < S360_BLOCK ? slots - base : S360_BLOCK);
            for (int i = 0; i < n; ++i) {
                p += s[i].x;
                q += s[i].y;
            }
        }
        __syncthreads();
    }
    if (tid == 0) *loss = (float)(p / nx + q / ny);
}

// S = sum over the terms of one axis that hold the pixel of coef sgn(t) e.  dp / ip point to the pixel, pos is its index along
// the axis and len the axis' length.
template <bool SECOND, bool BILATERAL>
__device__ __forceinline__ double ds_axis_grad(const float* __restrict__ dp, const float* __restrict__ ip, int pos, int len, ptrdiff_t stride,
                                               size_t cstride, int C, double ln, double lf, double span, double sigma) {
    constexpr int R = SECOND ? 2 : 1;
    double n[2 * R + 1], cd[2 * R];
#pragma unroll
    for (int k = -R; k <= R; ++k) {
        const int q = pos + k;
        n[k + R] = (q >= 0 && q < len) ? ds_norm(dp[k * stride], ln, lf, span) : 0.0;
    }
    if constexpr (BILATERAL) {
#pragma unroll
        for (int k = -R; k < R; ++k) {
            const int q = pos + k;
            cd[k + R] = (q >= 0 && q + 1 < len) ? ds_colour(ip + k * stride, (size_t)stride, cstride, C) : 0.0;
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i <= R; ++i) {                            // the term that starts at pos - R + i
        const int j = pos - R + i;
        if (j < 0 || j + R >= len) continue;
        const double coef = SECOND ? (i == 1 ? -2.0 : 1.0) : (i == 0 ? 1.0 : -1.0);
        double t = n[i + 1] - n[i], e = 1.0;
        if constexpr (SECOND) t = (n[i + 2] - n[i + 1]) - t;
        if constexpr (BILATERAL) {
            double c = cd[i];
            if constexpr (SECOND) c = ds_max(cd[i + 1], c);
            e = exp(-c * sigma);
            t = t * e;
        }
        acc += coef * ds_sgn(t) * e;
    }
    return acc;
}

template <bool SECOND, bool BILATERAL>
__global__ __launch_bounds__(S360_BLOCK) void k_ds_backward(DSArgs a, double nx, double ny, const float* __restrict__ grad_loss,
                                                            float* __restrict__ grad_depth) {
    const int tid = threadIdx.x, lane = tid & (S360_WAVE - 1), wave = tid / S360_WAVE;
    const int plane = blockIdx.x / a.tiles_per_plane, tile = blockIdx.x - plane * a.tiles_per_plane;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x = tx * DS_TW + lane, y0 = ty * DS_TH;
    const int H = a.H, W = a.W;
    if (x >= W) return;
    const int b = plane / a.V, v = plane - b * a.V, bound = b * (a.V / a.vdiv) + v / a.vdiv;
    const double ln = (double)a.ln[bound], lf = (double)a.lf[bound], span = lf - ln, sigma = (double)a.sigma;
    const double g = (double)*grad_loss;
    const size_t hw = (size_t)H * W;
    const float* dplane = a.depth + (size_t)plane * hw;
    const float* iplane = BILATERAL ? a.image + (size_t)plane * a.C * hw : nullptr;
    float* gplane = grad_depth + (size_t)plane * hw;
#pragma unroll 2
    for (int j = 0; j < DS_ROWS; ++j) {
        const int y = y0 + wave + DS_WAVES * j;
        if (y >= H) break;
        const size_t o = (size_t)y * W + x;
        const double sx = ds_axis_grad<SECOND, BILATERAL>(dplane + o, iplane + o, x, W, 1, hw, a.C, ln, lf, span, sigma);
        const double sy = ds_axis_grad<SECOND, BILATERAL>(dplane + o, iplane + o, y, H, (ptrdiff_t)W, hw, a.C, ln, lf, span, sigma);
        const double d = (double)dplane[o], m = ds_min(d, lf);
        const double gate = (d > lf ? 0.0 : d == lf ? 0.5 : 1.0) * (m < ln ? 0.0 : m == ln ? 0.5 : 1.0);
        gplane[o] = (float)(g * (sx / nx + sy / ny) * gate / span);
    }
}

}  // namespace s360

using namespace s360;

namespace {

struct DSGrid {
    DSArgs args;
    long long blocks;
    double nx, ny;
};

// shared argument check of the forward and the backward; returns S360_OK and the grid, or an error
int ds_setup(const float* depth, const float* log_near, const float* log_far, const float* image, int32_t B, int32_t V, int32_t Vn,
             int32_t C, int32_t H, int32_t W, float sigma, int32_t flags, DSGrid* g) {
    const int ord = (flags & S360_DS_SECOND) ? 2 : 1;
    if (B < 1 || V < 1 || Vn < 1 || V % Vn != 0 || H <= ord || W <= ord || (flags & ~(S360_DS_SECOND | S360_DS_BILATERAL))) return S360_E_BADARG;
    if ((flags & S360_DS_BILATERAL) && C < 1) return S360_E_BADARG;
    const int tiles_x = (W + DS_TW - 1) / DS_TW;
    const long long tiles_per_plane = (long long)tiles_x * ((H + DS_TH - 1) / DS_TH);
    g->blocks = tiles_per_plane * B * V;
    if (!s360_grid_fits(g->blocks)) return S360_E_BADARG;
    const long long planes = (long long)B * V;                // the element counts, in 64-bit
    g->nx = (double)(planes * H * (long long)(W - ord));
    g->ny = (double)(planes * (long long)(H - ord) * W);
    g->args = DSArgs{depth, log_near, log_far, (flags & S360_DS_BILATERAL) ? image : nullptr, V, V / Vn, C, H, W, tiles_x, (int)tiles_per_plane, sigma};
    return S360_OK;
}

}  // namespace

extern "C" int s360_depth_smooth_forward(const float* depth, const float* log_near, const float* log_far, const float* image, int32_t batch,
                                         int32_t views, int32_t bound_views, int32_t channels, int32_t height, int32_t width,
                                         float sigma_image, int32_t flags, float* loss, void* workspace, size_t* workspace_bytes,
                                         void* stream) {
    if (!workspace_bytes) return S360_E_BADARG;
    DSGrid g;
    const int rc = ds_setup(depth, log_near, log_far, image, batch, views, bound_views, channels, height, width, sigma_image, flags, &g);
    if (rc != S360_OK) return rc;
    const size_t need = (size_t)g.blocks * sizeof(double2);
    const int ws = s360_workspace(workspace, workspace_bytes, need, 16,
                                  depth && log_near && log_far && loss && (!(flags & S360_DS_BILATERAL) || image));
    if (ws != S360_WS_READY) return ws;
    double2* partials = (double2*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.blocks), block(S360_BLOCK);
    switch (flags & (S360_DS_SECOND | S360_DS_BILATERAL)) {
        case 0: hipLaunchKernelGGL((k_ds_forward<false, false>), grid, block, 0, st, g.args, partials); break;
        case S360_DS_SECOND: hipLaunchKernelGGL((k_ds_forward<true, false>), grid, block, 0, st, g.args, partials); break;
        case S360_DS_BILATERAL: hipLaunchKernelGGL((k_ds_forward<false, true>), grid, block, 0, st, g.args, partials); break;
        default: hipLaunchKernelGGL((k_ds_forward<true, true>), grid, block, 0, st, g.args, partials); break;
    }
    S360_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ds_finish, dim3(1), block, 0, st, (const double2*)partials, g.blocks, g.nx, g.ny, loss);
    return s360_launch_status();
}

extern "C" int s360_depth_smooth_backward(const float* depth, const float* log_near, const float* log_far, const float* image, int32_t batch,
                                          int32_t views, int32_t bound_views, int32_t channels, int32_t height, int32_t width,
                                          float sigma_image, int32_t flags, const float* grad_loss, float* grad_depth, void* stream) {
    DSGrid g;
    const int rc = ds_setup(depth, log_near, log_far, image, batch, views, bound_views, channels, height, width, sigma_image, flags, &g);
    if (rc != S360_OK) return rc;
    if (!depth || !log_near || !log_far || !grad_loss || !grad_depth || ((flags & S360_DS_BILATERAL) && !image)) return S360_E_BADARG;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g.blocks), block(S360_BLOCK);
    switch (flags & (S360_DS_SECOND | S360_DS_BILATERAL)) {
        case 0: hipLaunchKernelGGL((k_ds_backward<false, false>), grid, block, 0, st, g.args, g.nx, g.ny, grad_loss, grad_depth); break;
        case S360_DS_SECOND: hipLaunchKernelGGL((k_ds_backward<true, false>), grid, block, 0, st, g.args, g.nx, g.ny, grad_loss, grad_depth); break;
        case S360_DS_BILATERAL: hipLaunchKernelGGL((k_ds_backward<false, true>), grid, block, 0, st, g.args, g.nx, g.ny, grad_loss, grad_depth); break;
        default: hipLaunchKernelGGL((k_ds_backward<true, true>), grid, block, 0, st, g.args, g.nx, g.ny, grad_loss, grad_depth); break;
    }
    return s360_launch_status();
}
