// s360_depth_loss.hip — the training step's context-depth loss (the reference's src/model/model_wrapper_erp.py:242-287 with
// erode and compute_l1_sphere_loss of src/model/model_wrapper_helper.py:4-24, :63-90), forward and backward.  gfx950 only.
//
//   erode(x, k)   1 - max over the k x k window of (1 - x), reflect padding by (k - 1) / 2 (index -1 -> 1, H -> H - 2; no
//                 longitude wrap).  The literal 1 - x and 1 - max keep it bit-identical to torch for any float input; the max
//                 takes a NaN wherever one is in the window, as torch's max_pool2d does.  Max is exact, so the separable
//                 row / column form gives the same bits as the 2-D window.
//   loss          sum |t - p| (w_h m) / clamp_away_from(sum w_h m, 0, 1e-10) over [V, H, W] (keep_batch) or [B, V, H, W],
//                 w_h = sin((h + 0.5) pi / H) (an input: the Python layer builds it with torch's own float32 expression).  Every
//                 term is the reference's float32 product with w_h m rounded first; terms are summed in float64.
//   fused mode    mask == NULL: m = erode(depth > near) and t = far where depth < fill_below (else depth), from the same tile
//                 with a halo.  The erosion of a {0, 1} mask is the AND over the window.  The tiling
//                 and every sum are those of the mask mode, so the fused loss is bit-identical to the mask mode fed with the
//                 eroded mask and the filled target.  The halo's mask is staged as bits (one ballot per 64 columns);
//                 the erosion is shifts and ANDs of 64-bit words, along rows and then down the columns.
//   backward      grad_p = -(((g / den') (w_h m)) sgn(t - p)), grad_t = -grad_p: torch's autograd chain (DivBackward, the sum's
//                 expand, MulBackward, AbsBackward with sgn = (0 < x) - (x < 0), so sgn(NaN) = 0, SubBackward), given the
//                 clamped denominator den' the forward wrote.  The fused backward recomputes the eroded mask from the halo.
//
// Determinism: every 32 x 256 tile writes its (num, den) double pair to its own workspace slot (fixed lane / wave order);
// k_l1_finish sums the slots of a batch element (or all of them) in a fixed order (block_tree_sum).  No atomics, no memset,
// no host synchronisation; far is read on the device.
#include "s360_device.h"

namespace s360 {

constexpr int DL_TW = 256, DL_TH = 32;                        // tile: 32 rows x 256 columns; a lane covers 4 adjacent columns
constexpr int DL_WAVES = S360_BLOCK / S360_WAVE, DL_ROWS = DL_TH / DL_WAVES;
constexpr int DL_MAXPAD = 8;                                  // fused mode: ksize <= 17
constexpr int DL_HH = DL_TH + 2 * DL_MAXPAD;
constexpr int DL_TWORDS = DL_TW / 64, DL_HWORDS = (DL_TW + 2 * DL_MAXPAD + 63) / 64;  // 64-column mask words: tile, halo
constexpr int ER_TW = 64, ER_TH = 16, ER_MAXPAD = 8;          // erode: tiles for pad <= 8, a direct window beyond
constexpr int ER_HW = ER_TW + 2 * ER_MAXPAD, ER_HH = ER_TH + 2 * ER_MAXPAD;

__device__ __forceinline__ int reflect_index(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// torch's max_pool2d update: a NaN is taken, and nothing replaces it (fmaxf would drop it)
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

__device__ __forceinline__ float sgn(float x) { return (float)((0.f < x) - (x < 0.f)); }

__global__ __launch_bounds__(S360_BLOCK) void k_erode(const float* __restrict__ x, float* __restrict__ y, int H, int W, int tiles_x,
                                                      int tiles_per_plane, int pad) {
    __shared__ float s[ER_HH * ER_HW];
    __shared__ float rm[ER_HH * ER_TW];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / tiles_per_plane, tile = blockIdx.x - plane * tiles_per_plane;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * ER_TH, x0 = tx * ER_TW;
    const size_t pofs = (size_t)plane * H * W;
    const float* xp = x + pofs;
    const int hh = ER_TH + 2 * pad, hw = ER_TW + 2 * pad;
    for (int i = tid; i < hh * hw; i += S360_BLOCK) {
        const int r = i / hw, c = i - r * hw;
        const int gy = y0 - pad + r, gx = x0 - pad + c;
        float v = 0.f;                                        // beyond the reflected border: feeds only pixels outside the plane
        if (gy < H + pad && gx < W + pad) v = 1.f - xp[(size_t)reflect_index(gy, H) * W + reflect_index(gx, W)];
        s[r * ER_HW + c] = v;
    }
    __syncthreads();
    for (int i = tid; i < hh * ER_TW; i += S360_BLOCK) {
        const int r = i / ER_TW, c = i - r * ER_TW;
        float m = -INFINITY;
        for (int k = 0; k <= 2 * pad; ++k) m = max_nan(m, s[r * ER_HW + c + k]);
        rm[r * ER_TW + c] = m;
    }
    __syncthreads();
    float* yp = y + pofs;
    for (int i = tid; i < ER_TH * ER_TW; i += S360_BLOCK) {
        const int r = i / ER_TW, c = i - r * ER_TW;
        if (y0 + r >= H || x0 + c >= W) continue;
        float m = -INFINITY;
        for (int k = 0; k <= 2 * pad; ++k) m = max_nan(m, rm[(r + k) * ER_TW + c]);
        yp[(size_t)(y0 + r) * W + x0 + c] = 1.f - m;
    }
}

// pad > ER_MAXPAD: the k x k window straight from global memory, one thread per pixel
__global__ __launch_bounds__(S360_BLOCK) void k_erode_direct(const float* __restrict__ x, float* __restrict__ y, long long n, int H, int W,
                                                             int pad) {
    const long long i = (long long)blockIdx.x * S360_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long hw = (long long)H * W;
    const long long plane = i / hw;
    const int rem = (int)(i - plane * hw), py = rem / W, px = rem - py * W;
    const float* xp = x + plane * hw;
    float m = -INFINITY;
    for (int dy = -pad; dy <= pad; ++dy) {
        const float* row = xp + (size_t)reflect_index(py + dy, H) * W;
        for (int dx = -pad; dx <= pad; ++dx) m = max_nan(m, 1.f - row[reflect_index(px + dx, W)]);
    }
    y[i] = 1.f - m;
}

struct DLFused {
    const float* far;                                         // device scalar
    float near_threshold, fill_below;
    int pad;
};

// One workgroup per 32 x 256 tile of one [H, W] plane (plane = b * V + v).  Lane l of wave w covers columns 4l .. 4l + 3 of the
// tile's rows w, w + 4, ..., w + 28; float4 loads where W % 4 == 0 and the pointers are 16-byte aligned (`vec`).  The order of
// the terms does not depend on `vec` or FUSED.  BWD: writes the gradients instead of the sums.
template <bool FUSED, bool BWD>
__global__ __launch_bounds__(S360_BLOCK) void k_l1_sphere(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                          const float* __restrict__ mask, const float* __restrict__ rw, int H, int W,
                                                          int tiles_x, int tiles_per_plane, int planes_per_batch, int keep_batch, int vec,
                                                          DLFused fz, double2* __restrict__ partials, const float* __restrict__ grad_loss,
                                                          const float* __restrict__ den, float* __restrict__ grad_pred,
                                                          float* __restrict__ grad_tgt) {
    __shared__ uint64_t hb[FUSED ? DL_HH * DL_HWORDS : 1];   // depth > near over the halo, one bit per column
    __shared__ uint64_t rb[FUSED ? DL_HH * DL_TWORDS : 1];   // its AND along rows, for the tile's 256 columns
    __shared__ double wsum[2][DL_WAVES];
    const int tid = threadIdx.x, lane = tid & (S360_WAVE - 1), wave = tid / S360_WAVE;
    const int plane = blockIdx.x / tiles_per_plane, tile = blockIdx.x - plane * tiles_per_plane;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * DL_TH, x0 = tx * DL_TW;
    const size_t pofs = (size_t)plane * H * W;
    const float* pp = pred + pofs;
    const float* tp = tgt + pofs;
    const float* mp = FUSED ? nullptr : mask + pofs;
    float far = 0.f;
    if constexpr (FUSED) {
        far = *fz.far;
        const int pad = fz.pad, hh = DL_TH + 2 * pad, hw = DL_TW + 2 * pad, nw = (hw + S360_WAVE - 1) / S360_WAVE;
        for (int r = wave; r < hh; r += DL_WAVES) {           // wave-uniform loops: every lane takes part in the ballots
            const int gy = y0 - pad + r;
            const float* row = gy < H + pad ? tp + (size_t)reflect_index(gy, H) * W : nullptr;
            for (int k = 0; k < nw; ++k) {
                const int c = S360_WAVE * k + lane, gx = x0 - pad + c;
                bool v = true;                                // beyond the reflected border: feeds only pixels outside the plane
                if (row && c < hw && gx < W + pad) v = row[reflect_index(gx, W)] > fz.near_threshold;
                const uint64_t bits = __ballot(v);
                if (lane == 0) hb[r * DL_HWORDS + k] = bits;
            }
        }
        __syncthreads();
        // bit i of word j of halo row r: AND of halo columns 64 j + i .. 64 j + i + 2 pad (the tile's column 64 j + i)
        for (int i = tid; i < hh * DL_TWORDS; i += S360_BLOCK) {
            const int r = i / DL_TWORDS, j = i - r * DL_TWORDS;
            const uint64_t a = hb[r * DL_HWORDS + j], b = hb[r * DL_HWORDS + j + 1];
            uint64_t v = a;
            for (int k = 1; k <= 2 * pad; ++k) v &= (a >> k) | (b << (64 - k));
            rb[i] = v;
        }
        __syncthreads();
    }
    float q = 0.f;
    if constexpr (BWD) {
        const int b = keep_batch ? plane / planes_per_batch : 0;
        q = grad_loss[b] / den[b];                            // DivBackward: g / den'
    }
    double num = 0.0, dsum = 0.0;
    const int c0 = 4 * lane, gx0 = x0 + c0;
    const bool full = vec && gx0 + 3 < W;
#pragma unroll 2
    for (int j = 0; j < DL_ROWS; ++j) {
        const int r = wave + DL_WAVES * j, gy = y0 + r;
        if (gy >= H || gx0 >= W) break;
        const size_t o = (size_t)gy * W + gx0;
        float p[4], t[4], m[4];
        if (full) {
            const float4 a = *reinterpret_cast<const float4*>(pp + o), b = *reinterpret_cast<const float4*>(tp + o);
            p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w;
            t[0] = b.x; t[1] = b.y; t[2] = b.z; t[3] = b.w;
            if constexpr (!FUSED) {
                const float4 c = *reinterpret_cast<const float4*>(mp + o);
                m[0] = c.x; m[1] = c.y; m[2] = c.z; m[3] = c.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = gx0 + e < W;
                p[e] = in ? pp[o + e] : 0.f;
                t[e] = in ? tp[o + e] : 0.f;
                if constexpr (!FUSED) m[e] = in ? mp[o + e] : 0.f;
            }
        }
        const float wh = rw[gy];
        uint64_t mw = ~0ull;                                  // fused: the eroded mask of the tile row's 64-column word
        if constexpr (FUSED)
            for (int k = 0; k <= 2 * fz.pad; ++k) mw &= rb[(r + k) * DL_TWORDS + (c0 >> 6)];
        float g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (FUSED) {
                m[e] = (mw >> ((c0 & 63) + e)) & 1 ? 1.f : 0.f;
                t[e] = t[e] < fz.fill_below ? far : t[e];
            }
            const float wm = wh * m[e];                       // sin_phi * mask, rounded first as in the reference
            const float d = t[e] - p[e];
            if constexpr (BWD) {
                g[e] = (q * wm) * sgn(d);                     // MulBackward then AbsBackward; SubBackward: grad_t = g, grad_p = -g
            } else if (gx0 + e < W) {
                num += (double)(fabsf(d) * wm);
                dsum += (double)wm;
            }
        }
        if constexpr (BWD) {
            if (full) {
                *reinterpret_cast<float4*>(grad_pred + pofs + o) = make_float4(-g[0], -g[1], -g[2], -g[3]);
                if (grad_tgt) *reinterpret_cast<float4*>(grad_tgt + pofs + o) = make_float4(g[0], g[1], g[2], g[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (gx0 + e < W) {
                        grad_pred[pofs + o + e] = -g[e];
                        if (grad_tgt) grad_tgt[pofs + o + e] = g[e];
                    }
            }
        }
    }
    if constexpr (!BWD) {
        // block_sum's order, written out: through block_sum the mask-mode kernel's register count moved (30 to 29)
#pragma unroll
        for (int off = S360_WAVE / 2; off > 0; off >>= 1) {
            num += __shfl_down(num, off, S360_WAVE);
            dsum += __shfl_down(dsum, off, S360_WAVE);
        }
        if (lane == 0) {
            wsum[0][wave] = num;
            wsum[1][wave] = dsum;
        }
        __syncthreads();
        if (tid == 0) {
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int w = 0; w < DL_WAVES; ++w) {
                a += wsum[0][w];
                b += wsum[1][w];
            }
            partials[blockIdx.x] = make_double2(a, b);
        }
    }
}

// One workgroup per output (a batch element, or the whole batch): thread t sums slots t, t + 256, ... in order, then a fixed
// tree.  num and den are rounded to float32 (the reference's sums are float32), den is clamped away from 0 by 1e-10 as
// clamp_away_from does (>= 0: max(den, 1e-10); else min(den, -1e-10); NaN stays NaN), and the quotient is taken in float32.
__global__ __launch_bounds__(S360_BLOCK) void k_l1_finish(const double2* __restrict__ partials, int slots_per_out, float* __restrict__ loss,
                                                          float* __restrict__ den_out) {
    __shared__ double red[2][S360_BLOCK];                     // num, den
    const int tid = threadIdx.x, o = blockIdx.x;
    const double2* p = partials + (size_t)o * slots_per_out;
    double s[2] = {0.0, 0.0};
    for (int j = tid; j < slots_per_out; j += S360_BLOCK) {
        const double2 v = p[j];
        s[0] += v.x;
        s[1] += v.y;
    }
    block_tree_sum(s, red);
    if (tid == 0) {
        const float nf = (float)red[0][0], df = (float)red[1][0];
        float dc;
        if (df >= 0.f) dc = df > 1e-10f ? df : 1e-10f;
        else dc = (df < -1e-10f || df != df) ? df : -1e-10f;
        loss[o] = nf / dc;
        den_out[o] = dc;
    }
}

}  // namespace s360

using namespace s360;

extern "C" int s360_erode(const float* x, float* out, int32_t n_planes, int32_t height, int32_t width, int32_t ksize, void* stream) {
    if (!x || !out || n_planes < 1 || height < 1 || width < 1 || ksize < 1 || !(ksize & 1)) return S360_E_BADARG;
    const int pad = (ksize - 1) / 2;
    if (pad >= height || pad >= width) return S360_E_BADARG;
    const hipStream_t st = (hipStream_t)stream;
    if (pad <= ER_MAXPAD) {
        const int tiles_x = (width + ER_TW - 1) / ER_TW, tiles_y = (height + ER_TH - 1) / ER_TH;
        const long long tiles_per_plane = (long long)tiles_x * tiles_y, blocks = tiles_per_plane * n_planes;
        if (!s360_grid_fits(blocks)) return S360_E_BADARG;
        hipLaunchKernelGGL(k_erode, dim3((unsigned)blocks), dim3(S360_BLOCK), 0, st, x, out, (int)height, (int)width, tiles_x,
                           (int)tiles_per_plane, pad);
    } else {
        const long long n = (long long)n_planes * height * width, blocks = (n + S360_BLOCK - 1) / S360_BLOCK;
        if (!s360_grid_fits(blocks)) return S360_E_BADARG;
        hipLaunchKernelGGL(k_erode_direct, dim3((unsigned)blocks), dim3(S360_BLOCK), 0, st, x, out, n, (int)height, (int)width, pad);
    }
    return s360_launch_status();
}

namespace {

struct DLGrid {
    int tiles_x, tiles_per_plane;
    long long blocks;
};

// shared argument check of the forward and the backward; returns S360_OK and the grid, or an error
int dl_setup(const float* mask, int32_t batch, int32_t views, int32_t height, int32_t width, int32_t ksize, const float* far, DLGrid* g) {
    if (batch < 1 || views < 1 || height < 1 || width < 1) return S360_E_BADARG;
    if (!mask) {
        if (!far || ksize < 1 || !(ksize & 1) || (ksize - 1) / 2 > DL_MAXPAD) return S360_E_BADARG;
        const int pad = (ksize - 1) / 2;
        if (pad >= height || pad >= width) return S360_E_BADARG;
    }
    g->tiles_x = (width + DL_TW - 1) / DL_TW;
    const long long tiles_per_plane = (long long)g->tiles_x * ((height + DL_TH - 1) / DL_TH);
    g->blocks = tiles_per_plane * batch * views;
    if (!s360_grid_fits(g->blocks)) return S360_E_BADARG;
    g->tiles_per_plane = (int)tiles_per_plane;
    return S360_OK;
}

}  // namespace

extern "C" int s360_l1_sphere_forward(const float* pred, const float* target, const float* mask, const float* row_weights,
                                      int32_t batch, int32_t views, int32_t height, int32_t width, int32_t keep_batch,
                                      const float* far, float near_threshold, float fill_below, int32_t ksize, float* loss_out,
                                      float* den_out, void* workspace, size_t* workspace_bytes, void* stream) {
    if (!workspace_bytes) return S360_E_BADARG;
    DLGrid g;
    const int rc = dl_setup(mask, batch, views, height, width, ksize, far, &g);
    if (rc != S360_OK) return rc;
    const int ws = s360_workspace(workspace, workspace_bytes, (size_t)g.blocks * sizeof(double2), 16,
                                  pred && target && row_weights && loss_out && den_out);
    if (ws != S360_WS_READY) return ws;
    const int vec = (width % 4 == 0) && s360_aligned(pred, 16) && s360_aligned(target, 16) && (!mask || s360_aligned(mask, 16));
    const DLFused fz{far, near_threshold, fill_below, mask ? 0 : (ksize - 1) / 2};
    double2* partials = (double2*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    if (mask)
        hipLaunchKernelGGL((k_l1_sphere<false, false>), dim3((unsigned)g.blocks), dim3(S360_BLOCK), 0, st, pred, target, mask, row_weights,
                           (int)height, (int)width, g.tiles_x, g.tiles_per_plane, (int)views, 0, vec, fz, partials, nullptr, nullptr,
                           nullptr, nullptr);
    else
        hipLaunchKernelGGL((k_l1_sphere<true, false>), dim3((unsigned)g.blocks), dim3(S360_BLOCK), 0, st, pred, target, mask, row_weights,
                           (int)height, (int)width, g.tiles_x, g.tiles_per_plane, (int)views, 0, vec, fz, partials, nullptr, nullptr,
                           nullptr, nullptr);
    S360_CHECK_LAUNCH();
    const int outs = keep_batch ? batch : 1;
    const long long slots = g.blocks / outs;
    hipLaunchKernelGGL(k_l1_finish, dim3((unsigned)outs), dim3(S360_BLOCK), 0, st, (const double2*)partials, (int)slots, loss_out, den_out);
    return s360_launch_status();
}

extern "C" int s360_l1_sphere_backward(const float* pred, const float* target, const float* mask, const float* row_weights,
                                       int32_t batch, int32_t views, int32_t height, int32_t width, int32_t keep_batch,
                                       const float* far, float near_threshold, float fill_below, int32_t ksize,
                                       const float* grad_loss, const float* den, float* grad_pred, float* grad_target, void* stream) {
    DLGrid g;
    const int rc = dl_setup(mask, batch, views, height, width, ksize, far, &g);
    if (rc != S360_OK) return rc;
    if (!pred || !target || !row_weights || !grad_loss || !den || !grad_pred) return S360_E_BADARG;
    const int vec = (width % 4 == 0) && s360_aligned(pred, 16) && s360_aligned(target, 16) && (!mask || s360_aligned(mask, 16)) && s360_aligned(grad_pred, 16) &&
                    (!grad_target || s360_aligned(grad_target, 16));
    const DLFused fz{far, near_threshold, fill_below, mask ? 0 : (ksize - 1) / 2};
    const hipStream_t st = (hipStream_t)stream;
    if (mask)
        hipLaunchKernelGGL((k_l1_sphere<false, true>), dim3((unsigned)g.blocks), dim3(S360_BLOCK), 0, st, pred, target, mask, row_weights,
                           (int)height, (int)width, g.tiles_x, g.tiles_per_plane, (int)views, keep_batch ? 1 : 0, vec, fz, nullptr,
                           grad_loss, den, grad_pred, grad_target);
    else
        hipLaunchKernelGGL((k_l1_sphere<true, true>), dim3((unsigned)g.blocks), dim3(S360_BLOCK), 0, st, pred, target, mask, row_weights,
                           (int)height, (int)width, g.tiles_x, g.tiles_per_plane, (int)views, keep_batch ? 1 : 0, vec, fz, nullptr,
                           grad_loss, den, grad_pred, grad_target);
    return s360_launch_status();
}
