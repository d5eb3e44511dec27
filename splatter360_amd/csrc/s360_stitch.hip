// s360_stitch.hip — cube -> equirectangular stitch (Cube2Equirec) as one gather kernel, plus
// library-level entry points.  gfx950 only.
//
// Semantics restated from torch's 5-D grid_sample as the reference uses it
// (/root/reference/src/geometry/layers.py:108-116): input [C, D=6, fw, fw], grid (x=u, y=v, z=face),
// mode trilinear, padding_mode "border", align_corners=True:
//   i = ((g + 1) / 2) * (size - 1), clipped to [0, size-1]; 8 corner taps with the usual
//   (1-f) / f weights; a tap outside the volume is skipped, an in-range tap is added even with weight 0
//   (so an inf texel under a 0 weight gives NaN, as in torch).
// The face-z coordinate lands on an integer face +- 6e-8, so up to two faces are blended with
// a ~1e-7 weight — reproduced here rather than "fixed" (SURVEY.md §8 a10).
//
// The adjoint has no atomics: the caller passes the grid's inverse (a CSR "plan", built once per grid on the host:
// splatter360_amd/stitch.py adjoint_plan) that lists, per texel of the slot-space volume, the (pixel, tap) pairs that read it,
// sorted by pixel.  One thread per (texel, channel) recomputes each weight with the forward's own expressions (stitch_frac)
// and sums in plan order: gradients are bit-reproducible.
#include "s360_device.h"
#include "s360_prof.h"
#include "s360_stitch_taps.h"  // unnorm_clip, StitchFrac, stitch_frac

#include <climits>
#include <mutex>
#include <vector>

namespace s360 {

struct FaceMap {
    int src[6];   // source face index for Cube2Equirec slot s
    int flip[6];  // 1: read the face flipped on both image axes
    long long fs, cs, rs;  // element strides between faces / channels / rows of the face tensor
};

__global__ __launch_bounds__(S360_BLOCK) void k_cube2erp_fwd(const float* __restrict__ faces, const float* __restrict__ grid,
                                                            float* __restrict__ erp, int C, int fw, int eh, int ew, FaceMap fm) {
    const size_t n = (size_t)eh * ew;
    const size_t i = (size_t)blockIdx.x * S360_BLOCK + threadIdx.x;
    if (i >= n) return;
    const StitchFrac f = stitch_frac(grid, i, fw);
    // The eight taps once per pixel (offset + weight), then per channel eight INDEPENDENT loads in flight before the first use
    // (the per-channel, per-tap branches of the plain loop nest issued one dependent load at a time: 19 us for 19 MB).  A tap
    // outside the volume keeps a clamped (valid) address so its load is safe, and its product is not added (a select: acc + v * 0
    // would turn an inf texel into NaN where grid_sample skips the tap).  For finite inputs this is the same sum in the same
    // dz, dy, dx order as the old "weight 0" form: acc never holds -0, so dropping a +-0 addend changes no bit.
    size_t off[8];
    float wgt[8];
    unsigned in_mask = 0u;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        const int z = f.z0 + dz, zc = min(max(z, 0), 5);
        const bool zin = z >= 0 && z <= 5;
        const size_t fo = (size_t)fm.src[zc] * fm.fs;
        const bool fl = fm.flip[zc] != 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = f.y0 + dy, yc = min(max(y, 0), fw - 1);
            const bool yin = y >= 0 && y < fw;
            const int yy = fl ? fw - 1 - yc : yc;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = f.x0 + dx, xc = min(max(x, 0), fw - 1);
                const bool xin = x >= 0 && x < fw;
                const int xx = fl ? fw - 1 - xc : xc;
                const int k = 4 * dz + 2 * dy + dx;
                off[k] = fo + (size_t)yy * fm.rs + xx;
                wgt[k] = f.wx[dx] * f.wy[dy] * f.wz[dz];
                in_mask |= (zin && yin && xin) ? 1u << k : 0u;
            }
        }
    }
    for (int c = 0; c < C; ++c) {
        const float* fp = faces + (size_t)c * fm.cs;
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = fp[off[k]];
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = (in_mask >> k) & 1u ? acc + v[k] * wgt[k] : acc;
        erp[(size_t)c * n + i] = acc;
    }
}

// acc + the plan entries of slot-space texel ts, one entry at a time in plan order (pixel * 8 + tap): shared by the colour and the
// distance adjoint, so both sum the same float32 terms in the same order.
__device__ __forceinline__ float plan_sum(float acc, const float* __restrict__ gc, const float* __restrict__ grid,
                                          const int32_t* __restrict__ plan_off, const int32_t* __restrict__ plan_ent, int ts, int fw) {
    const int e1 = plan_off[ts + 1];
    int e = plan_off[ts];
    // Entries in batches of 8: every load of a batch (entry, grid, d_erp) is in flight before the first use.  The texels under
    // the poles have up to ~2 900 entries, and one chain of dependent loads per entry made them the kernel's whole duration.
    // The sum is still taken one entry at a time in plan order.
    for (; e + 8 <= e1; e += 8) {
        int pk[8];
        float g[8], w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) pk[j] = plan_ent[e + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const size_t p = (size_t)(pk[j] >> 3);
            const int k = pk[j] & 7;
            const StitchFrac f = stitch_frac(grid, p, fw);
            w[j] = f.wx[k & 1] * f.wy[(k >> 1) & 1] * f.wz[k >> 2];
            g[j] = gc[p];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += g[j] * w[j];
    }
    for (; e < e1; ++e) {
        const int pk = plan_ent[e];
        const size_t p = (size_t)(pk >> 3);
        const int k = pk & 7;
        const StitchFrac f = stitch_frac(grid, p, fw);
        const float w = f.wx[k & 1] * f.wy[(k >> 1) & 1] * f.wz[k >> 2];
        acc += gc[p] * w;
    }
    return acc;
}

// One thread per (texel of the dense [6,C,fw,fw] output, channel = blockIdx.y).  Output face f gathers from every slot s whose
// source is f (one for a permutation; none leaves the texel 0), reading slot s's texel under s's flip, then that texel's plan
// entries pixel * 8 + tap in order.  Every output element is written: no memset.
__global__ __launch_bounds__(S360_BLOCK) void k_cube2erp_bwd(const float* __restrict__ d_erp, const float* __restrict__ grid,
                                                            const int32_t* __restrict__ plan_off, const int32_t* __restrict__ plan_ent,
                                                            float* __restrict__ d_faces, int C, int fw, int eh, int ew, FaceMap fm) {
    const int ff = fw * fw;
    const int t = (int)(blockIdx.x * S360_BLOCK + threadIdx.x);
    if (t >= 6 * ff) return;
    const int c = (int)blockIdx.y;
    const size_t n = (size_t)eh * ew;
    const int face = t / ff, r = t - face * ff, y = r / fw, x = r - y * fw;
    const float* gc = d_erp + (size_t)c * n;
    float acc = 0.f;
    for (int s = 0; s < 6; ++s) {
        if (fm.src[s] != face) continue;
        const int ys = fm.flip[s] ? fw - 1 - y : y, xs = fm.flip[s] ? fw - 1 - x : x;
        acc = plan_sum(acc, gc, grid, plan_off, plan_ent, s * ff + ys * fw + xs, fw);
    }
    d_faces[((size_t)face * C + c) * ff + r] = acc;
}

// ---------------------------------------------------------------------------- z-depth -> ray distance, alone and fused into the stitch
// Replaces depth_to_distance_map_batch (/root/reference/src/geometry/z_depth_to_distance.py:4-34): sqrt(X^2 + Y^2 + d^2) with
// X = (u - cx) d / fx, Y = (v - cy) d / fy, which is |d| s with s = sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1).  s and the product
// are float64 from the float32 inputs, rounded once.  d = 0 gives 0, a negative d gives |d| s, inf and NaN propagate.  The gradient
// is sign(d) s, 0 at d = 0 (torch's autograd of the sqrt gives NaN there).
//   S360_D2D_REFERENCE: u is the ROW index and v the column index — the reference's torch.meshgrid(arange(width), arange(height)) is
//     "ij"-indexed, so the row pairs with cx / fx (and the function only broadcasts for square maps).
//   S360_D2D_PIXEL: u is the column (x with fx, cx) and v the row (y with fy, cy).
// The same three functions serve the stand-alone kernels and the fused stitch: the fused results are the two-step's bits.
__device__ __forceinline__ double dist_axis(int p, float c, float f) { return ((double)p - (double)c) / (double)f; }
__device__ __forceinline__ double dist_scale(double a, double b) { return sqrt(a * a + b * b + 1.0); }
__device__ __forceinline__ float dist_value(float d, double s) { return (float)(fabs((double)d) * s); }
__device__ __forceinline__ float dist_grad(float g, float d, double s) {
    const double sg = d > 0.f ? 1.0 : d < 0.f ? -1.0 : (double)d;  // 0 at d == 0, NaN stays NaN
    return (float)((double)g * (sg * s));
}

// s of pixel (row, col) under intrinsics k4 = (fx, fy, cx, cy)
template <int CONV>
__device__ __forceinline__ double dist_scale_at(const float* __restrict__ k4, int row, int col) {
    const int u = CONV == S360_D2D_REFERENCE ? row : col, v = CONV == S360_D2D_REFERENCE ? col : row;
    return dist_scale(dist_axis(u, k4[2], k4[0]), dist_axis(v, k4[3], k4[1]));
}

// One thread per pixel of depth[N, H, W]; map n reads row n of k4[N, 4]: distance = |d| s.
template <int CONV>
__global__ __launch_bounds__(S360_BLOCK) void k_depth2dist_fwd(const float* __restrict__ depth, const float* __restrict__ k4,
                                                              float* __restrict__ dist, size_t total, int H, int W) {
    const size_t i = (size_t)blockIdx.x * S360_BLOCK + threadIdx.x;
    if (i >= total) return;
    const size_t hw = (size_t)H * W, n = i / hw;
    const int r = (int)(i - n * hw), row = r / W, col = r - row * W;
    dist[i] = dist_value(depth[i], dist_scale_at<CONV>(k4 + 4 * n, row, col));
}

// The same thread map: d_depth = g sign(d) s.
template <int CONV>
__global__ __launch_bounds__(S360_BLOCK) void k_depth2dist_bwd(const float* __restrict__ g, const float* __restrict__ depth,
                                                              const float* __restrict__ k4, float* __restrict__ d_depth, size_t total,
                                                              int H, int W) {
    const size_t i = (size_t)blockIdx.x * S360_BLOCK + threadIdx.x;
    if (i >= total) return;
    const size_t hw = (size_t)H * W, n = i / hw;
    const int r = (int)(i - n * hw), row = r / W, col = r - row * W;
    d_depth[i] = dist_grad(g[i], depth[i], dist_scale_at<CONV>(k4 + 4 * n, row, col));
}

// k_cube2erp_fwd with one channel, panorama = blockIdx.y, and each tap value replaced by float32(|d_tap| s): same taps, weights,
// in-range select and dz, dy, dx order.  The eight depth loads are issued first, the float64 scales are computed while they
// are in flight (eight divisions and eight square roots per pixel: an axis term is shared by the two taps along the other axis).
//   S360_D2D_REFERENCE: the conversion happens in SLOT space, after the reorder — slot z uses row z of k4[N, 6, 4] and the slot-space
//     texel position (so the two flipped faces see (fw - 1 - u) - cx where their own image has u - cx), as the reference's lines do.
//   S360_D2D_PIXEL: each face is converted in its own image — slot z uses row src[z] and the pre-flip (source) texel position.
template <int CONV>
__global__ __launch_bounds__(S360_BLOCK) void k_cube2erp_dist_fwd(const float* __restrict__ depth, const float* __restrict__ k4,
                                                                 const float* __restrict__ grid, float* __restrict__ erp, int fw, int eh,
                                                                 int ew, FaceMap fm, long long ns) {
    const size_t n = (size_t)eh * ew;
    const size_t i = (size_t)blockIdx.x * S360_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t nb = blockIdx.y;
    const StitchFrac f = stitch_frac(grid, i, fw);
    const float* dp = depth + nb * (size_t)ns;
    size_t off[8];
    float wgt[8];
    int ia[2][2], ib[2][2];  // per face: the two positions along the axis paired with (cx, fx) and with (cy, fy)
    const float* kz[2];
    unsigned in_mask = 0u;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        const int z = f.z0 + dz, zc = min(max(z, 0), 5);
        const bool zin = z >= 0 && z <= 5;
        const size_t fo = (size_t)fm.src[zc] * fm.fs;
        const bool fl = fm.flip[zc] != 0;
        kz[dz] = k4 + (nb * 6 + (CONV == S360_D2D_REFERENCE ? zc : fm.src[zc])) * 4;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = f.y0 + dy, yc = min(max(y, 0), fw - 1);
            const bool yin = y >= 0 && y < fw;
            const int yy = fl ? fw - 1 - yc : yc;
            if (CONV == S360_D2D_REFERENCE) ia[dz][dy] = yc; else ib[dz][dy] = yy;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = f.x0 + dx, xc = min(max(x, 0), fw - 1);
                const bool xin = x >= 0 && x < fw;
                const int xx = fl ? fw - 1 - xc : xc;
                if (CONV == S360_D2D_REFERENCE) ib[dz][dx] = xc; else ia[dz][dx] = xx;
                const int k = 4 * dz + 2 * dy + dx;
                off[k] = fo + (size_t)yy * fm.rs + xx;
                wgt[k] = f.wx[dx] * f.wy[dy] * f.wz[dz];
                in_mask |= (zin && yin && xin) ? 1u << k : 0u;
            }
        }
    }
    float d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = dp[off[k]];
    double a[2][2], b[2][2];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        const float fx = kz[dz][0], fy = kz[dz][1], cx = kz[dz][2], cy = kz[dz][3];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            a[dz][j] = dist_axis(ia[dz][j], cx, fx);
            b[dz][j] = dist_axis(ib[dz][j], cy, fy);
        }
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dz = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
        const double s = CONV == S360_D2D_REFERENCE ? dist_scale(a[dz][dy], b[dz][dx]) : dist_scale(a[dz][dx], b[dz][dy]);
        acc = (in_mask >> k) & 1u ? acc + dist_value(d[k], s) * wgt[k] : acc;
    }
    erp[nb * n + i] = acc;
}

// k_cube2erp_bwd with one channel and panorama = blockIdx.y: the plan-ordered float32 sum of a slot-space texel, then ONE multiply
// by sign(d) s in float64, rounded once — the two-step's bits (stitch adjoint, then k_depth2dist's backward).  A face that several
// slots read adds their rounded terms in slot order; one that no slot reads gets 0.  Every element is written.
template <int CONV>
__global__ __launch_bounds__(S360_BLOCK) void k_cube2erp_dist_bwd(const float* __restrict__ d_erp, const float* __restrict__ depth,
                                                                 const float* __restrict__ k4, const float* __restrict__ grid,
                                                                 const int32_t* __restrict__ plan_off, const int32_t* __restrict__ plan_ent,
                                                                 float* __restrict__ d_depth, int fw, int eh, int ew, FaceMap fm) {
    const int ff = fw * fw;
    const int t = (int)(blockIdx.x * S360_BLOCK + threadIdx.x);
    if (t >= 6 * ff) return;
    const size_t nb = blockIdx.y;
    const size_t n = (size_t)eh * ew;
    const int face = t / ff, r = t - face * ff, y = r / fw, x = r - y * fw;
    const float* gc = d_erp + nb * n;
    const size_t o = nb * 6 * (size_t)ff + t;
    const float d = depth[o];
    float out = 0.f;
    bool any = false;
    for (int s = 0; s < 6; ++s) {
        if (fm.src[s] != face) continue;
        const int ys = fm.flip[s] ? fw - 1 - y : y, xs = fm.flip[s] ? fw - 1 - x : x;
        const float acc = plan_sum(0.f, gc, grid, plan_off, plan_ent, s * ff + ys * fw + xs, fw);
        const double sc = CONV == S360_D2D_REFERENCE ? dist_scale_at<CONV>(k4 + (nb * 6 + s) * 4, ys, xs)
                                                     : dist_scale_at<CONV>(k4 + (nb * 6 + face) * 4, y, x);
        const float term = dist_grad(acc, d, sc);
        out = any ? out + term : term;
        any = true;
    }
    d_depth[o] = out;
}

static bool make_face_map(const int32_t* face_map_host, const int64_t* strides_host, int C, int fw, FaceMap& fm) {
    fm.fs = strides_host ? strides_host[0] : (long long)C * fw * fw;
    fm.cs = strides_host ? strides_host[1] : (long long)fw * fw;
    fm.rs = strides_host ? strides_host[2] : (long long)fw;
    for (int s = 0; s < 6; ++s) {
        const int v = face_map_host ? face_map_host[s] : s;
        fm.src[s] = v & 7;
        fm.flip[s] = (v >> 3) & 1;
        if (fm.src[s] > 5) return false;
    }
    return true;
}

}  // namespace s360

using namespace s360;

extern "C" int s360_cube2erp_forward(const float* faces, const float* grid, float* erp, int32_t channels, int32_t face_w,
                                     int32_t equ_h, int32_t equ_w, const int32_t* face_map_host,
                                     const int64_t* strides_host, void* stream) {
    if (!faces || !grid || !erp || channels < 1 || face_w < 1 || equ_h < 1 || equ_w < 1) return S360_E_BADARG;
    FaceMap fm;
    if (!make_face_map(face_map_host, strides_host, channels, face_w, fm)) return S360_E_BADARG;
    const size_t n = (size_t)equ_h * equ_w;
    ProfScope ps(PS_STITCH, (hipStream_t)stream);
    hipLaunchKernelGGL(k_cube2erp_fwd, dim3((unsigned)((n + S360_BLOCK - 1) / S360_BLOCK)), dim3(S360_BLOCK), 0,
                       (hipStream_t)stream, faces, grid, erp, channels, face_w, equ_h, equ_w, fm);
    return s360_launch_status();
}

extern "C" int s360_cube2erp_backward(const float* d_erp, const float* grid, const int32_t* plan_offsets,
                                      const int32_t* plan_entries, float* d_faces, int32_t channels, int32_t face_w,
                                      int32_t equ_h, int32_t equ_w, const int32_t* face_map_host, const int64_t* strides_host,
                                      void* stream) {
    if (!d_erp || !grid || !plan_offsets || !plan_entries || !d_faces || channels < 1 || channels > 65535 || face_w < 1 ||
        equ_h < 1 || equ_w < 1)
        return S360_E_BADARG;
    // plan entries are pixel * 8 + tap and texel indices 6 * fw * fw + 1 offsets, both int32
    if ((long long)equ_h * equ_w * 8 > INT_MAX || 6LL * face_w * face_w + 1 > INT_MAX) return S360_E_BADARG;
    if (strides_host) return S360_E_UNSUPPORTED;  // the adjoint writes a dense [6,C,fw,fw] tensor
    FaceMap fm;
    if (!make_face_map(face_map_host, strides_host, channels, face_w, fm)) return S360_E_BADARG;
    const size_t texels = (size_t)6 * face_w * face_w;
    ProfScope ps(PS_STITCH_BWD, (hipStream_t)stream);
    hipLaunchKernelGGL(k_cube2erp_bwd, dim3((unsigned)((texels + S360_BLOCK - 1) / S360_BLOCK), (unsigned)channels), dim3(S360_BLOCK),
                       0, (hipStream_t)stream, d_erp, grid, plan_offsets, plan_entries, d_faces, channels, face_w, equ_h, equ_w, fm);
    return s360_launch_status();
}

extern "C" int s360_depth_to_distance_forward(const float* depth, const float* fxfycxcy, float* distance, int32_t n, int32_t height,
                                              int32_t width, int32_t convention, void* stream) {
    if (!depth || !fxfycxcy || !distance || n < 1 || height < 1 || width < 1) return S360_E_BADARG;
    if (convention != S360_D2D_REFERENCE && convention != S360_D2D_PIXEL) return S360_E_BADARG;
    if (convention == S360_D2D_REFERENCE && height != width) return S360_E_BADARG;
    const size_t total = (size_t)n * height * width, blocks = (total + S360_BLOCK - 1) / S360_BLOCK;
    if (blocks > (size_t)INT_MAX) return S360_E_BADARG;
    if (convention == S360_D2D_REFERENCE)
        hipLaunchKernelGGL(k_depth2dist_fwd<S360_D2D_REFERENCE>, dim3((unsigned)blocks), dim3(S360_BLOCK), 0, (hipStream_t)stream, depth,
                           fxfycxcy, distance, total, height, width);
    else
        hipLaunchKernelGGL(k_depth2dist_fwd<S360_D2D_PIXEL>, dim3((unsigned)blocks), dim3(S360_BLOCK), 0, (hipStream_t)stream, depth,
                           fxfycxcy, distance, total, height, width);
    return s360_launch_status();
}

extern "C" int s360_depth_to_distance_backward(const float* d_distance, const float* depth, const float* fxfycxcy, float* d_depth,
                                               int32_t n, int32_t height, int32_t width, int32_t convention, void* stream) {
    if (!d_distance || !depth || !fxfycxcy || !d_depth || n < 1 || height < 1 || width < 1) return S360_E_BADARG;
    if (convention != S360_D2D_REFERENCE && convention != S360_D2D_PIXEL) return S360_E_BADARG;
    if (convention == S360_D2D_REFERENCE && height != width) return S360_E_BADARG;
    const size_t total = (size_t)n * height * width, blocks = (total + S360_BLOCK - 1) / S360_BLOCK;
    if (blocks > (size_t)INT_MAX) return S360_E_BADARG;
    if (convention == S360_D2D_REFERENCE)
        hipLaunchKernelGGL(k_depth2dist_bwd<S360_D2D_REFERENCE>, dim3((unsigned)blocks), dim3(S360_BLOCK), 0, (hipStream_t)stream,
                           d_distance, depth, fxfycxcy, d_depth, total, height, width);
    else
        hipLaunchKernelGGL(k_depth2dist_bwd<S360_D2D_PIXEL>, dim3((unsigned)blocks), dim3(S360_BLOCK), 0, (hipStream_t)stream,
                           d_distance, depth, fxfycxcy, d_depth, total, height, width);
    return s360_launch_status();
}

// sizes, convention and the int32 limits shared by the fused stitch's two entry points (panoramas go in gridDim.y)
static bool dist_stitch_args_ok(int32_t n, int32_t face_w, int32_t equ_h, int32_t equ_w, int32_t convention) {
    if (n < 1 || n > 65535 || face_w < 1 || equ_h < 1 || equ_w < 1) return false;
    if (convention != S360_D2D_REFERENCE && convention != S360_D2D_PIXEL) return false;
    return (long long)n * equ_h * equ_w * 8 <= INT_MAX && 6LL * face_w * face_w + 1 <= INT_MAX;
}

extern "C" int s360_cube2erp_distance_forward(const float* depth_faces, const float* fxfycxcy, const float* grid, float* erp, int32_t n,
                                              int32_t face_w, int32_t equ_h, int32_t equ_w, int32_t convention,
                                              const int32_t* face_map_host, const int64_t* strides_host, void* stream) {
    if (!depth_faces || !fxfycxcy || !grid || !erp || !dist_stitch_args_ok(n, face_w, equ_h, equ_w, convention)) return S360_E_BADARG;
    FaceMap fm;
    if (!make_face_map(face_map_host, nullptr, 1, face_w, fm)) return S360_E_BADARG;
    long long ns = 6LL * face_w * face_w;
    if (strides_host) {
        ns = strides_host[0];
        fm.fs = strides_host[1];
        fm.rs = strides_host[2];
    }
    const size_t px = (size_t)equ_h * equ_w;
    const dim3 blocks((unsigned)((px + S360_BLOCK - 1) / S360_BLOCK), (unsigned)n);
    if (convention == S360_D2D_REFERENCE)
        hipLaunchKernelGGL(k_cube2erp_dist_fwd<S360_D2D_REFERENCE>, blocks, dim3(S360_BLOCK), 0, (hipStream_t)stream, depth_faces, fxfycxcy,
                           grid, erp, face_w, equ_h, equ_w, fm, ns);
    else
        hipLaunchKernelGGL(k_cube2erp_dist_fwd<S360_D2D_PIXEL>, blocks, dim3(S360_BLOCK), 0, (hipStream_t)stream, depth_faces, fxfycxcy,
                           grid, erp, face_w, equ_h, equ_w, fm, ns);
    return s360_launch_status();
}

extern "C" int s360_cube2erp_distance_backward(const float* d_erp, const float* depth_faces, const float* fxfycxcy, const float* grid,
                                               const int32_t* plan_offsets, const int32_t* plan_entries, float* d_depth_faces, int32_t n,
                                               int32_t face_w, int32_t equ_h, int32_t equ_w, int32_t convention,
                                               const int32_t* face_map_host, const int64_t* strides_host, void* stream) {
    if (!d_erp || !depth_faces || !fxfycxcy || !grid || !plan_offsets || !plan_entries || !d_depth_faces ||
        !dist_stitch_args_ok(n, face_w, equ_h, equ_w, convention))
        return S360_E_BADARG;
    FaceMap fm;
    if (!make_face_map(face_map_host, nullptr, 1, face_w, fm)) return S360_E_BADARG;
    if (strides_host) return S360_E_UNSUPPORTED;  // the adjoint reads and writes dense [N,6,fw,fw] tensors
    const size_t texels = (size_t)6 * face_w * face_w;
    const dim3 blocks((unsigned)((texels + S360_BLOCK - 1) / S360_BLOCK), (unsigned)n);
    if (convention == S360_D2D_REFERENCE)
        hipLaunchKernelGGL(k_cube2erp_dist_bwd<S360_D2D_REFERENCE>, blocks, dim3(S360_BLOCK), 0, (hipStream_t)stream, d_erp, depth_faces,
                           fxfycxcy, grid, plan_offsets, plan_entries, d_depth_faces, face_w, equ_h, equ_w, fm);
    else
        hipLaunchKernelGGL(k_cube2erp_dist_bwd<S360_D2D_PIXEL>, blocks, dim3(S360_BLOCK), 0, (hipStream_t)stream, d_erp, depth_faces,
                           fxfycxcy, grid, plan_offsets, plan_entries, d_depth_faces, face_w, equ_h, equ_w, fm);
    return s360_launch_status();
}

// ---------------------------------------------------------------------------- profiler
namespace s360 {
namespace {
struct Rec {
    int slot;
    hipEvent_t a, b;
};
std::mutex g_mu;
bool g_on = false;
std::vector<Rec> g_recs;          // completed or open records of the current window
std::vector<hipEvent_t> g_pool;   // recycled events
hipEvent_t get_event() {
    if (!g_pool.empty()) {
        hipEvent_t e = g_pool.back();
        g_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
}  // namespace
bool prof_enabled() { return g_on; }
void prof_mark(int slot, hipStream_t st, bool end) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!end) {
        Rec r{slot, get_event(), get_event()};
        (void)hipEventRecord(r.a, st);
        g_recs.push_back(r);
    } else {
        for (size_t i = g_recs.size(); i-- > 0;)
            if (g_recs[i].slot == slot) {
                (void)hipEventRecord(g_recs[i].b, st);
                break;
            }
    }
}
}  // namespace s360

static const char* kSlotNames[PS_NSLOTS] = {"preprocess", "tile_scan", "emit", "sort_tiles", "render",
                                            "render_bwd", "preprocess_bwd", "cube2erp", "cube2erp_bwd", "sh_eval", "gather_slots",
                                            "sh_bwd", "order_units"};

extern "C" int s360_profile_slots(void) { return PS_NSLOTS; }
extern "C" const char* s360_profile_slot_name(int slot) { return slot >= 0 && slot < PS_NSLOTS ? kSlotNames[slot] : ""; }
extern "C" int s360_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(s360::g_mu);
    s360::g_on = on != 0;
    return S360_OK;
}
extern "C" int s360_profile_collect(float* total_ms, int32_t* calls) {
    if (!total_ms || !calls) return S360_E_BADARG;
    std::lock_guard<std::mutex> lk(s360::g_mu);
    for (int i = 0; i < PS_NSLOTS; ++i) {
        total_ms[i] = 0.f;
        calls[i] = 0;
    }
    for (auto& r : s360::g_recs) {
        if (hipEventSynchronize(r.b) == hipSuccess) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
                total_ms[r.slot] += ms;
                calls[r.slot] += 1;
            }
        }
        s360::g_pool.push_back(r.a);
        s360::g_pool.push_back(r.b);
    }
    s360::g_recs.clear();
    return S360_OK;
}

extern "C" int s360_abi_version(void) { return S360_ABI_VERSION; }

extern "C" const char* s360_error_string(int code) {
    switch (code) {
        case S360_OK: return "ok";
        case S360_E_BADARG: return "bad argument";
        case S360_E_WORKSPACE: return "workspace too small";
        case S360_E_LAUNCH: return "HIP launch / runtime error";
        case S360_E_UNSUPPORTED: return "unsupported configuration";
        default: return "unknown error";
    }
}
