// s360_equirec2cube.hip — equirectangular -> cube resampler (Equirec2Cube.run) as one gather kernel, and its adjoint as a second
// gather over the coordinate plane's inverse.  gfx950 only.
//
// Semantics restated from the reference's host path (src/geometry/util.py:71-96): the ERP plane [H, W] gets two
// pole rows (row H = row H-1 rolled by W/2, row H+1 = row 0 rolled by W/2) and is sampled by scipy.ndimage.map_coordinates at the
// float32 coordinate plane (coor_y, coor_x) with mode='wrap', order 1 (bilinear) or 0 (nearest).  scipy's 'wrap' has the period
// n - 1, not n, over n = H + 2 rows and n = W columns:
//   s = n - 1;  c < 0: c += s (trunc(-c / s) + 1);  c > n - 1: c -= s trunc(c / s)
//   bilinear: i0 = floor(c), upper weight c - i0, i1 = i0 + 1, and i1 > n - 1: i1 -= s (i1 / s);  nearest: floor(c + 0.5)
// so coor_x = W - 0.5 blends columns 0 and 1 and coor_y = -0.5 blends the two pole rows.  That rule is E2C_REFERENCE; E2C_PERIODIC
// is what the padding was meant to do: x modulo W with taps floor(x) mod W and (floor(x) + 1) mod W, row -1 = row 0 rolled and
// row H = row H-1 rolled, y held in [-1, H].  Pole-row taps are folded onto their real texel, so the plane is never padded.
//
// Everything after the float32 coordinate is float64, in scipy's own order: t = 0; t += (v * wy) * wx over (ky, kx) =
// (0,0) (0,1) (1,0) (1,1) with wy = (1 - fy, fy); one rounding to float32, or floor(t + 0.5) clipped to 0..255 for uint8.
// Every tap index is clamped into the plane after conversion: no coordinate value makes a read leave the buffers.
//
// The adjoint has no atomics: the caller passes the inverse of the coordinate plane (a CSR plan over the H W ERP texels, built once
// per (plane, boundary, mode) on the host: splatter360_amd/equirec2cube.py adjoint_plan), entries cube_texel * 4 + tap, sorted.
// One thread per ERP texel recomputes each weight with the forward's own expressions (e2c_taps) and sums in plan order in float64.
#include "s360_device.h"

#include <climits>

namespace s360 {

struct CubeMap {
    int src[6];   // slot face (F R B L U D) that output face j shows
    int flip[6];  // 1: shown flipped on both image axes
    long long bs, fs, cs, rs;  // element strides between batches / faces / channels / rows of the cube tensor
};

struct E2CTaps {
    int off[4];       // k = 2 ky + kx: texel offset row * W + col inside one ERP plane, pole rows folded
    double wy[2], wx[2];
};

__device__ __forceinline__ int e2c_index(double v, int n) {   // clamp, then convert: NaN and out-of-range values land inside
    return (int)fmin(fmax(v, 0.0), (double)(n - 1));
}

// scipy's mode='wrap' on an axis of n samples (n >= 2): the two taps and the upper weight, or the nearest tap
__device__ __forceinline__ void e2c_axis_reference(double c, int n, bool nearest, int& i0, int& i1, double& f) {
    const double s = (double)(n - 1);
    if (c < 0.0)
        c += s * (trunc(-c / s) + 1.0);
    else if (c > s)
        c -= s * trunc(c / s);
    if (nearest) {
        i0 = i1 = e2c_index(floor(c + 0.5), n);
        f = 0.0;
        return;
    }
    const double f0 = floor(c);
    double f1 = f0 + 1.0;
    if (f1 > s) f1 -= s * floor(f1 / s);
    f = c - f0;
    i0 = e2c_index(f0, n);
    i1 = e2c_index(f1, n);
}

__device__ __forceinline__ E2CTaps e2c_taps(const float* __restrict__ coor, int ct, int H, int W, bool nearest, bool periodic) {
    const double y = (double)coor[2 * (size_t)ct], x = (double)coor[2 * (size_t)ct + 1];
    int py[2], px[2];   // padded row 0 .. H+1 (H: row H-1 rolled, H+1: row 0 rolled), column 0 .. W-1
    double fy, fx;
    if (!periodic) {
        e2c_axis_reference(y, H + 2, nearest, py[0], py[1], fy);
        e2c_axis_reference(x, W, nearest, px[0], px[1], fx);
    } else {
        const double cy = fmin(fmax(y, -1.0), (double)H);
        const double cx = x - (double)W * floor(x / (double)W);
        const double y0 = nearest ? floor(cy + 0.5) : floor(cy), x0 = nearest ? floor(cx + 0.5) : floor(cx);
        fy = nearest ? 0.0 : cy - y0;
        fx = nearest ? 0.0 : cx - x0;
        const int r0 = e2c_index(y0 + 1.0, H + 2) - 1;                      // -1 .. H
        const int r1 = nearest ? r0 : min(r0 + 1, H);
        py[0] = r0 < 0 ? H + 1 : r0;
        py[1] = r1 < 0 ? H + 1 : r1;
        px[0] = e2c_index(x0, W + 1) % W;
        px[1] = nearest ? px[0] : (px[0] + 1) % W;
    }
    E2CTaps t;
    t.wy[0] = 1.0 - fy;
    t.wy[1] = fy;
    t.wx[0] = 1.0 - fx;
    t.wx[1] = fx;
#pragma unroll
    for (int ky = 0; ky < 2; ++ky) {
        const bool pole = py[ky] >= H;
        const int row = py[ky] < H ? py[ky] : (py[ky] == H ? H - 1 : 0);
#pragma unroll
        for (int kx = 0; kx < 2; ++kx) {
            const int col = pole ? (px[kx] - W / 2 + W) % W : px[kx];
            t.off[2 * ky + kx] = row * W + col;
        }
    }
    return t;
}

__device__ __forceinline__ void e2c_store(float* p, double t) { *p = (float)t; }
__device__ __forceinline__ void e2c_store(uint8_t* p, double t) {   // scipy's integer output: t + 0.5 truncated, clipped
    double v = t > 0.0 ? t + 0.5 : 0.0;
    v = v > 255.0 ? 255.0 : v;
    *p = (uint8_t)(int)v;
}

// One thread per output texel (face j, row yo, column xo), in the order of the dense [fw, 6 fw] plane; it computes its taps once and
// loops over the B C planes.  Output face j shows slot src[j], flipped on both axes if flip[j]: the thread reads the coordinate of
// the slot texel it shows.
template <typename T>
__global__ __launch_bounds__(S360_BLOCK) void k_erp2cube_fwd(const T* __restrict__ erp, const float* __restrict__ coor,
                                                            const float* __restrict__ scale, T* __restrict__ cube, int B, int C, int H,
                                                            int W, int fw, int nearest, int periodic, CubeMap cm) {
    const int t = (int)(blockIdx.x * S360_BLOCK + threadIdx.x);
    if (t >= 6 * fw * fw) return;
    const int yo = t / (6 * fw), r = t - yo * 6 * fw, j = r / fw, xo = r - j * fw;
    const int y = cm.flip[j] ? fw - 1 - yo : yo, x = cm.flip[j] ? fw - 1 - xo : xo;
    const int ct = (y * 6 + cm.src[j]) * fw + x;
    const E2CTaps tp = e2c_taps(coor, ct, H, W, nearest != 0, periodic != 0);
    const double sc = scale ? (double)scale[ct] : 1.0;
    const size_t plane = (size_t)H * W;
    const size_t o = (size_t)j * cm.fs + (size_t)yo * cm.rs + xo;
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) {
            const T* src = erp + ((size_t)b * C + c) * plane;
            double acc;
            if (nearest) {
                acc = (double)src[tp.off[0]];
            } else {
                const double v0 = (double)src[tp.off[0]], v1 = (double)src[tp.off[1]], v2 = (double)src[tp.off[2]],
                             v3 = (double)src[tp.off[3]];
                acc = 0.0;
                acc += (v0 * tp.wy[0]) * tp.wx[0];
                acc += (v1 * tp.wy[0]) * tp.wx[1];
                acc += (v2 * tp.wy[1]) * tp.wx[0];
                acc += (v3 * tp.wy[1]) * tp.wx[1];
            }
            if (scale) acc *= sc;
            e2c_store(cube + (size_t)b * cm.bs + (size_t)c * cm.cs + o, acc);
        }
}

// One thread per (ERP texel, group of E2C_BWD_PLANES planes = blockIdx.y).  Each plan entry names a slot-space cube texel and one
// of its taps; the weight is recomputed once per entry and applied to the group's planes.  The gradient of slot s arrives through
// every output face that shows it (one for a permutation).  Every element of d_erp is written: a texel with no entries gets 0.
#define E2C_BWD_PLANES 4
__global__ __launch_bounds__(S360_BLOCK) void k_erp2cube_bwd(const float* __restrict__ d_cube, const float* __restrict__ coor,
                                                            const float* __restrict__ scale, const int32_t* __restrict__ plan_off,
                                                            const int32_t* __restrict__ plan_ent, float* __restrict__ d_erp, int B, int C,
                                                            int H, int W, int fw, int nearest, int periodic, CubeMap cm) {
    const int e = (int)(blockIdx.x * S360_BLOCK + threadIdx.x);
    if (e >= H * W) return;
    const int planes = B * C, p0 = (int)blockIdx.y * E2C_BWD_PLANES;
    const int texels = 6 * fw * fw;
    size_t base[E2C_BWD_PLANES];
    double acc[E2C_BWD_PLANES];
#pragma unroll
    for (int q = 0; q < E2C_BWD_PLANES; ++q) {
        const int p = min(p0 + q, planes - 1);   // the tail group repeats the last plane: loads stay legal, nothing is stored
        base[q] = (size_t)(p / C) * cm.bs + (size_t)(p % C) * cm.cs;
        acc[q] = 0.0;
    }
    const int i1 = plan_off[e + 1];
    for (int i = plan_off[e]; i < i1; ++i) {
        const int ent = plan_ent[i];
        const int ct = min(max(ent >> 2, 0), texels - 1), k = ent & 3;
        const E2CTaps tp = e2c_taps(coor, ct, H, W, nearest != 0, periodic != 0);
        const double wy = tp.wy[k >> 1], wx = tp.wx[k & 1];
        const double sc = scale ? (double)scale[ct] : 1.0;
        const int y = ct / (6 * fw), r = ct - y * 6 * fw, s = r / fw, x = r - s * fw;
        for (int j = 0; j < 6; ++j) {
            if (cm.src[j] != s) continue;
            const int yo = cm.flip[j] ? fw - 1 - y : y, xo = cm.flip[j] ? fw - 1 - x : x;
            const size_t o = (size_t)j * cm.fs + (size_t)yo * cm.rs + xo;
            double g[E2C_BWD_PLANES];
#pragma unroll
            for (int q = 0; q < E2C_BWD_PLANES; ++q) g[q] = (double)d_cube[base[q] + o];
#pragma unroll
            for (int q = 0; q < E2C_BWD_PLANES; ++q) {
                const double gs = scale ? g[q] * sc : g[q];
                acc[q] += nearest ? gs : (gs * wy) * wx;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < E2C_BWD_PLANES; ++q)
        if (p0 + q < planes) d_erp[(size_t)(p0 + q) * H * W + e] = (float)acc[q];
}

static bool make_cube_map(const int32_t* face_map_host, const int64_t* strides_host, int C, int fw, CubeMap& cm) {
    // default: the dense [B, C, fw, 6 fw] plane of the reference, faces side by side
    cm.bs = strides_host ? strides_host[0] : (long long)C * fw * 6 * fw;
    cm.fs = strides_host ? strides_host[1] : (long long)fw;
    cm.cs = strides_host ? strides_host[2] : (long long)fw * 6 * fw;
    cm.rs = strides_host ? strides_host[3] : (long long)6 * fw;
    if (cm.bs < 0 || cm.fs < 0 || cm.cs < 0 || cm.rs < 0) return false;
    for (int j = 0; j < 6; ++j) {
        const int v = face_map_host ? face_map_host[j] : j;
        if (v < 0 || v > 15 || (v & 7) > 5) return false;
        cm.src[j] = v & 7;
        cm.flip[j] = (v >> 3) & 1;
    }
    return true;
}

static bool e2c_sizes_ok(int B, int C, int H, int W, int fw) {
    if (B < 1 || C < 1 || H < 1 || W < 2 || fw < 1) return false;
    // texel offsets and plan entries (cube_texel * 4 + tap, H W + 1 offsets) are int32
    return (long long)H * W + 1 <= INT_MAX && 6LL * fw * fw * 4 <= INT_MAX && (long long)B * C <= INT_MAX;
}

}  // namespace s360

using namespace s360;

extern "C" int s360_erp2cube_forward(const void* erp, const float* coor, const float* scale, void* cube, int32_t batch,
                                     int32_t channels, int32_t equ_h, int32_t equ_w, int32_t face_w, int32_t mode, int32_t boundary,
                                     int32_t dtype, const int32_t* face_map_host, const int64_t* strides_host, void* stream) {
    if (!erp || !coor || !cube || !e2c_sizes_ok(batch, channels, equ_h, equ_w, face_w)) return S360_E_BADARG;
    if ((mode != S360_E2C_BILINEAR && mode != S360_E2C_NEAREST) || (boundary != S360_E2C_REFERENCE && boundary != S360_E2C_PERIODIC) ||
        (dtype != S360_E2C_FLOAT32 && dtype != S360_E2C_UINT8))
        return S360_E_BADARG;
    if (scale && dtype != S360_E2C_FLOAT32) return S360_E_UNSUPPORTED;   // a scaled uint8 plane has no reference counterpart
    CubeMap cm;
    if (!make_cube_map(face_map_host, strides_host, channels, face_w, cm)) return S360_E_BADARG;
    const unsigned blocks = (unsigned)((6LL * face_w * face_w + S360_BLOCK - 1) / S360_BLOCK);
    if (dtype == S360_E2C_FLOAT32)
        hipLaunchKernelGGL(k_erp2cube_fwd<float>, dim3(blocks), dim3(S360_BLOCK), 0, (hipStream_t)stream, (const float*)erp, coor, scale,
                           (float*)cube, batch, channels, equ_h, equ_w, face_w, mode, boundary, cm);
    else
        hipLaunchKernelGGL(k_erp2cube_fwd<uint8_t>, dim3(blocks), dim3(S360_BLOCK), 0, (hipStream_t)stream, (const uint8_t*)erp, coor,
                           scale, (uint8_t*)cube, batch, channels, equ_h, equ_w, face_w, mode, boundary, cm);
    return s360_launch_status();
}

extern "C" int s360_erp2cube_backward(const float* d_cube, const float* coor, const float* scale, const int32_t* plan_offsets,
                                      const int32_t* plan_entries, float* d_erp, int32_t batch, int32_t channels, int32_t equ_h,
                                      int32_t equ_w, int32_t face_w, int32_t mode, int32_t boundary, const int32_t* face_map_host,
                                      const int64_t* strides_host, void* stream) {
    if (!d_cube || !coor || !plan_offsets || !plan_entries || !d_erp || !e2c_sizes_ok(batch, channels, equ_h, equ_w, face_w))
        return S360_E_BADARG;
    if ((mode != S360_E2C_BILINEAR && mode != S360_E2C_NEAREST) || (boundary != S360_E2C_REFERENCE && boundary != S360_E2C_PERIODIC))
        return S360_E_BADARG;
    const long long groups = ((long long)batch * channels + E2C_BWD_PLANES - 1) / E2C_BWD_PLANES;
    if (groups > 65535) return S360_E_BADARG;
    CubeMap cm;
    if (!make_cube_map(face_map_host, strides_host, channels, face_w, cm)) return S360_E_BADARG;
    const unsigned blocks = (unsigned)(((long long)equ_h * equ_w + S360_BLOCK - 1) / S360_BLOCK);
    hipLaunchKernelGGL(k_erp2cube_bwd, dim3(blocks, (unsigned)groups), dim3(S360_BLOCK), 0, (hipStream_t)stream, d_cube, coor, scale,
                       plan_offsets, plan_entries, d_erp, batch, channels, equ_h, equ_w, face_w, mode, boundary, cm);
    return s360_launch_status();
}
