// s360_cost_volume.hip — the encoder's spherical plane-sweep cost volume (the reference's
// src/model/encoder/costvolume/depth_predictor_multiview_360.py:588-630 with warp_with_pose_depth_candidates, :159-214, and the
// 'hm3d' / 'replica' convention of src/geometry/utils360.py), forward and backward, without the [n, C, D, h, w] warped tensor.
// gfx950 only.
//
//   out[n, d, y, x] = scale * sum_pairing sum_c f_own[n, c, y, x] * bilinear(f_partner[slot(pairing, n), c], warp(pairing, n, d, y, x))
//
//   warp          pixel -> theta = (0.5 - (x + 0.5) / w) 2 pi, phi = -((y + 0.5) / h - 0.5) pi -> the ray (cos phi sin theta,
//                 sin phi, cos phi cos theta) * depth_d -> q = R p + t -> theta' = atan2(q_x, q_z), phi' = atan2(q_y,
//                 sqrt(q_x^2 + q_z^2)) -> x' = (-theta' / 2 pi + 0.5) w - 0.5, y' = (-phi' / pi + 0.5) h - 0.5 -> the reference's
//                 u = (x' + 0.5) / w * 2 - 1 handed to an align_corners=True sampler, i.e. ix = (u + 1) / 2 * (w - 1): an
//                 off-by-half that is reproduced, not fixed.  The chain is evaluated in float64 from the float32 poses and
//                 depths: it is per (d, pixel) and amortised over all channels, so its cost does not show, and the kernel's
//                 distance from a float64 statement is then that of the float32 products and sums alone.  A tap outside the map
//                 contributes zero, and so does a sample whose warped position is not finite.
//   layout        the kernels read channels-last copies [slot, y, x, CP] (CP = C rounded up to 4, zero filled) that k_cv_to_cl
//                 writes into the workspace: a bilinear tap is then CP contiguous floats and a half-wave of 32 lanes reads 512
//                 bytes of it in one instruction (C = 128).  No tensor with C * D elements exists in either direction.
//   forward       a half-wave owns one pixel: lane l evaluates the warp of depth dbase + l, the 32 results are handed round with
//                 shuffles, every lane multiplies its four channels of the pixel's own features (registers) with the four taps,
//                 and the 32 per-lane partial sums are transposed and reduced in 31 shuffles, which leaves lane l with depth
//                 dbase + l.  A block covers 32 pixels and writes [32 depths][32 pixels] tiles through LDS (128-byte rows).
//                 Fixed order throughout: bit-identical from run to run and stream to stream.
//   backward      own side: the same walk, each lane accumulating g * bilinear(f_partner) for its four channels in registers; no
//                 cross-lane step, deterministic.  Partner side: float32 vector atomics (global_atomic_add_f32), as grid_sample's
//                 own backward uses: lane l holds channels l, l + 32, l + 64, l + 96, so that one atomic instruction covers two
//                 128-byte segments, and consecutive depths that fall into the same 2 x 2 tap cell are summed in registers first
//                 and sent as one set of adds.  Its sums depend on arrival order in the last bits.
#include "s360_device.h"

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace s360 {

constexpr int CV_PX = 32;                                     // pixels per block
constexpr int CV_HALVES = S360_BLOCK / 32;                    // half-waves per block: one pixel each per pass
constexpr int CV_PASSES = CV_PX / CV_HALVES;
constexpr int CV_MAX_SIDE = 65534;                            // x0 + 1 and y0 + 1 are packed into 16 bits each
constexpr double CV_PI = 3.14159265358979323846;

struct CVArgs {
    const float* own_cl;        // [n, h w, CP]
    const float* partner_cl;    // [m, h w, CP]
    const int32_t* slot;        // [pairs, n] or null (identity)
    const float* poses;         // [pairs, n, 4, 4]
    const float* depths;        // [n, D]
    int n, m, pairs, C, CP, h, w, D;
    float scale;
};

// the unit ray of pixel p = y w + x
__device__ __forceinline__ void cv_ray(int p, int h, int w, double ray[3]) {
    const int y = p / w, x = p - y * w;
    const double theta = (0.5 - (x + 0.5) / w) * 2.0 * CV_PI;
    const double phi = -((y + 0.5) / h - 0.5) * CV_PI;
    double st, ct, sp, cp;
    sincos(theta, &st, &ct);
    sincos(phi, &sp, &cp);
    ray[0] = cp * st;
    ray[1] = sp;
    ray[2] = cp * ct;
}

// the sampling position of ray * depth under `pose` (row-major 4 x 4, partner from own): the top-left tap packed as
// (x0 + 1) | (y0 + 1) << 16 and the two weights; -1 when the position is not inside (-1, w) x (-1, h) (NaN included)
__device__ __forceinline__ void cv_sample(const float* __restrict__ pose, const double ray[3], double depth, int h, int w, int& packed,
                                          float& wx, float& wy) {
    const double px = ray[0] * depth, py = ray[1] * depth, pz = ray[2] * depth;
    const double qx = (double)pose[0] * px + (double)pose[1] * py + (double)pose[2] * pz + (double)pose[3];
    const double qy = (double)pose[4] * px + (double)pose[5] * py + (double)pose[6] * pz + (double)pose[7];
    const double qz = (double)pose[8] * px + (double)pose[9] * py + (double)pose[10] * pz + (double)pose[11];
    const double theta = atan2(qx, qz);
    const double phi = atan2(qy, sqrt(qx * qx + qz * qz));
    const double xl = (-theta / (2.0 * CV_PI) + 0.5) * w - 0.5;
    const double yl = (-phi / CV_PI + 0.5) * h - 0.5;
    const double u = (xl + 0.5) / w * 2.0 - 1.0;
    const double v = (yl + 0.5) / h * 2.0 - 1.0;
    const double ix = (u + 1.0) / 2.0 * (w - 1);
    const double iy = (v + 1.0) / 2.0 * (h - 1);
    packed = -1;
    wx = wy = 0.f;
    if (ix > -1.0 && ix < (double)w && iy > -1.0 && iy < (double)h) {
        const double fx = floor(ix), fy = floor(iy);
        packed = ((int)fx + 1) | (((int)fy + 1) << 16);
        wx = (float)(ix - fx);
        wy = (float)(iy - fy);
    }
}

__device__ __forceinline__ void cv_unpack(int packed, int& x0, int& y0) {
    x0 = (packed & 0xffff) - 1;                               // packed == -1: 65534, outside every map (sides <= CV_MAX_SIDE)
    y0 = ((packed >> 16) & 0xffff) - 1;
}

// the bilinear sample of four consecutive channels: base points at channel 4 j of slot's plane
__device__ __forceinline__ float4 cv_bilinear4(const float* __restrict__ base, int CP, int h, int w, int x0, int y0, float wx, float wy) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool xa = (unsigned)x0 < (unsigned)w, xb = (unsigned)(x0 + 1) < (unsigned)w;
    const bool ya = (unsigned)y0 < (unsigned)h, yb = (unsigned)(y0 + 1) < (unsigned)h;
    const size_t o = ((size_t)y0 * w + x0) * CP;              // only dereferenced where the tap is inside
    const float4 t00 = (xa && ya) ? *(const float4*)(base + (ptrdiff_t)o) : z;
    const float4 t01 = (xb && ya) ? *(const float4*)(base + (ptrdiff_t)((size_t)y0 * w + x0 + 1) * CP) : z;
    const float4 t10 = (xa && yb) ? *(const float4*)(base + (ptrdiff_t)((size_t)(y0 + 1) * w + x0) * CP) : z;
    const float4 t11 = (xb && yb) ? *(const float4*)(base + (ptrdiff_t)((size_t)(y0 + 1) * w + x0 + 1) * CP) : z;
    const float w00 = (1.f - wx) * (1.f - wy), w01 = wx * (1.f - wy), w10 = (1.f - wx) * wy, w11 = wx * wy;
    float4 s;
    s.x = fmaf(w11, t11.x, fmaf(w10, t10.x, fmaf(w01, t01.x, w00 * t00.x)));
    s.y = fmaf(w11, t11.y, fmaf(w10, t10.y, fmaf(w01, t01.y, w00 * t00.y)));
    s.z = fmaf(w11, t11.z, fmaf(w10, t10.z, fmaf(w01, t01.z, w00 * t00.z)));
    s.w = fmaf(w11, t11.w, fmaf(w10, t10.w, fmaf(w01, t01.w, w00 * t00.w)));
    return s;
}

// [S, C, HW] -> [S, HW, CP], channels C..CP-1 zero
__global__ __launch_bounds__(S360_BLOCK) void k_cv_to_cl(const float* __restrict__ in, float* __restrict__ out, int C, int CP, int HW) {
    __shared__ float t[32][65];
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 32, s = blockIdx.z;
    for (int i = threadIdx.x; i < 32 * 64; i += S360_BLOCK) {
        const int c = i >> 6, p = i & 63;
        t[c][p] = (c0 + c < C && p0 + p < HW) ? in[((size_t)s * C + c0 + c) * HW + p0 + p] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * 64; i += S360_BLOCK) {
        const int p = i >> 5, c = i & 31;
        if (c0 + c < CP && p0 + p < HW) out[((size_t)s * HW + p0 + p) * CP + c0 + c] = t[c][p];
    }
}

// [S, HW, CP] -> [S, C, HW]
__global__ __launch_bounds__(S360_BLOCK) void k_cv_from_cl(const float* __restrict__ in, float* __restrict__ out, int C, int CP, int HW) {
    __shared__ float t[32][65];
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 32, s = blockIdx.z;
    for (int i = threadIdx.x; i < 32 * 64; i += S360_BLOCK) {
        const int p = i >> 5, c = i & 31;
        t[c][p] = (c0 + c < C && p0 + p < HW) ? in[((size_t)s * HW + p0 + p) * CP + c0 + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * 64; i += S360_BLOCK) {
        const int c = i >> 6, p = i & 63;
        if (c0 + c < C && p0 + p < HW) out[((size_t)s * C + c0 + c) * HW + p0 + p] = t[c][p];
    }
}

// one step of the transpose-reduce over a half-wave: N values per lane become N / 2, lane bit O picks the upper half
template <int O>
__device__ __forceinline__ void cv_fold(float* acc, int lane) {
    const bool up = lane & O;
#pragma unroll
    for (int i = 0; i < O; ++i) {
        const float keep = up ? acc[i + O] : acc[i];
        const float send = up ? acc[i] : acc[i + O];
        acc[i] = keep + __shfl_xor(send, O, 32);
    }
}

__global__ __launch_bounds__(S360_BLOCK) void k_cv_forward(CVArgs a, float* __restrict__ out) {
    __shared__ float tile[32][CV_PX + 1];
    const int tid = threadIdx.x, l = tid & 31, half = tid >> 5;
    const int HW = a.h * a.w;
    const int blocks_per_n = (HW + CV_PX - 1) / CV_PX;
    const int ni = blockIdx.x / blocks_per_n, p0 = (blockIdx.x - ni * blocks_per_n) * CV_PX;
    const int nvec = a.CP >> 2;
    for (int dbase = 0; dbase < a.D; dbase += 32) {
        const int d = dbase + l;
        const int dcount = min(32, a.D - dbase);
        const double depth = d < a.D ? (double)a.depths[(size_t)ni * a.D + d] : 1.0;
        for (int pass = 0; pass < CV_PASSES; ++pass) {
            const int pl = pass * CV_HALVES + half, p = p0 + pl;
            float tot = 0.f;
            if (p < HW) {                                     // uniform over the half-wave; the shuffles stay inside it
                double ray[3];
                cv_ray(p, a.h, a.w, ray);
                for (int pair = 0; pair < a.pairs; ++pair) {
                    const int slot = a.slot ? a.slot[(size_t)pair * a.n + ni] : ni;
                    if ((unsigned)slot >= (unsigned)a.m) continue;
                    int pk;
                    float wx, wy;
                    cv_sample(a.poses + ((size_t)pair * a.n + ni) * 16, ray, depth, a.h, a.w, pk, wx, wy);
                    if (d >= a.D) pk = -1;
                    float acc[32];
#pragma unroll
                    for (int i = 0; i < 32; ++i) acc[i] = 0.f;
                    const float* pbase = a.partner_cl + (size_t)slot * HW * a.CP;
                    for (int jb = 0; jb < nvec; jb += 32) {
                        const int j = jb + l;
                        const bool act = j < nvec;
                        const float4 o = act ? *(const float4*)(a.own_cl + ((size_t)ni * HW + p) * a.CP + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                        for (int dd = 0; dd < 32; ++dd) {
                            if (dd < dcount) {
                                const int spk = __shfl(pk, dd, 32);
                                const float swx = __shfl(wx, dd, 32), swy = __shfl(wy, dd, 32);
                                if (act) {
                                    int x0, y0;
                                    cv_unpack(spk, x0, y0);
                                    const float4 s = cv_bilinear4(pbase + 4 * j, a.CP, a.h, a.w, x0, y0, swx, swy);
                                    acc[dd] += fmaf(o.w, s.w, fmaf(o.z, s.z, fmaf(o.y, s.y, o.x * s.x)));
                                }
                            }
                        }
                    }
                    cv_fold<16>(acc, l);
                    cv_fold<8>(acc, l);
                    cv_fold<4>(acc, l);
                    cv_fold<2>(acc, l);
                    cv_fold<1>(acc, l);
                    tot += acc[0];                            // lane l: depth dbase + l
                }
            }
            tile[l][pl] = tot * a.scale;
        }
        __syncthreads();
        for (int i = tid; i < 32 * CV_PX; i += S360_BLOCK) {
            const int dd = i / CV_PX, px = i - dd * CV_PX;
            if (dd < dcount && p0 + px < HW) out[((size_t)ni * a.D + dbase + dd) * HW + p0 + px] = tile[dd][px];
        }
        __syncthreads();
    }
}

// own side of the backward: g_own_cl[n, p, c] = scale * sum_pairing sum_d g[n, d, p] * bilinear(f_partner[slot, c], warp)
__global__ __launch_bounds__(S360_BLOCK) void k_cv_backward_own(CVArgs a, const float* __restrict__ g, float* __restrict__ g_own_cl) {
    const int tid = threadIdx.x, l = tid & 31, half = tid >> 5;
    const int HW = a.h * a.w;
    const int blocks_per_n = (HW + CV_PX - 1) / CV_PX;
    const int ni = blockIdx.x / blocks_per_n, p0 = (blockIdx.x - ni * blocks_per_n) * CV_PX;
    const int nvec = a.CP >> 2;
    for (int pass = 0; pass < CV_PASSES; ++pass) {
        const int p = p0 + pass * CV_HALVES + half;
        if (p >= HW) continue;
        double ray[3];
        cv_ray(p, a.h, a.w, ray);
        for (int jb = 0; jb < nvec; jb += 32) {
            const int j = jb + l;
            const bool act = j < nvec;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int pair = 0; pair < a.pairs; ++pair) {
                const int slot = a.slot ? a.slot[(size_t)pair * a.n + ni] : ni;
                if ((unsigned)slot >= (unsigned)a.m) continue;
                const float* pbase = a.partner_cl + (size_t)slot * HW * a.CP + 4 * j;
                for (int dbase = 0; dbase < a.D; dbase += 32) {
                    const int d = dbase + l;
                    const int dcount = min(32, a.D - dbase);
                    int pk = -1;
                    float wx = 0.f, wy = 0.f, gv = 0.f;
                    if (d < a.D) {
                        cv_sample(a.poses + ((size_t)pair * a.n + ni) * 16, ray, (double)a.depths[(size_t)ni * a.D + d], a.h, a.w, pk, wx, wy);
                        gv = g[((size_t)ni * a.D + d) * HW + p];
                    }
                    for (int dd = 0; dd < dcount; ++dd) {
                        const int spk = __shfl(pk, dd, 32);
                        const float swx = __shfl(wx, dd, 32), swy = __shfl(wy, dd, 32), sg = __shfl(gv, dd, 32);
                        if (act) {
                            int x0, y0;
                            cv_unpack(spk, x0, y0);
                            const float4 s = cv_bilinear4(pbase, a.CP, a.h, a.w, x0, y0, swx, swy);
                            acc.x = fmaf(sg, s.x, acc.x);
                            acc.y = fmaf(sg, s.y, acc.y);
                            acc.z = fmaf(sg, s.z, acc.z);
                            acc.w = fmaf(sg, s.w, acc.w);
                        }
                    }
                }
            }
            if (act)
                *(float4*)(g_own_cl + ((size_t)ni * HW + p) * a.CP + 4 * j) =
                    make_float4(acc.x * a.scale, acc.y * a.scale, acc.z * a.scale, acc.w * a.scale);
        }
    }
}

// the pending adds of one 2 x 2 tap cell, four channels per lane (c0, c0 + 32, c0 + 64, c0 + 96)
__device__ __forceinline__ void cv_flush(float* __restrict__ plane, int CP, int h, int w, int cell, int c0, float (&A)[4][4]) {
    if (cell == -1) return;
    int x0, y0;
    cv_unpack(cell, x0, y0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int xx = x0 + (t & 1), yy = y0 + (t >> 1);
        if ((unsigned)xx < (unsigned)w && (unsigned)yy < (unsigned)h) {
            float* dst = plane + ((size_t)yy * w + xx) * CP;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + 32 * k < CP) unsafeAtomicAdd(dst + c0 + 32 * k, A[t][k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) A[t][k] = 0.f;
    }
}

// partner side of the backward: g_partner_cl[slot, tap, c] += scale * g[n, d, p] * weight(tap) * f_own[n, c, p]   (atomics)
__global__ __launch_bounds__(S360_BLOCK) void k_cv_backward_partner(CVArgs a, const float* __restrict__ g, float* __restrict__ g_partner_cl) {
    const int tid = threadIdx.x, l = tid & 31, half = tid >> 5;
    const int HW = a.h * a.w;
    const int blocks_per_n = (HW + CV_PX - 1) / CV_PX;
    const int ni = blockIdx.x / blocks_per_n, p0 = (blockIdx.x - ni * blocks_per_n) * CV_PX;
    for (int pass = 0; pass < CV_PASSES; ++pass) {
        const int p = p0 + pass * CV_HALVES + half;
        if (p >= HW) continue;
        double ray[3];
        cv_ray(p, a.h, a.w, ray);
        for (int cb = 0; cb < a.CP; cb += 128) {
            const int c0 = cb + l;
            float own[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                own[k] = c0 + 32 * k < a.CP ? a.own_cl[((size_t)ni * HW + p) * a.CP + c0 + 32 * k] * a.scale : 0.f;
            for (int pair = 0; pair < a.pairs; ++pair) {
                const int slot = a.slot ? a.slot[(size_t)pair * a.n + ni] : ni;
                if ((unsigned)slot >= (unsigned)a.m) continue;
                float* plane = g_partner_cl + (size_t)slot * HW * a.CP;
                int cell = -1;
                float A[4][4];
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int k = 0; k < 4; ++k) A[t][k] = 0.f;
                for (int dbase = 0; dbase < a.D; dbase += 32) {
                    const int d = dbase + l;
                    const int dcount = min(32, a.D - dbase);
                    int pk = -1;
                    float wx = 0.f, wy = 0.f, gv = 0.f;
                    if (d < a.D) {
                        cv_sample(a.poses + ((size_t)pair * a.n + ni) * 16, ray, (double)a.depths[(size_t)ni * a.D + d], a.h, a.w, pk, wx, wy);
                        gv = g[((size_t)ni * a.D + d) * HW + p];
                    }
                    for (int dd = 0; dd < dcount; ++dd) {
                        const int spk = __shfl(pk, dd, 32);
                        const float swx = __shfl(wx, dd, 32), swy = __shfl(wy, dd, 32), sg = __shfl(gv, dd, 32);
                        if (spk == -1) continue;
                        if (spk != cell) {
                            cv_flush(plane, a.CP, a.h, a.w, cell, c0, A);
                            cell = spk;
                        }
                        const float wt[4] = {(1.f - swx) * (1.f - swy) * sg, swx * (1.f - swy) * sg, (1.f - swx) * swy * sg, swx * swy * sg};
#pragma unroll
                        for (int t = 0; t < 4; ++t)
#pragma unroll
                            for (int k = 0; k < 4; ++k) A[t][k] = fmaf(wt[t], own[k], A[t][k]);
                    }
                }
                cv_flush(plane, a.CP, a.h, a.w, cell, c0, A);
            }
        }
    }
}

// the drop-in's materialised warp: warped[n, c, d, y, x] = bilinear(f_partner[slot(n), c], warp(n, d, y, x)), NCHW in and out
__global__ __launch_bounds__(S360_BLOCK) void k_cv_warp(const float* __restrict__ f, const int32_t* __restrict__ slots, const float* __restrict__ poses,
                                                        const float* __restrict__ depths, int n, int m, int C, int h, int w, int D,
                                                        float* __restrict__ warped) {
    const int HW = h * w;
    const long long i = (long long)blockIdx.x * S360_BLOCK + threadIdx.x;
    if (i >= (long long)n * D * HW) return;
    const int p = (int)(i % HW), d = (int)((i / HW) % D), ni = (int)(i / ((long long)HW * D));
    const int slot = slots ? slots[ni] : ni;
    double ray[3];
    cv_ray(p, h, w, ray);
    int pk, x0, y0;
    float wx, wy;
    cv_sample(poses + (size_t)ni * 16, ray, (double)depths[(size_t)ni * D + d], h, w, pk, wx, wy);
    if ((unsigned)slot >= (unsigned)m) pk = -1;
    cv_unpack(pk, x0, y0);
    const bool xa = (unsigned)x0 < (unsigned)w, xb = (unsigned)(x0 + 1) < (unsigned)w;
    const bool ya = (unsigned)y0 < (unsigned)h, yb = (unsigned)(y0 + 1) < (unsigned)h;
    const float w00 = (1.f - wx) * (1.f - wy), w01 = wx * (1.f - wy), w10 = (1.f - wx) * wy, w11 = wx * wy;
    for (int c = 0; c < C; ++c) {
        const float* pl = f + ((size_t)(pk == -1 ? 0 : slot) * C + c) * HW;
        const float t00 = (xa && ya) ? pl[(size_t)y0 * w + x0] : 0.f;
        const float t01 = (xb && ya) ? pl[(size_t)y0 * w + x0 + 1] : 0.f;
        const float t10 = (xa && yb) ? pl[(size_t)(y0 + 1) * w + x0] : 0.f;
        const float t11 = (xb && yb) ? pl[(size_t)(y0 + 1) * w + x0 + 1] : 0.f;
        warped[(((size_t)ni * C + c) * D + d) * HW + p] = fmaf(w11, t11, fmaf(w10, t10, fmaf(w01, t01, w00 * t00)));
    }
}

}  // namespace s360

using namespace s360;

namespace {

struct CVPlan {
    int CP;
    size_t own_bytes, partner_bytes;      // the channels-last copies
    unsigned blocks;
};

int cv_setup(int32_t n, int32_t m, int32_t pairs, int32_t C, int32_t h, int32_t w, int32_t D, int32_t convention, CVPlan* pl) {
    if (n < 1 || m < 1 || pairs < 1 || C < 1 || h < 1 || w < 1 || D < 1 || convention != S360_CV_HM3D) return S360_E_BADARG;
    if (h > CV_MAX_SIDE || w > CV_MAX_SIDE || (long long)h * w > 0x3fffffffLL) return S360_E_BADARG;
    const long long HW = (long long)h * w, bpn = (HW + CV_PX - 1) / CV_PX;
    if (!s360_grid_fits(bpn * n) || (long long)n * D * HW > (long long)INT32_MAX * S360_BLOCK) return S360_E_BADARG;
    if ((HW + 63) / 64 > INT32_MAX || (C + 31) / 32 > 65535 || n > 65535 || m > 65535) return S360_E_BADARG;
    pl->CP = (C + 3) & ~3;
    pl->own_bytes = (size_t)n * HW * pl->CP * sizeof(float);
    pl->partner_bytes = (size_t)m * HW * pl->CP * sizeof(float);
    pl->blocks = (unsigned)(bpn * n);
    return S360_OK;
}

void cv_to_cl(const float* in, float* out, int S, int C, int CP, int HW, hipStream_t st) {
    hipLaunchKernelGGL(k_cv_to_cl, dim3((unsigned)((HW + 63) / 64), (unsigned)((CP + 31) / 32), (unsigned)S), dim3(S360_BLOCK), 0, st, in, out, C, CP, HW);
}

void cv_from_cl(const float* in, float* out, int S, int C, int CP, int HW, hipStream_t st) {
    hipLaunchKernelGGL(k_cv_from_cl, dim3((unsigned)((HW + 63) / 64), (unsigned)((C + 31) / 32), (unsigned)S), dim3(S360_BLOCK), 0, st, in, out, C, CP, HW);
}

}  // namespace

extern "C" int s360_cost_volume_forward(const float* f_own, const float* f_partner, const int32_t* partner_slot, const float* poses,
                                        const float* depths, int32_t n, int32_t m, int32_t pairs, int32_t C, int32_t h, int32_t w,
                                        int32_t D, int32_t convention, float scale, float* out, void* workspace,
                                        size_t* workspace_bytes, void* stream) {
    if (!workspace_bytes) return S360_E_BADARG;
    CVPlan pl;
    const int rc = cv_setup(n, m, pairs, C, h, w, D, convention, &pl);
    if (rc != S360_OK) return rc;
    const int ws = s360_workspace(workspace, workspace_bytes, pl.own_bytes + pl.partner_bytes, 16,
                                  f_own && f_partner && poses && depths && out && (partner_slot || m == n));
    if (ws != S360_WS_READY) return ws;
    const hipStream_t st = (hipStream_t)stream;
    const int HW = h * w;
    float* own_cl = (float*)workspace;
    float* partner_cl = (f_partner == f_own && m == n) ? own_cl : (float*)((char*)workspace + pl.own_bytes);
    cv_to_cl(f_own, own_cl, n, C, pl.CP, HW, st);
    if (partner_cl != own_cl) cv_to_cl(f_partner, partner_cl, m, C, pl.CP, HW, st);
    S360_CHECK_LAUNCH();
    const CVArgs a{own_cl, partner_cl, partner_slot, poses, depths, n, m, pairs, C, pl.CP, h, w, D, scale};
    hipLaunchKernelGGL(k_cv_forward, dim3(pl.blocks), dim3(S360_BLOCK), 0, st, a, out);
    return s360_launch_status();
}

extern "C" int s360_cost_volume_backward(const float* f_own, const float* f_partner, const int32_t* partner_slot, const float* poses,
                                         const float* depths, int32_t n, int32_t m, int32_t pairs, int32_t C, int32_t h, int32_t w,
                                         int32_t D, int32_t convention, float scale, const float* grad_out, float* grad_own,
                                         float* grad_partner, void* workspace, size_t* workspace_bytes, void* stream) {
    if (!workspace_bytes) return S360_E_BADARG;
    CVPlan pl;
    const int rc = cv_setup(n, m, pairs, C, h, w, D, convention, &pl);
    if (rc != S360_OK) return rc;
    const int wsr = s360_workspace(workspace, workspace_bytes, 2 * (pl.own_bytes + pl.partner_bytes), 16,
                                   f_own && f_partner && poses && depths && grad_out && grad_own && grad_partner && (partner_slot || m == n));
    if (wsr != S360_WS_READY) return wsr;
    const hipStream_t st = (hipStream_t)stream;
    const int HW = h * w;
    char* ws = (char*)workspace;
    float* own_cl = (float*)ws;
    float* partner_cl = (f_partner == f_own && m == n) ? own_cl : (float*)(ws + pl.own_bytes);
    float* g_own_cl = (float*)(ws + pl.own_bytes + pl.partner_bytes);
    float* g_partner_cl = (float*)(ws + 2 * pl.own_bytes + pl.partner_bytes);
    cv_to_cl(f_own, own_cl, n, C, pl.CP, HW, st);
    if (partner_cl != own_cl) cv_to_cl(f_partner, partner_cl, m, C, pl.CP, HW, st);
    if (hipMemsetAsync(g_partner_cl, 0, pl.partner_bytes, st) != hipSuccess) return S360_E_LAUNCH;
    S360_CHECK_LAUNCH();
    const CVArgs a{own_cl, partner_cl, partner_slot, poses, depths, n, m, pairs, C, pl.CP, h, w, D, scale};
    hipLaunchKernelGGL(k_cv_backward_own, dim3(pl.blocks), dim3(S360_BLOCK), 0, st, a, grad_out, g_own_cl);
    hipLaunchKernelGGL(k_cv_backward_partner, dim3(pl.blocks), dim3(S360_BLOCK), 0, st, a, grad_out, g_partner_cl);
    S360_CHECK_LAUNCH();
    cv_from_cl(g_own_cl, grad_own, n, C, pl.CP, HW, st);
    cv_from_cl(g_partner_cl, grad_partner, m, C, pl.CP, HW, st);
    return s360_launch_status();
}

extern "C" int s360_cost_volume_warp(const float* f_partner, const int32_t* partner_slot, const float* poses, const float* depths,
                                     int32_t n, int32_t m, int32_t C, int32_t h, int32_t w, int32_t D, int32_t convention,
                                     float* warped, void* stream) {
    CVPlan pl;
    const int rc = cv_setup(n, m, 1, C, h, w, D, convention, &pl);
    if (rc != S360_OK) return rc;
    if (!f_partner || !poses || !depths || !warped || (!partner_slot && m != n)) return S360_E_BADARG;
    const long long total = (long long)n * D * h * w;
    hipLaunchKernelGGL(k_cv_warp, dim3((unsigned)((total + S360_BLOCK - 1) / S360_BLOCK)), dim3(S360_BLOCK), 0, (hipStream_t)stream, f_partner,
                       partner_slot, poses, depths, (int)n, (int)m, (int)C, (int)h, (int)w, (int)D, warped);
    return s360_launch_status();
}
