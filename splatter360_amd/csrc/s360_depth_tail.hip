// s360_depth_tail.hip — the encoder's fine-depth and opacity tail: what the reference's predictor does between its depth head and
// its refinement U-Net (src/model/encoder/costvolume/depth_predictor_multiview_360.py:650-658), after that U-Net (:694-719), and
// the encoder's map_pdf_to_opacity (src/model/encoder/encoder_costvolume.py:228-241, :420), forward and backward.  gfx950 only.
//
//   upsample      one [n, 1, h, w] map to [n, 1, h s, w s]: nearest (source index Y / s) or bilinear with align_corners=True, whose
//                 source coordinate is exact in integers: t = Y (h - 1), y0 = t / (H - 1), weight (t % (H - 1)) / (H - 1), the
//                 upper neighbour clamped to h - 1 (up_tap).  `reciprocal` samples 1 / src.  The backward is the adjoint in gather
//                 form: a coarse texel walks the fine pixels whose footprint can hold it in ascending (Y, X) and weighs each with
//                 the same up_tap, so forward and adjoint cannot disagree on a tap; no atomics.
//   tail          per pixel and surface k < gpp:  fine = clamp(fullres + delta[k], lo, hi),  depth = 1 / fine, the sum unrounded;
//                 p = sigmoid(delta[gpp + k]),  opacity = (1 - (1 - p)^e + p^(1 / e)) / (2 gpp).  The three outputs are stored as
//                 [b, v, H W, 1, gpp] straight from the [(v b), ., H, W] inputs.  The backward is elementwise from the inputs alone:
//                 -g_depth / fine^2 where lo <= float32(fullres + delta[k]) <= hi — bounds included, and decided on the float32
//                 sum, so the pattern of zeros is torch's element for element — and for the logit x
//                     d opacity / d x = (e (1 - p)^e p + (1 / e) p^(1 / e) (1 - p)) / (2 gpp),
//                 which is finite for every finite x: log p = -softplus(-x) and log(1 - p) = -softplus(x) are formed directly,
//                 so a sigmoid that float32 would round to 0 or 1 never meets an infinite derivative of pow.
//   opacity map   map_pdf_to_opacity on a flat array of probabilities, derivative in p: mirrors the reference, infinities included.
//   arithmetic    float64, one rounding to float32 per output (only the backward's inside / outside decision uses a float32 sum).
//                 Fixed order, no atomics, every element written: bit-identical from run to run and stream to stream.
//   memory        lanes run along x; float4 loads and stores where a row (upsample) or a plane (tail) is a multiple of 4 floats
//                 and the pointers are 16-byte aligned, scalar kernels otherwise; the flat opacity map takes float4 for its body
//                 and scalars for the ragged end.  With gpp > 1 the tail's channel-last stores are scalar.
#include "s360_device.h"

#include <math.h>

namespace s360 {

constexpr int UP_NEAREST = 0, UP_BILINEAR = 1;

// the two source taps of fine index Y and the weight of the upper one.  nearest: one tap, weight 0
__device__ __forceinline__ void up_tap(int mode, int Y, int h, int H, int s, int& y0, int& y1, double& wy) {
    if (mode == UP_NEAREST) {
        y0 = y1 = Y / s;
        wy = 0.0;
        return;
    }
    if (H == 1) {
        y0 = y1 = 0;
        wy = 0.0;
        return;
    }
    const long long t = (long long)Y * (h - 1);
    const int d = H - 1;
    int r;
    if (t <= INT32_MAX) {                                     // the usual case: one 32-bit division
        y0 = (int)t / d;
        r = (int)t % d;
    } else {
        y0 = (int)(t / d);
        r = (int)(t % d);
    }
    y1 = min(y0 + 1, h - 1);
    wy = (double)r / (double)d;
}

// the weight of coarse index y in fine index Y: the forward's taps, read the other way
__device__ __forceinline__ double up_weight(int mode, int Y, int y, int h, int H, int s) {
    int y0, y1;
    double wy;
    up_tap(mode, Y, h, H, s, y0, y1, wy);
    return (y0 == y ? 1.0 - wy : 0.0) + (y1 == y ? wy : 0.0);
}

// the fine indices [lo, hi] whose taps can include coarse index y (a superset is harmless: up_weight gives 0 outside)
__device__ __forceinline__ void up_range(int mode, int y, int h, int H, int s, int& lo, int& hi) {
    if (mode == UP_NEAREST) {
        lo = y * s;
        hi = lo + s - 1;
    } else if (h == 1) {
        lo = 0;
        hi = H - 1;
    } else {                                                  // y0 in {y - 1, y}: (y - 1)(H - 1) <= Y (h - 1) < (y + 1)(H - 1)
        const long long d = h - 1, a = (long long)(y - 1) * (H - 1), b = (long long)(y + 1) * (H - 1);
        lo = a <= 0 ? 0 : (int)((a + d - 1) / d);
        hi = (int)min((long long)(H - 1), (b + d - 1) / d - 1);
    }
}

template <int V>
__global__ __launch_bounds__(S360_BLOCK) void k_up_forward(const float* __restrict__ src, float* __restrict__ dst, int h, int w, int s,
                                                           int mode, int reciprocal) {
    const int H = h * s, W = w * s, Wv = W / V;               // V == 4: W % 4 == 0
    const long long t = (long long)blockIdx.x * S360_BLOCK + threadIdx.x;
    if (t >= (long long)H * Wv) return;
    const int Y = (int)(t / Wv), X0 = (int)(t % Wv) * V;
    const float* __restrict__ in = src + (size_t)blockIdx.y * h * w;
    int y0, y1;
    double wy;
    up_tap(mode, Y, h, H, s, y0, y1, wy);
    const float* __restrict__ r0 = in + (size_t)y0 * w;
    const float* __restrict__ r1 = in + (size_t)y1 * w;
    float o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        int x0, x1;
        double wx;
        up_tap(mode, X0 + j, w, W, s, x0, x1, wx);
        if (mode == UP_NEAREST) {
            o[j] = reciprocal ? (float)(1.0 / (double)r0[x0]) : r0[x0];
        } else {
            double v00 = r0[x0], v01 = r0[x1], v10 = r1[x0], v11 = r1[x1];
            if (reciprocal) v00 = 1.0 / v00, v01 = 1.0 / v01, v10 = 1.0 / v10, v11 = 1.0 / v11;
            o[j] = (float)((1.0 - wy) * ((1.0 - wx) * v00 + wx * v01) + wy * ((1.0 - wx) * v10 + wx * v11));
        }
    }
    float* out = dst + (size_t)blockIdx.y * H * W + (size_t)Y * W + X0;
    if constexpr (V == 4) *(float4*)out = make_float4(o[0], o[1], o[2], o[3]);
    else *out = o[0];
}

// one coarse texel per thread: g_src[y, x] = sum over (Y, X) ascending of weight(Y, y) weight(X, x) g_dst[Y, X]
__global__ __launch_bounds__(S360_BLOCK) void k_up_backward(const float* __restrict__ g_dst, const float* __restrict__ src,
                                                            float* __restrict__ g_src, int h, int w, int s, int mode, int reciprocal) {
    const int H = h * s, W = w * s;
    const long long t = (long long)blockIdx.x * S360_BLOCK + threadIdx.x;
    if (t >= (long long)h * w) return;
    const int y = (int)(t / w), x = (int)(t % w);
    const float* __restrict__ g = g_dst + (size_t)blockIdx.y * H * W;
    int Ylo, Yhi, Xlo, Xhi;
    up_range(mode, y, h, H, s, Ylo, Yhi);
    up_range(mode, x, w, W, s, Xlo, Xhi);
    double acc = 0.0;
    for (int Y = Ylo; Y <= Yhi; ++Y) {
        const double cy = up_weight(mode, Y, y, h, H, s);
        if (cy == 0.0) continue;
        const float* __restrict__ row = g + (size_t)Y * W;
        for (int X = Xlo; X <= Xhi; ++X) {
            const double cx = up_weight(mode, X, x, w, W, s);
            if (cx != 0.0) acc += cy * cx * (double)row[X];
        }
    }
    const size_t o = (size_t)blockIdx.y * h * w + (size_t)t;
    if (reciprocal) {
        const double v = (double)src[o];
        acc *= -1.0 / (v * v);
    }
    g_src[o] = (float)acc;
}

// V pixels per lane: 4 (float4; P % 4 == 0 and 16-byte aligned pointers) or 1
template <int V>
__device__ __forceinline__ void dt_load(const float* __restrict__ src, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 x = *(const float4*)src;
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    } else {
        v[0] = *src;
    }
}

template <int V>
__device__ __forceinline__ void dt_store(float* __restrict__ dst, const float (&v)[V]) {
    if constexpr (V == 4) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    else *dst = v[0];
}

__device__ __forceinline__ double dt_softplus(double t) { return t > 0.0 ? t + log1p(exp(-t)) : log1p(exp(t)); }

// clamp(sum, lo, hi) of the unrounded sum, as torch orders it (min(max(sum, lo), hi): NaN stays NaN)
__device__ __forceinline__ double dt_fine(double sum, float lo, float hi) {
    const double a = sum < (double)lo ? (double)lo : sum;
    return a > (double)hi ? (double)hi : a;
}

// of the logit x: p = sigmoid, A = (1 - p)^e, B = p^(1 / e), opacity = (1 - A + B) / (2 gpp), and its derivative in x
struct DtOpacity {
    double p, q, opacity, slope;
};

__device__ __forceinline__ DtOpacity dt_opacity(double x, double e, double inv_2g) {
    const double lp = -dt_softplus(-x), lq = -dt_softplus(x);        // log p, log(1 - p): finite for finite x
    DtOpacity r;
    r.p = exp(lp);
    r.q = exp(lq);
    const double B = exp(lp / e);
    r.opacity = (B - expm1(e * lq)) * inv_2g;                        // 1 - A without the cancellation
    r.slope = (e * exp(e * lq) * r.p + B * r.q / e) * inv_2g;
    return r;
}

// the [b, v, P, 1, gpp] element of (ni = vi b + bi, pixel p, surface k)
__device__ __forceinline__ size_t dt_out_index(int ni, int b, int v, int P, int gpp, long long p, int k) {
    const int vi = ni / b, bi = ni % b;
    return (((size_t)bi * v + vi) * P + (size_t)p) * gpp + k;
}

template <int V>
__global__ __launch_bounds__(S360_BLOCK) void k_dt_forward(const float* __restrict__ fullres, const float* __restrict__ dd,
                                                           const float* __restrict__ lo, const float* __restrict__ hi, double e, int gpp,
                                                           int v, int b, int P, float* __restrict__ depths, float* __restrict__ opacities,
                                                           float* __restrict__ densities) {
    const int ni = blockIdx.y;
    const long long p = ((long long)blockIdx.x * S360_BLOCK + threadIdx.x) * V;
    if (p >= P) return;                                       // V == 4: P % 4 == 0, so the lane's four pixels are all inside
    const float l = lo[ni], u = hi[ni];
    const double inv_2g = 0.5 / (double)gpp;
    float f[V];
    dt_load<V>(fullres + (size_t)ni * P + p, f);
    const float* __restrict__ plane = dd + (size_t)ni * 2 * gpp * P + p;
    for (int k = 0; k < gpp; ++k) {
        float d[V], x[V], od[V], oo[V], os[V];
        dt_load<V>(plane + (size_t)k * P, d);
        dt_load<V>(plane + (size_t)(gpp + k) * P, x);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            od[j] = (float)(1.0 / dt_fine((double)f[j] + (double)d[j], l, u));
            const DtOpacity r = dt_opacity((double)x[j], e, inv_2g);
            oo[j] = (float)r.opacity;
            os[j] = (float)r.p;
        }
        const size_t o = dt_out_index(ni, b, v, P, gpp, p, k);
        if (gpp == 1) {
            dt_store<V>(depths + o, od);
            dt_store<V>(opacities + o, oo);
            if (densities) dt_store<V>(densities + o, os);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                depths[o + (size_t)j * gpp] = od[j];
                opacities[o + (size_t)j * gpp] = oo[j];
                if (densities) densities[o + (size_t)j * gpp] = os[j];
            }
        }
    }
}

template <int V>
__device__ __forceinline__ void dt_load_out(const float* __restrict__ g, size_t o, int gpp, float (&v)[V]) {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = 0.f;
    if (!g) return;
    if (gpp == 1) {
        dt_load<V>(g + o, v);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = g[o + (size_t)j * gpp];
    }
}

template <int V>
__global__ __launch_bounds__(S360_BLOCK) void k_dt_backward(const float* __restrict__ g_depths, const float* __restrict__ g_opacities,
                                                            const float* __restrict__ g_densities, const float* __restrict__ fullres,
                                                            const float* __restrict__ dd, const float* __restrict__ lo,
                                                            const float* __restrict__ hi, double e, int gpp, int v, int b, int P,
                                                            float* __restrict__ g_fullres, float* __restrict__ g_dd) {
    const int ni = blockIdx.y;
    const long long p = ((long long)blockIdx.x * S360_BLOCK + threadIdx.x) * V;
    if (p >= P) return;
    const float l = lo[ni], u = hi[ni];
    const double inv_2g = 0.5 / (double)gpp;
    float f[V];
    dt_load<V>(fullres + (size_t)ni * P + p, f);
    const size_t po = (size_t)ni * 2 * gpp * P + p;
    double gf[V];
#pragma unroll
    for (int j = 0; j < V; ++j) gf[j] = 0.0;
    for (int k = 0; k < gpp; ++k) {                           // g_fullres sums the surfaces in this order
        float d[V], x[V], gd[V], go[V], gs[V], od[V], ox[V];
        dt_load<V>(dd + po + (size_t)k * P, d);
        dt_load<V>(dd + po + (size_t)(gpp + k) * P, x);
        const size_t o = dt_out_index(ni, b, v, P, gpp, p, k);
        dt_load_out<V>(g_depths, o, gpp, gd);
        dt_load_out<V>(g_opacities, o, gpp, go);
        dt_load_out<V>(g_densities, o, gpp, gs);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float sum = f[j] + d[j];                    // torch's own float32 sum decides, bounds included
            double g = 0.0;
            if (sum >= l && sum <= u) {
                const double fine = dt_fine((double)f[j] + (double)d[j], l, u);
                g = -(double)gd[j] / (fine * fine);
            }
            gf[j] += g;
            od[j] = (float)g;
            const DtOpacity r = dt_opacity((double)x[j], e, inv_2g);
            ox[j] = (float)((double)go[j] * r.slope + (double)gs[j] * (r.p * r.q));
        }
        dt_store<V>(g_dd + po + (size_t)k * P, od);
        dt_store<V>(g_dd + po + (size_t)(gpp + k) * P, ox);
    }
    float of[V];
#pragma unroll
    for (int j = 0; j < V; ++j) of[j] = (float)gf[j];
    dt_store<V>(g_fullres + (size_t)ni * P + p, of);
}

__device__ __forceinline__ float om_value(float pf, double e) {
    const double p = (double)pf;
    return (float)(0.5 * (1.0 - pow(1.0 - p, e) + pow(p, 1.0 / e)));
}

__device__ __forceinline__ float om_gradient(float pf, float g, double e) {
    const double p = (double)pf;
    return (float)((double)g * (0.5 * (e * pow(1.0 - p, e - 1.0) + pow(p, 1.0 / e - 1.0) / e)));
}

// four elements per thread: float4 for the body (vec: 16-byte aligned pointers), scalars for the ragged end
template <bool BWD>
__global__ __launch_bounds__(S360_BLOCK) void k_opacity_map(const float* __restrict__ pdf, const float* __restrict__ g_out,
                                                            float* __restrict__ out, long long count, double e, int vec) {
    const long long i = ((long long)blockIdx.x * S360_BLOCK + threadIdx.x) * 4;
    if (i >= count) return;
    if (vec && i + 4 <= count) {
        float p[4], g[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        dt_load<4>(pdf + i, p);
        if constexpr (BWD) dt_load<4>(g_out + i, g);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = BWD ? om_gradient(p[j], g[j], e) : om_value(p[j], e);
        dt_store<4>(out + i, o);
    } else {
        for (long long k = i; k < min(i + 4, count); ++k) out[k] = BWD ? om_gradient(pdf[k], g_out[k], e) : om_value(pdf[k], e);
    }
}

}  // namespace s360

using namespace s360;

namespace {

bool dt_exponent_ok(float e) { return isfinite(e) && e > 0.f; }

bool up_sizes_ok(int32_t n, int32_t h, int32_t w, int32_t s, int32_t mode) {
    return n >= 1 && h >= 1 && w >= 1 && s >= 1 && n <= 65535 && (mode == UP_NEAREST || mode == UP_BILINEAR) &&
           (long long)h * s <= 0x3fffffffLL && (long long)w * s <= 0x3fffffffLL && (long long)h * s * w * s <= 0x3fffffffLL;
}

bool dt_sizes_ok(int32_t n, int32_t H, int32_t W, int32_t gpp, int32_t v) {
    return n >= 1 && H >= 1 && W >= 1 && gpp >= 1 && v >= 1 && n % v == 0 && n <= 65535 && gpp <= 65535 && (long long)H * W <= 0x3fffffffLL;
}

unsigned dt_blocks(long long threads) { return (unsigned)((threads + S360_BLOCK - 1) / S360_BLOCK); }

}  // namespace

extern "C" int s360_upsample_forward(const float* src, float* dst, int32_t n, int32_t h, int32_t w, int32_t s, int32_t mode,
                                     int32_t reciprocal, void* stream) {
    if (!src || !dst || !up_sizes_ok(n, h, w, s, mode)) return S360_E_BADARG;
    const long long H = (long long)h * s, W = (long long)w * s;
    const hipStream_t st = (hipStream_t)stream;
    if (W % 4 == 0 && s360_aligned(dst, 16))                  // H W % 4 == 0 then: every image's rows stay aligned
        hipLaunchKernelGGL(k_up_forward<4>, dim3(dt_blocks(H * (W / 4)), (unsigned)n), dim3(S360_BLOCK), 0, st, src, dst, (int)h, (int)w,
                           (int)s, (int)mode, (int)(reciprocal != 0));
    else
        hipLaunchKernelGGL(k_up_forward<1>, dim3(dt_blocks(H * W), (unsigned)n), dim3(S360_BLOCK), 0, st, src, dst, (int)h, (int)w, (int)s,
                           (int)mode, (int)(reciprocal != 0));
    return s360_launch_status();
}

extern "C" int s360_upsample_backward(const float* g_dst, const float* src, float* g_src, int32_t n, int32_t h, int32_t w, int32_t s,
                                      int32_t mode, int32_t reciprocal, void* stream) {
    if (!g_dst || !g_src || (reciprocal && !src) || !up_sizes_ok(n, h, w, s, mode)) return S360_E_BADARG;
    hipLaunchKernelGGL(k_up_backward, dim3(dt_blocks((long long)h * w), (unsigned)n), dim3(S360_BLOCK), 0, (hipStream_t)stream, g_dst, src,
                       g_src, (int)h, (int)w, (int)s, (int)mode, (int)(reciprocal != 0));
    return s360_launch_status();
}

extern "C" int s360_depth_tail_forward(const float* fullres_disps, const float* delta_density, const float* lo, const float* hi,
                                       float exponent, int32_t gpp, int32_t v, float* depths_out, float* opacities_out,
                                       float* densities_out, int32_t n, int32_t H, int32_t W, void* stream) {
    if (!fullres_disps || !delta_density || !lo || !hi || !depths_out || !opacities_out || !dt_sizes_ok(n, H, W, gpp, v) ||
        !dt_exponent_ok(exponent))
        return S360_E_BADARG;
    const int P = H * W, b = n / v;
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = P % 4 == 0 && s360_aligned(fullres_disps, 16) && s360_aligned(delta_density, 16) && s360_aligned(depths_out, 16) &&
                     s360_aligned(opacities_out, 16) && s360_aligned(densities_out, 16);
    if (vec)
        hipLaunchKernelGGL(k_dt_forward<4>, dim3(dt_blocks(P / 4), (unsigned)n), dim3(S360_BLOCK), 0, st, fullres_disps, delta_density, lo, hi,
                           (double)exponent, (int)gpp, (int)v, b, P, depths_out, opacities_out, densities_out);
    else
        hipLaunchKernelGGL(k_dt_forward<1>, dim3(dt_blocks(P), (unsigned)n), dim3(S360_BLOCK), 0, st, fullres_disps, delta_density, lo, hi,
                           (double)exponent, (int)gpp, (int)v, b, P, depths_out, opacities_out, densities_out);
    return s360_launch_status();
}

extern "C" int s360_depth_tail_backward(const float* g_depths, const float* g_opacities, const float* g_densities,
                                        const float* fullres_disps, const float* delta_density, const float* lo, const float* hi,
                                        float exponent, int32_t gpp, int32_t v, float* g_fullres_disps, float* g_delta_density, int32_t n,
                                        int32_t H, int32_t W, void* stream) {
    if (!fullres_disps || !delta_density || !lo || !hi || !g_fullres_disps || !g_delta_density || !dt_sizes_ok(n, H, W, gpp, v) ||
        !dt_exponent_ok(exponent))
        return S360_E_BADARG;
    const int P = H * W, b = n / v;
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = P % 4 == 0 && s360_aligned(fullres_disps, 16) && s360_aligned(delta_density, 16) && s360_aligned(g_depths, 16) &&
                     s360_aligned(g_opacities, 16) && s360_aligned(g_densities, 16) && s360_aligned(g_fullres_disps, 16) && s360_aligned(g_delta_density, 16);
    if (vec)
        hipLaunchKernelGGL(k_dt_backward<4>, dim3(dt_blocks(P / 4), (unsigned)n), dim3(S360_BLOCK), 0, st, g_depths, g_opacities, g_densities,
                           fullres_disps, delta_density, lo, hi, (double)exponent, (int)gpp, (int)v, b, P, g_fullres_disps, g_delta_density);
    else
        hipLaunchKernelGGL(k_dt_backward<1>, dim3(dt_blocks(P), (unsigned)n), dim3(S360_BLOCK), 0, st, g_depths, g_opacities, g_densities,
                           fullres_disps, delta_density, lo, hi, (double)exponent, (int)gpp, (int)v, b, P, g_fullres_disps, g_delta_density);
    return s360_launch_status();
}

extern "C" int s360_opacity_map_forward(const float* pdf, float* out, size_t count, float exponent, void* stream) {
    if (!pdf || !out || count < 1 || count > (size_t)0x3fffffffffLL || !dt_exponent_ok(exponent)) return S360_E_BADARG;
    hipLaunchKernelGGL(k_opacity_map<false>, dim3(dt_blocks((count + 3) / 4)), dim3(S360_BLOCK), 0, (hipStream_t)stream, pdf,
                       (const float*)nullptr, out, (long long)count, (double)exponent, (int)(s360_aligned(pdf, 16) && s360_aligned(out, 16)));
    return s360_launch_status();
}

extern "C" int s360_opacity_map_backward(const float* pdf, const float* g_out, float* g_pdf, size_t count, float exponent, void* stream) {
    if (!pdf || !g_out || !g_pdf || count < 1 || count > (size_t)0x3fffffffffLL || !dt_exponent_ok(exponent)) return S360_E_BADARG;
    hipLaunchKernelGGL(k_opacity_map<true>, dim3(dt_blocks((count + 3) / 4)), dim3(S360_BLOCK), 0, (hipStream_t)stream, pdf, g_out, g_pdf,
                       (long long)count, (double)exponent, (int)(s360_aligned(pdf, 16) && s360_aligned(g_out, 16) && s360_aligned(g_pdf, 16)));
    return s360_launch_status();
}
