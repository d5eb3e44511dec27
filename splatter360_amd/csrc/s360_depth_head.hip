// s360_depth_head.hip — the encoder's softmax depth head (the reference's
// src/model/encoder/costvolume/depth_predictor_multiview_360.py:643-651), forward and backward, without the [n, D, h, w] softmax.
// gfx950 only.
//
//   pdf = softmax(logits, dim = 1);  depth[n, p] = sum_d c[n, d] pdf[n, d, p];  pmax[n, p] = max_d pdf[n, d, p]
//
//   layout        logits are [n, D, P] with P = h w contiguous: lanes run along p, so one depth step of a wave is one contiguous
//                 256-byte read (1 KiB in the backward's float4 form).  A block owns 64 (or 256) pixels of one n and all of D;
//                 its four waves take the depths d = wave, wave + 4, ... and meet once in LDS.
//   forward       one read of the logits.  Every wave keeps (m, a, s, t) per lane — the running maximum, the first depth that
//                 attains it, sum exp(z - m) and sum c exp(z - m) — loading DH_UNROLL depths at a time, moving m at most once per
//                 group (s and t are rescaled by exp(m_old - m_new)) and adding the group's terms.  The four partials are merged
//                 by wave 0 in the fixed order 0, 1, 2, 3: the larger m wins, on equal m the lower a, and the loser's sums are
//                 scaled by exp(m_loser - m_winner).  depth = t / s, pmax = 1 / s (= exp(z_a - m) / s), lse = m + log s.
//   backward      g_z[d] = p_d (g_depth (c_d - depth) - g_pmax pmax) + [d == a] g_pmax pmax with p_d = exp(z_d - lse), evaluated
//                 from the saved float32 lse, depth and argmax.  A float32 lse carries half an ulp of |lse| as a RELATIVE error of
//                 every p_d (3.8e-6 at |z| = 75, sixty times float32's own rounding), and a float32 depth the like for c_d - depth,
//                 so the kernel first measures what the saved scalars are off by, in one more pass over the block's logits
//                 (which the second pass then finds in cache):  q = sum_d e_d with e_d = exp(z_d - lse)  (1 for an exact lse),
//                 r = sum_d (c_d - depth) e_d / q  (0 for an exact depth), pmax = e_a / q, and then writes
//                     g_z[d] = (e_d / q) (g_depth ((c_d - depth) - r) - g_pmax pmax) + [d == a] g_pmax pmax.
//                 lse only has to keep the exponents small and depth to centre the candidates; what is left of their rounding
//                 is second order.  Elementwise writes of every element: no memset, no atomics.
//   arithmetic    exp, the sums and the quotients in float64, one rounding to float32 per output: a logit costs 4 bytes of HBM,
//                 so the kernels stay bandwidth-bound.  Fixed order throughout: bit-identical from run to run and stream to
//                 stream.  Finite logits of any size give finite results (the maximum, or lse, is subtracted first); non-finite
//                 logits give unspecified values, but argmax stays inside [0, D).
#include "s360_device.h"

#include <math.h>

namespace s360 {

constexpr int DH_WAVES = S360_BLOCK / 64;                     // the split of D
constexpr int DH_UNROLL = 8;                                  // depths a wave has in flight
constexpr int DH_NONE = 0x7fffffff;                           // the argmax of a partial that saw no depth

// (m, a, s, t) <- merge with (m2, a2, s2, t2): one exp, the winner's sums are taken as they are
__device__ __forceinline__ void dh_merge(float& m, int& a, double& s, double& t, float m2, int a2, double s2, double t2) {
    if (m2 > m || (m2 == m && a2 < a)) {
        const double r = exp((double)m - (double)m2);
        s = s * r + s2;
        t = t * r + t2;
        m = m2;
        a = a2;
    } else {
        const double r = exp((double)m2 - (double)m);
        s += s2 * r;
        t += t2 * r;
    }
}

__global__ __launch_bounds__(S360_BLOCK) void k_dh_forward(const float* __restrict__ logits, const float* __restrict__ cand, int D, int P,
                                                           float* __restrict__ depth, float* __restrict__ pmax, float* __restrict__ lse,
                                                           int32_t* __restrict__ argmax) {
    __shared__ float sh_m[DH_WAVES][64];
    __shared__ int sh_a[DH_WAVES][64];
    __shared__ double sh_s[DH_WAVES][64], sh_t[DH_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ni = blockIdx.y, p = blockIdx.x * 64 + lane;
    const bool live = p < P;
    const float* __restrict__ z = logits + (size_t)ni * D * P + (live ? p : 0);
    const float* __restrict__ c = cand + (size_t)ni * D;
    float m = -INFINITY;
    int a = wv == 0 ? 0 : DH_NONE;
    double s = 0.0, t = 0.0;
    for (int d0 = wv; d0 < D; d0 += DH_WAVES * DH_UNROLL) {
        float v[DH_UNROLL];
#pragma unroll
        for (int u = 0; u < DH_UNROLL; ++u) {
            const int d = d0 + u * DH_WAVES;
            v[u] = (live && d < D) ? z[(size_t)d * P] : -INFINITY;
        }
        float gm = m;
        int ga = a;
#pragma unroll
        for (int u = 0; u < DH_UNROLL; ++u)
            if (v[u] > gm) {                                  // strictly: the first depth keeps a tie; never true for NaN
                gm = v[u];
                ga = d0 + u * DH_WAVES;
            }
        if (gm > m) {
            const double r = exp((double)m - (double)gm);     // m = -inf on the first group: 0, and s = t = 0 stay 0
            s *= r;
            t *= r;
            m = gm;
            a = ga;
        }
#pragma unroll
        for (int u = 0; u < DH_UNROLL; ++u) {
            const int d = d0 + u * DH_WAVES;
            if (d < D) {                                      // uniform over the wave
                const double e = exp((double)v[u] - (double)m);
                s += e;
                t += (double)c[d] * e;
            }
        }
    }
    sh_m[wv][lane] = m;
    sh_a[wv][lane] = a;
    sh_s[wv][lane] = s;
    sh_t[wv][lane] = t;
    __syncthreads();
    if (wv != 0 || !live) return;
#pragma unroll
    for (int k = 1; k < DH_WAVES; ++k) dh_merge(m, a, s, t, sh_m[k][lane], sh_a[k][lane], sh_s[k][lane], sh_t[k][lane]);
    const size_t o = (size_t)ni * P + p;
    depth[o] = (float)(t / s);
    pmax[o] = (float)(1.0 / s);
    lse[o] = (float)((double)m + log(s));
    argmax[o] = min(max(a, 0), D - 1);
}

// V pixels per lane: 4 (float4 loads and stores; P % 4 == 0 and 16-byte aligned pointers) or 1
template <int V>
__device__ __forceinline__ void dh_load(const float* __restrict__ src, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 x = *(const float4*)src;
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    } else {
        v[0] = *src;
    }
}

template <int V>
__global__ __launch_bounds__(S360_BLOCK) void k_dh_backward(const float* __restrict__ logits, const float* __restrict__ cand,
                                                            const float* __restrict__ lse, const float* __restrict__ depth,
                                                            const int32_t* __restrict__ argmax, const float* __restrict__ g_depth,
                                                            const float* __restrict__ g_pmax, int D, int P, float* __restrict__ g_logits) {
    __shared__ double sh_q[DH_WAVES][64 * V], sh_r[DH_WAVES][64 * V], sh_e[DH_WAVES][64 * V];
    constexpr int U = V == 4 ? 2 : DH_UNROLL;                 // depths in flight: 2 x 16 bytes or 8 x 4 bytes per lane
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ni = blockIdx.y;
    const long long p = ((long long)blockIdx.x * 64 + lane) * V;
    const bool live = p < P;                                  // V == 4: P % 4 == 0, so the lane's four pixels are all inside
    const size_t o = (size_t)ni * P + (live ? p : 0);
    const size_t zo = (size_t)ni * D * P + (live ? p : 0);
    const float* __restrict__ c = cand + (size_t)ni * D;
    float L[V], dep[V], gd[V], gp[V];
    int a[V];
#pragma unroll
    for (int j = 0; j < V; ++j) L[j] = dep[j] = gd[j] = gp[j] = 0.f, a[j] = -1;
    if (live) {
        dh_load<V>(lse + o, L);
        dh_load<V>(depth + o, dep);
        if (g_depth) dh_load<V>(g_depth + o, gd);
        if (g_pmax) dh_load<V>(g_pmax + o, gp);
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = argmax[o + j];
    }
    double q[V], r[V], ea[V];
#pragma unroll
    for (int j = 0; j < V; ++j) q[j] = r[j] = ea[j] = 0.0;
    for (int d0 = wv; d0 < D; d0 += DH_WAVES * U) {
        float v[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int d = d0 + u * DH_WAVES;
#pragma unroll
            for (int j = 0; j < V; ++j) v[u][j] = 0.f;
            if (live && d < D) dh_load<V>(logits + zo + (size_t)d * P, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int d = d0 + u * DH_WAVES;
            if (d < D) {
                const double cd = (double)c[d];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const double e = exp((double)v[u][j] - (double)L[j]);
                    q[j] += e;
                    r[j] += (cd - (double)dep[j]) * e;
                    if (d == a[j]) ea[j] = e;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        sh_q[wv][lane * V + j] = q[j];
        sh_r[wv][lane * V + j] = r[j];
        sh_e[wv][lane * V + j] = ea[j];
    }
    __syncthreads();
    double w[V], rr[V], A[V];                                 // 1 / q, r / q, g_pmax pmax: every wave forms the same values
#pragma unroll
    for (int j = 0; j < V; ++j) {
        double qs = 0.0, rs = 0.0, es = 0.0;
#pragma unroll
        for (int k = 0; k < DH_WAVES; ++k) {
            qs += sh_q[k][lane * V + j];
            rs += sh_r[k][lane * V + j];
            es += sh_e[k][lane * V + j];
        }
        w[j] = 1.0 / qs;
        rr[j] = rs * w[j];
        A[j] = (double)gp[j] * (es * w[j]);
    }
    if (!live) return;
    for (int d0 = wv; d0 < D; d0 += DH_WAVES * U) {
        float v[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int d = d0 + u * DH_WAVES;
#pragma unroll
            for (int j = 0; j < V; ++j) v[u][j] = 0.f;
            if (d < D) dh_load<V>(logits + zo + (size_t)d * P, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int d = d0 + u * DH_WAVES;
            if (d < D) {
                const double cd = (double)c[d];
                float g[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const double pd = exp((double)v[u][j] - (double)L[j]) * w[j];
                    const double x = pd * ((double)gd[j] * ((cd - (double)dep[j]) - rr[j]) - A[j]);
                    g[j] = (float)(d == a[j] ? x + A[j] : x);
                }
                float* dst = g_logits + zo + (size_t)d * P;
                if constexpr (V == 4) *(float4*)dst = make_float4(g[0], g[1], g[2], g[3]);
                else *dst = g[0];
            }
        }
    }
}

}  // namespace s360

using namespace s360;

namespace {

bool dh_sizes_ok(int32_t n, int32_t d, int32_t h, int32_t w) {
    return n >= 1 && d >= 1 && h >= 1 && w >= 1 && n <= 65535 && (long long)h * w <= 0x3fffffffLL;
}

}  // namespace

extern "C" int s360_depth_head_forward(const float* logits, const float* candidates, int32_t n, int32_t d, int32_t h, int32_t w,
                                       float* depth, float* pmax, float* lse, int32_t* argmax, void* stream) {
    if (!logits || !candidates || !depth || !pmax || !lse || !argmax || !dh_sizes_ok(n, d, h, w)) return S360_E_BADARG;
    const int P = h * w;
    hipLaunchKernelGGL(k_dh_forward, dim3((unsigned)((P + 63) / 64), (unsigned)n), dim3(S360_BLOCK), 0, (hipStream_t)stream, logits,
                       candidates, (int)d, P, depth, pmax, lse, argmax);
    return s360_launch_status();
}

extern "C" int s360_depth_head_backward(const float* logits, const float* candidates, const float* lse, const float* depth,
                                        const int32_t* argmax, const float* g_depth, const float* g_pmax, int32_t n, int32_t d, int32_t h,
                                        int32_t w, float* g_logits, void* stream) {
    if (!logits || !candidates || !lse || !depth || !argmax || !g_logits || !dh_sizes_ok(n, d, h, w)) return S360_E_BADARG;
    const int P = h * w;
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = P % 4 == 0 && s360_aligned(logits, 16) && s360_aligned(lse, 16) && s360_aligned(depth, 16) && s360_aligned(g_depth, 16) &&
                     s360_aligned(g_pmax, 16) && s360_aligned(g_logits, 16);
    if (vec)
        hipLaunchKernelGGL(k_dh_backward<4>, dim3((unsigned)((P + 255) / 256), (unsigned)n), dim3(S360_BLOCK), 0, st, logits, candidates, lse,
                           depth, argmax, g_depth, g_pmax, (int)d, P, g_logits);
    else
        hipLaunchKernelGGL(k_dh_backward<1>, dim3((unsigned)((P + 63) / 64), (unsigned)n), dim3(S360_BLOCK), 0, st, logits, candidates, lse,
                           depth, argmax, g_depth, g_pmax, (int)d, P, g_logits);
    return s360_launch_status();
}
