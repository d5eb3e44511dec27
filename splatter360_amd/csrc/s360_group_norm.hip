// s360_group_norm.hip — the encoder's normalise-then-activate pair (GroupNorm / InstanceNorm2d + none | ReLU | SiLU | GELU, with an
// optional residual add) as one fused operator, forward and backward.  gfx950 only, wave64.
//
//   x[N, C, S] float32; G groups of cpg = C / G channels; the slab of (n, g) is M = cpg S contiguous floats
//   mu, var   the slab's mean and biased variance, r = 1 / sqrt(var + eps)
//   xh = (x - mu) r,  z = xh gamma_c + beta_c (gamma = 1, beta = 0 without affine),  y = residual + a(z)
//   backward  dz = g_out a'(z),  m1 = sum_c gamma_c sum_s dz / M,  m2 = sum_c gamma_c sum_s dz xh / M  over the slab,
//             g_x = r (gamma_c dz - m1 - xh m2),  g_weight[c] = sum_{n,s} dz xh,  g_bias[c] = sum_{n,s} dz
// Every per-element operation is float64 on the float32 inputs and the float64 statistics (the library is compiled with
// -ffp-contract=off: no FMA), rounded once to float32.  SiLU is z / (1 + exp(-z)) and GELU 0.5 z erfc(-z / sqrt 2) with the
// float64 library functions; none and ReLU evaluate no transcendental.
//
// Work split: a workgroup takes one chunk of GN_ROW_CHUNK floats of one (n, c) row — fixed, whatever the device — so the 16 slabs
// of the depth U-Net's top level become 8192 workgroups.  Sums: a thread's own elements in index order, then block_sum (lanes by
// a fixed shuffle tree, the four waves through LDS in wave order), one pair of doubles per chunk in the caller's scratch; the
// launch that needs a slab's (or a channel's) total adds the pairs thread-strided in index order and reduces by the same tree.
// No atomics, no memset, no host read: bit-identical from run to run and across streams.
//   forward   k_gn_stats: per chunk (mean, M2) from sums shifted by the chunk's first element (exact for a constant chunk, and a
//             large mean over a small spread costs nothing).  k_gn_apply: mu = sum n_i mean_i / M, var = sum (M2_i + n_i (mean_i
//             - mu)^2) / M (Chan's merge for all chunks at once: only non-negative terms), stats (mu, r) written by the slab's
//             first workgroup, then x (and residual) streamed to out.
//   backward  k_gn_bwd_sums: per chunk (sum dz, sum dz xh).  k_gn_bwd_apply: m1, m2 of the slab, then g_x.  k_gn_bwd_params: one
//             workgroup per channel adds that channel's pairs over n and chunks.
// Rows are read and written as float4 where every pointer of the launch is 16-byte aligned, with a scalar head up to the row's
// first aligned element and a scalar tail; otherwise element by element.
#include <math.h>

#include <initializer_list>

#include "s360_device.h"

namespace s360 {

constexpr int GN_ROW_CHUNK = 4096;
constexpr int GN_WAVES = S360_BLOCK / S360_WAVE;

struct GNArgs {
    const float* x;
    const float* weight;                                       // [C] or null (then bias is null too)
    const float* bias;
    long long S;
    int C, cpg, chunks;                                        // chunks = ceil(S / GN_ROW_CHUNK) per row
    int vec;                                                   // every pointer the launch streams is 16-byte aligned
    double eps;
};

struct GNChunk {
    long long row;                                             // n C + c
    int k, len;                                                // chunk index in the row, its length
    size_t off;                                                // element offset of the chunk
    int head, nvec, tail;                                      // scalar head, float4 body, scalar tail
};

__device__ __forceinline__ int gn_chunk_len(const GNArgs& a, int k) {
    const long long rest = a.S - (long long)k * GN_ROW_CHUNK;
    return rest < GN_ROW_CHUNK ? (int)rest : GN_ROW_CHUNK;
}

__device__ __forceinline__ GNChunk gn_chunk(const GNArgs& a) {
    GNChunk c;
    c.row = blockIdx.x / a.chunks;
    c.k = (int)(blockIdx.x - c.row * a.chunks);
    c.len = gn_chunk_len(a, c.k);
    c.off = (size_t)c.row * (size_t)a.S + (size_t)c.k * GN_ROW_CHUNK;
    c.head = a.vec ? (int)((4 - (c.off & 3)) & 3) : c.len;
    if (c.head > c.len) c.head = c.len;
    c.nvec = (c.len - c.head) >> 2;
    c.tail = c.len - c.head - 4 * c.nvec;
    return c;
}

template <int ACT>
__device__ __forceinline__ double gn_act(double z) {
    if constexpr (ACT == S360_GN_ACT_RELU) return z > 0.0 ? z : 0.0;
    if constexpr (ACT == S360_GN_ACT_SILU) return z / (1.0 + exp(-z));
    if constexpr (ACT == S360_GN_ACT_GELU) return 0.5 * z * erfc(-z * 0.70710678118654752440);
    return z;
}

template <int ACT>
__device__ __forceinline__ double gn_dact(double z) {
    if constexpr (ACT == S360_GN_ACT_RELU) return z > 0.0 ? 1.0 : 0.0;
    if constexpr (ACT == S360_GN_ACT_SILU) {
        const double s = 1.0 / (1.0 + exp(-z));
        return s * (1.0 + z * (1.0 - s));
    }
    if constexpr (ACT == S360_GN_ACT_GELU)
        return 0.5 * erfc(-z * 0.70710678118654752440) + z * exp(-0.5 * z * z) * 0.39894228040143267794;
    return 1.0;
}

__global__ __launch_bounds__(S360_BLOCK) void k_gn_stats(GNArgs a, double* __restrict__ partials) {
    __shared__ double sh[2][GN_WAVES];
    const int tid = threadIdx.x;
    const GNChunk c = gn_chunk(a);
    const float* __restrict__ p = a.x + c.off;
    const double shift = (double)p[0];
    double s1 = 0.0, s2 = 0.0;
    auto add = [&](float v) {
        const double d = (double)v - shift;
        s1 += d;
        s2 += d * d;
    };
    for (int i = tid; i < c.head; i += S360_BLOCK) add(p[i]);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + c.head);
    for (int i = tid; i < c.nvec; i += S360_BLOCK) {
        const float4 v = p4[i];
        add(v.x);
        add(v.y);
        add(v.z);
        add(v.w);
    }
    if (tid < c.tail) add(p[c.head + 4 * c.nvec + tid]);
    double v[2] = {s1, s2};
    block_sum<true>(v, sh);
    if (tid == 0) {
        const double n = (double)c.len, m2 = v[1] - v[0] * (v[0] / n);
        partials[2 * (size_t)blockIdx.x] = shift + v[0] / n;
        partials[2 * (size_t)blockIdx.x + 1] = m2 > 0.0 ? m2 : 0.0;
    }
}

template <int ACT, bool RES>
__global__ __launch_bounds__(S360_BLOCK) void k_gn_apply(GNArgs a, const double* __restrict__ partials, const float* __restrict__ residual,
                                                         double* __restrict__ stats, float* __restrict__ out) {
    __shared__ double sh[2][GN_WAVES];
    const int tid = threadIdx.x;
    const GNChunk c = gn_chunk(a);
    const long long n = c.row / a.C;
    const int ch = (int)(c.row - n * a.C), g = ch / a.cpg, groups = a.C / a.cpg;
    const double* __restrict__ slab = partials + 2 * (size_t)(n * a.C + (long long)g * a.cpg) * a.chunks;
    const int entries = a.cpg * a.chunks;
    const double M = (double)a.cpg * (double)a.S;
    double ws = 0.0;
    for (int e = tid; e < entries; e += S360_BLOCK) ws += (double)gn_chunk_len(a, e % a.chunks) * slab[2 * (size_t)e];
    double v[1] = {ws};
    block_sum<true>(v, sh);
    const double mu = v[0] / M;
    double m2 = 0.0;
    for (int e = tid; e < entries; e += S360_BLOCK) {
        const double d = slab[2 * (size_t)e] - mu;
        m2 += slab[2 * (size_t)e + 1] + (double)gn_chunk_len(a, e % a.chunks) * (d * d);
    }
    v[0] = m2;
    block_sum<true>(v, sh);
    const double r = 1.0 / sqrt(v[0] / M + a.eps);
    if (tid == 0 && c.k == 0 && ch == g * a.cpg) {
        stats[2 * (size_t)(n * groups + g)] = mu;
        stats[2 * (size_t)(n * groups + g) + 1] = r;
    }
    const double gam = a.weight ? (double)a.weight[ch] : 1.0, bet = a.bias ? (double)a.bias[ch] : 0.0;
    const float* __restrict__ p = a.x + c.off;
    const float* __restrict__ q = RES ? residual + c.off : nullptr;
    float* __restrict__ o = out + c.off;
    auto f = [&](float xv, float rv) -> float {
        const double y = gn_act<ACT>(((double)xv - mu) * r * gam + bet);
        return (float)(RES ? (double)rv + y : y);
    };
    for (int i = tid; i < c.head; i += S360_BLOCK) o[i] = f(p[i], RES ? q[i] : 0.f);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + c.head);
    const float4* __restrict__ q4 = RES ? reinterpret_cast<const float4*>(q + c.head) : nullptr;
    float4* __restrict__ o4 = reinterpret_cast<float4*>(o + c.head);
    for (int i = tid; i < c.nvec; i += S360_BLOCK) {
        const float4 v = p4[i];
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (RES) w = q4[i];
        o4[i] = make_float4(f(v.x, w.x), f(v.y, w.y), f(v.z, w.z), f(v.w, w.w));
    }
    if (tid < c.tail) {
        const int i = c.head + 4 * c.nvec + tid;
        o[i] = f(p[i], RES ? q[i] : 0.f);
    }
}

// per chunk: sum dz and sum dz xh
template <int ACT>
__global__ __launch_bounds__(S360_BLOCK) void k_gn_bwd_sums(GNArgs a, const double* __restrict__ stats, const float* __restrict__ g_out,
                                                            double* __restrict__ partials) {
    __shared__ double sh[2][GN_WAVES];
    const int tid = threadIdx.x;
    const GNChunk c = gn_chunk(a);
    const long long n = c.row / a.C;
    const int ch = (int)(c.row - n * a.C), g = ch / a.cpg, groups = a.C / a.cpg;
    const double mu = stats[2 * (size_t)(n * groups + g)], r = stats[2 * (size_t)(n * groups + g) + 1];
    const double gam = a.weight ? (double)a.weight[ch] : 1.0, bet = a.bias ? (double)a.bias[ch] : 0.0;
    const float* __restrict__ p = a.x + c.off;
    const float* __restrict__ q = g_out + c.off;
    double sa = 0.0, sb = 0.0;
    auto add = [&](float xv, float gv) {
        const double xh = ((double)xv - mu) * r, dz = (double)gv * gn_dact<ACT>(xh * gam + bet);
        sa += dz;
        sb += dz * xh;
    };
    for (int i = tid; i < c.head; i += S360_BLOCK) add(p[i], q[i]);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + c.head);
    const float4* __restrict__ q4 = reinterpret_cast<const float4*>(q + c.head);
    for (int i = tid; i < c.nvec; i += S360_BLOCK) {
        const float4 v = p4[i], w = q4[i];
        add(v.x, w.x);
        add(v.y, w.y);
        add(v.z, w.z);
        add(v.w, w.w);
    }
    if (tid < c.tail) {
        const int i = c.head + 4 * c.nvec + tid;
        add(p[i], q[i]);
    }
    double v[2] = {sa, sb};
    block_sum<true>(v, sh);
    if (tid == 0) {
        partials[2 * (size_t)blockIdx.x] = v[0];
        partials[2 * (size_t)blockIdx.x + 1] = v[1];
    }
}

template <int ACT>
__global__ __launch_bounds__(S360_BLOCK) void k_gn_bwd_apply(GNArgs a, const double* __restrict__ stats, const float* __restrict__ g_out,
                                                             const double* __restrict__ partials, float* __restrict__ g_x) {
    __shared__ double sh[2][GN_WAVES];
    const int tid = threadIdx.x;
    const GNChunk c = gn_chunk(a);
    const long long n = c.row / a.C;
    const int ch = (int)(c.row - n * a.C), g = ch / a.cpg, groups = a.C / a.cpg;
    const double mu = stats[2 * (size_t)(n * groups + g)], r = stats[2 * (size_t)(n * groups + g) + 1];
    const double* __restrict__ slab = partials + 2 * (size_t)(n * a.C + (long long)g * a.cpg) * a.chunks;
    const int entries = a.cpg * a.chunks;
    const double M = (double)a.cpg * (double)a.S;
    double m1 = 0.0, m2 = 0.0;
    for (int e = tid; e < entries; e += S360_BLOCK) {
        const double ge = a.weight ? (double)a.weight[g * a.cpg + e / a.chunks] : 1.0;
        m1 += ge * slab[2 * (size_t)e];
        m2 += ge * slab[2 * (size_t)e + 1];
    }
    double v[2] = {m1, m2};
    block_sum<true>(v, sh);
    m1 = v[0] / M;
    m2 = v[1] / M;
    const double gam = a.weight ? (double)a.weight[ch] : 1.0, bet = a.bias ? (double)a.bias[ch] : 0.0;
    const float* __restrict__ p = a.x + c.off;
    const float* __restrict__ q = g_out + c.off;
    float* __restrict__ o = g_x + c.off;
    auto f = [&](float xv, float gv) -> float {
        const double xh = ((double)xv - mu) * r, dz = (double)gv * gn_dact<ACT>(xh * gam + bet);
        return (float)(r * (gam * dz - m1 - xh * m2));
    };
    for (int i = tid; i < c.head; i += S360_BLOCK) o[i] = f(p[i], q[i]);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + c.head);
    const float4* __restrict__ q4 = reinterpret_cast<const float4*>(q + c.head);
    float4* __restrict__ o4 = reinterpret_cast<float4*>(o + c.head);
    for (int i = tid; i < c.nvec; i += S360_BLOCK) {
        const float4 v = p4[i], w = q4[i];
        o4[i] = make_float4(f(v.x, w.x), f(v.y, w.y), f(v.z, w.z), f(v.w, w.w));
    }
    if (tid < c.tail) {
        const int i = c.head + 4 * c.nvec + tid;
        o[i] = f(p[i], q[i]);
    }
}

// one workgroup per channel: g_bias[c] = sum over n and chunks of sum dz, g_weight[c] of sum dz xh
__global__ __launch_bounds__(S360_BLOCK) void k_gn_bwd_params(const double* __restrict__ partials, int N, int C, int chunks,
                                                              float* __restrict__ g_weight, float* __restrict__ g_bias) {
    __shared__ double sh[2][GN_WAVES];
    const int tid = threadIdx.x, ch = blockIdx.x;
    const long long entries = (long long)N * chunks;
    double sa = 0.0, sb = 0.0;
    for (long long e = tid; e < entries; e += S360_BLOCK) {
        const long long n = e / chunks, k = e - n * chunks;
        const size_t idx = 2 * (size_t)((n * C + ch) * chunks + k);
        sa += partials[idx];
        sb += partials[idx + 1];
    }
    double v[2] = {sa, sb};
    block_sum<true>(v, sh);
    if (tid == 0) {
        if (g_bias) g_bias[ch] = (float)v[0];
        if (g_weight) g_weight[ch] = (float)v[1];
    }
}

}  // namespace s360

using namespace s360;

namespace {

bool gn_overlap(const float* a, const float* b, size_t count) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, bytes = count * sizeof(float);
    return pa < pb + bytes && pb < pa + bytes;
}

bool gn_aligned(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (p && !s360_aligned(p, 16)) return false;
    return true;
}

// shared argument check; fills the kernel arguments and the grid, or returns an error
int gn_setup(const float* x, const float* weight, const float* bias, int32_t n, int32_t channels, size_t spatial, int32_t groups,
             const double* eps, int32_t activation, GNArgs* a, long long* blocks) {
    if (!x || n < 1 || channels < 1 || spatial < 1 || spatial > (size_t)1 << 62 || groups < 1 || channels % groups != 0 ||
        (weight == nullptr) != (bias == nullptr))
        return S360_E_BADARG;
    if (!eps || !(*eps > 0.0) || activation < S360_GN_ACT_NONE || activation > S360_GN_ACT_GELU) return S360_E_BADARG;
    const long long chunks = (long long)((spatial + GN_ROW_CHUNK - 1) / GN_ROW_CHUNK);
    const long long rows = (long long)n * channels;
    if (rows > INT32_MAX || chunks > INT32_MAX / rows) return S360_E_BADARG;             // 2^31 or more workgroups
    *blocks = chunks * rows;
    *a = GNArgs{x, weight, bias, (long long)spatial, channels, channels / groups, (int)chunks, 0, *eps};
    return S360_OK;
}

}  // namespace

extern "C" size_t s360_group_norm_scratch_doubles(int32_t n, int32_t channels, int64_t spatial) {
    if (n < 1 || channels < 1 || spatial < 1) return 0;
    return 2 * (size_t)n * (size_t)channels * (size_t)((spatial + GN_ROW_CHUNK - 1) / GN_ROW_CHUNK);
}

#define GN_LAUNCH_ACT(KERNEL, ...)                                                                                         \
    switch (activation) {                                                                                                  \
        case S360_GN_ACT_NONE: hipLaunchKernelGGL((KERNEL<S360_GN_ACT_NONE>), grid, block, 0, st, __VA_ARGS__); break;     \
        case S360_GN_ACT_RELU: hipLaunchKernelGGL((KERNEL<S360_GN_ACT_RELU>), grid, block, 0, st, __VA_ARGS__); break;     \
        case S360_GN_ACT_SILU: hipLaunchKernelGGL((KERNEL<S360_GN_ACT_SILU>), grid, block, 0, st, __VA_ARGS__); break;     \
        default: hipLaunchKernelGGL((KERNEL<S360_GN_ACT_GELU>), grid, block, 0, st, __VA_ARGS__); break;                   \
    }

extern "C" int s360_group_norm_forward(const float* x, const float* weight, const float* bias, const float* residual, int32_t n,
                                       int32_t channels, size_t spatial, int32_t groups, const double* eps, int32_t activation, double* scratch,
                                       double* stats, float* out, void* stream) {
    GNArgs a;
    long long blocks;
    const int rc = gn_setup(x, weight, bias, n, channels, spatial, groups, eps, activation, &a, &blocks);
    if (rc != S360_OK) return rc;
    if (!scratch || !stats || !out || gn_overlap(out, x, (size_t)n * channels * (size_t)spatial)) return S360_E_BADARG;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(S360_BLOCK);
    a.vec = gn_aligned({x});
    hipLaunchKernelGGL(k_gn_stats, grid, block, 0, st, a, scratch);
    S360_CHECK_LAUNCH();
    a.vec = gn_aligned({x, residual, out});
    if (residual) {
        switch (activation) {
            case S360_GN_ACT_NONE: hipLaunchKernelGGL((k_gn_apply<S360_GN_ACT_NONE, true>), grid, block, 0, st, a, (const double*)scratch, residual, stats, out); break;
            case S360_GN_ACT_RELU: hipLaunchKernelGGL((k_gn_apply<S360_GN_ACT_RELU, true>), grid, block, 0, st, a, (const double*)scratch, residual, stats, out); break;
            case S360_GN_ACT_SILU: hipLaunchKernelGGL((k_gn_apply<S360_GN_ACT_SILU, true>), grid, block, 0, st, a, (const double*)scratch, residual, stats, out); break;
            default: hipLaunchKernelGGL((k_gn_apply<S360_GN_ACT_GELU, true>), grid, block, 0, st, a, (const double*)scratch, residual, stats, out); break;
        }
    } else {
        switch (activation) {
            case S360_GN_ACT_NONE: hipLaunchKernelGGL((k_gn_apply<S360_GN_ACT_NONE, false>), grid, block, 0, st, a, (const double*)scratch, residual, stats, out); break;
            case S360_GN_ACT_RELU: hipLaunchKernelGGL((k_gn_apply<S360_GN_ACT_RELU, false>), grid, block, 0, st, a, (const double*)scratch, residual, stats, out); break;
            case S360_GN_ACT_SILU: hipLaunchKernelGGL((k_gn_apply<S360_GN_ACT_SILU, false>), grid, block, 0, st, a, (const double*)scratch, residual, stats, out); break;
            default: hipLaunchKernelGGL((k_gn_apply<S360_GN_ACT_GELU, false>), grid, block, 0, st, a, (const double*)scratch, residual, stats, out); break;
        }
    }
    return s360_launch_status();
}

extern "C" int s360_group_norm_backward(const float* x, const float* weight, const float* bias, const double* stats, const float* g_out,
                                        int32_t n, int32_t channels, size_t spatial, int32_t groups, const double* eps, int32_t activation,
                                        double* scratch, float* g_x, float* g_weight, float* g_bias, void* stream) {
    GNArgs a;
    long long blocks;
    const int rc = gn_setup(x, weight, bias, n, channels, spatial, groups, eps, activation, &a, &blocks);
    if (rc != S360_OK) return rc;
    if (!stats || !g_out || !scratch || (g_x && gn_overlap(g_x, x, (size_t)n * channels * (size_t)spatial))) return S360_E_BADARG;
    if (!weight && (g_weight || g_bias)) return S360_E_BADARG;   // no parameters, no parameter gradients
    if (!g_x && !g_weight && !g_bias) return S360_OK;
    const hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)blocks);
    const dim3 block(S360_BLOCK);
    a.vec = gn_aligned({x, g_out});
    GN_LAUNCH_ACT(k_gn_bwd_sums, a, stats, g_out, scratch)
    S360_CHECK_LAUNCH();
    if (g_x) {
        a.vec = gn_aligned({x, g_out, g_x});
        GN_LAUNCH_ACT(k_gn_bwd_apply, a, stats, g_out, (const double*)scratch, g_x)
        S360_CHECK_LAUNCH();
    }
    if (g_weight || g_bias) {
        grid = dim3((unsigned)channels);
        hipLaunchKernelGGL(k_gn_bwd_params, grid, block, 0, st, (const double*)scratch, n, channels, a.chunks, g_weight, g_bias);
        S360_CHECK_LAUNCH();
    }
    return S360_OK;
}
