// s360_transformer_ffn.hip — the tail of the multi-view transformer's TransformerLayer behind its attention (the reference's
// src/model/encoder/backbone/multiview_transformer.py:407-414), forward and backward, as fused kernels.  gfx950 only.
//
//   X    = cat(source, LN1(m))                 [T, 2C]   m = merge(message), the layer's last nn.Linear
//   h    = gelu(X W1^T)                        [T, 8C]   W1 [8C, 2C], W2 [C, 8C] in nn.Linear's layout, no biases; erf GELU
//   z    = h W2^T                              [T, C]
//   out  = source + LN2(z)                     [T, C]    LayerNorm: biased variance, eps as passed, affine
// and, for the layer with no_ffn, out = residual + LN(x) alone.  C = 128, 8C = 1024.
//
// Neither X nor h exists in memory, forward or backward.  Every product runs on v_mfma_f32_32x32x2_f32 (exact float32 products,
// float32 accumulation), as in s360_qkv_attention.hip: 32 "owner" rows sit on the lanes (the B operand, held in registers:
// element 2 s + hf of the owner's row at MFMA step s of lane half hf), the other side sits on the accumulator's rows (the A
// operand, read from LDS), and an accumulator tile is, register by register, the B operand of the next product, whose k index
// then runs over the tile's rows.
// Forward (k_ff_forward) and the token-owned backward pass (k_ff_backward_tokens): the owners are 32 tokens per wave, four waves
// (128 tokens) per workgroup, and the hidden width is walked in 32 chunks of 32 units.  A chunk's slices of W1 ([32, 2C]) and W2
// ([C, 32]) are staged ONCE per workgroup in LDS (48.6 KB, odd row strides: ds_read_b32 is banked per lane half over 32 banks,
// so both the row-on-lanes and the row-per-step reads are conflict-free) and serve all four waves: the weights cross L2 -> CU
// once per 128 tokens (12 KB per token), not once per wave.  Chains: X W1c^T is four float32 chains of 64 channels added in float64 (eight chains of 32 in the weight-owned
// pass; dz W2c in the backward: chains of 8, ff_dot_lds); z accumulates one 32-unit chain per chunk into FLOAT64 registers; dX (the backward's [tokens, 2C] tile, 128 float32
// registers per lane: float64 would not fit beside X) is one float32 chain per chunk from zero, the 32 chunks added in float32 —
// as ONE chain of 512 steps over the hidden width it missed the accuracy rule of the tests in g_source, g_m and norm1's
// parameter gradients (maxima 2.1 to 3.9 x float32 torch's, means 1.4 to 1.6 x).
// The weight-owned backward pass (k_ff_backward_weights): the owners are 32 hidden units per wave (their W1 rows in
// registers, their W2 columns in LDS), four waves = 128 units per workgroup, and the tokens of one chunk are walked in tiles of 32 staged in LDS (X with
// norm1 applied, dz = norm2's backward), shared by the four waves.  g_W1 / g_W2 partials of a (hidden group, token chunk) go to
// scratch; k_ff_reduce adds the chunks in the order 0, 1, ... in float64.  The LayerNorm parameter gradients are float64 partial
// sums per workgroup of the token pass (a fixed number of workgroups walks the token tiles), reduced the same way.
// LayerNorm rows: float64 mean, two-pass biased variance and rstd per token, saved as (mean, rstd) pairs; the backward reads them.
// No atomics; every sum has a fixed order: bit-identical from run to run and across streams.
#include "s360_device.h"
#include "s360_bf16x3.h"

namespace s360 {

constexpr int FF_C = 128;                                     // d_model
constexpr int FF_H = 1024;                                    // hidden width
constexpr int FF_X = 2 * FF_C;                                // width of the concatenation
constexpr int FF_T = 32;                                      // rows of an MFMA tile
constexpr int FF_WAVES = S360_BLOCK / S360_WAVE;
constexpr int FF_TM = FF_T * FF_WAVES;                        // tokens of a workgroup in the token-owned kernels
constexpr int FF_LD1 = FF_X + 1;                              // row stride of the staged W1 chunk / X tile (floats)
constexpr int FF_LD2 = FF_T + 1;                              // row stride of the staged W2 chunk [C][32]
constexpr int FF_LDZ = FF_C + 1;                              // row stride of the staged dz tile [32][C]
constexpr int FF_GW = FF_T * FF_WAVES;                        // hidden units of a workgroup of the weight-owned pass
constexpr int FF_MAX_CHUNKS = 16;                             // token chunks of the weight-gradient pass, at most
constexpr int FF_TOKEN_WGS = 512;                             // workgroups of the token-owned backward pass, at most
constexpr int FF_ROWS = S360_BLOCK / 32;                      // token rows a workgroup of the row kernels handles at a time
constexpr int FF_ROW_WGS = 256;                               // workgroups of the row backward, at most
constexpr double FF_INV_C = 1.0 / FF_C;
constexpr int FF_CHAIN = 32;                                  // MFMA steps of a float32 chain of ff_dot
// ... in the weight-owned pass: gelu' near 0 turns the rounding of a pre-activation that is a small difference of large terms
// (2e-6 at inputs of scale 6 with chains of 32 steps) into an error of dH and so of a whole row of g_W1 — the maximum of the
// 5-token test case stood at 1.67 x float32 torch's; with 16 steps it is 0.66 x, at the price of 56 spilled registers
constexpr int FF_W_CHAIN = 16;
constexpr int FF_LDS_CHAIN = 4;                               // and of ff_dot_lds

struct FFArgs {
    const float *source, *m, *n1w, *n1b, *w1, *w2, *n2w, *n2b;
    int T;
    double eps;
};

__device__ __forceinline__ float ff_gelu(float v) { return 0.5f * v * erfcf(-v * 0.70710678118654752440f); }
__device__ __forceinline__ float ff_gelu_grad(float v) {
    return 0.5f * erfcf(-v * 0.70710678118654752440f) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}

__device__ __forceinline__ double ff_sum32(double v) {        // over the 32 lanes of a lane half, the same bits in each
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// out[r] = float32 of the sum over 2 STEPS values of k of A[row][k] B[k][lane].  A is read from LDS at a[2 s ks] (a points at
// (row l31, k = hf), ks is the image's stride per k), B is b(s), a register.  Float32 chains of CHAIN steps (2 CHAIN values of k)
// from zero, added in float64, rounded once.  Each chain's zero tile passes an empty asm statement that depends on the sums as
// they stand (s360_qkv_attention.hip, qa_dot), so that the chains run one after the other, at most three tiles live, and the
// float64 adds of chain c - 1 run under the MFMAs of chain c.  With B in registers the chains are unrolled, and chains shorter
// than 32 steps make the compiler spill (240 to 940 registers at 8 and 4 steps in both backward passes, 56 at 16 steps in the
// weight-owned pass, which takes them: FF_W_CHAIN).
template <int STEPS, int CHAIN, class B>
__device__ __forceinline__ void ff_dot(const float* a, int ks, B b, float* out) {
    double sum[16];
    f32x16 prev;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = 0.0, prev[r] = 0.f;
#pragma unroll
    for (int c = 0; c < STEPS / CHAIN; ++c) {
        float zero = 0.f;
        asm volatile("" : "+v"(zero) : "v"(sum[15]));
        f32x16 t;
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = zero;
#pragma unroll
        for (int i = 0; i < CHAIN; ++i) t = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * (CHAIN * c + i) * ks], b(CHAIN * c + i), t, 0, 0, 0);
        if (c > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sum[r] += (double)prev[r];
        }
        prev = t;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r] = (float)(sum[r] + (double)prev[r]);
}

// The same with B read from a second LDS image at b[2 s bs] (b points at (k = hf, the lane's column)): the chains are a rolled
// loop, so they can be short — 4 steps, the attention kernels' 8-value chains.  This is dz W2c, whose float32 chains of 32 steps
// were a relative 2e-7 of dH: with them g_W1 of the 5-token test case at input scale 6 missed the accuracy rule (maximum 1.67 x
// float32 torch's).
template <int STEPS>
__device__ __forceinline__ void ff_dot_lds(const float* a, int ks, const float* b, int bs, float* out) {
    double sum[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = 0.0;
#pragma unroll 1
    for (int c = 0; c < STEPS / FF_LDS_CHAIN; ++c) {
        f32x16 t;
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = 0.f;
#pragma unroll
        for (int i = 0; i < FF_LDS_CHAIN; ++i) {
            const int s = FF_LDS_CHAIN * c + i;
            t = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s * ks], b[2 * s * bs], t, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) sum[r] += (double)t[r];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r] = (float)sum[r];
}

// t[row][lane] += sum over the 32 rows k of a tile w held register by register of A[row][k] w[k][lane]; a points at (k = 4 hf,
// row l31) of an LDS image with k-stride ld
__device__ __forceinline__ f32x16 ff_fold(const float* a, int ld, const float* w, f32x16 t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) t = __builtin_amdgcn_mfma_f32_32x32x2f32(a[((r & 3) + 8 * (r >> 2)) * ld], w[r], t, 0, 0, 0);
    return t;
}

// the slices of hidden units [j0, j0 + 32): W1 rows -> s_w1[32][FF_LD1], W2 columns -> s_w2[C][FF_LD2]; coalesced reads
__device__ __forceinline__ void ff_stage_weights(const float* __restrict__ w1, const float* __restrict__ w2, int j0, float* s_w1,
                                                 float* s_w2, int tid) {
    for (int idx = tid; idx < FF_T * FF_X; idx += S360_BLOCK)
        s_w1[(idx >> 8) * FF_LD1 + (idx & 255)] = w1[(size_t)(j0 + (idx >> 8)) * FF_X + (idx & 255)];
    for (int idx = tid; idx < FF_C * FF_T; idx += S360_BLOCK)
        s_w2[(idx >> 5) * FF_LD2 + (idx & 31)] = w2[(size_t)(idx >> 5) * FF_H + j0 + (idx & 31)];
}

__device__ __forceinline__ float ff_norm(float v, double mean, double rstd, float w, float b) {
    return (float)(((double)v - mean) * rstd * (double)w + (double)b);
}

// x[s] = X[token][2 s + hf]: source, then LN1(m) with the given statistics; zeros for a token past the end
__device__ __forceinline__ void ff_load_x(const FFArgs& a, int token, bool valid, int hf, double mean, double rstd, float* x) {
    const float* ps = a.source + (size_t)token * FF_C + hf;
    const float* pm = a.m + (size_t)token * FF_C + hf;
#pragma unroll
    for (int s = 0; s < FF_C / 2; ++s) {
        x[s] = valid ? ps[2 * s] : 0.f;
        x[FF_C / 2 + s] = valid ? ff_norm(pm[2 * s], mean, rstd, a.n1w[2 * s + hf], a.n1b[2 * s + hf]) : 0.f;
    }
}

// Forward.  stats[0][T][2] = (mean, rstd) of norm1, stats[1][T][2] of norm2 (taken over the float32 z that is written).
__global__ __launch_bounds__(S360_BLOCK) void k_ff_forward(FFArgs a, float* __restrict__ out, float* __restrict__ z, double* __restrict__ stats) {
    __shared__ float s_w1[FF_T * FF_LD1];
    __shared__ float s_w2[FF_C * FF_LD2];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int token = blockIdx.x * FF_TM + wave * FF_T + l31;
    const bool valid = token < a.T;
    double mean1 = 0.0, rstd1 = 0.0;
    {
        const float* pm = a.m + (size_t)token * FF_C + hf;
        double sum = 0.0, sq = 0.0;
        for (int s = 0; s < FF_C / 2; ++s) sum += valid ? (double)pm[2 * s] : 0.0;
        sum += __shfl_xor(sum, 32);
        mean1 = sum * FF_INV_C;
        for (int s = 0; s < FF_C / 2; ++s) {
            const double d = valid ? (double)pm[2 * s] - mean1 : 0.0;
            sq += d * d;
        }
        sq += __shfl_xor(sq, 32);
        rstd1 = 1.0 / sqrt(sq * FF_INV_C + a.eps);
    }
    float x[FF_X / 2];
    ff_load_x(a, token, valid, hf, mean1, rstd1, x);
    double zacc[FF_C / FF_T][16];
#pragma unroll
    for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) zacc[ct][r] = 0.0;
    for (int j0 = 0; j0 < FF_H; j0 += FF_T) {
        __syncthreads();                                      // the previous chunk has been read
        ff_stage_weights(a.w1, a.w2, j0, s_w1, s_w2, tid);
        __syncthreads();
        float h[16];
        ff_dot<FF_X / 2, FF_CHAIN>(s_w1 + l31 * FF_LD1 + hf, 1, [&](int s) { return x[s]; }, h);   // (X W1c^T)^T: rows = hidden units, lane = token
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = ff_gelu(h[r]);
#pragma unroll
        for (int ct = 0; ct < FF_C / FF_T; ++ct) {            // z^T += W2c h^T, two hidden units (one per lane half) a step
            f32x16 t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = 0.f;
            t = ff_fold(s_w2 + (ct * FF_T + l31) * FF_LD2 + 4 * hf, 1, h, t);
#pragma unroll
            for (int r = 0; r < 16; ++r) zacc[ct][r] += (double)t[r];
        }
    }
    // norm2 over the float32 z, the residual, the writes: register r of tile ct is channel 32 ct + mfma_acc_row(r, hf)
    float zf[FF_C / FF_T][16];
    double sum = 0.0, sq = 0.0;
#pragma unroll
    for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) zf[ct][r] = (float)zacc[ct][r], sum += (double)zf[ct][r];
    sum += __shfl_xor(sum, 32);
    const double mean2 = sum * FF_INV_C;
#pragma unroll
    for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const double d = (double)zf[ct][r] - mean2;
            sq += d * d;
        }
    sq += __shfl_xor(sq, 32);
    const double rstd2 = 1.0 / sqrt(sq * FF_INV_C + a.eps);
    if (!valid) return;
#pragma unroll
    for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c0 = ct * FF_T + 8 * q + 4 * hf;
            const size_t at = (size_t)token * FF_C + c0;
            const float4 sv = *reinterpret_cast<const float4*>(a.source + at);
            const float4 wv = *reinterpret_cast<const float4*>(a.n2w + c0);
            const float4 bv = *reinterpret_cast<const float4*>(a.n2b + c0);
            const float* zr = &zf[ct][4 * q];
            float4 o;
            o.x = sv.x + ff_norm(zr[0], mean2, rstd2, wv.x, bv.x);
            o.y = sv.y + ff_norm(zr[1], mean2, rstd2, wv.y, bv.y);
            o.z = sv.z + ff_norm(zr[2], mean2, rstd2, wv.z, bv.z);
            o.w = sv.w + ff_norm(zr[3], mean2, rstd2, wv.w, bv.w);
            *reinterpret_cast<float4*>(out + at) = o;
            *reinterpret_cast<float4*>(z + at) = make_float4(zr[0], zr[1], zr[2], zr[3]);
        }
    if (hf == 0) {
        stats[(size_t)token * 2] = mean1, stats[(size_t)token * 2 + 1] = rstd1;
        stats[((size_t)a.T + token) * 2] = mean2, stats[((size_t)a.T + token) * 2 + 1] = rstd2;
    }
}

// Backward, the pass owned by token tiles: g_source, g_m and the per-workgroup float64 partial sums of the four LayerNorm
// parameter gradients, ln_part[workgroup][g_n1w | g_n1b | g_n2w | g_n2b][C].  gridDim.x workgroups walk the tiles of 128 tokens.
__global__ __launch_bounds__(S360_BLOCK) void k_ff_backward_tokens(FFArgs a, const float* __restrict__ z, const double* __restrict__ stats,
                                                                   const float* __restrict__ g_out, float* __restrict__ g_source,
                                                                   float* __restrict__ g_m, double* __restrict__ ln_part) {
    __shared__ float s_w1[FF_T * FF_LD1];
    __shared__ float s_w2[FF_C * FF_LD2];
    __shared__ double s_wave[FF_WAVES][4 * FF_C];             // a wave's sums over its 32 tokens of the current tile
    __shared__ double s_ln[4 * FF_C];                         // the workgroup's sums over the tiles it has walked
    __shared__ float s_dz[FF_WAVES][FF_C / 2][S360_WAVE];     // dz, each lane's 64 values: written and read by that lane alone
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    for (int i = tid; i < 4 * FF_C; i += S360_BLOCK) s_ln[i] = 0.0;
    const int ntiles = (a.T + FF_TM - 1) / FF_TM;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int token = tile * FF_TM + wave * FF_T + l31;
        const bool valid = token < a.T;
        const size_t row = (size_t)token * FF_C;
        const double mean1 = valid ? stats[(size_t)token * 2] : 0.0, rstd1 = valid ? stats[(size_t)token * 2 + 1] : 0.0;
        const double mean2 = valid ? stats[((size_t)a.T + token) * 2] : 0.0, rstd2 = valid ? stats[((size_t)a.T + token) * 2 + 1] : 0.0;
        float x[FF_X / 2];
        float* dz = &s_dz[wave][0][lane];                     // dz[s * S360_WAVE]
        ff_load_x(a, token, valid, hf, mean1, rstd1, x);
        {   // norm2's backward: dz[s] is channel 2 s + hf
            double s1 = 0.0, s2 = 0.0;
            for (int s = 0; s < FF_C / 2; ++s) {
                const int c = 2 * s + hf;
                const double gy = valid ? (double)g_out[row + c] * (double)a.n2w[c] : 0.0;
                const double xh = valid ? ((double)z[row + c] - mean2) * rstd2 : 0.0;
                s1 += gy, s2 += gy * xh;
            }
            s1 += __shfl_xor(s1, 32), s2 += __shfl_xor(s2, 32);
            s1 *= FF_INV_C, s2 *= FF_INV_C;
#pragma unroll
            for (int s = 0; s < FF_C / 2; ++s) {
                const int c = 2 * s + hf;
                const double g = valid ? (double)g_out[row + c] : 0.0;
                const double xh = valid ? ((double)z[row + c] - mean2) * rstd2 : 0.0;
                dz[s * S360_WAVE] = (float)(rstd2 * (g * (double)a.n2w[c] - s1 - xh * s2));
                const double pw = ff_sum32(g * xh), pb = ff_sum32(g);
                if (l31 == 0) s_wave[wave][2 * FF_C + c] = pw, s_wave[wave][3 * FF_C + c] = pb;
            }
        }
        f32x16 dx[FF_X / FF_T];                            // dX^T: tile ct, register r is channel 32 ct + mfma_acc_row(r, hf) of the lane's token
#pragma unroll
        for (int ct = 0; ct < FF_X / FF_T; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) dx[ct][r] = 0.f;
        for (int j0 = 0; j0 < FF_H; j0 += FF_T) {
            __syncthreads();
            ff_stage_weights(a.w1, a.w2, j0, s_w1, s_w2, tid);
            __syncthreads();
            float pre[16], dh[16];
            ff_dot<FF_X / 2, FF_CHAIN>(s_w1 + l31 * FF_LD1 + hf, 1, [&](int s) { return x[s]; }, pre);        // X W1c^T again
            ff_dot_lds<FF_C / 2>(s_w2 + hf * FF_LD2 + l31, FF_LD2, dz, S360_WAVE / 2, dh);   // (dz W2c)^T: the channel is k, stride FF_LD2
#pragma unroll
            for (int r = 0; r < 16; ++r) dh[r] *= ff_gelu_grad(pre[r]);
#pragma unroll
            for (int ct = 0; ct < FF_X / FF_T; ++ct) {        // one chain per chunk from zero, the chunks added in float32 (see the header)
                f32x16 t;
#pragma unroll
                for (int r = 0; r < 16; ++r) t[r] = 0.f;
                dx[ct] += ff_fold(s_w1 + 4 * hf * FF_LD1 + ct * FF_T + l31, FF_LD1, dh, t);
            }
        }
        // g_source = g_out + dX[:, :C]
        if (valid) {
#pragma unroll
            for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const size_t at = row + ct * FF_T + 8 * q + 4 * hf;
                    const float4 g = *reinterpret_cast<const float4*>(g_out + at);
                    *reinterpret_cast<float4*>(g_source + at) =
                        make_float4(g.x + dx[ct][4 * q], g.y + dx[ct][4 * q + 1], g.z + dx[ct][4 * q + 2], g.w + dx[ct][4 * q + 3]);
                }
        }
        {   // norm1's backward on dX[:, C:]
            double s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = ct * FF_T + mfma_acc_row(r, hf);
                    const double gy = (double)dx[FF_C / FF_T + ct][r] * (double)a.n1w[c];
                    const double xh = valid ? ((double)a.m[row + c] - mean1) * rstd1 : 0.0;
                    s1 += gy, s2 += gy * xh;
                }
            s1 += __shfl_xor(s1, 32), s2 += __shfl_xor(s2, 32);
            s1 *= FF_INV_C, s2 *= FF_INV_C;
#pragma unroll
            for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = ct * FF_T + mfma_acc_row(r, hf);
                    const double g = (double)dx[FF_C / FF_T + ct][r];
                    const double xh = valid ? ((double)a.m[row + c] - mean1) * rstd1 : 0.0;
                    if (valid) g_m[row + c] = (float)(rstd1 * (g * (double)a.n1w[c] - s1 - xh * s2));
                    const double pw = ff_sum32(g * xh), pb = ff_sum32(g);
                    if (l31 == 0) s_wave[wave][c] = pw, s_wave[wave][FF_C + c] = pb;
                }
        }
        __syncthreads();
        for (int i = tid; i < 4 * FF_C; i += S360_BLOCK) {
            double v = s_ln[i];
#pragma unroll
            for (int w = 0; w < FF_WAVES; ++w) v += s_wave[w][i];
            s_ln[i] = v;
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = tid; i < 4 * FF_C; i += S360_BLOCK) ln_part[(size_t)blockIdx.x * 4 * FF_C + i] = s_ln[i];
}

// one token row of LayerNorm's backward, a thread holding 4 consecutive channels (lane l of the 32 lanes of the row: channels
// 4 l ..): g_x = rstd (g w - mean(g w) - xh mean(g w xh)); returns xh in `xh`
__device__ __forceinline__ float4 ff_row_backward(const float4 xv, const float4 gv, const float4 wv, double mean, double rstd, double* xh) {
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, gs[4] = {gv.x, gv.y, gv.z, gv.w}, ws[4] = {wv.x, wv.y, wv.z, wv.w};
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        xh[i] = ((double)xs[i] - mean) * rstd;
        const double gy = (double)gs[i] * (double)ws[i];
        s1 += gy, s2 += gy * xh[i];
    }
    s1 = ff_sum32(s1) * FF_INV_C, s2 = ff_sum32(s2) * FF_INV_C;
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (float)(rstd * ((double)gs[i] * (double)ws[i] - s1 - xh[i] * s2));
    return make_float4(o[0], o[1], o[2], o[3]);
}

__device__ __forceinline__ float4 ff_norm4(const float4 v, double mean, double rstd, const float4 w, const float4 b) {
    return make_float4(ff_norm(v.x, mean, rstd, w.x, b.x), ff_norm(v.y, mean, rstd, w.y, b.y), ff_norm(v.z, mean, rstd, w.z, b.z),
                       ff_norm(v.w, mean, rstd, w.w, b.w));
}

// Backward, the pass owned by (hidden group of 128 units, token chunk): wave w owns units [j0, j0 + 32) — row j0 + l31 of W1 in registers,
// column j0 + l31 of W2 in LDS — and the chunk's tokens are walked in tiles of 32 staged in LDS.  Partials:
// p_w1[chunk][8C][2C], p_w2[chunk][C][8C].
__global__ __launch_bounds__(S360_BLOCK) void k_ff_backward_weights(FFArgs a, const float* __restrict__ z, const double* __restrict__ stats,
                                                                    const float* __restrict__ g_out, int chunk_tokens,
                                                                    float* __restrict__ p_w1, float* __restrict__ p_w2) {
    __shared__ float s_x[FF_T * FF_LD1];
    __shared__ float s_dz[FF_T * FF_LDZ];
    __shared__ float s_w2[FF_C * FF_GW];                      // W2's columns of the workgroup's 128 units, [C][128]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int j0 = (blockIdx.x * FF_WAVES + wave) * FF_T, chunk = blockIdx.y;
    for (int idx = tid; idx < FF_C * FF_GW; idx += S360_BLOCK)
        s_w2[idx] = a.w2[(size_t)(idx / FF_GW) * FF_H + blockIdx.x * FF_GW + (idx % FF_GW)];
    const float* pw2 = s_w2 + hf * FF_GW + wave * FF_T + l31; // (channel hf, the lane's unit); read after the loop's first barriers
    const int first = chunk * chunk_tokens, last = min(a.T, first + chunk_tokens);
    float w1r[FF_X / 2];
#pragma unroll
    for (int s = 0; s < FF_X / 2; ++s) w1r[s] = a.w1[(size_t)(j0 + l31) * FF_X + 2 * s + hf];
    f32x16 gw1[FF_X / FF_T], gw2[FF_C / FF_T];             // g_W1^T, g_W2: rows = channels, lane = hidden unit
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int ct = 0; ct < FF_X / FF_T; ++ct) gw1[ct][r] = 0.f;
#pragma unroll
        for (int ct = 0; ct < FF_C / FF_T; ++ct) gw2[ct][r] = 0.f;
    }
    const int slot = tid >> 5, l = tid & 31;
    const float4 n1w = *reinterpret_cast<const float4*>(a.n1w + 4 * l), n1b = *reinterpret_cast<const float4*>(a.n1b + 4 * l);
    const float4 n2w = *reinterpret_cast<const float4*>(a.n2w + 4 * l);
    for (int t0 = first; t0 < last; t0 += FF_T) {
        __syncthreads();                                      // the previous tile has been read
#pragma unroll
        for (int it = 0; it < FF_T / FF_ROWS; ++it) {
            const int tl = it * FF_ROWS + slot, token = t0 + tl;
            float4 sv = make_float4(0.f, 0.f, 0.f, 0.f), xv = sv, dv = sv;
            if (token < last) {                               // uniform over the 32 lanes of a row
                const size_t at = (size_t)token * FF_C + 4 * l;
                sv = *reinterpret_cast<const float4*>(a.source + at);
                xv = ff_norm4(*reinterpret_cast<const float4*>(a.m + at), stats[(size_t)token * 2], stats[(size_t)token * 2 + 1], n1w, n1b);
                double xh[4];
                dv = ff_row_backward(*reinterpret_cast<const float4*>(z + at), *reinterpret_cast<const float4*>(g_out + at), n2w,
                                     stats[((size_t)a.T + token) * 2], stats[((size_t)a.T + token) * 2 + 1], xh);
            }
            float* px = s_x + tl * FF_LD1 + 4 * l;
            px[0] = sv.x, px[1] = sv.y, px[2] = sv.z, px[3] = sv.w;
            px[FF_C] = xv.x, px[FF_C + 1] = xv.y, px[FF_C + 2] = xv.z, px[FF_C + 3] = xv.w;
            float* pd = s_dz + tl * FF_LDZ + 4 * l;
            pd[0] = dv.x, pd[1] = dv.y, pd[2] = dv.z, pd[3] = dv.w;
        }
        __syncthreads();
        float h[16], dh[16];
        ff_dot<FF_X / 2, FF_W_CHAIN>(s_x + l31 * FF_LD1 + hf, 1, [&](int s) { return w1r[s]; }, h);                 // X W1c^T: rows = tokens, lane = hidden unit
        ff_dot_lds<FF_C / 2>(s_dz + l31 * FF_LDZ + hf, 1, pw2, FF_GW, dh);   // dz W2c
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            dh[r] *= ff_gelu_grad(h[r]);
            h[r] = ff_gelu(h[r]);
        }
#pragma unroll
        for (int ct = 0; ct < FF_X / FF_T; ++ct) gw1[ct] = ff_fold(s_x + 4 * hf * FF_LD1 + ct * FF_T + l31, FF_LD1, dh, gw1[ct]);
#pragma unroll
        for (int ct = 0; ct < FF_C / FF_T; ++ct) gw2[ct] = ff_fold(s_dz + 4 * hf * FF_LDZ + ct * FF_T + l31, FF_LDZ, h, gw2[ct]);
    }
    float* q1 = p_w1 + ((size_t)chunk * FF_H + j0 + l31) * FF_X;
    float* q2 = p_w2 + (size_t)chunk * FF_C * FF_H + j0 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int ct = 0; ct < FF_X / FF_T; ++ct) q1[ct * FF_T + mfma_acc_row(r, hf)] = gw1[ct][r];
#pragma unroll
        for (int ct = 0; ct < FF_C / FF_T; ++ct) q2[(size_t)(ct * FF_T + mfma_acc_row(r, hf)) * FF_H] = gw2[ct][r];
    }
}

// The last step of both backwards: sums of partials in the order 0, 1, ..., float64, rounded once.  Elements [0, nw1) are g_W1,
// [nw1, nw1 + nw2) g_W2 (both from `chunks` float32 partials), then nln values from `parts` float64 partials of stride nln, which
// go to ln_out[i / C][i % C].
struct FFLnOut { float* p[4]; };
__global__ __launch_bounds__(S360_BLOCK) void k_ff_reduce(const float* __restrict__ p_w1, const float* __restrict__ p_w2, int chunks, int nw1,
                                                          int nw2, float* __restrict__ g_w1, float* __restrict__ g_w2,
                                                          const double* __restrict__ ln_part, int parts, int nln, FFLnOut ln_out) {
    const int i = blockIdx.x * S360_BLOCK + threadIdx.x;
    if (i < nw1 + nw2) {
        const bool first = i < nw1;
        const float* p = first ? p_w1 + i : p_w2 + (i - nw1);
        const size_t stride = first ? nw1 : nw2;
        double v = 0.0;
        for (int c = 0; c < chunks; ++c) v += (double)p[c * stride];
        if (first) g_w1[i] = (float)v;
        else g_w2[i - nw1] = (float)v;
    } else if (i < nw1 + nw2 + nln) {
        const int k = i - nw1 - nw2;
        double v = 0.0;
        for (int c = 0; c < parts; ++c) v += ln_part[(size_t)c * nln + k];
        ln_out.p[k / FF_C][k % FF_C] = (float)v;
    }
}

// out = residual + LN(x) w + b: 32 lanes a token row, 4 channels a lane
__global__ __launch_bounds__(S360_BLOCK) void k_ff_norm_residual_forward(const float* __restrict__ x, const float* __restrict__ w,
                                                                         const float* __restrict__ b, const float* __restrict__ residual,
                                                                         int T, double eps, float* __restrict__ out, double* __restrict__ stats) {
    const int token = blockIdx.x * FF_ROWS + (threadIdx.x >> 5), l = threadIdx.x & 31;
    if (token >= T) return;                                   // uniform over the 32 lanes of a row
    const size_t at = (size_t)token * FF_C + 4 * l;
    const float4 v = *reinterpret_cast<const float4*>(x + at);
    const double mean = ff_sum32((double)v.x + (double)v.y + (double)v.z + (double)v.w) * FF_INV_C;
    const double d0 = (double)v.x - mean, d1 = (double)v.y - mean, d2 = (double)v.z - mean, d3 = (double)v.w - mean;
    const double rstd = 1.0 / sqrt(ff_sum32(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3) * FF_INV_C + eps);
    const float4 y = ff_norm4(v, mean, rstd, *reinterpret_cast<const float4*>(w + 4 * l), *reinterpret_cast<const float4*>(b + 4 * l));
    const float4 r = *reinterpret_cast<const float4*>(residual + at);
    *reinterpret_cast<float4*>(out + at) = make_float4(r.x + y.x, r.y + y.y, r.z + y.z, r.w + y.w);
    if (l == 0) stats[(size_t)token * 2] = mean, stats[(size_t)token * 2 + 1] = rstd;
}

// g_x, g_residual = g_out and the workgroup's float64 partial sums ln_part[workgroup][g_w | g_b][C]
__global__ __launch_bounds__(S360_BLOCK) void k_ff_norm_residual_backward(const float* __restrict__ x, const float* __restrict__ w,
                                                                          const double* __restrict__ stats, const float* __restrict__ g_out,
                                                                          int T, float* __restrict__ g_x, float* __restrict__ g_residual,
                                                                          double* __restrict__ ln_part) {
    __shared__ double s_part[FF_ROWS][2 * FF_C];
    const int slot = threadIdx.x >> 5, l = threadIdx.x & 31;
    const float4 wv = *reinterpret_cast<const float4*>(w + 4 * l);
    double pw[4] = {0.0, 0.0, 0.0, 0.0}, pb[4] = {0.0, 0.0, 0.0, 0.0};
    for (int token = blockIdx.x * FF_ROWS + slot; token < T; token += gridDim.x * FF_ROWS) {
        const size_t at = (size_t)token * FF_C + 4 * l;
        const float4 g = *reinterpret_cast<const float4*>(g_out + at);
        double xh[4];
        *reinterpret_cast<float4*>(g_x + at) =
            ff_row_backward(*reinterpret_cast<const float4*>(x + at), g, wv, stats[(size_t)token * 2], stats[(size_t)token * 2 + 1], xh);
        *reinterpret_cast<float4*>(g_residual + at) = g;
        const float gs[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) pw[i] += (double)gs[i] * xh[i], pb[i] += (double)gs[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s_part[slot][4 * l + i] = pw[i], s_part[slot][FF_C + 4 * l + i] = pb[i];
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * FF_C; i += S360_BLOCK) {
        double v = 0.0;
#pragma unroll
        for (int s = 0; s < FF_ROWS; ++s) v += s_part[s][i];
        ln_part[(size_t)blockIdx.x * 2 * FF_C + i] = v;
    }
}

// the weight-gradient pass's token chunks: a multiple of 32 tokens each, at most FF_MAX_CHUNKS
static int ff_chunk_tokens(int64_t T) {
    const int64_t tiles = (T + FF_T - 1) / FF_T;
    return (int)((tiles + FF_MAX_CHUNKS - 1) / FF_MAX_CHUNKS) * FF_T;
}
static int ff_chunks(int64_t T) { return (int)((T + ff_chunk_tokens(T) - 1) / ff_chunk_tokens(T)); }
static int ff_token_wgs(int64_t T) { return (int)min((int64_t)FF_TOKEN_WGS, (T + FF_TM - 1) / FF_TM); }
static int ff_row_wgs(int64_t T) { return (int)min((int64_t)FF_ROW_WGS, (T + FF_ROWS - 1) / FF_ROWS); }
static int ff_sizes(int32_t tokens, int32_t channels, int32_t hidden) {
    if (tokens < 1 || channels < 1 || hidden < 1) return S360_E_BADARG;
    if (channels != FF_C || hidden != FF_H) return S360_E_UNSUPPORTED;
    if ((int64_t)tokens * FF_C >= (int64_t)1 << 31) return S360_E_BADARG;
    return S360_OK;
}

}  // namespace s360

// ---------------------------------------------------------------------------------------------- the "high" mode (bf16 x 3)
// The same function with its two products, and the four of the backward, as bf16x3 products (s360_bf16x3.h: the split, the
// three terms and their order, the B-operand register rule), both operands split from their float32 values.  The LayerNorm
// rows, their statistics and the parameter gradients' partial sums are float64 as above; h, z, dz and dpre are rounded to
// float32 where the kernels above round them.
// A pre-pass (k_ffh_split, one launch) splits W1 and W2 once per call into bf16 planes in the caller's scratch, each in the two
// layouts its two uses need (3 MiB, whatever T): w1_r [8C][2C] for X W1^T (a lane reads 8 consecutive channels of a unit's row),
// w1_t [2C][8C] for dpre W1 (2 x 4 consecutive units of a channel's row: bx3_ld44, the k permutation of an accumulator tile used
// as the B operand), w2_r [C][8C] for h W2^T and w2_t [8C][C] for dz W2.  The kernels read the planes from
// global memory (L1 / L2: 3 MiB shared by every workgroup), so the token-owned kernels have no staging and no barrier in the walk
// over the hidden width.  The token side is split where it is produced: X and dz in registers / the lane's own LDS slots, h and
// dpre register by register from the accumulator tile, the weight-owned pass's X and dz tiles as they are staged in LDS (rows
// and transposed).  No plane that grows with T exists.  Orientation, launch geometry, partials and k_ff_reduce are those above.
// A product's terms are in (weight, token side) order — (wh, th), (wh, tl), (wl, th) — whichever side is the A operand: SWAP =
// false where A is the weight, true where B is.
namespace s360 {

constexpr size_t FFH_W1 = (size_t)FF_H * FF_X, FFH_W2 = (size_t)FF_C * FF_H;
constexpr size_t FFH_PLANE_BYTES = 2 * 2 * (FFH_W1 + FFH_W2) * sizeof(__bf16);   // two layouts x (hi, lo) of both weights
constexpr int FFH_LDR = FF_X + 8;                             // row stride of the staged X tile [32][2C] (bf16; rows 16-byte aligned)
constexpr int FFH_LDD = FF_C + 8;                             // of the staged dz tile [32][C]
constexpr int FFH_LDT = FF_T + 4;                             // of the transposed tiles [2C][32], [C][32] (rows 8-byte aligned)

struct FFHPlanes {
    __bf16 *w1_rh, *w1_rl, *w1_th, *w1_tl, *w2_rh, *w2_rl, *w2_th, *w2_tl;
};

// 8 consecutive floats (p 16-byte aligned), zeros unless valid
__device__ __forceinline__ void ffh_load8(const float* p, bool valid, float* x) {
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
    if (valid) u = *reinterpret_cast<const float4*>(p), v = *reinterpret_cast<const float4*>(p + 4);
    x[0] = u.x, x[1] = u.y, x[2] = u.z, x[3] = u.w, x[4] = v.x, x[5] = v.y, x[6] = v.z, x[7] = v.w;
}

// The pre-pass: element i of W1 (then of W2) into its four planes.
__global__ __launch_bounds__(S360_BLOCK) void k_ffh_split(const float* __restrict__ w1, const float* __restrict__ w2, FFHPlanes pl) {
    const size_t i = (size_t)blockIdx.x * S360_BLOCK + threadIdx.x;
    __bf16 h, l;
    if (i < FFH_W1) {
        const size_t unit = i / FF_X, c = i % FF_X;
        bx3_split(w1[i], h, l);
        pl.w1_rh[i] = h, pl.w1_rl[i] = l;
        pl.w1_th[c * FF_H + unit] = h, pl.w1_tl[c * FF_H + unit] = l;
    } else if (i < FFH_W1 + FFH_W2) {
        const size_t k = i - FFH_W1, c = k / FF_H, unit = k % FF_H;
        bx3_split(w2[k], h, l);
        pl.w2_rh[k] = h, pl.w2_rl[k] = l;
        pl.w2_th[unit * FF_C + c] = h, pl.w2_tl[unit * FF_C + c] = l;
    }
}

// the lane's float64 (mean, rstd) of its token's m row: lane half hf sums channels 16 s + 8 hf + j, the halves are added
__device__ __forceinline__ void ffh_row_stats(const float* m_row, bool valid, int hf, double eps, double& mean, double& rstd) {
    float v[FF_C / 2];
#pragma unroll
    for (int s = 0; s < FF_C / 16; ++s) ffh_load8(m_row + 16 * s + 8 * hf, valid, v + 8 * s);
    double sum = 0.0, sq = 0.0;
#pragma unroll
    for (int i = 0; i < FF_C / 2; ++i) sum += (double)v[i];
    sum += __shfl_xor(sum, 32);
    mean = sum * FF_INV_C;
#pragma unroll
    for (int i = 0; i < FF_C / 2; ++i) {
        const double d = valid ? (double)v[i] - mean : 0.0;
        sq += d * d;
    }
    sq += __shfl_xor(sq, 32);
    rstd = 1.0 / sqrt(sq * FF_INV_C + eps);
}

// the token's row of X = [source, LN1(m)] as the B fragments of 16 k-steps: element j of step s is channel 16 s + 8 hf + j
__device__ __forceinline__ void ffh_load_x(const FFArgs& a, int token, bool valid, int hf, double mean, double rstd, bf16x8* xh, bf16x8* xl) {
    const size_t row = (size_t)token * FF_C;
#pragma unroll
    for (int s = 0; s < FF_C / 16; ++s) {
        float v[8];
        ffh_load8(a.source + row + 16 * s + 8 * hf, valid, v);
        bx3_split8(v, xh[s], xl[s]);
        ffh_load8(a.m + row + 16 * s + 8 * hf, valid, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = 16 * s + 8 * hf + j;
            v[j] = valid ? ff_norm(v[j], mean, rstd, a.n1w[c], a.n1b[c]) : 0.f;
        }
        bx3_split8(v, xh[FF_C / 16 + s], xl[FF_C / 16 + s]);
    }
}

// (X W1c^T)^T for the 32 units from j0: rows = hidden units, lane = token; w1h / w1l: the lane's row l31 of w1_r at channel 8 hf
__device__ __forceinline__ f32x16 ffh_pre(const __bf16* w1h, const __bf16* w1l, int j0, const bf16x8* xh, const bf16x8* xl) {
    f32x16 t = bx3_zero();
#pragma unroll
    for (int s = 0; s < FF_X / 16; ++s)
        t = bx3_mfma3<false>(bx3_ld8(w1h + (size_t)j0 * FF_X + 16 * s), bx3_ld8(w1l + (size_t)j0 * FF_X + 16 * s), xh[s], xl[s], t);
    return t;
}

// Forward, as k_ff_forward: 32 tokens per wave on the lanes, the hidden width in 32 chunks of 32 units.  Held to 256 registers (two
// waves per SIMD: one wave's erfc runs under the other's MFMAs and loads; 0.66 -> 0.54 ms at 65 536 tokens) at the price of 6
// spilled registers, outside the loop over the chunks.
__global__ __launch_bounds__(S360_BLOCK, 2) void k_ffh_forward(FFArgs a, FFHPlanes pl, float* __restrict__ out, float* __restrict__ z,
                                                               double* __restrict__ stats) {
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int token = blockIdx.x * FF_TM + wave * FF_T + l31;
    const bool valid = token < a.T;
    double mean1, rstd1;
    ffh_row_stats(a.m + (size_t)token * FF_C, valid, hf, a.eps, mean1, rstd1);
    bf16x8 xh[FF_X / 16], xl[FF_X / 16];
    ffh_load_x(a, token, valid, hf, mean1, rstd1, xh, xl);
    f32x16 zt[FF_C / FF_T];
#pragma unroll
    for (int ct = 0; ct < FF_C / FF_T; ++ct) zt[ct] = bx3_zero();
    const __bf16* w1h = pl.w1_rh + l31 * FF_X + 8 * hf;
    const __bf16* w1l = pl.w1_rl + l31 * FF_X + 8 * hf;
    const __bf16* w2h = pl.w2_rh + l31 * FF_H + 4 * hf;
    const __bf16* w2l = pl.w2_rl + l31 * FF_H + 4 * hf;
    for (int j0 = 0; j0 < FF_H; j0 += FF_T) {
        const f32x16 pre = ffh_pre(w1h, w1l, j0, xh, xl);
        float h[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = ff_gelu(pre[r]);
        bf16x8 hh[2], hl[2];
        bx3_split_tile(h, hh, hl);
#pragma unroll
        for (int ct = 0; ct < FF_C / FF_T; ++ct)              // z^T += W2c h^T
#pragma unroll
            for (int s = 0; s < 2; ++s)
                zt[ct] = bx3_mfma3<false>(bx3_ld44(w2h + ct * FF_T * FF_H + j0 + 16 * s), bx3_ld44(w2l + ct * FF_T * FF_H + j0 + 16 * s),
                                          hh[s], hl[s], zt[ct]);
    }
    // norm2 over the float32 z, the residual, the writes: as k_ff_forward
    double sum = 0.0, sq = 0.0;
#pragma unroll
    for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += (double)zt[ct][r];
    sum += __shfl_xor(sum, 32);
    const double mean2 = sum * FF_INV_C;
#pragma unroll
    for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const double d = (double)zt[ct][r] - mean2;
            sq += d * d;
        }
    sq += __shfl_xor(sq, 32);
    const double rstd2 = 1.0 / sqrt(sq * FF_INV_C + a.eps);
    if (!valid) return;
#pragma unroll
    for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c0 = ct * FF_T + 8 * q + 4 * hf;
            const size_t at = (size_t)token * FF_C + c0;
            const float4 sv = *reinterpret_cast<const float4*>(a.source + at);
            const float4 wv = *reinterpret_cast<const float4*>(a.n2w + c0);
            const float4 bv = *reinterpret_cast<const float4*>(a.n2b + c0);
            const float zr[4] = {zt[ct][4 * q], zt[ct][4 * q + 1], zt[ct][4 * q + 2], zt[ct][4 * q + 3]};
            float4 o;
            o.x = sv.x + ff_norm(zr[0], mean2, rstd2, wv.x, bv.x);
            o.y = sv.y + ff_norm(zr[1], mean2, rstd2, wv.y, bv.y);
            o.z = sv.z + ff_norm(zr[2], mean2, rstd2, wv.z, bv.z);
            o.w = sv.w + ff_norm(zr[3], mean2, rstd2, wv.w, bv.w);
            *reinterpret_cast<float4*>(out + at) = o;
            *reinterpret_cast<float4*>(z + at) = make_float4(zr[0], zr[1], zr[2], zr[3]);
        }
    if (hf == 0) {
        stats[(size_t)token * 2] = mean1, stats[(size_t)token * 2 + 1] = rstd1;
        stats[((size_t)a.T + token) * 2] = mean2, stats[((size_t)a.T + token) * 2 + 1] = rstd2;
    }
}

// Backward, the pass owned by token tiles, as k_ff_backward_tokens; dX is one float32 MFMA accumulation over the hidden width.
__global__ __launch_bounds__(S360_BLOCK) void k_ffh_backward_tokens(FFArgs a, FFHPlanes pl, const float* __restrict__ z,
                                                                    const double* __restrict__ stats, const float* __restrict__ g_out,
                                                                    float* __restrict__ g_source, float* __restrict__ g_m,
                                                                    double* __restrict__ ln_part) {
    __shared__ double s_wave[FF_WAVES][4 * FF_C];
    __shared__ double s_ln[4 * FF_C];
    __shared__ uint4 s_dz[FF_WAVES][2][FF_C / 16][S360_WAVE];  // dz's (hi, lo) fragments, each lane's 8 k-steps: written and read by that lane alone
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    for (int i = tid; i < 4 * FF_C; i += S360_BLOCK) s_ln[i] = 0.0;
    const __bf16* w1h = pl.w1_rh + l31 * FF_X + 8 * hf;
    const __bf16* w1l = pl.w1_rl + l31 * FF_X + 8 * hf;
    const __bf16* w2th = pl.w2_th + l31 * FF_C + 8 * hf;
    const __bf16* w2tl = pl.w2_tl + l31 * FF_C + 8 * hf;
    const __bf16* w1th = pl.w1_th + l31 * FF_H + 4 * hf;
    const __bf16* w1tl = pl.w1_tl + l31 * FF_H + 4 * hf;
    const int ntiles = (a.T + FF_TM - 1) / FF_TM;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int token = tile * FF_TM + wave * FF_T + l31;
        const bool valid = token < a.T;
        const size_t row = (size_t)token * FF_C;
        const double mean1 = valid ? stats[(size_t)token * 2] : 0.0, rstd1 = valid ? stats[(size_t)token * 2 + 1] : 0.0;
        const double mean2 = valid ? stats[((size_t)a.T + token) * 2] : 0.0, rstd2 = valid ? stats[((size_t)a.T + token) * 2 + 1] : 0.0;
        bf16x8 xh[FF_X / 16], xl[FF_X / 16];
        ffh_load_x(a, token, valid, hf, mean1, rstd1, xh, xl);
        {   // norm2's backward: element j of k-step s is channel 16 s + 8 hf + j
            double s1 = 0.0, s2 = 0.0;
            for (int s = 0; s < FF_C / 16; ++s) {
                float g[8], zz[8];
                ffh_load8(g_out + row + 16 * s + 8 * hf, valid, g);
                ffh_load8(z + row + 16 * s + 8 * hf, valid, zz);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const double gy = (double)g[j] * (double)a.n2w[16 * s + 8 * hf + j];
                    const double xn = valid ? ((double)zz[j] - mean2) * rstd2 : 0.0;
                    s1 += gy, s2 += gy * xn;
                }
            }
            s1 += __shfl_xor(s1, 32), s2 += __shfl_xor(s2, 32);
            s1 *= FF_INV_C, s2 *= FF_INV_C;
            for (int s = 0; s < FF_C / 16; ++s) {
                float g[8], zz[8], d[8];
                ffh_load8(g_out + row + 16 * s + 8 * hf, valid, g);
                ffh_load8(z + row + 16 * s + 8 * hf, valid, zz);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = 16 * s + 8 * hf + j;
                    const double gd = (double)g[j];
                    const double xn = valid ? ((double)zz[j] - mean2) * rstd2 : 0.0;
                    d[j] = (float)(rstd2 * (gd * (double)a.n2w[c] - s1 - xn * s2));
                    const double pw = ff_sum32(gd * xn), pb = ff_sum32(gd);
                    if (l31 == 0) s_wave[wave][2 * FF_C + c] = pw, s_wave[wave][3 * FF_C + c] = pb;
                }
                bf16x8 dh, dl;
                bx3_split8(d, dh, dl);
                s_dz[wave][0][s][lane] = __builtin_bit_cast(uint4, dh);
                s_dz[wave][1][s][lane] = __builtin_bit_cast(uint4, dl);
            }
        }
        f32x16 dx[FF_X / FF_T];                            // dX^T: tile ct, register r is channel 32 ct + mfma_acc_row(r, hf) of the lane's token
#pragma unroll
        for (int ct = 0; ct < FF_X / FF_T; ++ct) dx[ct] = bx3_zero();
        for (int j0 = 0; j0 < FF_H; j0 += FF_T) {
            const f32x16 pre = ffh_pre(w1h, w1l, j0, xh, xl);                   // X W1c^T again
            f32x16 dh = bx3_zero();                                             // (dz W2c)^T
#pragma unroll
            for (int s = 0; s < FF_C / 16; ++s)
                dh = bx3_mfma3<false>(bx3_ld8(w2th + (size_t)j0 * FF_C + 16 * s), bx3_ld8(w2tl + (size_t)j0 * FF_C + 16 * s),
                                      __builtin_bit_cast(bf16x8, s_dz[wave][0][s][lane]), __builtin_bit_cast(bf16x8, s_dz[wave][1][s][lane]), dh);
            float dp[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[r] = dh[r] * ff_gelu_grad(pre[r]);
            bf16x8 ph[2], pw[2];
            bx3_split_tile(dp, ph, pw);
#pragma unroll
            for (int ct = 0; ct < FF_X / FF_T; ++ct)          // dX^T += W1c^T dpre^T
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    dx[ct] = bx3_mfma3<false>(bx3_ld44(w1th + ct * FF_T * FF_H + j0 + 16 * s), bx3_ld44(w1tl + ct * FF_T * FF_H + j0 + 16 * s),
                                              ph[s], pw[s], dx[ct]);
        }
        // g_source = g_out + dX[:, :C]
        if (valid) {
#pragma unroll
            for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const size_t at = row + ct * FF_T + 8 * q + 4 * hf;
                    const float4 g = *reinterpret_cast<const float4*>(g_out + at);
                    *reinterpret_cast<float4*>(g_source + at) =
                        make_float4(g.x + dx[ct][4 * q], g.y + dx[ct][4 * q + 1], g.z + dx[ct][4 * q + 2], g.w + dx[ct][4 * q + 3]);
                }
        }
        {   // norm1's backward on dX[:, C:]
            double s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = ct * FF_T + mfma_acc_row(r, hf);
                    const double gy = (double)dx[FF_C / FF_T + ct][r] * (double)a.n1w[c];
                    const double xn = valid ? ((double)a.m[row + c] - mean1) * rstd1 : 0.0;
                    s1 += gy, s2 += gy * xn;
                }
            s1 += __shfl_xor(s1, 32), s2 += __shfl_xor(s2, 32);
            s1 *= FF_INV_C, s2 *= FF_INV_C;
#pragma unroll
            for (int ct = 0; ct < FF_C / FF_T; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = ct * FF_T + mfma_acc_row(r, hf);
                    const double g = (double)dx[FF_C / FF_T + ct][r];
                    const double xn = valid ? ((double)a.m[row + c] - mean1) * rstd1 : 0.0;
                    if (valid) g_m[row + c] = (float)(rstd1 * (g * (double)a.n1w[c] - s1 - xn * s2));
                    const double pw = ff_sum32(g * xn), pb = ff_sum32(g);
                    if (l31 == 0) s_wave[wave][c] = pw, s_wave[wave][FF_C + c] = pb;
                }
        }
        __syncthreads();
        for (int i = tid; i < 4 * FF_C; i += S360_BLOCK) {
            double v = s_ln[i];
#pragma unroll
            for (int w = 0; w < FF_WAVES; ++w) v += s_wave[w][i];
            s_ln[i] = v;
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = tid; i < 4 * FF_C; i += S360_BLOCK) ln_part[(size_t)blockIdx.x * 4 * FF_C + i] = s_ln[i];
}

// Backward, the pass owned by (hidden group of 128 units, token chunk), as k_ff_backward_weights: a tile of 32 tokens is staged
// in LDS as split bf16 — X [32][2C] and dz [32][C] by rows (the A operand of X W1c^T and dz W2c) and transposed (the A operand of
// dpre^T X and dz^T h, whose B operand is the accumulator tile) — and the unit's W1 row and W2 column are read from the planes.
__global__ __launch_bounds__(S360_BLOCK) void k_ffh_backward_weights(FFArgs a, FFHPlanes pl, const float* __restrict__ z,
                                                                     const double* __restrict__ stats, const float* __restrict__ g_out,
                                                                     int chunk_tokens, float* __restrict__ p_w1, float* __restrict__ p_w2) {
    __shared__ __attribute__((aligned(16))) __bf16 s_xr[2][FF_T * FFH_LDR];
    __shared__ __attribute__((aligned(16))) __bf16 s_dr[2][FF_T * FFH_LDD];
    __shared__ __attribute__((aligned(16))) __bf16 s_xt[2][FF_X * FFH_LDT];
    __shared__ __attribute__((aligned(16))) __bf16 s_dt[2][FF_C * FFH_LDT];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int j0 = (blockIdx.x * FF_WAVES + wave) * FF_T, chunk = blockIdx.y;
    const int first = chunk * chunk_tokens, last = min(a.T, first + chunk_tokens);
    const __bf16* w1h = pl.w1_rh + (size_t)(j0 + l31) * FF_X + 8 * hf;
    const __bf16* w1l = pl.w1_rl + (size_t)(j0 + l31) * FF_X + 8 * hf;
    const __bf16* w2th = pl.w2_th + (size_t)(j0 + l31) * FF_C + 8 * hf;
    const __bf16* w2tl = pl.w2_tl + (size_t)(j0 + l31) * FF_C + 8 * hf;
    f32x16 gw1[FF_X / FF_T], gw2[FF_C / FF_T];             // g_W1^T, g_W2: rows = channels, lane = hidden unit
#pragma unroll
    for (int ct = 0; ct < FF_X / FF_T; ++ct) gw1[ct] = bx3_zero();
#pragma unroll
    for (int ct = 0; ct < FF_C / FF_T; ++ct) gw2[ct] = bx3_zero();
    const int slot = tid >> 5, l = tid & 31;
    const float4 n1w = *reinterpret_cast<const float4*>(a.n1w + 4 * l), n1b = *reinterpret_cast<const float4*>(a.n1b + 4 * l);
    const float4 n2w = *reinterpret_cast<const float4*>(a.n2w + 4 * l);
    for (int t0 = first; t0 < last; t0 += FF_T) {
        __syncthreads();                                      // the previous tile has been read
#pragma unroll
        for (int it = 0; it < FF_T / FF_ROWS; ++it) {
            const int tl = it * FF_ROWS + slot, token = t0 + tl;
            float4 sv = make_float4(0.f, 0.f, 0.f, 0.f), xv = sv, dv = sv;
            if (token < last) {                               // uniform over the 32 lanes of a row
                const size_t at = (size_t)token * FF_C + 4 * l;
                sv = *reinterpret_cast<const float4*>(a.source + at);
                xv = ff_norm4(*reinterpret_cast<const float4*>(a.m + at), stats[(size_t)token * 2], stats[(size_t)token * 2 + 1], n1w, n1b);
                double xn[4];
                dv = ff_row_backward(*reinterpret_cast<const float4*>(z + at), *reinterpret_cast<const float4*>(g_out + at), n2w,
                                     stats[((size_t)a.T + token) * 2], stats[((size_t)a.T + token) * 2 + 1], xn);
            }
            const float xs[8] = {sv.x, sv.y, sv.z, sv.w, xv.x, xv.y, xv.z, xv.w}, ds[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = (i < 4 ? 0 : FF_C - 4) + 4 * l + i;
                __bf16 h, lo;
                bx3_split(xs[i], h, lo);
                s_xr[0][tl * FFH_LDR + c] = h, s_xr[1][tl * FFH_LDR + c] = lo;
                s_xt[0][c * FFH_LDT + tl] = h, s_xt[1][c * FFH_LDT + tl] = lo;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 4 * l + i;
                __bf16 h, lo;
                bx3_split(ds[i], h, lo);
                s_dr[0][tl * FFH_LDD + c] = h, s_dr[1][tl * FFH_LDD + c] = lo;
                s_dt[0][c * FFH_LDT + tl] = h, s_dt[1][c * FFH_LDT + tl] = lo;
            }
        }
        __syncthreads();
        f32x16 pre = bx3_zero(), dh = bx3_zero();             // X W1c^T, dz W2c: rows = tokens, lane = hidden unit
#pragma unroll
        for (int s = 0; s < FF_X / 16; ++s)
            pre = bx3_mfma3<true>(bx3_ld8(s_xr[0] + l31 * FFH_LDR + 16 * s + 8 * hf), bx3_ld8(s_xr[1] + l31 * FFH_LDR + 16 * s + 8 * hf),
                                  bx3_ld8(w1h + 16 * s), bx3_ld8(w1l + 16 * s), pre);
#pragma unroll
        for (int s = 0; s < FF_C / 16; ++s)
            dh = bx3_mfma3<true>(bx3_ld8(s_dr[0] + l31 * FFH_LDD + 16 * s + 8 * hf), bx3_ld8(s_dr[1] + l31 * FFH_LDD + 16 * s + 8 * hf),
                                 bx3_ld8(w2th + 16 * s), bx3_ld8(w2tl + 16 * s), dh);
        float dp[16], h[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            dp[r] = dh[r] * ff_gelu_grad(pre[r]);
            h[r] = ff_gelu(pre[r]);
        }
        bf16x8 ph[2], pw[2], hh[2], hl[2];
        bx3_split_tile(dp, ph, pw);
        bx3_split_tile(h, hh, hl);
#pragma unroll
        for (int ct = 0; ct < FF_X / FF_T; ++ct)              // g_W1^T += X^T dpre
#pragma unroll
            for (int s = 0; s < 2; ++s)
                gw1[ct] = bx3_mfma3<true>(bx3_ld44(s_xt[0] + (ct * FF_T + l31) * FFH_LDT + 16 * s + 4 * hf),
                                          bx3_ld44(s_xt[1] + (ct * FF_T + l31) * FFH_LDT + 16 * s + 4 * hf), ph[s], pw[s], gw1[ct]);
#pragma unroll
        for (int ct = 0; ct < FF_C / FF_T; ++ct)              // g_W2 += dz^T h
#pragma unroll
            for (int s = 0; s < 2; ++s)
                gw2[ct] = bx3_mfma3<true>(bx3_ld44(s_dt[0] + (ct * FF_T + l31) * FFH_LDT + 16 * s + 4 * hf),
                                          bx3_ld44(s_dt[1] + (ct * FF_T + l31) * FFH_LDT + 16 * s + 4 * hf), hh[s], hl[s], gw2[ct]);
    }
    float* q1 = p_w1 + ((size_t)chunk * FF_H + j0 + l31) * FF_X;
    float* q2 = p_w2 + (size_t)chunk * FF_C * FF_H + j0 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int ct = 0; ct < FF_X / FF_T; ++ct) q1[ct * FF_T + mfma_acc_row(r, hf)] = gw1[ct][r];
#pragma unroll
        for (int ct = 0; ct < FF_C / FF_T; ++ct) q2[(size_t)(ct * FF_T + mfma_acc_row(r, hf)) * FF_H] = gw2[ct][r];
    }
}

// the planes in the first FFH_PLANE_BYTES of a scratch, and the pre-pass
static FFHPlanes ffh_planes(void* scratch) {
    Bx3Carver c{static_cast<char*>(scratch)};
    FFHPlanes pl;
    c.take(FFH_W1, &pl.w1_rh, &pl.w1_rl);
    c.take(FFH_W1, &pl.w1_th, &pl.w1_tl);
    c.take(FFH_W2, &pl.w2_rh, &pl.w2_rl);
    c.take(FFH_W2, &pl.w2_th, &pl.w2_tl);
    return pl;
}
static void ffh_split_launch(const float* w1, const float* w2, const FFHPlanes& pl, hipStream_t st) {
    hipLaunchKernelGGL(k_ffh_split, dim3((unsigned)((FFH_W1 + FFH_W2 + S360_BLOCK - 1) / S360_BLOCK)), dim3(S360_BLOCK), 0, st, w1, w2, pl);
}

// ---------------------------------------------------------------------------------------------- the entry points, both modes
// The caller's scratch, one order in both modes: in "high" the weights' bf16 planes at the front, then, for a backward, the
// per-chunk partials of g_w1, those of g_w2 and the LayerNorm partial sums (of the token pass or the row backward, whichever has
// more workgroups).  Byte offsets; `bytes` is what the *_scratch_bytes functions report.
struct FFLayout {
    size_t p_w1, p_w2, ln_part, bytes;
};
static FFLayout ff_layout(int64_t T, bool high, bool backward) {
    const size_t chunks = backward ? ff_chunks(T) : 0, wgs = backward ? max(ff_token_wgs(T), ff_row_wgs(T)) : 0;
    FFLayout l;
    l.p_w1 = high ? FFH_PLANE_BYTES : 0;
    l.p_w2 = l.p_w1 + chunks * FF_H * FF_X * sizeof(float);
    l.ln_part = l.p_w2 + chunks * FF_C * FF_H * sizeof(float);
    l.bytes = l.ln_part + wgs * 4 * FF_C * sizeof(double);
    return l;
}

// What every launch entry starts with, in the order of include/s360.h's refusals: the pointer rule, eps (has_eps: every entry
// but the row backward, which reads rstd from stats), the sizes.  After S360_OK *eps may be read.
template <size_t NI, size_t NO>
static int ff_setup(const void* const (&in)[NI], const void* const (&outs)[NO], bool has_eps, const double* eps, int32_t tokens,
                    int32_t channels, int32_t hidden) {
    if (!s360_pointers_ok(in, outs)) return S360_E_BADARG;
    if (has_eps && (!eps || !(*eps > 0.0))) return S360_E_BADARG;
    return ff_sizes(tokens, channels, hidden);
}

struct FFGrads {
    float *source, *m, *w1, *w2, *n1w, *n1b, *n2w, *n2b;
};

// s360_ffn_tail_backward (HIGH = false) and s360_ffn_tail_high_backward (true): the pre-pass and the two kernels differ.
// `a` comes with its pointers set.
template <bool HIGH>
static int ff_backward(FFArgs a, const float* z, const double* stats, const float* g_out, int32_t tokens, int32_t channels, int32_t hidden,
                       const double* eps, void* scratch, size_t scratch_bytes, const FFGrads& g, hipStream_t st) {
    const void* const in[] = {a.source, a.m, a.n1w, a.n1b, a.w1, a.w2, a.n2w, a.n2b, z, stats, g_out};
    const void* const outs[] = {g.source, g.m, g.w1, g.w2, g.n1w, g.n1b, g.n2w, g.n2b, scratch};
    const int rc = ff_setup(in, outs, true, eps, tokens, channels, hidden);
    if (rc != S360_OK) return rc;
    a.T = tokens, a.eps = *eps;
    const FFLayout l = ff_layout(tokens, HIGH, true);
    if (scratch_bytes < l.bytes) return S360_E_WORKSPACE;
    const int chunks = ff_chunks(tokens), wgs = ff_token_wgs(tokens);
    char* base = static_cast<char*>(scratch);
    float *p_w1 = reinterpret_cast<float*>(base + l.p_w1), *p_w2 = reinterpret_cast<float*>(base + l.p_w2);
    double* ln_part = reinterpret_cast<double*>(base + l.ln_part);
    if constexpr (HIGH) {
        const FFHPlanes pl = ffh_planes(scratch);
        ffh_split_launch(a.w1, a.w2, pl, st);
        S360_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_ffh_backward_tokens, dim3(wgs), dim3(S360_BLOCK), 0, st, a, pl, z, stats, g_out, g.source, g.m, ln_part);
        S360_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_ffh_backward_weights, dim3(FF_H / (FF_T * FF_WAVES), chunks), dim3(S360_BLOCK), 0, st, a, pl, z, stats, g_out,
                           ff_chunk_tokens(tokens), p_w1, p_w2);
    } else {
        hipLaunchKernelGGL(k_ff_backward_tokens, dim3(wgs), dim3(S360_BLOCK), 0, st, a, z, stats, g_out, g.source, g.m, ln_part);
        S360_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_ff_backward_weights, dim3(FF_H / (FF_T * FF_WAVES), chunks), dim3(S360_BLOCK), 0, st, a, z, stats, g_out,
                           ff_chunk_tokens(tokens), p_w1, p_w2);
    }
    S360_CHECK_LAUNCH();
    const int nw1 = FF_H * FF_X, nw2 = FF_C * FF_H, nln = 4 * FF_C;
    const FFLnOut lo = {{g.n1w, g.n1b, g.n2w, g.n2b}};
    hipLaunchKernelGGL(k_ff_reduce, dim3((nw1 + nw2 + nln + S360_BLOCK - 1) / S360_BLOCK), dim3(S360_BLOCK), 0, st, p_w1, p_w2, chunks, nw1,
                       nw2, g.w1, g.w2, ln_part, wgs, nln, lo);
    return s360_launch_status();
}

}  // namespace s360

using namespace s360;

extern "C" size_t s360_ffn_tail_scratch_bytes(int32_t tokens) { return tokens < 1 ? 0 : ff_layout(tokens, false, true).bytes; }

extern "C" size_t s360_ffn_tail_high_scratch_bytes(int32_t tokens, int32_t backward) {
    return tokens < 1 ? 0 : ff_layout(tokens, true, backward != 0).bytes;
}

extern "C" int s360_ffn_tail_weight_chunks(int32_t tokens) { return tokens < 1 ? 0 : ff_chunks(tokens); }

extern "C" int s360_ffn_tail_forward(const float* source, const float* m, const float* norm1_weight, const float* norm1_bias,
                                     const float* w1, const float* w2, const float* norm2_weight, const float* norm2_bias, int32_t tokens,
                                     int32_t channels, int32_t hidden, const double* eps, float* out, float* z, double* stats, void* stream) {
    const void* const in[] = {source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias};
    const void* const outs[] = {out, z, stats};
    const int rc = ff_setup(in, outs, true, eps, tokens, channels, hidden);
    if (rc != S360_OK) return rc;
    const FFArgs a = {source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, tokens, *eps};
    hipLaunchKernelGGL(k_ff_forward, dim3((tokens + FF_TM - 1) / FF_TM), dim3(S360_BLOCK), 0, (hipStream_t)stream, a, out, z, stats);
    return s360_launch_status();
}

extern "C" int s360_ffn_tail_high_forward(const float* source, const float* m, const float* norm1_weight, const float* norm1_bias,
                                          const float* w1, const float* w2, const float* norm2_weight, const float* norm2_bias,
                                          int32_t tokens, int32_t channels, int32_t hidden, const double* eps, float* out, float* z,
                                          double* stats, void* scratch, size_t scratch_bytes, void* stream) {
    const void* const in[] = {source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias};
    const void* const outs[] = {out, z, stats, scratch};
    const int rc = ff_setup(in, outs, true, eps, tokens, channels, hidden);
    if (rc != S360_OK) return rc;
    const FFArgs a = {source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, tokens, *eps};
    if (scratch_bytes < ff_layout(tokens, true, false).bytes) return S360_E_WORKSPACE;   // after the sizes, as the size depends on them
    const FFHPlanes pl = ffh_planes(scratch);
    ffh_split_launch(w1, w2, pl, (hipStream_t)stream);
    S360_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ffh_forward, dim3((tokens + FF_TM - 1) / FF_TM), dim3(S360_BLOCK), 0, (hipStream_t)stream, a, pl, out, z, stats);
    return s360_launch_status();
}

extern "C" int s360_ffn_tail_backward(const float* source, const float* m, const float* norm1_weight, const float* norm1_bias,
                                      const float* w1, const float* w2, const float* norm2_weight, const float* norm2_bias, const float* z,
                                      const double* stats, const float* g_out, int32_t tokens, int32_t channels, int32_t hidden,
                                      const double* eps, void* scratch, size_t scratch_bytes, float* g_source, float* g_m, float* g_w1,
                                      float* g_w2, float* g_norm1_weight, float* g_norm1_bias, float* g_norm2_weight, float* g_norm2_bias,
                                      void* stream) {
    return ff_backward<false>({source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias}, z, stats, g_out, tokens, channels, hidden,
                              eps, scratch, scratch_bytes,
                              {g_source, g_m, g_w1, g_w2, g_norm1_weight, g_norm1_bias, g_norm2_weight, g_norm2_bias}, (hipStream_t)stream);
}

extern "C" int s360_ffn_tail_high_backward(const float* source, const float* m, const float* norm1_weight, const float* norm1_bias,
                                           const float* w1, const float* w2, const float* norm2_weight, const float* norm2_bias,
                                           const float* z, const double* stats, const float* g_out, int32_t tokens, int32_t channels,
                                           int32_t hidden, const double* eps, void* scratch, size_t scratch_bytes, float* g_source,
                                           float* g_m, float* g_w1, float* g_w2, float* g_norm1_weight, float* g_norm1_bias,
                                           float* g_norm2_weight, float* g_norm2_bias, void* stream) {
    return ff_backward<true>({source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias}, z, stats, g_out, tokens, channels, hidden,
                             eps, scratch, scratch_bytes,
                             {g_source, g_m, g_w1, g_w2, g_norm1_weight, g_norm1_bias, g_norm2_weight, g_norm2_bias}, (hipStream_t)stream);
}

extern "C" int s360_layer_norm_residual_forward(const float* x, const float* weight, const float* bias, const float* residual, int32_t tokens,
                                                int32_t channels, const double* eps, float* out, double* stats, void* stream) {
    const void* const in[] = {x, weight, bias, residual};
    const void* const outs[] = {out, stats};
    const int rc = ff_setup(in, outs, true, eps, tokens, channels, FF_H);
    if (rc != S360_OK) return rc;
    hipLaunchKernelGGL(k_ff_norm_residual_forward, dim3((tokens + FF_ROWS - 1) / FF_ROWS), dim3(S360_BLOCK), 0, (hipStream_t)stream, x, weight,
                       bias, residual, tokens, *eps, out, stats);
    return s360_launch_status();
}

extern "C" int s360_layer_norm_residual_backward(const float* x, const float* weight, const double* stats, const float* g_out, int32_t tokens,
                                                 int32_t channels, void* scratch, size_t scratch_bytes, float* g_x, float* g_residual,
                                                 float* g_weight, float* g_bias, void* stream) {
    const void* const in[] = {x, weight, stats, g_out};
    const void* const outs[] = {g_x, g_residual, g_weight, g_bias, scratch};
    const int rc = ff_setup(in, outs, false, nullptr, tokens, channels, FF_H);
    if (rc != S360_OK) return rc;
    if (scratch_bytes < ff_layout(tokens, false, true).bytes) return S360_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int wgs = ff_row_wgs(tokens);
    double* ln_part = static_cast<double*>(scratch);                                          // alone in the scratch, at its start
    hipLaunchKernelGGL(k_ff_norm_residual_backward, dim3(wgs), dim3(S360_BLOCK), 0, st, x, weight, stats, g_out, tokens, g_x, g_residual, ln_part);
    S360_CHECK_LAUNCH();
    const int nln = 2 * FF_C;
    const FFLnOut lo = {{g_weight, g_bias, nullptr, nullptr}};
    hipLaunchKernelGGL(k_ff_reduce, dim3((nln + S360_BLOCK - 1) / S360_BLOCK), dim3(S360_BLOCK), 0, st, nullptr, nullptr, 0, 0, 0, nullptr,
                       nullptr, ln_part, wgs, nln, lo);
    return s360_launch_status();
}
