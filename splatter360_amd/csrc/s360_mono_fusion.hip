// s360_mono_fusion.hip — the mono-feature fusion of the cost-volume encoder (the reference's
// src/model/encoder/encoder_costvolume.py:297, :351-354 with the rgbd_fusion of :119-125), forward and backward, as fused
// kernels.  gfx950 only.
//
//   m    = Cube2Equirec(mono_cube)                [T, Cm]      the 8-tap float32 stitch, a constant (no gradient)
//   X    = cat(erp_feat, m)                       [T, C + Cm]  token t = (n, y, x), T = N H W
//   yv   = X W1^T                                 [T, C]       W1 [C, C + Cm], W2 [C, C] in nn.Linear's layout, no biases
//   a    = relu(LN(yv))                           [T, C]       LayerNorm: biased variance, eps as passed, affine
//   out  = a W2^T                                 [N, C, H, W]
// C = 128, Cm a multiple of 64 up to 1024.  Neither the stitched map [N, Cm, H, W] nor X (nor its channel-last copy) exists in
// memory, forward or backward.
//
// Every product runs on v_mfma_f32_32x32x2_f32 (exact float32 products, float32 accumulation) in the orientation of
// s360_transformer_ffn.hip: in the token-owned kernels 32 tokens of a wave sit on the lanes (the B operand, in registers:
// element 2 s + hf of the token's row at MFMA step s of lane half hf), the weights sit on the accumulator's rows (the A operand,
// read from LDS), and an accumulator tile is, register by register, the B operand of the next product.  Four waves = 128 tokens
// per workgroup; tokens are flattened over N H W, so a tile may span two panoramas.
// Forward (k_mf_forward): K = C + Cm is walked in chunks of 64 channels.  A chunk's slice of W1 ([C, 64], 33 KB, odd row stride)
// is staged once per workgroup in LDS and serves the four waves.  The lane's 32 values of the chunk come from erp_feat
// (token-contiguous per channel: coalesced) or from the stitch: the eight tap offsets and weights are formed once per token
// (s360_stitch_taps.h, the expressions of s360_cube2erp_forward; a tap outside the volume — always one of weight 0 at index fw or
// face 6 — is clamped to a valid address and not added) and reused for all Cm channels.  Each chunk is one float32 chain of 32
// MFMA steps from zero per output tile; the chunks are added in float64.  The LayerNorm row (float64 mean, two-pass biased
// variance, rstd; float64 per element, rounded once) and the ReLU are the epilogue; a W2^T follows from the accumulator tiles
// with W2 staged in two halves (float32 chains of 32 channels added in float64).  The call writes out (NCHW), y = yv [T, C]
// float32 and stats [T, 2] float64 (mean, rstd).
// Backward, three launches:
//   k_mf_backward_tokens   one workgroup per token tile: g_a = g_out W2 (two float32 chains of 64 added in
//                          float64), ReLU's mask from the forward's own float32 LN value (derivative 0 at exactly 0), LayerNorm's
//                          backward -> g_y, g_erp_feat = g_y W1[:, :C] (chains of 32 added in float64) written NCHW, float64
//                          partial sums of g_ln_weight / g_ln_bias per workgroup.  g_y is HANDED OVER to the next launch through
//                          scratch (T C 4 bytes) rather than recomputed: the weight pass then needs no product of its own to
//                          get it.
//   k_mf_backward_weights  (64 columns of g_W1 or g_W2, token chunk): g_W1 = sum_t g_y[t] (x) X[t] (the mono taps are gathered
//                          again), g_W2 = sum_t g_out[t] (x) a[t] (a recomputed from y and stats).  Tiles of 64 tokens staged in
//                          LDS, one float32 chain per tile, the tiles of a chunk added in float64; per-chunk float32 partials to
//                          scratch.
//   k_mf_reduce            the partials added in the order 0, 1, ... in float64, rounded once.
// Scratch: T C 4 (g_y) + chunks (C (C + Cm) + C C) 4 (partials) + workgroups 2 C 8 (LayerNorm partials) bytes,
// s360_mono_fusion_scratch_bytes.  No atomics; every sum has a fixed order; every output element is written exactly once:
// bit-identical from run to run and across streams.
// Measured on one MI355X (profiles/mono_fusion_timing.json, profiles/mono_fusion_kernel_trace.txt; this / the reference's lines in
// float32 torch): 65 536 tokens, Cm = 384: forward 0.408 / 1.136 ms, forward + backward 1.190 / 1.999 ms — ahead of torch by 2.79 x and 1.68 x;
// Cm = 768: 0.736 / 2.169 ms and 1.802 / 3.174 ms, 2.95 x and 1.76 x.
// Kernels at Cm = 384: forward 386 us (27.8 TFLOP/s of the two products, 17.7 % of the float32 MFMA peak, the gather not counted),
// token-owned pass 143 us, weight-owned pass 535 us, reduction 23 us.  Forward + backward peak memory 246 / 553 MiB.
//
// The "high" precision mode (the k_mfh_* kernels at the end of this file; s360_mono_fusion_high_*): the same function with all six
// products as bf16x3 products on v_mfma_f32_32x32x16_bf16 (s360_bf16x3.h), what torch.set_float32_matmul_precision('high') asks for.
// Order of each product's operand pair: (weight, token side) for X W1^T, a W2^T, g_out W2 and g_y W1[:, :C] — the weight is the A
// operand in all four — and (gradient, activation) for the two token-by-token products g_y^T X and g_out^T a, the gradient being
// the A operand; SWAP = false throughout.  W1 and W2 are split once per call into bf16 planes in the caller's scratch; the token
// side is split where it is loaded, gathered or produced.  Launch geometry, g_y's hand-over, partials and k_mf_reduce as above.
// Measured on the same MI355X (profiles/mono_fusion_high_timing.json, profiles/mono_fusion_high_kernel_trace.txt; "high" /
// "highest" / the reference's lines under torch's 'high' / in float32 torch, medians of 50 calls, three collections):
// Cm = 384 forward 0.349 / 0.409 / 1.111 / 1.149 ms, forward + backward 1.049 / 1.191 / 2.236 / 1.992 ms; Cm = 768 forward
// 0.618 / 0.740 / 2.105 / 2.170 ms, forward + backward 1.568 / 1.771 / 3.347 / 3.168 ms: "high" is ahead of "highest" by 1.17 x,
// 1.14 x, 1.20 x and 1.13 x and of torch under 'high' by 3.18 x, 2.13 x, 3.41 x and 2.13 x, in every leg by more than the spread of
// the three medians (forward at most 0.009 ms; forward + backward at most 0.050 ms, where the smallest lead is 0.142 ms).  Kernels
// at Cm = 384: forward 314 us (386), token-owned pass 127 us (143), weight-owned pass 452 us (535), reduction 24 us, the pre-pass
// 5 us per call.  With the matrix cycles cut the forward is bound by the gather of 8 x Cm taps per token at one wave per SIMD, and the
// weight-owned pass by the latency of a tile's loads: 320 workgroups walk 32 tiles each, alone on their compute units.
#include "s360_device.h"
#include "s360_bf16x3.h"
#include "s360_stitch_taps.h"

namespace s360 {

constexpr int MF_C = 128;                                     // channels of erp_feat and of the output
constexpr int MF_T = 32;                                      // rows of an MFMA tile
constexpr int MF_WAVES = S360_BLOCK / S360_WAVE;
constexpr int MF_TM = MF_T * MF_WAVES;                        // tokens of a workgroup in the token-owned kernels
constexpr int MF_KC = 64;                                     // channels of a K chunk (32 MFMA steps: one float32 chain)
constexpr int MF_LDK = MF_KC + 1;                             // row stride of a staged [C][64] slice (floats)
constexpr int MF_LDC = MF_C + 1;                              // row stride of a staged [64][C] slice
constexpr int MF_STAGE = MF_C * MF_LDK > MF_KC * MF_LDC ? MF_C * MF_LDK : MF_KC * MF_LDC;
constexpr int MF_WT = 64;                                     // tokens of a tile of the weight-owned pass
constexpr int MF_MAX_CM = 1024;
constexpr int MF_MAX_CHUNKS = 32;                             // token chunks of the weight-gradient pass, at most
constexpr double MF_INV_C = 1.0 / MF_C;

struct MFArgs {
    const float *erp, *cube, *grid, *w1, *lnw, *lnb, *w2;
    int T, HW, Cm, fw;
    double eps;
};

__device__ __forceinline__ double mf_sum32(double v) {        // over the 32 lanes of a lane half, the same bits in each
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ float mf_norm(float v, double mean, double rstd, float w, float b) {
    return (float)(((double)v - mean) * rstd * (double)w + (double)b);
}

// The eight taps of a pixel over a channel plane [fw, 6 fw] of mono_cube (faces side by side): offsets, weights and the mask of
// the taps inside the volume, in the order 4 dz + 2 dy + dx of k_cube2erp_fwd.
struct MFTaps {
    int off[8];
    float wgt[8];
    unsigned in;
};

__device__ __forceinline__ MFTaps mf_taps(const float* __restrict__ grid, int pixel, int fw) {
    const StitchFrac f = stitch_frac(grid, (size_t)pixel, fw);
    MFTaps t;
    t.in = 0u;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        const int z = f.z0 + dz, zc = min(max(z, 0), 5);
        const bool zin = z >= 0 && z <= 5;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = f.y0 + dy, yc = min(max(y, 0), fw - 1);
            const bool yin = y >= 0 && y < fw;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = f.x0 + dx, xc = min(max(x, 0), fw - 1);
                const bool xin = x >= 0 && x < fw;
                const int k = 4 * dz + 2 * dy + dx;
                t.off[k] = (yc * 6 + zc) * fw + xc;
                t.wgt[k] = f.wx[dx] * f.wy[dy] * f.wz[dz];
                t.in |= (zin && yin && xin) ? 1u << k : 0u;
            }
        }
    }
    return t;
}

// the stitch's value of one channel plane: eight independent loads, then the sum in tap order (k_cube2erp_fwd's)
__device__ __forceinline__ float mf_gather(const float* __restrict__ plane, const MFTaps& t) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = plane[t.off[k]];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = (t.in >> k) & 1u ? acc + v[k] * t.wgt[k] : acc;
    return acc;
}

// x[s] = X[token][64 kc + 2 s + hf]: chunks 0 and 1 are erp_feat, the others the stitch of mono_cube; zeros unless valid
// (n, pixel are those of a token inside the tensor either way)
__device__ __forceinline__ void mf_load_x(const MFArgs& a, int kc, int n, int pixel, bool valid, int hf, const MFTaps& tp, float* x) {
    if (kc < MF_C / MF_KC) {
        const float* p = a.erp + ((size_t)n * MF_C + kc * MF_KC + hf) * a.HW + pixel;
#pragma unroll
        for (int s = 0; s < MF_KC / 2; ++s) {
            const float v = p[(size_t)(2 * s) * a.HW];
            x[s] = valid ? v : 0.f;
        }
    } else {
        const size_t cs = (size_t)6 * a.fw * a.fw;
        const float* p = a.cube + ((size_t)n * a.Cm + (kc * MF_KC - MF_C) + hf) * cs;
#pragma unroll
        for (int s = 0; s < MF_KC / 2; ++s) {
            const float v = mf_gather(p + (size_t)(2 * s) * cs, tp);
            x[s] = valid ? v : 0.f;
        }
    }
}

// t[row][lane] += sum over the 32 rows k of a tile w held register by register of A[row][k] w[k][lane]; a points at (k = 4 hf,
// row l31) of an LDS image with k-stride ld
__device__ __forceinline__ f32x16 mf_fold(const float* a, int ld, const float* w, f32x16 t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) t = __builtin_amdgcn_mfma_f32_32x32x2f32(a[((r & 3) + 8 * (r >> 2)) * ld], w[r], t, 0, 0, 0);
    return t;
}

__device__ __forceinline__ f32x16 mf_zero() {
    f32x16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.f;
    return t;
}

// rows [0, rows) x columns [c0, c0 + 64) of a row-major matrix of row length ld_src -> s[row][MF_LDK]
__device__ __forceinline__ void mf_stage_columns(const float* __restrict__ src, int ld_src, int c0, float* s, int tid) {
    for (int idx = tid; idx < MF_C * MF_KC; idx += S360_BLOCK) s[(idx >> 6) * MF_LDK + (idx & 63)] = src[(size_t)(idx >> 6) * ld_src + c0 + (idx & 63)];
}

// Forward: out [N, C, H, W], y [T, C] (the first Linear's output, float32), stats [T, 2] = (mean, rstd) over the float32 y.
__global__ __launch_bounds__(S360_BLOCK) void k_mf_forward(MFArgs a, float* __restrict__ out, float* __restrict__ y, double* __restrict__ stats) {
    __shared__ float s_w[MF_STAGE];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int token = blockIdx.x * MF_TM + wave * MF_T + l31;
    const bool valid = token < a.T;
    const int tk = valid ? token : 0, n = tk / a.HW, pixel = tk - n * a.HW;
    const MFTaps tp = mf_taps(a.grid, pixel, a.fw);
    const int K = MF_C + a.Cm;
    double acc[MF_C / MF_T][16];
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ot][r] = 0.0;
    for (int kc = 0; kc < K / MF_KC; ++kc) {
        float x[MF_KC / 2];
        mf_load_x(a, kc, n, pixel, valid, hf, tp, x);
        __syncthreads();                                      // the previous chunk has been read
        mf_stage_columns(a.w1, K, kc * MF_KC, s_w, tid);
        __syncthreads();
#pragma unroll
        for (int ot = 0; ot < MF_C / MF_T; ++ot) {            // (X W1c^T)^T: rows = output channels, lane = token
            const float* ap = s_w + (ot * MF_T + l31) * MF_LDK + hf;
            f32x16 t = mf_zero();
#pragma unroll
            for (int s = 0; s < MF_KC / 2; ++s) t = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], x[s], t, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ot][r] += (double)t[r];
        }
    }
    // LayerNorm over the float32 y and the ReLU: register r of tile ot is channel 32 ot + mfma_acc_row(r, hf)
    float av[MF_C / MF_T][16];
    double sum = 0.0, sq = 0.0;
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
        for (int r = 0; r < 16; ++r) av[ot][r] = (float)acc[ot][r], sum += (double)av[ot][r];
    sum += __shfl_xor(sum, 32);
    const double mean = sum * MF_INV_C;
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const double d = (double)av[ot][r] - mean;
            sq += d * d;
        }
    sq += __shfl_xor(sq, 32);
    const double rstd = 1.0 / sqrt(sq * MF_INV_C + a.eps);
    if (valid) {
#pragma unroll
        for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<float4*>(y + (size_t)token * MF_C + ot * MF_T + 8 * q + 4 * hf) =
                    make_float4(av[ot][4 * q], av[ot][4 * q + 1], av[ot][4 * q + 2], av[ot][4 * q + 3]);
        if (hf == 0) stats[(size_t)token * 2] = mean, stats[(size_t)token * 2 + 1] = rstd;
    }
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = ot * MF_T + mfma_acc_row(r, hf);
            av[ot][r] = fmaxf(mf_norm(av[ot][r], mean, rstd, a.lnw[c], a.lnb[c]), 0.f);
            acc[ot][r] = 0.0;
        }
    // out^T = W2 a^T: W2's columns in two halves of 64, each tile of 32 a float32 chain added in float64
#pragma unroll
    for (int h = 0; h < MF_C / MF_KC; ++h) {
        __syncthreads();
        mf_stage_columns(a.w2, MF_C, h * MF_KC, s_w, tid);
        __syncthreads();
#pragma unroll
        for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
            for (int jt = 0; jt < MF_KC / MF_T; ++jt) {
                const f32x16 t = mf_fold(s_w + (ot * MF_T + l31) * MF_LDK + jt * MF_T + 4 * hf, 1, av[h * (MF_KC / MF_T) + jt], mf_zero());
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ot][r] += (double)t[r];
            }
    }
    if (!valid) return;
    float* po = out + (size_t)n * MF_C * a.HW + pixel;
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
        for (int r = 0; r < 16; ++r) po[(size_t)(ot * MF_T + mfma_acc_row(r, hf)) * a.HW] = (float)acc[ot][r];
}

// Backward, the pass owned by token tiles: g_erp [N, C, H, W], g_y [T, C] (scratch, for the weight pass) and the per-workgroup
// float64 partial sums ln_part[workgroup][g_ln_weight | g_ln_bias][C].  One workgroup per tile of 128 tokens (walking several
// tiles in a loop lets the compiler keep the 128 LayerNorm parameters of a lane live across it: 216 spilled registers).
__global__ __launch_bounds__(S360_BLOCK) void k_mf_backward_tokens(MFArgs a, const float* __restrict__ y, const double* __restrict__ stats,
                                                                   const float* __restrict__ g_out, float* __restrict__ g_erp,
                                                                   float* __restrict__ g_y, double* __restrict__ ln_part) {
    __shared__ float s_w[MF_STAGE];
    __shared__ double s_wave[MF_WAVES][2 * MF_C];             // a wave's sums over its 32 tokens of the current tile
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int K = MF_C + a.Cm;
    {
        const int token = blockIdx.x * MF_TM + wave * MF_T + l31;
        const bool valid = token < a.T;
        const int tk = valid ? token : 0, n = tk / a.HW, pixel = tk - n * a.HW;
        const size_t plane0 = (size_t)n * MF_C * a.HW + pixel;
        f32x16 ga[MF_C / MF_T];                              // g_a^T, then (as float32) the sum of its two chains
        {   // g_a^T = W2^T g_out^T: go[s] is channel 2 s + hf of the lane's token
            float go[MF_C / 2];
#pragma unroll
            for (int s = 0; s < MF_C / 2; ++s) {
                const float v = g_out[plane0 + (size_t)(2 * s + hf) * a.HW];
                go[s] = valid ? v : 0.f;
            }
#pragma unroll
            for (int h = 0; h < MF_C / MF_KC; ++h) {
                __syncthreads();                              // the previous image has been read
                // s_w[j][cc] = W2[64 h + cc][j]: coalesced reads along j, odd row stride
                for (int idx = tid; idx < MF_KC * MF_C; idx += S360_BLOCK)
                    s_w[(idx & 127) * MF_LDK + (idx >> 7)] = a.w2[(size_t)(h * MF_KC + (idx >> 7)) * MF_C + (idx & 127)];
                __syncthreads();
#pragma unroll
                for (int jt = 0; jt < MF_C / MF_T; ++jt) {
                    const float* ap = s_w + (jt * MF_T + l31) * MF_LDK + hf;
                    f32x16 t = mf_zero();
#pragma unroll
                    for (int s = 0; s < MF_KC / 2; ++s) t = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s], go[h * (MF_KC / 2) + s], t, 0, 0, 0);
                    if (h == 0) ga[jt] = t;
                    else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) ga[jt][r] = (float)((double)ga[jt][r] + (double)t[r]);   // two chains of 64, added in float64
                    }
                }
            }
        }
        // ReLU's mask and LayerNorm's backward: register r of tile jt is channel 32 jt + mfma_acc_row(r, hf)
        const double mean = valid ? stats[(size_t)token * 2] : 0.0, rstd = valid ? stats[(size_t)token * 2 + 1] : 0.0;
        float gy[MF_C / MF_T][16], yv[MF_C / MF_T][16];
#pragma unroll
        for (int jt = 0; jt < MF_C / MF_T; ++jt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (valid) v = *reinterpret_cast<const float4*>(y + (size_t)token * MF_C + jt * MF_T + 8 * q + 4 * hf);
                yv[jt][4 * q] = v.x, yv[jt][4 * q + 1] = v.y, yv[jt][4 * q + 2] = v.z, yv[jt][4 * q + 3] = v.w;
            }
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int jt = 0; jt < MF_C / MF_T; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = jt * MF_T + mfma_acc_row(r, hf);
                const float w = a.lnw[c];
                const bool on = valid && mf_norm(yv[jt][r], mean, rstd, w, a.lnb[c]) > 0.f;
                gy[jt][r] = on ? ga[jt][r] : 0.f;            // the gradient at LN's output
                const double g = (double)gy[jt][r] * (double)w, xh = ((double)yv[jt][r] - mean) * rstd;
                s1 += g, s2 += g * xh;
            }
        s1 += __shfl_xor(s1, 32), s2 += __shfl_xor(s2, 32);
        s1 *= MF_INV_C, s2 *= MF_INV_C;
#pragma unroll
        for (int jt = 0; jt < MF_C / MF_T; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = jt * MF_T + mfma_acc_row(r, hf);
                const double g = (double)gy[jt][r], xh = ((double)yv[jt][r] - mean) * rstd;
                const double pw = mf_sum32(g * xh), pb = mf_sum32(g);
                if (l31 == 0) s_wave[wave][c] = pw, s_wave[wave][MF_C + c] = pb;
                gy[jt][r] = (float)(rstd * (g * (double)a.lnw[c] - s1 - xh * s2));
            }
        if (valid) {
#pragma unroll
            for (int jt = 0; jt < MF_C / MF_T; ++jt)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(g_y + (size_t)token * MF_C + jt * MF_T + 8 * q + 4 * hf) =
                        make_float4(gy[jt][4 * q], gy[jt][4 * q + 1], gy[jt][4 * q + 2], gy[jt][4 * q + 3]);
        }
        // g_erp^T = W1[:, :C]^T g_y^T: W1's rows in two halves of 64, each tile of 32 a float32 chain added in float64
        double acc[MF_C / MF_T][16];
#pragma unroll
        for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ot][r] = 0.0;
#pragma unroll
        for (int h = 0; h < MF_C / MF_KC; ++h) {
            __syncthreads();
            for (int idx = tid; idx < MF_KC * MF_C; idx += S360_BLOCK)
                s_w[(idx >> 7) * MF_LDC + (idx & 127)] = a.w1[(size_t)(h * MF_KC + (idx >> 7)) * K + (idx & 127)];
            __syncthreads();
#pragma unroll
            for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
                for (int jt = 0; jt < MF_KC / MF_T; ++jt) {
                    const f32x16 t = mf_fold(s_w + (jt * MF_T + 4 * hf) * MF_LDC + ot * MF_T + l31, MF_LDC, gy[h * (MF_KC / MF_T) + jt], mf_zero());
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[ot][r] += (double)t[r];
                }
        }
        if (valid) {
#pragma unroll
            for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
                for (int r = 0; r < 16; ++r) g_erp[plane0 + (size_t)(ot * MF_T + mfma_acc_row(r, hf)) * a.HW] = (float)acc[ot][r];
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * MF_C; i += S360_BLOCK) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < MF_WAVES; ++w) v += s_wave[w][i];
        ln_part[(size_t)blockIdx.x * 2 * MF_C + i] = v;
    }
}

// Backward, the pass owned by (column group, token chunk).  Group g < (C + Cm) / 64: columns [64 g, 64 g + 64) of g_W1 — the
// accumulator's rows are g_y's 128 channels, its columns X's 64 channels of the group (erp_feat for g < 2, the stitch gathered
// again otherwise).  The two last groups: columns [64 gg, 64 gg + 64) of g_W2 — rows g_out's 128 channels, columns a's 64.  Wave w
// owns rows [32 w, 32 w + 32).  The chunk's tokens [first, last) are walked in tiles of 64 staged in LDS.  Partials:
// p_w1[chunk][C][C + Cm], p_w2[chunk][C][C].
__global__ __launch_bounds__(S360_BLOCK) void k_mf_backward_weights(MFArgs a, const float* __restrict__ y, const double* __restrict__ stats,
                                                                    const float* __restrict__ g_out, const float* __restrict__ g_y,
                                                                    int tiles, int chunks, float* __restrict__ p_w1, float* __restrict__ p_w2) {
    __shared__ float s_x[MF_WT * MF_LDK];                     // [token][64 channels of the column side]
    __shared__ float s_g[MF_WT * MF_LDC];                     // [token][128 channels of the row side]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int K = MF_C + a.Cm, group = blockIdx.x, chunk = blockIdx.y;
    const bool second = group >= K / MF_KC;                   // a column group of g_W2
    const int c0 = (second ? group - K / MF_KC : group) * MF_KC;
    const int first = (int)((long long)chunk * tiles / chunks) * MF_WT, last = min(a.T, (int)((long long)(chunk + 1) * tiles / chunks) * MF_WT);
    double acc[MF_KC / MF_T][16];
#pragma unroll
    for (int ct = 0; ct < MF_KC / MF_T; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ct][r] = 0.0;
    const size_t cs = (size_t)6 * a.fw * a.fw;
    for (int t0 = first; t0 < last; t0 += MF_WT) {
        // staging: thread = (token `lane` of the tile, quarter `wave` of the channels)
        const int token = t0 + lane;
        const bool valid = token < last;
        const int tk = valid ? token : 0, n = tk / a.HW, pixel = tk - n * a.HW;
        float xs[MF_KC / MF_WAVES], gs[MF_C / MF_WAVES];
        if (second) {
            const double mean = stats[(size_t)tk * 2], rstd = stats[(size_t)tk * 2 + 1];
            const int j0 = c0 + wave * (MF_KC / MF_WAVES);
#pragma unroll
            for (int i = 0; i < MF_KC / MF_WAVES; ++i)
                xs[i] = fmaxf(mf_norm(y[(size_t)tk * MF_C + j0 + i], mean, rstd, a.lnw[j0 + i], a.lnb[j0 + i]), 0.f);
            const float* pg = g_out + ((size_t)n * MF_C + wave * (MF_C / MF_WAVES)) * a.HW + pixel;
#pragma unroll
            for (int i = 0; i < MF_C / MF_WAVES; ++i) gs[i] = pg[(size_t)i * a.HW];
        } else {
            if (c0 < MF_C) {
                const float* px = a.erp + ((size_t)n * MF_C + c0 + wave * (MF_KC / MF_WAVES)) * a.HW + pixel;
#pragma unroll
                for (int i = 0; i < MF_KC / MF_WAVES; ++i) xs[i] = px[(size_t)i * a.HW];
            } else {
                const MFTaps tp = mf_taps(a.grid, pixel, a.fw);
                const float* px = a.cube + ((size_t)n * a.Cm + (c0 - MF_C) + wave * (MF_KC / MF_WAVES)) * cs;
#pragma unroll
                for (int i = 0; i < MF_KC / MF_WAVES; ++i) xs[i] = mf_gather(px + (size_t)i * cs, tp);
            }
            const float* pg = g_y + (size_t)tk * MF_C + wave * (MF_C / MF_WAVES);
#pragma unroll
            for (int i = 0; i < MF_C / MF_WAVES; i += 4) {
                const float4 v = *reinterpret_cast<const float4*>(pg + i);
                gs[i] = v.x, gs[i + 1] = v.y, gs[i + 2] = v.z, gs[i + 3] = v.w;
            }
        }
        __syncthreads();                                      // the previous tile has been read
#pragma unroll
        for (int i = 0; i < MF_KC / MF_WAVES; ++i) s_x[lane * MF_LDK + wave * (MF_KC / MF_WAVES) + i] = valid ? xs[i] : 0.f;
#pragma unroll
        for (int i = 0; i < MF_C / MF_WAVES; ++i) s_g[lane * MF_LDC + wave * (MF_C / MF_WAVES) + i] = valid ? gs[i] : 0.f;
        __syncthreads();
        const float* ap = s_g + hf * MF_LDC + wave * MF_T + l31;   // (token hf, the wave's row l31)
#pragma unroll
        for (int ct = 0; ct < MF_KC / MF_T; ++ct) {
            const float* bp = s_x + hf * MF_LDK + ct * MF_T + l31;
            f32x16 t = mf_zero();
#pragma unroll
            for (int s = 0; s < MF_WT / 2; ++s) t = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * MF_LDC], bp[2 * s * MF_LDK], t, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][r] += (double)t[r];
        }
    }
    const int ld = second ? MF_C : K;
    float* p = (second ? p_w2 : p_w1) + (size_t)chunk * MF_C * ld + c0 + l31;
#pragma unroll
    for (int ct = 0; ct < MF_KC / MF_T; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) p[(size_t)(wave * MF_T + mfma_acc_row(r, hf)) * ld + ct * MF_T] = (float)acc[ct][r];
}

// The last launch: sums of partials in the order 0, 1, ..., float64, rounded once.  Elements [0, nw1) are g_W1, [nw1, nw1 + nw2)
// g_W2 (both from `chunks` float32 partials), then 2 C values from `parts` float64 partials: g_ln_weight, g_ln_bias.
__global__ __launch_bounds__(S360_BLOCK) void k_mf_reduce(const float* __restrict__ p_w1, const float* __restrict__ p_w2, int chunks, int nw1,
                                                          int nw2, float* __restrict__ g_w1, float* __restrict__ g_w2,
                                                          const double* __restrict__ ln_part, int parts, float* __restrict__ g_lnw,
                                                          float* __restrict__ g_lnb) {
    const int i = blockIdx.x * S360_BLOCK + threadIdx.x;
    if (i < nw1 + nw2) {
        const bool first = i < nw1;
        const float* p = first ? p_w1 + i : p_w2 + (i - nw1);
        const size_t stride = first ? nw1 : nw2;
        double v = 0.0;
        for (int c = 0; c < chunks; ++c) v += (double)p[c * stride];
        if (first) g_w1[i] = (float)v;
        else g_w2[i - nw1] = (float)v;
    } else if (i < nw1 + nw2 + 2 * MF_C) {
        const int k = i - nw1 - nw2;
        const double* p = ln_part + k;
        double v = 0.0;
        int c = 0;
        // batches of 16: every load of a batch is in flight before the first add (one workgroup per 128 tokens leaves 512 partials
        // at the ERP shape, and a chain of dependent loads per partial made this launch 123 us, against 23 us now); the sum is still taken one
        // partial at a time in the order 0, 1, ...
        for (; c + 16 <= parts; c += 16) {
            double b[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) b[j] = p[(size_t)(c + j) * 2 * MF_C];
#pragma unroll
            for (int j = 0; j < 16; ++j) v += b[j];
        }
        for (; c < parts; ++c) v += p[(size_t)c * 2 * MF_C];
        if (k < MF_C) g_lnw[k] = (float)v;
        else g_lnb[k - MF_C] = (float)v;
    }
}

// the weight-gradient pass's token chunks: runs of tiles of 64 tokens, as even as integer division makes them, at most MF_MAX_CHUNKS
static int mf_tiles(int64_t T) { return (int)((T + MF_WT - 1) / MF_WT); }
static int mf_chunks(int64_t T) { return min(MF_MAX_CHUNKS, mf_tiles(T)); }
static int mf_token_wgs(int64_t T) { return (int)((T + MF_TM - 1) / MF_TM); }
static bool mf_widths(int32_t channels, int32_t mono_channels) {
    return channels == MF_C && mono_channels >= MF_KC && mono_channels <= MF_MAX_CM && mono_channels % MF_KC == 0;
}

// S360_OK and the token count, or the refusal of the sizes
static int mf_sizes(int32_t n, int32_t channels, int32_t mono_channels, int32_t face_w, int32_t equ_h, int32_t equ_w, int64_t* tokens) {
    if (n < 1 || channels < 1 || mono_channels < 1 || face_w < 1 || equ_h < 1 || equ_w < 1) return S360_E_BADARG;
    if (!mf_widths(channels, mono_channels)) return S360_E_UNSUPPORTED;
    const int64_t lim = (int64_t)1 << 31, hw = (int64_t)equ_h * equ_w;
    if (hw * 8 >= lim) return S360_E_BADARG;
    if ((int64_t)face_w * face_w * 6 >= lim / mono_channels / n) return S360_E_BADARG;   // elements of mono_cube
    if (hw >= lim / MF_C / n) return S360_E_BADARG;                                       // elements of erp_feat, out, y
    *tokens = hw * n;
    return S360_OK;
}

}  // namespace s360

// ---------------------------------------------------------------------------------------------- the "high" mode (bf16 x 3)
// The same function with its two products, and the four of the backward, as bf16x3 products (s360_bf16x3.h: the split, the
// three terms and their order, the B-operand register rule), both operands split from their float32 values: X = [erp_feat, m]
// with m the float32 8-tap stitch taken in the kernel as above, a = float32(relu(LN(y))), g_out, g_y as float32, W1 and W2.  The
// LayerNorm rows, their statistics, the ReLU mask and the parameter gradients' partial sums are float64 as above; y, a, g_y and the
// partials are rounded to float32 where the kernels above round them.  No float64 chunk sums: a product is one float32 MFMA
// accumulation over its whole k range (in the weight-owned pass: over the tokens of a chunk).
// A pre-pass (k_mfh_split, one launch) splits W1 and W2 once per call into bf16 (hi, lo) planes in the caller's scratch, in the
// layouts their uses need (4 C (4 C + Cm) bytes, 0.75 MiB at Cm = 1024, whatever T):
//   w1_r [(C + Cm) / 8][C][8]   X W1^T: the row layout in k-groups of 8 — a lane reads the 8 consecutive channels of k-group
//                               2 s + hf of its output row, and the 32 lanes of a half read 512 consecutive bytes (bx3_ld8)
//   w2_r [C][C]                 a W2^T: W2 as it is; 2 x 4 consecutive channels of a row (bx3_ld44, the k permutation of an
//                               accumulator tile used as the B operand)
//   w2_t [C / 8][C][8]          g_out W2: W2 transposed, in k-groups of 8 as w1_r
//   w1_t [C][C]                 g_y W1[:, :C]: the first C columns of W1 transposed, read as w2_r
// The kernels read the planes from global memory (L1 / L2), so the forward has no LDS staging of W1 and no barrier in its walk
// over K.  The token side is split where it is loaded, gathered or produced: X and g_out in registers, a and g_y register by
// register from the accumulator tile, the weight-owned pass's tiles as they are staged in LDS (transposed: tokens are its k).
// No plane that grows with T exists, and neither do the stitched map and the concatenation.  Launch geometry, g_y's hand-over,
// the partials and k_mf_reduce are those above.
// Order of a product's operand pair: (weight, token side) where a weight is an operand — (wh, th), (wh, tl), (wl, th); the weight
// is the A operand in all four, so SWAP = false — and (gradient, activation) for the two token-by-token products g_y^T X and
// g_out^T a, the gradient being the A operand: SWAP = false as well.
// Resource usage (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DESIGN.md section 6.
namespace s360 {

constexpr int MFH_LDT = MF_WT + 8;                            // row stride of a staged transposed tile [channel][64 tokens] (bf16; rows 16-byte aligned)

struct MFHPlanes {
    __bf16 *w1_rh, *w1_rl, *w1_th, *w1_tl, *w2_rh, *w2_rl, *w2_th, *w2_tl;
};

// bytes of the four plane pairs
static size_t mfh_plane_bytes(int32_t mono_channels) { return (size_t)4 * MF_C * (4 * MF_C + mono_channels); }

// where element (row, k) of a matrix of C rows lies in a plane of k-groups of 8
__device__ __forceinline__ int mfh_grouped(int row, int k) { return ((k >> 3) * MF_C + row) * 8 + (k & 7); }

// The pre-pass: element i of W1 (then of W2) into its planes.
__global__ __launch_bounds__(S360_BLOCK) void k_mfh_split(const float* __restrict__ w1, const float* __restrict__ w2, int K, MFHPlanes pl) {
    const int i = blockIdx.x * S360_BLOCK + threadIdx.x;
    __bf16 h, l;
    if (i < MF_C * K) {
        const int row = i / K, k = i - row * K;
        bx3_split(w1[i], h, l);
        const int o = mfh_grouped(row, k);
        pl.w1_rh[o] = h, pl.w1_rl[o] = l;
        if (k < MF_C) pl.w1_th[k * MF_C + row] = h, pl.w1_tl[k * MF_C + row] = l;
    } else if (i < MF_C * K + MF_C * MF_C) {
        const int idx = i - MF_C * K, c = idx / MF_C, j = idx - c * MF_C;
        bx3_split(w2[idx], h, l);
        pl.w2_rh[idx] = h, pl.w2_rl[idx] = l;
        const int o = mfh_grouped(j, c);
        pl.w2_th[o] = h, pl.w2_tl[o] = l;
    }
}

// x[8 s + j] = X[token][64 kc + 16 s + 8 hf + j], the B fragments of the chunk's four k-steps before the split: chunks 0 and 1
// are erp_feat, the others the stitch of mono_cube; zeros unless valid
__device__ __forceinline__ void mfh_load_x(const MFArgs& a, int kc, int n, int pixel, bool valid, int hf, const MFTaps& tp, float* x) {
    if (kc < MF_C / MF_KC) {
        const float* p = a.erp + ((size_t)n * MF_C + kc * MF_KC + 8 * hf) * a.HW + pixel;
#pragma unroll
        for (int i = 0; i < MF_KC / 2; ++i) {
            const float v = p[(size_t)(16 * (i >> 3) + (i & 7)) * a.HW];
            x[i] = valid ? v : 0.f;
        }
    } else {
        const size_t cs = (size_t)6 * a.fw * a.fw;
        const float* p = a.cube + ((size_t)n * a.Cm + (kc * MF_KC - MF_C) + 8 * hf) * cs;
#pragma unroll
        for (int i = 0; i < MF_KC / 2; ++i) {
            const float v = mf_gather(p + (size_t)(16 * (i >> 3) + (i & 7)) * cs, tp);
            x[i] = valid ? v : 0.f;
        }
    }
}

// Forward, as k_mf_forward: 32 tokens per wave on the lanes, K walked in chunks of 64 channels = four k-steps of 16.  The next
// chunk's loads and gathers are issued before the current chunk's MFMAs.
__global__ __launch_bounds__(S360_BLOCK) void k_mfh_forward(MFArgs a, MFHPlanes pl, float* __restrict__ out, float* __restrict__ y,
                                                            double* __restrict__ stats) {
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int token = blockIdx.x * MF_TM + wave * MF_T + l31;
    const bool valid = token < a.T;
    const int tk = valid ? token : 0, n = tk / a.HW, pixel = tk - n * a.HW;
    const MFTaps tp = mf_taps(a.grid, pixel, a.fw);
    const int nk = (MF_C + a.Cm) / MF_KC;
    f32x16 acc[MF_C / MF_T];                                 // y^T: tile ot, register r is channel 32 ot + mfma_acc_row(r, hf) of the lane's token
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot) acc[ot] = bx3_zero();
    const __bf16* w1h = pl.w1_rh + (size_t)(hf * MF_C + l31) * 8;   // k-group hf of row l31
    const __bf16* w1l = pl.w1_rl + (size_t)(hf * MF_C + l31) * 8;
    float x[MF_KC / 2];
    mfh_load_x(a, 0, n, pixel, valid, hf, tp, x);
    for (int kc = 0; kc < nk; ++kc) {
        bf16x8 xh[MF_KC / 16], xl[MF_KC / 16];
#pragma unroll
        for (int s = 0; s < MF_KC / 16; ++s) bx3_split8(x + 8 * s, xh[s], xl[s]);
        if (kc + 1 < nk) mfh_load_x(a, kc + 1, n, pixel, valid, hf, tp, x);
#pragma unroll
        for (int s = 0; s < MF_KC / 16; ++s) {               // (X W1^T)^T: rows = output channels, lane = token
            const size_t o = (size_t)(2 * (kc * (MF_KC / 16) + s)) * MF_C * 8;
#pragma unroll
            for (int ot = 0; ot < MF_C / MF_T; ++ot)
                acc[ot] = bx3_mfma3<false>(bx3_ld8(w1h + o + ot * MF_T * 8), bx3_ld8(w1l + o + ot * MF_T * 8), xh[s], xl[s], acc[ot]);
        }
    }
    // LayerNorm over the float32 y and the ReLU, as k_mf_forward
    float av[MF_C / MF_T][16];
    double sum = 0.0, sq = 0.0;
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
        for (int r = 0; r < 16; ++r) av[ot][r] = acc[ot][r], sum += (double)av[ot][r];
    sum += __shfl_xor(sum, 32);
    const double mean = sum * MF_INV_C;
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const double d = (double)av[ot][r] - mean;
            sq += d * d;
        }
    sq += __shfl_xor(sq, 32);
    const double rstd = 1.0 / sqrt(sq * MF_INV_C + a.eps);
    if (valid) {
#pragma unroll
        for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<float4*>(y + (size_t)token * MF_C + ot * MF_T + 8 * q + 4 * hf) =
                    make_float4(av[ot][4 * q], av[ot][4 * q + 1], av[ot][4 * q + 2], av[ot][4 * q + 3]);
        if (hf == 0) stats[(size_t)token * 2] = mean, stats[(size_t)token * 2 + 1] = rstd;
    }
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = ot * MF_T + mfma_acc_row(r, hf);
            av[ot][r] = fmaxf(mf_norm(av[ot][r], mean, rstd, a.lnw[c], a.lnb[c]), 0.f);
        }
    // out^T = W2 a^T: a's tiles are, register by register, the B operand
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot) acc[ot] = bx3_zero();
    const __bf16* w2h = pl.w2_rh + l31 * MF_C + 4 * hf;
    const __bf16* w2l = pl.w2_rl + l31 * MF_C + 4 * hf;
#pragma unroll
    for (int jt = 0; jt < MF_C / MF_T; ++jt) {
        bf16x8 ah[2], al[2];
        bx3_split_tile(av[jt], ah, al);
#pragma unroll
        for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                acc[ot] = bx3_mfma3<false>(bx3_ld44(w2h + ot * MF_T * MF_C + jt * MF_T + 16 * s), bx3_ld44(w2l + ot * MF_T * MF_C + jt * MF_T + 16 * s),
                                           ah[s], al[s], acc[ot]);
    }
    if (!valid) return;
    float* po = out + (size_t)n * MF_C * a.HW + pixel;
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
        for (int r = 0; r < 16; ++r) po[(size_t)(ot * MF_T + mfma_acc_row(r, hf)) * a.HW] = acc[ot][r];
}

// Backward, the pass owned by token tiles, as k_mf_backward_tokens: g_erp, g_y (scratch) and the per-workgroup float64 partial
// sums of g_ln_weight / g_ln_bias.
__global__ __launch_bounds__(S360_BLOCK) void k_mfh_backward_tokens(MFArgs a, MFHPlanes pl, const float* __restrict__ y,
                                                                    const double* __restrict__ stats, const float* __restrict__ g_out,
                                                                    float* __restrict__ g_erp, float* __restrict__ g_y,
                                                                    double* __restrict__ ln_part) {
    __shared__ double s_wave[MF_WAVES][2 * MF_C];             // a wave's sums over its 32 tokens
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int token = blockIdx.x * MF_TM + wave * MF_T + l31;
    const bool valid = token < a.T;
    const int tk = valid ? token : 0, n = tk / a.HW, pixel = tk - n * a.HW;
    const size_t plane0 = (size_t)n * MF_C * a.HW + pixel;
    f32x16 ga[MF_C / MF_T];                                  // g_a^T = W2^T g_out^T
#pragma unroll
    for (int jt = 0; jt < MF_C / MF_T; ++jt) ga[jt] = bx3_zero();
    {
        const __bf16* w2th = pl.w2_th + (size_t)(hf * MF_C + l31) * 8;
        const __bf16* w2tl = pl.w2_tl + (size_t)(hf * MF_C + l31) * 8;
#pragma unroll
        for (int s = 0; s < MF_C / 16; ++s) {                 // element j of k-step s is channel 16 s + 8 hf + j of the lane's token
            float go[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = g_out[plane0 + (size_t)(16 * s + 8 * hf + j) * a.HW];
                go[j] = valid ? v : 0.f;
            }
            bf16x8 gh, gl;
            bx3_split8(go, gh, gl);
#pragma unroll
            for (int jt = 0; jt < MF_C / MF_T; ++jt)
                ga[jt] = bx3_mfma3<false>(bx3_ld8(w2th + (size_t)(2 * s) * MF_C * 8 + jt * MF_T * 8),
                                          bx3_ld8(w2tl + (size_t)(2 * s) * MF_C * 8 + jt * MF_T * 8), gh, gl, ga[jt]);
        }
    }
    // ReLU's mask and LayerNorm's backward, as k_mf_backward_tokens
    const double mean = valid ? stats[(size_t)token * 2] : 0.0, rstd = valid ? stats[(size_t)token * 2 + 1] : 0.0;
    float gy[MF_C / MF_T][16], yv[MF_C / MF_T][16];
#pragma unroll
    for (int jt = 0; jt < MF_C / MF_T; ++jt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid) v = *reinterpret_cast<const float4*>(y + (size_t)token * MF_C + jt * MF_T + 8 * q + 4 * hf);
            yv[jt][4 * q] = v.x, yv[jt][4 * q + 1] = v.y, yv[jt][4 * q + 2] = v.z, yv[jt][4 * q + 3] = v.w;
        }
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int jt = 0; jt < MF_C / MF_T; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = jt * MF_T + mfma_acc_row(r, hf);
            const float w = a.lnw[c];
            const bool on = valid && mf_norm(yv[jt][r], mean, rstd, w, a.lnb[c]) > 0.f;
            gy[jt][r] = on ? ga[jt][r] : 0.f;                // the gradient at LN's output
            const double g = (double)gy[jt][r] * (double)w, xh = ((double)yv[jt][r] - mean) * rstd;
            s1 += g, s2 += g * xh;
        }
    s1 += __shfl_xor(s1, 32), s2 += __shfl_xor(s2, 32);
    s1 *= MF_INV_C, s2 *= MF_INV_C;
#pragma unroll
    for (int jt = 0; jt < MF_C / MF_T; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = jt * MF_T + mfma_acc_row(r, hf);
            const double g = (double)gy[jt][r], xh = ((double)yv[jt][r] - mean) * rstd;
            const double pw = mf_sum32(g * xh), pb = mf_sum32(g);
            if (l31 == 0) s_wave[wave][c] = pw, s_wave[wave][MF_C + c] = pb;
            gy[jt][r] = (float)(rstd * (g * (double)a.lnw[c] - s1 - xh * s2));
        }
    if (valid) {
#pragma unroll
        for (int jt = 0; jt < MF_C / MF_T; ++jt)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<float4*>(g_y + (size_t)token * MF_C + jt * MF_T + 8 * q + 4 * hf) =
                    make_float4(gy[jt][4 * q], gy[jt][4 * q + 1], gy[jt][4 * q + 2], gy[jt][4 * q + 3]);
    }
    // g_erp^T = W1[:, :C]^T g_y^T: g_y's tiles are, register by register, the B operand
    f32x16 ge[MF_C / MF_T];
#pragma unroll
    for (int ot = 0; ot < MF_C / MF_T; ++ot) ge[ot] = bx3_zero();
    const __bf16* w1th = pl.w1_th + l31 * MF_C + 4 * hf;
    const __bf16* w1tl = pl.w1_tl + l31 * MF_C + 4 * hf;
#pragma unroll
    for (int jt = 0; jt < MF_C / MF_T; ++jt) {
        bf16x8 ph[2], pw[2];
        bx3_split_tile(gy[jt], ph, pw);
#pragma unroll
        for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                ge[ot] = bx3_mfma3<false>(bx3_ld44(w1th + ot * MF_T * MF_C + jt * MF_T + 16 * s), bx3_ld44(w1tl + ot * MF_T * MF_C + jt * MF_T + 16 * s),
                                          ph[s], pw[s], ge[ot]);
    }
    if (valid) {
#pragma unroll
        for (int ot = 0; ot < MF_C / MF_T; ++ot)
#pragma unroll
            for (int r = 0; r < 16; ++r) g_erp[plane0 + (size_t)(ot * MF_T + mfma_acc_row(r, hf)) * a.HW] = ge[ot][r];
    }
    __syncthreads();
    for (int i = tid; i < 2 * MF_C; i += S360_BLOCK) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < MF_WAVES; ++w) v += s_wave[w][i];
        ln_part[(size_t)blockIdx.x * 2 * MF_C + i] = v;
    }
}

// A tile of 64 tokens of the weight-owned pass in registers, before the split: thread = (token `lane` of the tile, quarter `wave`
// of the channels); xs the column side (X or a), gs the row side (g_y or g_out); valid: the token is inside the chunk
struct MFHTile {
    float xs[MF_KC / MF_WAVES], gs[MF_C / MF_WAVES];
    bool valid;
};

// the loads, gathers and (for g_W2's groups) the recomputation of a, as k_mf_backward_weights stages them
__device__ __forceinline__ void mfh_tile_load(const MFArgs& a, const float* __restrict__ y, const double* __restrict__ stats,
                                              const float* __restrict__ g_out, const float* __restrict__ g_y, bool second, int c0, int t0,
                                              int last, int wave, int lane, MFHTile& t) {
    const int token = t0 + lane;
    t.valid = token < last;
    const int tk = t.valid ? token : 0, n = tk / a.HW, pixel = tk - n * a.HW;
    if (second) {
        const double mean = stats[(size_t)tk * 2], rstd = stats[(size_t)tk * 2 + 1];
        const int j0 = c0 + wave * (MF_KC / MF_WAVES);
#pragma unroll
        for (int i = 0; i < MF_KC / MF_WAVES; ++i)
            t.xs[i] = fmaxf(mf_norm(y[(size_t)tk * MF_C + j0 + i], mean, rstd, a.lnw[j0 + i], a.lnb[j0 + i]), 0.f);
        const float* pg = g_out + ((size_t)n * MF_C + wave * (MF_C / MF_WAVES)) * a.HW + pixel;
#pragma unroll
        for (int i = 0; i < MF_C / MF_WAVES; ++i) t.gs[i] = pg[(size_t)i * a.HW];
    } else {
        if (c0 < MF_C) {
            const float* px = a.erp + ((size_t)n * MF_C + c0 + wave * (MF_KC / MF_WAVES)) * a.HW + pixel;
#pragma unroll
            for (int i = 0; i < MF_KC / MF_WAVES; ++i) t.xs[i] = px[(size_t)i * a.HW];
        } else {
            const size_t cs = (size_t)6 * a.fw * a.fw;
            const MFTaps tp = mf_taps(a.grid, pixel, a.fw);
            const float* px = a.cube + ((size_t)n * a.Cm + (c0 - MF_C) + wave * (MF_KC / MF_WAVES)) * cs;
#pragma unroll
            for (int i = 0; i < MF_KC / MF_WAVES; ++i) t.xs[i] = mf_gather(px + (size_t)i * cs, tp);
        }
        const float* pg = g_y + (size_t)tk * MF_C + wave * (MF_C / MF_WAVES);
#pragma unroll
        for (int i = 0; i < MF_C / MF_WAVES; i += 4) {
            const float4 v = *reinterpret_cast<const float4*>(pg + i);
            t.gs[i] = v.x, t.gs[i + 1] = v.y, t.gs[i + 2] = v.z, t.gs[i + 3] = v.w;
        }
    }
}

// the tile split into the transposed LDS images (hi, lo) x [channel][token]; zeros for a token outside the chunk
__device__ __forceinline__ void mfh_tile_stage(const MFHTile& t, int wave, int lane, __bf16 (*s_xt)[MF_KC * MFH_LDT], __bf16 (*s_gt)[MF_C * MFH_LDT]) {
    __syncthreads();                                          // the previous tile has been read
#pragma unroll
    for (int i = 0; i < MF_KC / MF_WAVES; ++i) {
        const int o = (wave * (MF_KC / MF_WAVES) + i) * MFH_LDT + lane;
        __bf16 h, l;
        bx3_split(t.valid ? t.xs[i] : 0.f, h, l);
        s_xt[0][o] = h, s_xt[1][o] = l;
    }
#pragma unroll
    for (int i = 0; i < MF_C / MF_WAVES; ++i) {
        const int o = (wave * (MF_C / MF_WAVES) + i) * MFH_LDT + lane;
        __bf16 h, l;
        bx3_split(t.valid ? t.gs[i] : 0.f, h, l);
        s_gt[0][o] = h, s_gt[1][o] = l;
    }
    __syncthreads();
}

// acc += G^T X over the staged tile's 64 tokens: rows = the wave's 32 channels of the row side, columns = the 64 of the column side
__device__ __forceinline__ void mfh_tile_fold(const __bf16 (*s_xt)[MF_KC * MFH_LDT], const __bf16 (*s_gt)[MF_C * MFH_LDT], int wave, int l31, int hf,
                                              f32x16* acc) {
    const int ao = (wave * MF_T + l31) * MFH_LDT + 8 * hf;   // (the wave's row l31, token 8 hf)
#pragma unroll
    for (int s = 0; s < MF_WT / 16; ++s) {
        const bf16x8 gh = bx3_ld8(s_gt[0] + ao + 16 * s), gl = bx3_ld8(s_gt[1] + ao + 16 * s);
#pragma unroll
        for (int ct = 0; ct < MF_KC / MF_T; ++ct) {
            const int bo = (ct * MF_T + l31) * MFH_LDT + 8 * hf + 16 * s;
            acc[ct] = bx3_mfma3<false>(gh, gl, bx3_ld8(s_xt[0] + bo), bx3_ld8(s_xt[1] + bo), acc[ct]);
        }
    }
}

// Backward, the pass owned by (column group, token chunk), as k_mf_backward_weights: a tile of 64 tokens is staged in LDS as split
// bf16, TRANSPOSED (tokens are the k index of both operands): the row side [128 channels][64 tokens] is the A operand (the
// gradient: g_y or g_out), the column side [64 channels][64 tokens] the B operand (X or a).  One float32 MFMA accumulation over
// the chunk's tokens, tile after tile.  Two tiles are held in registers: the loads and gathers of tile i + 2 are issued when tile
// i has been written to LDS, so they are in flight under the MFMAs of tile i and the whole of tile i + 1 (a workgroup walks its
// tiles alone on its compute unit: 320 workgroups at the ERP shape, and nothing else hides the latency of a tile's loads).
__global__ __launch_bounds__(S360_BLOCK) void k_mfh_backward_weights(MFArgs a, const float* __restrict__ y, const double* __restrict__ stats,
                                                                     const float* __restrict__ g_out, const float* __restrict__ g_y,
                                                                     int tiles, int chunks, float* __restrict__ p_w1, float* __restrict__ p_w2) {
    __shared__ __attribute__((aligned(16))) __bf16 s_xt[2][MF_KC * MFH_LDT];   // (hi, lo) x [column channel][token]
    __shared__ __attribute__((aligned(16))) __bf16 s_gt[2][MF_C * MFH_LDT];    // (hi, lo) x [row channel][token]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int K = MF_C + a.Cm, group = blockIdx.x, chunk = blockIdx.y;
    const bool second = group >= K / MF_KC;                   // a column group of g_W2
    const int c0 = (second ? group - K / MF_KC : group) * MF_KC;
    const int first = (int)((long long)chunk * tiles / chunks) * MF_WT, last = min(a.T, (int)((long long)(chunk + 1) * tiles / chunks) * MF_WT);
    f32x16 acc[MF_KC / MF_T];
#pragma unroll
    for (int ct = 0; ct < MF_KC / MF_T; ++ct) acc[ct] = bx3_zero();
    MFHTile ta, tb;
    if (first < last) mfh_tile_load(a, y, stats, g_out, g_y, second, c0, first, last, wave, lane, ta);
    if (first + MF_WT < last) mfh_tile_load(a, y, stats, g_out, g_y, second, c0, first + MF_WT, last, wave, lane, tb);
    for (int t0 = first; t0 < last; t0 += 2 * MF_WT) {       // every condition is uniform over the workgroup
        mfh_tile_stage(ta, wave, lane, s_xt, s_gt);
        if (t0 + 2 * MF_WT < last) mfh_tile_load(a, y, stats, g_out, g_y, second, c0, t0 + 2 * MF_WT, last, wave, lane, ta);
        mfh_tile_fold(s_xt, s_gt, wave, l31, hf, acc);
        if (t0 + MF_WT < last) {
            mfh_tile_stage(tb, wave, lane, s_xt, s_gt);
            if (t0 + 3 * MF_WT < last) mfh_tile_load(a, y, stats, g_out, g_y, second, c0, t0 + 3 * MF_WT, last, wave, lane, tb);
            mfh_tile_fold(s_xt, s_gt, wave, l31, hf, acc);
        }
    }
    const int ld = second ? MF_C : K;
    float* p = (second ? p_w2 : p_w1) + (size_t)chunk * MF_C * ld + c0 + l31;
#pragma unroll
    for (int ct = 0; ct < MF_KC / MF_T; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) p[(size_t)(wave * MF_T + mfma_acc_row(r, hf)) * ld + ct * MF_T] = acc[ct][r];
}

// the planes at the start of a scratch, and the pre-pass
static MFHPlanes mfh_planes(void* scratch, int K) {
    Bx3Carver c{static_cast<char*>(scratch)};
    MFHPlanes pl;
    c.take((size_t)MF_C * K, &pl.w1_rh, &pl.w1_rl);
    c.take((size_t)MF_C * MF_C, &pl.w1_th, &pl.w1_tl);
    c.take((size_t)MF_C * MF_C, &pl.w2_rh, &pl.w2_rl);
    c.take((size_t)MF_C * MF_C, &pl.w2_th, &pl.w2_tl);
    return pl;
}
static void mfh_split_launch(const float* w1, const float* w2, int K, const MFHPlanes& pl, hipStream_t st) {
    hipLaunchKernelGGL(k_mfh_split, dim3((unsigned)((MF_C * K + MF_C * MF_C + S360_BLOCK - 1) / S360_BLOCK)), dim3(S360_BLOCK), 0, st, w1, w2, K, pl);
}

// ---------------------------------------------------------------------------------------------- the entry points, both modes
// The caller's scratch, one order in both modes: in "high" the weights' bf16 planes at the front, then, for a backward, g_y
// [tokens, C], the per-chunk partials of g_w1, those of g_w2 and the LayerNorm partial sums of the token pass's workgroups.
// Byte offsets; `bytes` is what the *_scratch_bytes functions report.
struct MFLayout {
    size_t g_y, p_w1, p_w2, ln_part, bytes;
};
static MFLayout mf_layout(int64_t T, int32_t mono_channels, bool high, bool backward) {
    const size_t tokens = backward ? T : 0, chunks = backward ? mf_chunks(T) : 0, wgs = backward ? mf_token_wgs(T) : 0;
    MFLayout l;
    l.g_y = high ? mfh_plane_bytes(mono_channels) : 0;
    l.p_w1 = l.g_y + tokens * MF_C * sizeof(float);
    l.p_w2 = l.p_w1 + chunks * MF_C * (MF_C + mono_channels) * sizeof(float);
    l.ln_part = l.p_w2 + chunks * MF_C * MF_C * sizeof(float);
    l.bytes = l.ln_part + wgs * 2 * MF_C * sizeof(double);
    return l;
}

// What every launch entry starts with, in the order of include/s360.h's refusals: the pointer rule, eps, the sizes.  Completes
// `a` (the caller has set its pointers) with the sizes and eps, and gives the token count.
template <size_t NI, size_t NO>
static int mf_setup(const void* const (&in)[NI], const void* const (&outs)[NO], const double* eps, int32_t n, int32_t channels,
                    int32_t mono_channels, int32_t face_w, int32_t equ_h, int32_t equ_w, MFArgs& a, int64_t& tokens) {
    if (!s360_pointers_ok(in, outs)) return S360_E_BADARG;
    if (!eps || !(*eps > 0.0)) return S360_E_BADARG;
    const int rc = mf_sizes(n, channels, mono_channels, face_w, equ_h, equ_w, &tokens);
    if (rc != S360_OK) return rc;
    a.T = (int)tokens, a.HW = equ_h * equ_w, a.Cm = mono_channels, a.fw = face_w, a.eps = *eps;
    return S360_OK;
}

struct MFGrads {
    float *erp, *w1, *lnw, *lnb, *w2;
};

// s360_mono_fusion_backward (HIGH = false) and s360_mono_fusion_high_backward (true).  Only declared here and defined behind
// the two entries, at the end of the file: tests/test_mono_fusion_high_spec.py reads the backward's launches from the text
// that follows `extern "C" int s360_mono_fusion_high_backward`, so the body has to stay below that entry.
template <bool HIGH>
static int mf_backward(MFArgs a, const float* y, const double* stats, const float* g_out, int32_t n, int32_t channels, int32_t mono_channels,
                       int32_t face_w, int32_t equ_h, int32_t equ_w, const double* eps, void* scratch, size_t scratch_bytes, const MFGrads& g,
                       hipStream_t st);

}  // namespace s360

using namespace s360;

extern "C" size_t s360_mono_fusion_scratch_bytes(int32_t tokens, int32_t mono_channels) {
    return tokens < 1 || !mf_widths(MF_C, mono_channels) ? 0 : mf_layout(tokens, mono_channels, false, true).bytes;
}

extern "C" size_t s360_mono_fusion_high_scratch_bytes(int32_t tokens, int32_t mono_channels, int32_t backward) {
    return tokens < 1 || !mf_widths(MF_C, mono_channels) ? 0 : mf_layout(tokens, mono_channels, true, backward != 0).bytes;
}

extern "C" int s360_mono_fusion_weight_chunks(int32_t tokens) { return tokens < 1 ? 0 : mf_chunks(tokens); }

extern "C" int s360_mono_fusion_forward(const float* erp_feat, const float* mono_cube, const float* grid, const float* w1, const float* ln_weight,
                                        const float* ln_bias, const float* w2, int32_t n, int32_t channels, int32_t mono_channels,
                                        int32_t face_w, int32_t equ_h, int32_t equ_w, const double* eps, float* out, float* y, double* stats,
                                        void* stream) {
    MFArgs a = {erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2};
    const void* const in[] = {erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2};
    const void* const outs[] = {out, y, stats};
    int64_t tokens = 0;
    const int rc = mf_setup(in, outs, eps, n, channels, mono_channels, face_w, equ_h, equ_w, a, tokens);
    if (rc != S360_OK) return rc;
    hipLaunchKernelGGL(k_mf_forward, dim3((unsigned)((tokens + MF_TM - 1) / MF_TM)), dim3(S360_BLOCK), 0, (hipStream_t)stream, a, out, y, stats);
    return s360_launch_status();
}

extern "C" int s360_mono_fusion_high_forward(const float* erp_feat, const float* mono_cube, const float* grid, const float* w1,
                                             const float* ln_weight, const float* ln_bias, const float* w2, int32_t n, int32_t channels,
                                             int32_t mono_channels, int32_t face_w, int32_t equ_h, int32_t equ_w, const double* eps, float* out,
                                             float* y, double* stats, void* scratch, size_t scratch_bytes, void* stream) {
    MFArgs a = {erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2};
    const void* const in[] = {erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2};
    const void* const outs[] = {out, y, stats, scratch};
    int64_t tokens = 0;
    const int rc = mf_setup(in, outs, eps, n, channels, mono_channels, face_w, equ_h, equ_w, a, tokens);
    if (rc != S360_OK) return rc;
    if (scratch_bytes < mf_layout(tokens, mono_channels, true, false).bytes) return S360_E_WORKSPACE;   // after the sizes, as the size depends on them
    const MFHPlanes pl = mfh_planes(scratch, MF_C + mono_channels);
    mfh_split_launch(w1, w2, MF_C + mono_channels, pl, (hipStream_t)stream);
    S360_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mfh_forward, dim3((unsigned)((tokens + MF_TM - 1) / MF_TM)), dim3(S360_BLOCK), 0, (hipStream_t)stream, a, pl, out, y, stats);
    return s360_launch_status();
}

extern "C" int s360_mono_fusion_backward(const float* erp_feat, const float* mono_cube, const float* grid, const float* w1,
                                         const float* ln_weight, const float* ln_bias, const float* w2, const float* y, const double* stats,
                                         const float* g_out, int32_t n, int32_t channels, int32_t mono_channels, int32_t face_w,
                                         int32_t equ_h, int32_t equ_w, const double* eps, void* scratch, size_t scratch_bytes,
                                         float* g_erp_feat, float* g_w1, float* g_ln_weight, float* g_ln_bias, float* g_w2, void* stream) {
    return mf_backward<false>({erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2}, y, stats, g_out, n, channels, mono_channels, face_w, equ_h,
                              equ_w, eps, scratch, scratch_bytes, {g_erp_feat, g_w1, g_ln_weight, g_ln_bias, g_w2}, (hipStream_t)stream);
}

extern "C" int s360_mono_fusion_high_backward(const float* erp_feat, const float* mono_cube, const float* grid, const float* w1,
                                              const float* ln_weight, const float* ln_bias, const float* w2, const float* y,
                                              const double* stats, const float* g_out, int32_t n, int32_t channels, int32_t mono_channels,
                                              int32_t face_w, int32_t equ_h, int32_t equ_w, const double* eps, void* scratch,
                                              size_t scratch_bytes, float* g_erp_feat, float* g_w1, float* g_ln_weight, float* g_ln_bias,
                                              float* g_w2, void* stream) {
    return mf_backward<true>({erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2}, y, stats, g_out, n, channels, mono_channels, face_w, equ_h,
                             equ_w, eps, scratch, scratch_bytes, {g_erp_feat, g_w1, g_ln_weight, g_ln_bias, g_w2}, (hipStream_t)stream);
}

// The body of the two backward entries above: the pre-pass and the two kernels differ.  It stays below them (see its
// declaration).
namespace s360 {

template <bool HIGH>
static int mf_backward(MFArgs a, const float* y, const double* stats, const float* g_out, int32_t n, int32_t channels, int32_t mono_channels,
                       int32_t face_w, int32_t equ_h, int32_t equ_w, const double* eps, void* scratch, size_t scratch_bytes, const MFGrads& g,
                       hipStream_t st) {
    const void* const in[] = {a.erp, a.cube, a.grid, a.w1, a.lnw, a.lnb, a.w2, y, stats, g_out};
    const void* const outs[] = {g.erp, g.w1, g.lnw, g.lnb, g.w2, scratch};
    int64_t tokens = 0;
    const int rc = mf_setup(in, outs, eps, n, channels, mono_channels, face_w, equ_h, equ_w, a, tokens);
    if (rc != S360_OK) return rc;
    const MFLayout l = mf_layout(tokens, mono_channels, HIGH, true);
    if (scratch_bytes < l.bytes) return S360_E_WORKSPACE;
    const int K = MF_C + mono_channels, chunks = mf_chunks(tokens), wgs = mf_token_wgs(tokens);
    char* base = static_cast<char*>(scratch);
    float *g_y = reinterpret_cast<float*>(base + l.g_y), *p_w1 = reinterpret_cast<float*>(base + l.p_w1);
    float* p_w2 = reinterpret_cast<float*>(base + l.p_w2);
    double* ln_part = reinterpret_cast<double*>(base + l.ln_part);
    if constexpr (HIGH) {
        const MFHPlanes pl = mfh_planes(scratch, K);
        mfh_split_launch(a.w1, a.w2, K, pl, st);
        S360_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_mfh_backward_tokens, dim3(wgs), dim3(S360_BLOCK), 0, st, a, pl, y, stats, g_out, g.erp, g_y, ln_part);
        S360_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_mfh_backward_weights, dim3(K / MF_KC + MF_C / MF_KC, chunks), dim3(S360_BLOCK), 0, st, a, y, stats, g_out, g_y,
                           mf_tiles(tokens), chunks, p_w1, p_w2);
    } else {
        hipLaunchKernelGGL(k_mf_backward_tokens, dim3(wgs), dim3(S360_BLOCK), 0, st, a, y, stats, g_out, g.erp, g_y, ln_part);
        S360_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_mf_backward_weights, dim3(K / MF_KC + MF_C / MF_KC, chunks), dim3(S360_BLOCK), 0, st, a, y, stats, g_out, g_y,
                           mf_tiles(tokens), chunks, p_w1, p_w2);
    }
    S360_CHECK_LAUNCH();
    const int nw1 = MF_C * K, nw2 = MF_C * MF_C;
    hipLaunchKernelGGL(k_mf_reduce, dim3((nw1 + nw2 + 2 * MF_C + S360_BLOCK - 1) / S360_BLOCK), dim3(S360_BLOCK), 0, st, p_w1, p_w2, chunks,
                       nw1, nw2, g.w1, g.w2, ln_part, wgs, g.lnw, g.lnb);
    return s360_launch_status();
}

}  // namespace s360
