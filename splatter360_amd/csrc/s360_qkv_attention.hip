// s360_qkv_attention.hip — the U-Nets' multi-head QKV attention, forward and backward (the reference's QKVAttentionLegacy and
// QKVAttention, src/model/encoder/costvolume/ldm_unet/unet.py:527-599), read from and written to the channel-major qkv tensor
// where it lies.  gfx950 only.
//
//   qkv      [N, heads 3 ch, T] float32, channel-major, ch = 32; B = N / views batch elements.  Joint token s < L = views T of
//            batch element bi is token s mod T of view u = s / T and lives in batch row u B + bi (the reference's
//            "(v b) n t -> b n (v t)"); views = 1 is attention within a row.
//   order    legacy (0): head hd owns channel rows [hd 3 ch, (hd + 1) 3 ch), q then k then v; new (1): the channel axis is
//            q | k | v chunks of heads ch rows and head hd owns [hd ch, (hd + 1) ch) of each.
//   score    (q . k) / sqrt(ch) — the reference's (q ch^-1/4) . (k ch^-1/4) with the scale applied once — q . k summed in float64
//            over float32 fma chains of 8 channels (qa_dot) and kept in float64 until the maximum or lse is subtracted
//   out      a[N, heads ch, T] = softmax over the L joint keys, times v, in the rows' (v b) order; lse[B, heads, L] float64
//
// The arithmetic is the window attention's (s360_window_attention.hip): every product on v_mfma_f32_32x32x2_f32; 32 "owner" rows
// (queries in the forward and the g_q pass, keys in the g_k / g_v pass) sit on the lanes and the other side is walked in tiles
// of 32 that sit on the accumulator's rows, so the score tile is, register by register, the B operand of the second product,
// and the softmax statistics of the owner are per lane.  What is new is the layout and the split of the walk.
// Layout.  In channel-major memory a token tile of one channel is 32 consecutive floats, so everything that wants the TOKEN on
// the lanes is a coalesced 128-byte read: the owner's rows (held in registers, channel 2 j + hf at MFMA step j of lane half hf)
// and the score product's walked operand.  The second product wants the CHANNEL on the lanes (A[i = channel][k = walked token]),
// a stride of T floats between lanes in memory.  So each walked tile pair (K and V; Q and dO in the key-owned pass) goes through
// LDS once: read along t, one dword per lane (any T, any alignment, a tile may straddle two views), into [channel][token] tiles
// of row stride 33, then read token-on-lanes for the score / dP chains (rows 2 j and 2 j + 1 of a step, 32 consecutive floats
// each) and channel-on-lanes for the second product (the odd stride keeps the 32 channels of a lane half on 32 banks).
// Split.  At the U-Nets' shapes there is ONE batch element with 4 or 1 heads and L = 4096: owner tiles alone are 512 or 128 waves
// for 1024 SIMDs, each walking 128 tiles in sequence.  So a workgroup is four waves on ONE owner tile: wave w walks tiles w, w + 4,
// w + 8, ... with buffers of its own (the loads of its next tile are issued before the products of the current one, and no
// workgroup barrier stands in the loop), and the four partial results are combined through LDS in the fixed order w = 0..3 —
// the forward's (max, sum, O) triples rescaled to the common maximum, Delta and the gradients' tiles by plain float64 addition.
// No atomics: the query-owned pass writes Delta and the q rows of g_qkv, the key-owned pass the k and v rows, every element once,
// by one wave, in place in the interleaved layout.  Backward: P = exp(score - lse) recomputed through the same chains (bit for
// bit the forward's), dS = P (dP - Delta), Delta = sum_s P dP / sum_s P (float64) from a first sweep of the query-owned pass
// over the very dP values dS subtracts it from.
#include "s360_device.h"
#include "s360_bf16x3.h"

namespace s360 {

constexpr int QA_CH = 32;                                     // channels per head
constexpr int QA_T = 32;                                      // rows of an MFMA tile
constexpr int QA_WAVES = S360_BLOCK / S360_WAVE;              // waves that share the walk of one owner tile
constexpr int QA_LD = QA_T + 1;                               // row stride of a staged tile in LDS (floats)
constexpr int QA_TILE = QA_CH * QA_LD;                        // floats of a staged tile
constexpr int QA_ND = 17;                                     // float64 values per lane a wave hands to the combine (16 + the sum)
// one buffer serves the waves' staged tile pairs in the walk and their partial results in the combine
constexpr int QA_RAW = QA_WAVES * QA_ND * S360_WAVE;          // float64 words
static_assert(QA_RAW * 8 >= QA_WAVES * 2 * QA_TILE * 4, "the combine area covers the staging area");

struct QAArgs {
    const float* qkv;
    int B, views, heads, T, L, W;                             // W = heads 3 ch channel rows of qkv
    int order;
    double inv_scale;                                         // 1 / sqrt(ch): multiplies the float64 score sums and g_q, g_k
};

// element offset of (channel row 0, joint token s) of batch element bi in a [N, width, T] tensor
__device__ __forceinline__ size_t qa_token(const QAArgs& a, int bi, int s, int width) {
    const int u = s / a.T, t = s - u * a.T;
    return ((size_t)(u * a.B + bi) * width) * a.T + t;
}

// first channel rows of head hd's q, k and v
__device__ __forceinline__ void qa_head(const QAArgs& a, int hd, int& qo, int& ko, int& vo) {
    if (a.order == 0) { qo = hd * 3 * QA_CH; ko = qo + QA_CH; vo = ko + QA_CH; }
    else { qo = hd * QA_CH; ko = a.heads * QA_CH + qo; vo = 2 * a.heads * QA_CH + qo; }
}

// channel rows hf, hf + 2, ... of one token (p: its channel row 0; null: zeros): the owner's row — channel 2 j + hf is the lane's
// operand of MFMA step j — and a lane's share of a staged tile, whose token l31 it reads: a wave's load is two coalesced
// 128-byte rows
__device__ __forceinline__ void qa_load_rows(const float* p, int T, int hf, float* x) {
#pragma unroll
    for (int j = 0; j < QA_CH / 2; ++j) x[j] = p ? p[(size_t)(2 * j + hf) * T] : 0.f;
}

// the wave's share of walked tile `tile` of a [N, width, T] tensor, channel rows from coff; tokens past L read as zeros
__device__ __forceinline__ void qa_stage_load(const QAArgs& a, const float* src, int width, int bi, int coff, int tile, int l31, int hf,
                                              float* x) {
    const int s = tile * QA_T + l31;
    qa_load_rows(s < a.L ? src + qa_token(a, bi, s, width) + (size_t)coff * a.T : nullptr, a.T, hf, x);
}

__device__ __forceinline__ void qa_stage_store(float* buf, int l31, int hf, const float* x) {
    float* p = buf + hf * QA_LD + l31;
#pragma unroll
    for (int j = 0; j < QA_CH / 2; ++j) p[2 * j * QA_LD] = x[j];
}

// Between a wave's writes of its own LDS buffer and its reads of it (and back): the LDS serves one wave's instructions in the
// order they were issued, so no hardware barrier is needed; this keeps the compiler from moving them across each other.
__device__ __forceinline__ void qa_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// out = mul * sum over the channels of walked-token row x owner row, in FLOAT64.  `tile` points at (channel hf, token l31) of a
// staged tile, b holds the owner's channels 2 j + hf.  The sum runs in chunks of 4 MFMA steps (8 channels): a chunk is one
// float32 fma chain from zero and the chunks are added in float64 (the window attention's wa_dot).  The sum is NOT rounded to
// float32: a score goes into exp as the float32 of (score - max) or (score - lse), a difference taken in float64, so that the
// rounding is relative to the difference and not to the score (at logits of +-100 the rounding of the score itself is 4e-6 in
// the exponent, which two keys of comparable weight show in full in dS), and dP meets Delta in float64.  The forward and both
// backward passes form every score and every dP through this one function, with the operands' roles exchanged in the key-owned
// pass (the products commute, their order does not change): recomputed tiles are the forward's bit for bit.  Each chunk's zero
// tile passes an empty asm statement that depends on the sums as they stand, so that at most three tiles are live and the
// float64 adds of chunk c - 1 run under the MFMAs of chunk c.
__device__ __forceinline__ void qa_dot(const float* tile, const float* b, double mul, double* out) {
    double sum[16];
    f32x16 prev;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = 0.0, prev[r] = 0.f;
#pragma unroll
    for (int c = 0; c < QA_CH / 8; ++c) {
        float z = 0.f;
        asm volatile("" : "+v"(z) : "v"(sum[15]));
        f32x16 t;
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = z;
#pragma unroll
        for (int i = 0; i < 4; ++i) t = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[2 * (4 * c + i) * QA_LD], b[4 * c + i], t, 0, 0, 0);
        if (c > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sum[r] += (double)prev[r];
        }
        prev = t;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r] = (sum[r] + (double)prev[r]) * mul;
}

// acc^T[channel][owner] += sum over the tile's 32 walked tokens of tile[channel][token] x w[token][owner]: `tile` points at
// (channel l31, token 4 hf) of a staged tile, w is a score-shaped tile held register by register.  The 32 tokens of a tile are
// one float32 fma chain from zero; the tiles are added in FLOAT64 (a float32 chain over all L tokens rounds at the size of the
// running sum at every step: at L = 640 it missed the accuracy rule of the tests in out).
__device__ __forceinline__ void qa_accumulate(const float* tile, const float* w, double* acc) {
    f32x16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[(r & 3) + 8 * (r >> 2)], w[r], t, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += (double)t[r];
}

// workgroup decomposition shared by the three kernels: owner tile ot of head hd of batch element bi
struct QABlock { int ot, hd, bi; };
__device__ __forceinline__ QABlock qa_block(const QAArgs& a) {
    const int otiles = (a.L + QA_T - 1) / QA_T;
    int blk = blockIdx.x;
    QABlock w;
    w.ot = blk % otiles; blk /= otiles;
    w.hd = blk % a.heads;
    w.bi = blk / a.heads;
    return w;
}

// the combine: wave `wave` hands x[0..n) per lane to the workgroup; callers put a barrier in front (the area is the waves'
// staging buffers) and behind
__device__ __forceinline__ void qa_hand_over(double* raw, int wave, int lane, const double* x, int n) {
#pragma unroll
    for (int i = 0; i < QA_ND; ++i)
        if (i < n) raw[(wave * QA_ND + i) * S360_WAVE + lane] = x[i];
}
__device__ __forceinline__ double qa_handed(const double* raw, int wave, int lane, int i) { return raw[(wave * QA_ND + i) * S360_WAVE + lane]; }

// Forward.  Owner: 32 queries.  Each wave walks its key tiles with a running maximum (float32: it is one of the scores) and a
// running sum (float64); wave 0 merges the four (m, sum, O) in the order w = 0..3 and writes.
__global__ __launch_bounds__(S360_BLOCK) void k_qa_forward(QAArgs a, float* __restrict__ out, double* __restrict__ lse) {
    __shared__ double s_raw[QA_RAW];
    __shared__ float s_m[QA_WAVES][S360_WAVE];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const QABlock w = qa_block(a);
    int qo, ko, vo;
    qa_head(a, w.hd, qo, ko, vo);
    const int sq = w.ot * QA_T + l31;
    const bool qvalid = sq < a.L;
    float qB[QA_CH / 2];
    qa_load_rows(qvalid ? a.qkv + qa_token(a, w.bi, sq, a.W) + (size_t)qo * a.T : nullptr, a.T, hf, qB);
    double o[QA_ND];                                          // O^T, and the running sum in o[16]
#pragma unroll
    for (int r = 0; r < QA_ND; ++r) o[r] = 0.0;
    float m = -INFINITY;
    const int ntiles = (a.L + QA_T - 1) / QA_T;
    float* ks = reinterpret_cast<float*>(s_raw) + wave * 2 * QA_TILE;
    float* vs = ks + QA_TILE;
    float rk[QA_CH / 2], rv[QA_CH / 2];
    if (wave < ntiles) {
        qa_stage_load(a, a.qkv, a.W, w.bi, ko, wave, l31, hf, rk);
        qa_stage_load(a, a.qkv, a.W, w.bi, vo, wave, l31, hf, rv);
    }
    for (int t = wave; t < ntiles; t += QA_WAVES) {
        qa_stage_store(ks, l31, hf, rk);
        qa_stage_store(vs, l31, hf, rv);
        qa_wave_sync();
        if (t + QA_WAVES < ntiles) {
            qa_stage_load(a, a.qkv, a.W, w.bi, ko, t + QA_WAVES, l31, hf, rk);
            qa_stage_load(a, a.qkv, a.W, w.bi, vo, t + QA_WAVES, l31, hf, rv);
        }
        double s[16];
        qa_dot(ks + hf * QA_LD + l31, qB, a.inv_scale, s);    // S^T / sqrt(ch): rows = keys, lane = query
        float p[16];
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (t * QA_T + mfma_acc_row(r, hf) < a.L) tmax = fmaxf(tmax, (float)s[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mnew = fmaxf(m, tmax);                    // finite: key 0 of every tile exists
        const float alpha = expf(m - mnew);                   // 0 at the wave's first tile
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            p[r] = t * QA_T + mfma_acc_row(r, hf) < a.L ? expf((float)(s[r] - (double)mnew)) : 0.f;
            rs += p[r];
        }
        rs += __shfl_xor(rs, 32);
        m = mnew;
#pragma unroll
        for (int r = 0; r < QA_ND; ++r) o[r] *= (double)alpha;
        o[16] += (double)rs;
        qa_accumulate(vs + l31 * QA_LD + 4 * hf, p, o);       // O^T += V P^T, two keys (one per lane half) a step
        qa_wave_sync();
    }
    __syncthreads();                                          // every wave has left its staging buffers
    qa_hand_over(s_raw, wave, lane, o, QA_ND);
    s_m[wave][lane] = m;
    __syncthreads();
    if (wave != 0 || !qvalid) return;
    float mall = m;                                           // wave 0 has tile 0: finite
#pragma unroll
    for (int u = 1; u < QA_WAVES; ++u) mall = fmaxf(mall, s_m[u][lane]);
#pragma unroll
    for (int r = 0; r < QA_ND; ++r) o[r] = 0.0;
#pragma unroll
    for (int u = 0; u < QA_WAVES; ++u) {
        const double f = (double)expf(s_m[u][lane] - mall);   // 0 for a wave without tiles (its maximum is -inf)
#pragma unroll
        for (int r = 0; r < QA_ND; ++r) o[r] += qa_handed(s_raw, u, lane, r) * f;
    }
    float* po = out + qa_token(a, w.bi, sq, a.heads * QA_CH) + (size_t)(w.hd * QA_CH) * a.T;
#pragma unroll
    for (int r = 0; r < 16; ++r) po[(size_t)mfma_acc_row(r, hf) * a.T] = (float)(o[r] / o[16]);
    if (hf == 0) lse[((size_t)w.bi * a.heads + w.hd) * a.L + sq] = (double)mall + log(o[16]);
}

// Backward, Delta and the q rows of g_qkv.  Owner: 32 queries (as the forward).  First sweep over the key tiles: sum_s P dP and
// sum_s P per query, float64 (the waves' partial sums added in the order w = 0..3); Delta = sum P dP / sum P is written to delta[]
// for the key-owned pass; second sweep: dS^T = P (dP - Delta), g_q^T += K dS^T.  Delta is formed from the very dP values dS
// subtracts it from (the same fma chains in both sweeps and in the key-owned pass), as torch's softmax backward forms it;
// rowsum(g_out out) does not have that property (s360_window_attention.hip, k_wa_backward_q).  The division by sum P, which is
// 1 but for the roundings of lse and of the recomputed exponentials (1e-7), makes sum_s dS = 0 hold for the P that are used: a
// common factor 1 + e on a row's P then costs dS a relative e, where P (dP - sum P dP) is off by e P Delta — the whole of dS
// at a row whose weight sits on one key, where dP - Delta is a small difference of large numbers (the 5-token case of the tests
// at logits of +-100 showed it: 2.4e-6 on gradients of 3e-6).  The two sweeps are two loops in the code (`sweep` is a constant in each).
__global__ __launch_bounds__(S360_BLOCK) void k_qa_backward_q(QAArgs a, const double* __restrict__ lse, const float* __restrict__ g_out,
                                                              double* __restrict__ delta, float* __restrict__ g_qkv) {
    __shared__ double s_raw[QA_RAW];
    __shared__ double s_sum[2][QA_WAVES][S360_WAVE];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const QABlock w = qa_block(a);
    int qo, ko, vo;
    qa_head(a, w.hd, qo, ko, vo);
    const int sq = w.ot * QA_T + l31;
    const bool qvalid = sq < a.L;
    const size_t qtok = qvalid ? qa_token(a, w.bi, sq, a.W) + (size_t)qo * a.T : 0;
    const size_t stat = ((size_t)w.bi * a.heads + w.hd) * a.L + sq;
    float qB[QA_CH / 2], gB[QA_CH / 2];
    qa_load_rows(qvalid ? a.qkv + qtok : nullptr, a.T, hf, qB);
    qa_load_rows(qvalid ? g_out + qa_token(a, w.bi, sq, a.heads * QA_CH) + (size_t)(w.hd * QA_CH) * a.T : nullptr, a.T, hf, gB);
    const double lq = qvalid ? lse[stat] : 0.0;
    double dsum = 0.0, psum = 0.0;
    double acc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0;
    const int ntiles = (a.L + QA_T - 1) / QA_T;
    float* ks = reinterpret_cast<float*>(s_raw) + wave * 2 * QA_TILE;
    float* vs = ks + QA_TILE;
    float rk[QA_CH / 2], rv[QA_CH / 2];
#pragma unroll
    for (int sweep = 0; sweep < 2; ++sweep) {
        if (wave < ntiles) {
            qa_stage_load(a, a.qkv, a.W, w.bi, ko, wave, l31, hf, rk);
            qa_stage_load(a, a.qkv, a.W, w.bi, vo, wave, l31, hf, rv);
        }
        for (int t = wave; t < ntiles; t += QA_WAVES) {
            qa_stage_store(ks, l31, hf, rk);
            qa_stage_store(vs, l31, hf, rv);
            qa_wave_sync();
            if (t + QA_WAVES < ntiles) {
                qa_stage_load(a, a.qkv, a.W, w.bi, ko, t + QA_WAVES, l31, hf, rk);
                qa_stage_load(a, a.qkv, a.W, w.bi, vo, t + QA_WAVES, l31, hf, rv);
            }
            double s[16], dp[16];
            float ds[16];
            qa_dot(ks + hf * QA_LD + l31, qB, a.inv_scale, s);                           // S^T / sqrt(ch)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool kvalid = t * QA_T + mfma_acc_row(r, hf) < a.L;
                ds[r] = (kvalid && qvalid) ? expf((float)(s[r] - lq)) : 0.f;             // P^T
            }
            qa_dot(vs + hf * QA_LD + l31, gB, 1.0, dp);                                  // dP^T = V^T dO
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (sweep == 0) dsum += (double)ds[r] * dp[r], psum += (double)ds[r];
                else ds[r] *= (float)(dp[r] - dsum);
            }
            if (sweep == 1) qa_accumulate(ks + l31 * QA_LD + 4 * hf, ds, acc);           // g_q^T += K dS^T
            qa_wave_sync();
        }
        if (sweep == 0) {
            dsum += __shfl_xor(dsum, 32);
            psum += __shfl_xor(psum, 32);
            s_sum[0][wave][lane] = dsum;
            s_sum[1][wave][lane] = psum;
            __syncthreads();
            dsum = psum = 0.0;
#pragma unroll
            for (int u = 0; u < QA_WAVES; ++u) dsum += s_sum[0][u][lane], psum += s_sum[1][u][lane];
            dsum = psum > 0.0 ? dsum / psum : 0.0;                                       // the same Delta in every wave; a query past L has no P
            if (wave == 0 && qvalid && hf == 0) delta[stat] = dsum;
        }
    }
    __syncthreads();                                          // every wave has left its staging buffers
    qa_hand_over(s_raw, wave, lane, acc, 16);
    __syncthreads();
    if (wave != 0 || !qvalid) return;
    float* pg = g_qkv + qtok;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        double x = 0.0;
#pragma unroll
        for (int u = 0; u < QA_WAVES; ++u) x += qa_handed(s_raw, u, lane, r);
        pg[(size_t)mfma_acc_row(r, hf) * a.T] = (float)(x * a.inv_scale);
    }
}

// Backward, the k and v rows of g_qkv.  Owner: 32 keys; the waves walk the query tiles, whose q and dO rows are staged with
// their lse and Delta.  S = Q^T K (rows = queries, lane = key), g_v^T += dO P, g_k^T += Q dS; the waves' partial tiles are added
// in the order w = 0..3, g_v first, then g_k through the same area.
__global__ __launch_bounds__(S360_BLOCK) void k_qa_backward_kv(QAArgs a, const double* __restrict__ lse, const double* __restrict__ delta,
                                                               const float* __restrict__ g_out, float* __restrict__ g_qkv) {
    __shared__ double s_raw[QA_RAW];
    __shared__ double s_stat[QA_WAVES][S360_WAVE];            // per wave: lse of the tile's 32 queries, then their Delta
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const QABlock w = qa_block(a);
    int qo, ko, vo;
    qa_head(a, w.hd, qo, ko, vo);
    const int sk = w.ot * QA_T + l31;
    const bool kvalid = sk < a.L;
    const size_t ktok = kvalid ? qa_token(a, w.bi, sk, a.W) : 0;
    const size_t stat = ((size_t)w.bi * a.heads + w.hd) * a.L;
    const double* stats = hf ? delta : lse;
    const int GW = a.heads * QA_CH, go = w.hd * QA_CH;
    float kB[QA_CH / 2], vB[QA_CH / 2];
    qa_load_rows(kvalid ? a.qkv + ktok + (size_t)ko * a.T : nullptr, a.T, hf, kB);
    qa_load_rows(kvalid ? a.qkv + ktok + (size_t)vo * a.T : nullptr, a.T, hf, vB);
    double dk[16], dv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[r] = dv[r] = 0.0;
    const int ntiles = (a.L + QA_T - 1) / QA_T;
    float* qs = reinterpret_cast<float*>(s_raw) + wave * 2 * QA_TILE;
    float* gs = qs + QA_TILE;
    const double* sl = s_stat[wave];
    const double* sd = s_stat[wave] + QA_T;
    float rq[QA_CH / 2], rg[QA_CH / 2];
    double rs = 0.0;
    if (wave < ntiles) {
        qa_stage_load(a, a.qkv, a.W, w.bi, qo, wave, l31, hf, rq);
        qa_stage_load(a, g_out, GW, w.bi, go, wave, l31, hf, rg);
        rs = wave * QA_T + l31 < a.L ? stats[stat + wave * QA_T + l31] : 0.0;
    }
    for (int t = wave; t < ntiles; t += QA_WAVES) {
        qa_stage_store(qs, l31, hf, rq);
        qa_stage_store(gs, l31, hf, rg);
        s_stat[wave][lane] = rs;
        qa_wave_sync();
        if (t + QA_WAVES < ntiles) {
            const int tn = t + QA_WAVES;
            qa_stage_load(a, a.qkv, a.W, w.bi, qo, tn, l31, hf, rq);
            qa_stage_load(a, g_out, GW, w.bi, go, tn, l31, hf, rg);
            rs = tn * QA_T + l31 < a.L ? stats[stat + tn * QA_T + l31] : 0.0;
        }
        double s[16];
        float p[16];
        qa_dot(qs + hf * QA_LD + l31, kB, a.inv_scale, s);    // S / sqrt(ch): rows = queries, lane = key; the forward's chain, bit for bit
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = mfma_acc_row(r, hf);
            p[r] = (kvalid && t * QA_T + qq < a.L) ? expf((float)(s[r] - sl[qq])) : 0.f;
        }
        qa_accumulate(gs + l31 * QA_LD + 4 * hf, p, dv);      // g_v^T += dO P
        qa_dot(gs + hf * QA_LD + l31, vB, 1.0, s);            // dP = dO^T V
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] *= (float)(s[r] - sd[mfma_acc_row(r, hf)]);      // dS = P (dP - Delta)
        qa_accumulate(qs + l31 * QA_LD + 4 * hf, p, dk);      // g_k^T += Q dS
        qa_wave_sync();
    }
    float* pk = g_qkv + ktok + (size_t)ko * a.T;
    float* pv = g_qkv + ktok + (size_t)vo * a.T;
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        __syncthreads();                                      // every wave has left its staging buffers / wave 0 has read part 0
        qa_hand_over(s_raw, wave, lane, part == 0 ? dv : dk, 16);
        __syncthreads();
        if (wave == 0 && kvalid) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                double x = 0.0;
#pragma unroll
                for (int u = 0; u < QA_WAVES; ++u) x += qa_handed(s_raw, u, lane, r);
                const size_t c = (size_t)mfma_acc_row(r, hf) * a.T;
                if (part == 0) pv[c] = (float)x;
                else pk[c] = (float)(x * a.inv_scale);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- the "high" mode (bf16 x 3)
// The same function with every product as a bf16x3 product (s360_bf16x3.h: the split, the three terms and their order, the
// B-operand register rule); q and k are split unscaled and 1 / sqrt(ch) multiplies the summed score (and g_q, g_k) once.
// Orientation, decomposition and combine are those of the kernels above: the owner on the lanes, the walked tile on the
// accumulator's rows, four waves on one owner tile, their partial results combined through LDS in the order w = 0..3.  A
// score is the MFMA's float32 sum, and tiles are accumulated in float32 in the MFMA's accumulator, rescaled by the running
// maximum's factor in the forward.  The forward's softmax is float32 (score x float32(1 / sqrt(ch)), minus the running maximum);
// the backward's P = exp(float32(sum / sqrt(ch) - lse)) and dS = P float32(dP - Delta) take their differences in float64, as the
// kernels above do: P is then the float32 number next to the exact softmax of the summed scores, which is what its split depends on
// (a P a few float32 steps off rounds its lo part the other way now and then, 2^-17 P each time; qah_exp).
// A pre-pass (k_qah_split, one launch per operand) resolves the (v b) row gather, the head interleave and the channel order
// once per call and writes bf16 planes in joint-sequence order per (batch element, head) into the caller's scratch, L padded
// to a multiple of 32 (Lpad) with zeros — every byte the main kernels read is written, so the scratch needs no initialisation:
//   rows       [B, heads, Lpad, 32]: a lane reads 8 consecutive channels of its token, 16 bytes (scores, dP)
//   transposed [B, heads, 32, Lpad]: the walked token is the k-dimension (O, g_q, g_k, g_v).  Within a tile of 32 tokens the
//              order is the one the B-operand register rule imposes: token u = 16 s + 8 (j / 4) + 4 h + j % 4 of a tile is
//              stored at qah_tpos(u) = 16 h + 8 s + j, and a lane reads its 8 tokens of a step as 16 consecutive bytes.
// The terms of a score are in (q, k) order — (qh, kh), (ql, kh), (qh, kl) — and those of dP in (g, v) order, whichever side is
// walked: the P recomputed in both backward passes is formed from the forward's sums bit for bit.
// Walked fragments are read straight from the planes (they stay in L2: 256 KB per plane and head at L = 4096), the next tile's
// loads issued before the current tile's products.

struct QAHPlanes {                                            // hi and lo planes of the operands; null where a call has none
    __bf16 *q_rh, *q_rl, *q_th, *q_tl;
    __bf16 *k_rh, *k_rl, *k_th, *k_tl;
    __bf16 *v_rh, *v_rl, *v_th, *v_tl;
    __bf16 *g_rh, *g_rl, *g_th, *g_tl;
};

__host__ __device__ __forceinline__ int qah_pad(int n) { return (n + QA_T - 1) & ~(QA_T - 1); }

// position of token u (< 32) of a tile in a transposed plane (above)
__device__ __forceinline__ int qah_tpos(int u) { return 16 * ((u >> 2) & 1) + 8 * (u >> 4) + 4 * ((u >> 3) & 1) + (u & 3); }

// exp(x) of a float64 x as a float32 number: expf of x's leading float32 part e, times 1 + the rest.  The backward's P through
// this is within a float32 step or two of the exact exp(x); expf((float)x) alone is off by the rounding of x, up to 2^-24 |x| of P.
__device__ __forceinline__ float qah_exp(double x) {
    const float h = (float)x, e = expf(h);
    return fmaf(e, (float)(x - (double)h), e);
}

// the two k-steps of one operand tile, hi and lo: of a rows plane channels 8 hf + 16 s .. + 7 of the lane's token, of a
// transposed plane the lane's channel at the 8 tokens of step s
struct QAHFrag { bf16x8 h[2], l[2]; };

// p: element offset of the lane's first 8 values; step: elements between the k-steps (16 in a rows plane, 8 in a transposed one)
__device__ __forceinline__ QAHFrag qah_load(const __bf16* hi, const __bf16* lo, size_t p, int step) {
    QAHFrag f;
#pragma unroll
    for (int s = 0; s < 2; ++s) f.h[s] = bx3_ld8(hi + p + s * step), f.l[s] = bx3_ld8(lo + p + s * step);
    return f;
}

// tile[walked][owner] = sum over the 32 channels of walked row x owner row: walked fragments as A, the owner's as B
template <bool SWAP>
__device__ __forceinline__ f32x16 qah_dot(const QAHFrag& w, const QAHFrag& o) {
    f32x16 acc = bx3_zero();
#pragma unroll
    for (int s = 0; s < 2; ++s) acc = bx3_mfma3<SWAP>(w.h[s], w.l[s], o.h[s], o.l[s], acc);
    return acc;
}

// acc^T[channel][owner] += sum over the tile's 32 walked tokens of t[channel][token] x[token][owner]: x[16] is the lane's column
// of a score-shaped tile, split here register by register
__device__ __forceinline__ f32x16 qah_accumulate(f32x16 acc, const QAHFrag& t, const float* x) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        bf16x8 xh, xl;
        bx3_split8(x + 8 * s, xh, xl);
        acc = bx3_mfma3<false>(t.h[s], t.l[s], xh, xl, acc);
    }
    return acc;
}

// The pre-pass: one operand (which: 0 q, 1 k, 2 v of qkv; 3 g_out) into its planes.  Thread i takes 8 channels of one joint
// token of one (batch element, head), the token fastest: a wave's reads are 8 coalesced rows along t and its 2-byte stores into
// the transposed plane fill whole 64-byte tiles.  Tokens from L to Lpad are written as zeros.  rh / rl or th / tl may be null.
__global__ __launch_bounds__(S360_BLOCK) void k_qah_split(QAArgs a, const float* __restrict__ src, int which, __bf16* __restrict__ rh,
                                                          __bf16* __restrict__ rl, __bf16* __restrict__ th, __bf16* __restrict__ tl) {
    const int lpad = qah_pad(a.L);
    const size_t i = (size_t)blockIdx.x * S360_BLOCK + threadIdx.x;
    const size_t per = (size_t)lpad * (QA_CH / 8), nbh = (size_t)a.B * a.heads;
    if (i >= nbh * per) return;
    const size_t bh = i / per;
    const int rem = (int)(i - bh * per), cg = rem / lpad, s = rem - cg * lpad;
    const int bi = (int)(bh / a.heads), hd = (int)(bh - (size_t)bi * a.heads);
    int width = a.heads * QA_CH, coff = hd * QA_CH;
    if (which != 3) {
        int qo, ko, vo;
        qa_head(a, hd, qo, ko, vo);
        width = a.W;
        coff = which == 0 ? qo : which == 1 ? ko : vo;
    }
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = 0.f;
    if (s < a.L) {
        const float* p = src + qa_token(a, bi, s, width) + (size_t)(coff + 8 * cg) * a.T;
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = p[(size_t)j * a.T];
    }
    bf16x8 hi, lo;
    bx3_split8(x, hi, lo);
    if (rh) bx3_st8(rh, rl, (bh * lpad + s) * QA_CH + 8 * cg, hi, lo);
    if (th) {
        const int pos = (s & ~(QA_T - 1)) + qah_tpos(s & (QA_T - 1));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const size_t o = (bh * QA_CH + 8 * cg + j) * lpad + pos;
            th[o] = hi[j];
            tl[o] = lo[j];
        }
    }
}

// what the three main kernels share: the lane's offsets into the planes of its (batch element, head)
struct QAHLane {
    size_t rows;                                              // rows plane: (token l31 of tile 0, channel 8 hf); a tile is QA_T QA_CH further
    size_t cols;                                              // transposed plane: (channel l31, position 16 hf of tile 0); a tile is QA_T further
    size_t own;                                               // rows plane: (the lane's owner token, channel 8 hf)
};
__device__ __forceinline__ QAHLane qah_lane(const QAArgs& a, const QABlock& w, int l31, int hf) {
    const size_t lpad = qah_pad(a.L), bh = (size_t)w.bi * a.heads + w.hd;
    QAHLane o;
    o.rows = (bh * lpad + l31) * QA_CH + 8 * hf;
    o.cols = (bh * QA_CH + l31) * lpad + 16 * hf;
    o.own = o.rows + (size_t)w.ot * QA_T * QA_CH;
    return o;
}
constexpr int QAH_ROWS_TILE = QA_T * QA_CH;

// Forward.  Owner: 32 queries, their split rows in registers.  Each wave walks its key tiles with a float32 running maximum, a
// float64 running sum and O^T in the MFMA's accumulator; wave 0 merges the four (m, sum, O) in the order w = 0..3 and writes.
__global__ __launch_bounds__(S360_BLOCK) void k_qah_forward(QAArgs a, QAHPlanes pl, float* __restrict__ out, double* __restrict__ lse) {
    __shared__ float s_o[QA_WAVES][16][S360_WAVE];
    __shared__ double s_l[QA_WAVES][S360_WAVE];
    __shared__ float s_m[QA_WAVES][S360_WAVE];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const QABlock w = qa_block(a);
    const QAHLane at = qah_lane(a, w, l31, hf);
    const int sq = w.ot * QA_T + l31;
    const bool qvalid = sq < a.L;
    const float sc = (float)a.inv_scale;
    const QAHFrag q = qah_load(pl.q_rh, pl.q_rl, at.own, 16);
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    float m = -INFINITY;
    double lsum = 0.0;
    const int ntiles = (a.L + QA_T - 1) / QA_T;
    QAHFrag k = q, v = q;                                     // a wave without tiles never uses them
    if (wave < ntiles) {
        k = qah_load(pl.k_rh, pl.k_rl, at.rows + (size_t)wave * QAH_ROWS_TILE, 16);
        v = qah_load(pl.v_th, pl.v_tl, at.cols + (size_t)wave * QA_T, 8);
    }
    for (int t = wave; t < ntiles; t += QA_WAVES) {
        QAHFrag kn = k, vn = v;
        if (t + QA_WAVES < ntiles) {
            kn = qah_load(pl.k_rh, pl.k_rl, at.rows + (size_t)(t + QA_WAVES) * QAH_ROWS_TILE, 16);
            vn = qah_load(pl.v_th, pl.v_tl, at.cols + (size_t)(t + QA_WAVES) * QA_T, 8);
        }
        const f32x16 s = qah_dot<false>(k, q);                // S^T: rows = keys, lane = query
        float p[16];
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            p[r] = t * QA_T + mfma_acc_row(r, hf) < a.L ? s[r] * sc : -INFINITY;
            tmax = fmaxf(tmax, p[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mnew = fmaxf(m, tmax);                    // finite: key 0 of every tile exists
        const float alpha = expf(m - mnew);                   // 0 at the wave's first tile
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            p[r] = expf(p[r] - mnew);
            rs += p[r];
        }
        rs += __shfl_xor(rs, 32);
        lsum = lsum * (double)alpha + (double)rs;
        m = mnew;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= alpha;
        o = qah_accumulate(o, v, p);                          // O^T += V P^T
        k = kn;
        v = vn;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s_o[wave][r][lane] = o[r];
    s_l[wave][lane] = lsum;
    s_m[wave][lane] = m;
    __syncthreads();
    if (wave != 0 || !qvalid) return;
    float mall = m;                                           // wave 0 has tile 0: finite
#pragma unroll
    for (int u = 1; u < QA_WAVES; ++u) mall = fmaxf(mall, s_m[u][lane]);
    double x[16], l = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = 0.0;
#pragma unroll
    for (int u = 0; u < QA_WAVES; ++u) {
        const double f = (double)expf(s_m[u][lane] - mall);   // 0 for a wave without tiles (its maximum is -inf)
        l += s_l[u][lane] * f;
#pragma unroll
        for (int r = 0; r < 16; ++r) x[r] += (double)s_o[u][r][lane] * f;
    }
    float* po = out + qa_token(a, w.bi, sq, a.heads * QA_CH) + (size_t)(w.hd * QA_CH) * a.T;
#pragma unroll
    for (int r = 0; r < 16; ++r) po[(size_t)mfma_acc_row(r, hf) * a.T] = (float)(x[r] / l);
    if (hf == 0) lse[((size_t)w.bi * a.heads + w.hd) * a.L + sq] = (double)mall + log(l);
}

// Backward, Delta and the q rows of g_qkv.  Owner: 32 queries; two sweeps, as k_qa_backward_q: Delta = sum P dP / sum P from the
// first, every term and the waves' partial sums (w = 0..3) in float64 — a tile's terms summed in float32 first missed the
// accuracy rule at the 5-token shape at logits of +-100 (4.1e-6 on gradients of 2.9e-6: dS of a one-hot row is P (dP - Delta),
// a small difference of numbers of 30) —, dS^T = P (dP - Delta) and g_q^T += K dS^T in the second.
__global__ __launch_bounds__(S360_BLOCK) void k_qah_backward_q(QAArgs a, QAHPlanes pl, const double* __restrict__ lse,
                                                               double* __restrict__ delta, float* __restrict__ g_qkv) {
    __shared__ float s_acc[QA_WAVES][16][S360_WAVE];
    __shared__ double s_sum[2][QA_WAVES][S360_WAVE];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const QABlock w = qa_block(a);
    const QAHLane at = qah_lane(a, w, l31, hf);
    int qo, ko, vo;
    qa_head(a, w.hd, qo, ko, vo);
    const int sq = w.ot * QA_T + l31;
    const bool qvalid = sq < a.L;
    const size_t stat = ((size_t)w.bi * a.heads + w.hd) * a.L + sq;
    const QAHFrag q = qah_load(pl.q_rh, pl.q_rl, at.own, 16), g = qah_load(pl.g_rh, pl.g_rl, at.own, 16);
    const double lq = qvalid ? lse[stat] : 0.0;
    double dsum = 0.0, psum = 0.0;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int ntiles = (a.L + QA_T - 1) / QA_T;
#pragma unroll
    for (int sweep = 0; sweep < 2; ++sweep) {
        QAHFrag k = q, v = q, kt = q;
        if (wave < ntiles) {
            k = qah_load(pl.k_rh, pl.k_rl, at.rows + (size_t)wave * QAH_ROWS_TILE, 16);
            v = qah_load(pl.v_rh, pl.v_rl, at.rows + (size_t)wave * QAH_ROWS_TILE, 16);
            if (sweep == 1) kt = qah_load(pl.k_th, pl.k_tl, at.cols + (size_t)wave * QA_T, 8);
        }
        for (int t = wave; t < ntiles; t += QA_WAVES) {
            QAHFrag kn = k, vn = v, ktn = kt;
            if (t + QA_WAVES < ntiles) {
                kn = qah_load(pl.k_rh, pl.k_rl, at.rows + (size_t)(t + QA_WAVES) * QAH_ROWS_TILE, 16);
                vn = qah_load(pl.v_rh, pl.v_rl, at.rows + (size_t)(t + QA_WAVES) * QAH_ROWS_TILE, 16);
                if (sweep == 1) ktn = qah_load(pl.k_th, pl.k_tl, at.cols + (size_t)(t + QA_WAVES) * QA_T, 8);
            }
            const f32x16 s = qah_dot<false>(k, q);            // S^T
            const f32x16 dp = qah_dot<false>(v, g);           // dP^T = V^T dO
            float ds[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool kvalid = t * QA_T + mfma_acc_row(r, hf) < a.L;
                const float p = (kvalid && qvalid) ? qah_exp((double)s[r] * a.inv_scale - lq) : 0.f;     // P^T
                if (sweep == 0) dsum += (double)p * (double)dp[r], psum += (double)p;
                else ds[r] = p * (float)((double)dp[r] - dsum);
            }
            if (sweep == 1) acc = qah_accumulate(acc, kt, ds);           // g_q^T += K dS^T
            k = kn;
            v = vn;
            kt = ktn;
        }
        if (sweep == 0) {
            dsum += __shfl_xor(dsum, 32);
            psum += __shfl_xor(psum, 32);
            s_sum[0][wave][lane] = dsum;
            s_sum[1][wave][lane] = psum;
            __syncthreads();
            dsum = psum = 0.0;
#pragma unroll
            for (int u = 0; u < QA_WAVES; ++u) dsum += s_sum[0][u][lane], psum += s_sum[1][u][lane];
            dsum = psum > 0.0 ? dsum / psum : 0.0;            // the same Delta in every wave; a query past L has no P
            if (wave == 0 && qvalid && hf == 0) delta[stat] = dsum;
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s_acc[wave][r][lane] = acc[r];
    __syncthreads();
    if (wave != 0 || !qvalid) return;
    float* pg = g_qkv + qa_token(a, w.bi, sq, a.W) + (size_t)qo * a.T;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        double x = 0.0;
#pragma unroll
        for (int u = 0; u < QA_WAVES; ++u) x += (double)s_acc[u][r][lane];
        pg[(size_t)mfma_acc_row(r, hf) * a.T] = (float)(x * a.inv_scale);
    }
}

// Backward, the k and v rows of g_qkv.  Owner: 32 keys; the waves walk the query tiles, whose lse and Delta a wave stages in LDS.  S = Q^T K (rows = queries, lane = key), g_v^T += dO P, g_k^T += Q dS; the waves' partial tiles are
// added in the order w = 0..3, g_v first, then g_k through the same area.
__global__ __launch_bounds__(S360_BLOCK) void k_qah_backward_kv(QAArgs a, QAHPlanes pl, const double* __restrict__ lse,
                                                                const double* __restrict__ delta, float* __restrict__ g_qkv) {
    __shared__ float s_acc[QA_WAVES][16][S360_WAVE];
    __shared__ double s_stat[QA_WAVES][S360_WAVE];            // per wave: lse of the tile's 32 queries, then their Delta
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const QABlock w = qa_block(a);
    const QAHLane at = qah_lane(a, w, l31, hf);
    int qo, ko, vo;
    qa_head(a, w.hd, qo, ko, vo);
    const int sk = w.ot * QA_T + l31;
    const bool kvalid = sk < a.L;
    const size_t stat = ((size_t)w.bi * a.heads + w.hd) * a.L;
    const double* stats = hf ? delta : lse;
    const QAHFrag k = qah_load(pl.k_rh, pl.k_rl, at.own, 16), v = qah_load(pl.v_rh, pl.v_rl, at.own, 16);
    f32x16 dk, dv;
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[r] = dv[r] = 0.f;
    const int ntiles = (a.L + QA_T - 1) / QA_T;
    QAHFrag q = k, g = k, qt = k, gt = k;
    const double* sl = s_stat[wave];
    const double* sd = s_stat[wave] + QA_T;
    double rs = 0.0;                                          // lse (lanes 0..31) or Delta (32..63) of query l31 of the tile
    if (wave < ntiles) {
        q = qah_load(pl.q_rh, pl.q_rl, at.rows + (size_t)wave * QAH_ROWS_TILE, 16);
        g = qah_load(pl.g_rh, pl.g_rl, at.rows + (size_t)wave * QAH_ROWS_TILE, 16);
        qt = qah_load(pl.q_th, pl.q_tl, at.cols + (size_t)wave * QA_T, 8);
        gt = qah_load(pl.g_th, pl.g_tl, at.cols + (size_t)wave * QA_T, 8);
        if (wave * QA_T + l31 < a.L) rs = stats[stat + wave * QA_T + l31];
    }
    for (int t = wave; t < ntiles; t += QA_WAVES) {
        s_stat[wave][lane] = rs;
        qa_wave_sync();
        QAHFrag qn = q, gn = g, qtn = qt, gtn = gt;
        if (t + QA_WAVES < ntiles) {
            const int tn = t + QA_WAVES;
            qn = qah_load(pl.q_rh, pl.q_rl, at.rows + (size_t)tn * QAH_ROWS_TILE, 16);
            gn = qah_load(pl.g_rh, pl.g_rl, at.rows + (size_t)tn * QAH_ROWS_TILE, 16);
            qtn = qah_load(pl.q_th, pl.q_tl, at.cols + (size_t)tn * QA_T, 8);
            gtn = qah_load(pl.g_th, pl.g_tl, at.cols + (size_t)tn * QA_T, 8);
            rs = tn * QA_T + l31 < a.L ? stats[stat + tn * QA_T + l31] : 0.0;
        }
        const f32x16 s = qah_dot<true>(q, k);                 // S: rows = queries, lane = key; the forward's sums, bit for bit
        const f32x16 dp = qah_dot<true>(g, v);                // dP = dO^T V
        float p[16], ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = mfma_acc_row(r, hf);
            p[r] = (kvalid && t * QA_T + qq < a.L) ? qah_exp((double)s[r] * a.inv_scale - sl[qq]) : 0.f;
            ds[r] = p[r] * (float)((double)dp[r] - sd[qq]);   // dS = P (dP - Delta)
        }
        dv = qah_accumulate(dv, gt, p);                       // g_v^T += dO P
        dk = qah_accumulate(dk, qt, ds);                      // g_k^T += Q dS
        qa_wave_sync();
        q = qn;
        g = gn;
        qt = qtn;
        gt = gtn;
    }
    const size_t ktok = kvalid ? qa_token(a, w.bi, sk, a.W) : 0;
    float* pk = g_qkv + ktok + (size_t)ko * a.T;
    float* pv = g_qkv + ktok + (size_t)vo * a.T;
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        if (part == 1) __syncthreads();                       // wave 0 has read part 0
#pragma unroll
        for (int r = 0; r < 16; ++r) s_acc[wave][r][lane] = part == 0 ? dv[r] : dk[r];
        __syncthreads();
        if (wave == 0 && kvalid) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                double x = 0.0;
#pragma unroll
                for (int u = 0; u < QA_WAVES; ++u) x += (double)s_acc[u][r][lane];
                const size_t c = (size_t)mfma_acc_row(r, hf) * a.T;
                if (part == 0) pv[c] = (float)x;
                else pk[c] = (float)(x * a.inv_scale);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- the entry points, both modes
// The size rules of a call; "high" also asks that Lpad is an int and that both its grids fit.  Fills the size fields of `a`.
static int qa_sizes(int32_t rows, int32_t views, int32_t heads, int32_t ch, int32_t tokens, int32_t order, bool high, QAArgs& a) {
    if (rows < 1 || views < 1 || heads < 1 || ch < 1 || tokens < 1 || (order != 0 && order != 1) || rows % views != 0) return S360_E_BADARG;
    if (ch != QA_CH) return S360_E_UNSUPPORTED;
    const int64_t L = (int64_t)views * tokens, B = rows / views;
    if (L >= (int64_t)1 << 31 || (int64_t)heads * 3 * ch >= (int64_t)1 << 31) return S360_E_BADARG;
    const int64_t grid = B * heads * ((L + QA_T - 1) / QA_T);
    if (grid >= (int64_t)1 << 31 || (high && (L > INT32_MAX - QA_T || !s360_grid_fits(grid)))) return S360_E_BADARG;
    a.B = (int)B; a.views = views; a.heads = heads; a.T = tokens; a.L = (int)L; a.W = heads * 3 * ch;
    a.order = order; a.inv_scale = 1.0 / sqrt((double)ch);
    return S360_OK;
}

// The scratch of a "high" call: the planes in the order q, k, v, g (rows, then transposed; hi, then lo), n = B heads Lpad 32
// elements each.  Forward: rows of q and k, transposed v (12 n bytes: the padded qkv's).  Backward: rows of all four, transposed
// q, k and g (28 n bytes: 1.75 x the padded qkv and g_out).
static size_t qah_layout(const QAArgs& a, bool backward, char* base, QAHPlanes* pl) {
    const size_t n = (size_t)a.B * a.heads * qah_pad(a.L) * QA_CH;
    Bx3Carver c{base};
    QAHPlanes none = {};
    if (pl) *pl = none;
    QAHPlanes* p = pl ? pl : &none;
    c.take(n, &p->q_rh, &p->q_rl);
    c.take(n, &p->k_rh, &p->k_rl);
    if (!backward) {
        c.take(n, &p->v_th, &p->v_tl);
        return c.off;
    }
    c.take(n, &p->v_rh, &p->v_rl);
    c.take(n, &p->g_rh, &p->g_rl);
    c.take(n, &p->q_th, &p->q_tl);
    c.take(n, &p->k_th, &p->k_tl);
    c.take(n, &p->g_th, &p->g_tl);
    return c.off;
}

// What every launch entry starts with, in the order of include/s360.h's refusals: the pointer rule (a tensor, lse and delta too,
// is held to a float's alignment, the planes of a "high" call's scratch to 16 bytes), the sizes, the scratch size.  Completes `a`.
template <bool HIGH, size_t NI, size_t NO>
static int qa_setup(const void* const (&in)[NI], const void* const (&outs)[NO], const void* scratch, size_t scratch_bytes, bool backward,
                    int32_t rows, int32_t views, int32_t heads, int32_t ch, int32_t tokens, int32_t order, QAArgs& a) {
    const void* const opt[] = {scratch};
    if ((HIGH && (!scratch || !s360_aligned(scratch, 16))) || !s360_pointers_ok(in, outs, opt, alignof(float))) return S360_E_BADARG;
    const int rc = qa_sizes(rows, views, heads, ch, tokens, order, HIGH, a);
    if (rc != S360_OK) return rc;
    return HIGH && scratch_bytes < qah_layout(a, backward, nullptr, nullptr) ? S360_E_WORKSPACE : S360_OK;
}

static unsigned qa_grid(const QAArgs& a) { return (unsigned)((int64_t)a.B * a.heads * ((a.L + QA_T - 1) / QA_T)); }

static void qah_split_launch(const QAArgs& a, const float* src, int which, __bf16* rh, __bf16* rl, __bf16* th, __bf16* tl, hipStream_t st) {
    const size_t n = (size_t)a.B * a.heads * qah_pad(a.L) * (QA_CH / 8);        // qa_grid(a) / 2 workgroups
    hipLaunchKernelGGL(k_qah_split, dim3((unsigned)((n + S360_BLOCK - 1) / S360_BLOCK)), dim3(S360_BLOCK), 0, st, a, src, which, rh, rl, th, tl);
}

// s360_qkv_attention_forward (HIGH = false: no scratch) and s360_qkv_attention_high_forward (true)
template <bool HIGH>
static int qa_forward(QAArgs a, int32_t rows, int32_t views, int32_t heads, int32_t ch, int32_t tokens, int32_t order, float* out,
                      double* lse, void* scratch, size_t scratch_bytes, hipStream_t st) {
    const void* const in[] = {a.qkv};
    const void* const outs[] = {out, lse};
    const int rc = qa_setup<HIGH>(in, outs, scratch, scratch_bytes, false, rows, views, heads, ch, tokens, order, a);
    if (rc != S360_OK) return rc;
    if constexpr (HIGH) {
        QAHPlanes pl;
        qah_layout(a, false, static_cast<char*>(scratch), &pl);
        qah_split_launch(a, a.qkv, 0, pl.q_rh, pl.q_rl, nullptr, nullptr, st);
        qah_split_launch(a, a.qkv, 1, pl.k_rh, pl.k_rl, nullptr, nullptr, st);
        qah_split_launch(a, a.qkv, 2, nullptr, nullptr, pl.v_th, pl.v_tl, st);
        S360_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_qah_forward, dim3(qa_grid(a)), dim3(S360_BLOCK), 0, st, a, pl, out, lse);
    } else hipLaunchKernelGGL(k_qa_forward, dim3(qa_grid(a)), dim3(S360_BLOCK), 0, st, a, out, lse);
    return s360_launch_status();
}

// s360_qkv_attention_backward (HIGH = false) and s360_qkv_attention_high_backward; the query-owned pass first: it writes Delta
template <bool HIGH>
static int qa_backward(QAArgs a, const double* lse, const float* g_out, int32_t rows, int32_t views, int32_t heads, int32_t ch,
                       int32_t tokens, int32_t order, double* delta, float* g_qkv, void* scratch, size_t scratch_bytes, hipStream_t st) {
    const void* const in[] = {a.qkv, lse, g_out};
    const void* const outs[] = {delta, g_qkv};
    const int rc = qa_setup<HIGH>(in, outs, scratch, scratch_bytes, true, rows, views, heads, ch, tokens, order, a);
    if (rc != S360_OK) return rc;
    const dim3 grid(qa_grid(a)), block(S360_BLOCK);
    if constexpr (HIGH) {
        QAHPlanes pl;
        qah_layout(a, true, static_cast<char*>(scratch), &pl);
        qah_split_launch(a, a.qkv, 0, pl.q_rh, pl.q_rl, pl.q_th, pl.q_tl, st);
        qah_split_launch(a, a.qkv, 1, pl.k_rh, pl.k_rl, pl.k_th, pl.k_tl, st);
        qah_split_launch(a, a.qkv, 2, pl.v_rh, pl.v_rl, nullptr, nullptr, st);
        qah_split_launch(a, g_out, 3, pl.g_rh, pl.g_rl, pl.g_th, pl.g_tl, st);
        S360_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_qah_backward_q, grid, block, 0, st, a, pl, lse, delta, g_qkv);
        S360_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_qah_backward_kv, grid, block, 0, st, a, pl, lse, delta, g_qkv);
    } else {
        hipLaunchKernelGGL(k_qa_backward_q, grid, block, 0, st, a, lse, g_out, delta, g_qkv);
        S360_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_qa_backward_kv, grid, block, 0, st, a, lse, delta, g_out, g_qkv);
    }
    return s360_launch_status();
}

}  // namespace s360

using namespace s360;

extern "C" int s360_qkv_attention_forward(const float* qkv, int32_t rows, int32_t views, int32_t heads, int32_t ch, int32_t tokens,
                                          int32_t order, float* out, double* lse, void* stream) {
    return qa_forward<false>({qkv}, rows, views, heads, ch, tokens, order, out, lse, nullptr, 0, (hipStream_t)stream);
}

extern "C" int s360_qkv_attention_backward(const float* qkv, const double* lse, const float* g_out, int32_t rows, int32_t views,
                                           int32_t heads, int32_t ch, int32_t tokens, int32_t order, double* delta, float* g_qkv,
                                           void* stream) {
    return qa_backward<false>({qkv}, lse, g_out, rows, views, heads, ch, tokens, order, delta, g_qkv, nullptr, 0, (hipStream_t)stream);
}

extern "C" size_t s360_qkv_attention_high_scratch_bytes(int32_t rows, int32_t views, int32_t heads, int32_t ch, int32_t tokens,
                                                        int32_t backward) {
    QAArgs a;
    return qa_sizes(rows, views, heads, ch, tokens, 0, true, a) != S360_OK ? 0 : qah_layout(a, backward != 0, nullptr, nullptr);
}

extern "C" int s360_qkv_attention_high_forward(const float* qkv, int32_t rows, int32_t views, int32_t heads, int32_t ch, int32_t tokens,
                                               int32_t order, float* out, double* lse, void* scratch, size_t scratch_bytes,
                                               void* stream) {
    return qa_forward<true>({qkv}, rows, views, heads, ch, tokens, order, out, lse, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int s360_qkv_attention_high_backward(const float* qkv, const double* lse, const float* g_out, int32_t rows, int32_t views,
                                                int32_t heads, int32_t ch, int32_t tokens, int32_t order, double* delta, float* g_qkv,
                                                void* scratch, size_t scratch_bytes, void* stream) {
    return qa_backward<true>({qkv}, lse, g_out, rows, views, heads, ch, tokens, order, delta, g_qkv, scratch, scratch_bytes, (hipStream_t)stream);
}
