// s360_window_attention.hip — the multi-view transformer's single-head (shifted-)window attention, forward and backward (the
// reference's single_head_split_window_attention and single_head_full_attention,
// src/model/encoder/backbone/multiview_transformer.py:8-16, :60-210).  gfx950 only.
//
//   tokens   q[B, L, C], k, v[B, M, L, C], L = H W in (y, x) order; K = num_splits, wh = H / K, ww = W / K, Lw = wh ww, Lk = Lw M
//   window   (wy, wx) holds the ROLLED positions ry = wy wh + i, rx = wx ww + j; its token p = i ww + j is the original token
//            ((ry + sh) mod H) W + (rx + sw) mod W, sh = wh / 2, sw = ww / 2 with shift, else 0 (roll by -shift, split); the
//            output row goes back to that token (merge, roll back).  Key j of the window is token p = j / M of partner view
//            u = j mod M.
//   score    float32((q . k) / sqrt(C)) + mask, q . k summed in float64 over float32 chunks of 8 channels (wa_dot); with shift,
//            mask = 0 where region(query) == region(key), else -100.0 (finite,
//            as the reference's), region(ry, rx) = 3 r(ry, H, wh, sh) + r(rx, W, ww, sw), r(i, n, win, s) = [i >= n - win] +
//            [i >= n - s]; the key's region is that of window token j mod Lw (rule 0, the reference's tiled mask) or j / M (rule 1)
//   out      softmax over the window's keys, times v; lse = max + log(sum) per query, float64
//
// Every product runs on v_mfma_f32_32x32x2_f32 (exact f32 fma chains; the score and dP chains are 8 channels long and are
// added in float64, wa_dot).  A wave owns 32 rows ("owner": queries in the forward
// and the g_q pass, keys in the g_k / g_v pass) and walks the other side in tiles of 32; a workgroup is four waves on four
// consecutive owner tiles of ONE window, so its waves walk the same tiles and share their (row, region) table in LDS.
// Orientation: the score tile is computed with the WALKED index on the accumulator's rows (registers) and the owner on the
// lanes — forward S^T = K Q^T — so that (a) softmax statistics, lse and Delta of the owner are per lane, one exchange with
// lane ^ 32 completes a row reduction, and (b) the tile is, register by register, the B operand of the second product, which
// sums over the walked index: O^T = V^T P^T with A = one value of V per lane.  No lane movement, no LDS for the tile.
// The contraction order over channels is free (it only has to match between the two operands): lane half h of a row holds
// channels [h C/2, (h+1) C/2), read with dwordx4 loads (one per chunk); output channel slot i of block cb is channel (C/32) i + cb, so the 16
// rows a lane holds of an output tile are C/32 consecutive channels each: vector loads of V and vector stores of the result.
// Gathered rows (roll, split) are read straight from [B, L, C]; ragged last tiles are masked by index.
// No atomics: each output row is written by one wave.  Backward: P = exp(score - lse) recomputed (float64 difference, float32
// exp), dS = P (dP - Delta), Delta = sum_k P dP (float64 sum) from a first sweep of the query-owned pass.
#include "s360_device.h"
#include "s360_bf16x3.h"

#include <type_traits>

namespace s360 {

constexpr int WA_T = 32;                                      // rows of an MFMA tile
constexpr int WA_WAVES = S360_BLOCK / S360_WAVE;              // owner tiles of a workgroup
constexpr int WA_ROWS = WA_T * WA_WAVES;

struct WAArgs {
    const float* q;
    const float* k;
    const float* v;
    int B, M, H, W, C, K, wh, ww, sh, sw, Lw, Lk, L;
    int shift, aligned;
    float scale;                                              // float32(sqrt(C)): divides g_q and g_k
    double inv_scale;                                         // 1 / sqrt(C): multiplies the float64 score sums
};

// original token and mask region of window token p of window (wy, wx)
__device__ __forceinline__ void wa_token(const WAArgs& a, int wy, int wx, int p, int& tok, int& region) {
    const int i = p / a.ww, j = p - i * a.ww;
    const int ry = wy * a.wh + i, rx = wx * a.ww + j;
    int oy = ry + a.sh, ox = rx + a.sw;
    if (oy >= a.H) oy -= a.H;
    if (ox >= a.W) ox -= a.W;
    tok = oy * a.W + ox;
    region = 3 * ((ry >= a.H - a.wh) + (ry >= a.H - a.sh)) + (rx >= a.W - a.ww) + (rx >= a.W - a.sw);
}

// row of k / v (in units of C floats) and mask region of window key j < Lk of batch element b
__device__ __forceinline__ void wa_key(const WAArgs& a, int b, int wy, int wx, int j, int& row, int& region) {
    const int p = j / a.M, u = j - p * a.M;
    int tok, reg;
    wa_token(a, wy, wx, p, tok, reg);
    row = (b * a.M + u) * a.L + tok;
    region = reg;
    if (!a.aligned && a.M > 1) {
        int t2;
        wa_token(a, wy, wx, j % a.Lw, t2, region);
    }
}

// N4 dwordx4 loads of 4 N4 consecutive floats (p 16-byte aligned), or zeros for p == null
template <int N4>
__device__ __forceinline__ void wa_load(const float* p, float* x) {
#pragma unroll
    for (int i = 0; i < N4; ++i) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p) t = reinterpret_cast<const float4*>(p)[i];
        x[4 * i] = t.x; x[4 * i + 1] = t.y; x[4 * i + 2] = t.z; x[4 * i + 3] = t.w;
    }
}

// NCB consecutive floats (p aligned to NCB floats for NCB 2 and 4), or zeros
template <int NCB>
__device__ __forceinline__ void wa_load_c(const float* p, float* x) {
#pragma unroll
    for (int i = 0; i < NCB; ++i) x[i] = 0.f;
    if (!p) return;
    if constexpr (NCB == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else if constexpr (NCB == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        x[0] = t.x; x[1] = t.y;
    } else {
#pragma unroll
        for (int i = 0; i < NCB; ++i) x[i] = p[i];
    }
}

template <int NCB>
__device__ __forceinline__ void wa_store_c(float* p, const float* x) {
    if constexpr (NCB == 4) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    else if constexpr (NCB == 2) *reinterpret_cast<float2*>(p) = make_float2(x[0], x[1]);
    else {
#pragma unroll
        for (int i = 0; i < NCB; ++i) p[i] = x[i];
    }
}

// tile = float32(mul * sum over the lane's HC channels of A-row x B-row) (the two halves of a wave cover all C channels).  The
// sum runs in chunks of WA_CHUNK MFMA steps (2 WA_CHUNK channels): a chunk is one float32 fma chain from zero, whose partial
// sums stay small, and the chunks are added in FLOAT64; the result is rounded once.  One chain over all C channels rounds at
// the full size of the sum at every step; in its largest elements it misses the accuracy rule of the tests, and so did four
// float32 chains added pairwise.  The forward and both backward passes form every score and every dP through this one
// arithmetic (wa_dot, wa_dot_mem), so the recomputed tiles are the forward's bit for bit.
constexpr int WA_CHUNK = 4;
__device__ __forceinline__ float4 wa_ld4(const float* p, int chunk) {
    return p ? reinterpret_cast<const float4*>(p)[chunk] : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ f32x16 wa_round(const double* sum, double mul) {
    f32x16 out;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r] = (float)(sum[r] * mul);
    return out;
}

__device__ __forceinline__ f32x16 wa_chunk(const float4& x, const float4& y, float z) {
    f32x16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = z;
    t = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, y.x, t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, y.y, t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, y.z, t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, y.w, t, 0, 0, 0);
    return t;
}

// The forward's form: the walked row `arow` (null: zeros) is read chunk by chunk, the owner's row `b` is held in HC registers.
// Left to itself the compiler issues the MFMAs of all chunks first and keeps 16 tiles alive (256 accumulator registers and
// 0.5 KB of scratch per lane, measured); so each chunk's zero tile passes an empty asm statement that depends on the sums as
// they stand (chunks up to c - 2 added): at most three tiles are live, and the float64 adds of chunk c - 1 run under the
// MFMAs of chunk c.
template <int HC>
__device__ __forceinline__ f32x16 wa_dot(const float* arow, const float* b, double mul) {
    static_assert(WA_CHUNK == 4 && HC % WA_CHUNK == 0, "a chunk is one dwordx4 of a row");
    double sum[16];
    f32x16 prev;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = 0.0, prev[r] = 0.f;
#pragma unroll
    for (int c = 0; c < HC / WA_CHUNK; ++c) {
        float z = 0.f;
        asm volatile("" : "+v"(z) : "v"(sum[15]));
        const f32x16 t = wa_chunk(wa_ld4(arow, c), make_float4(b[4 * c], b[4 * c + 1], b[4 * c + 2], b[4 * c + 3]), z);
        if (c > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sum[r] += (double)prev[r];
        }
        prev = t;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] += (double)prev[r];
    return wa_round(sum, mul);
}

// The backward passes' form: both rows are read from memory chunk by chunk (either may be null: zeros) — their two products,
// the float64 sums and two or four output tiles do not fit the 256 VALU-visible registers with the owner's rows resident
// (measured: 0.8 to 1.5 KB of scratch per lane); the owner's rows are the same every tile and stay in cache.  A real loop,
// not an unrolled one, with the loads three chunks (768 MFMA cycles) in front of their use in rotating registers.
template <int HC>
__device__ __forceinline__ f32x16 wa_dot_mem(const float* arow, const float* brow, double mul) {
    constexpr int NCH = HC / WA_CHUNK;
    static_assert(WA_CHUNK == 4 && HC % WA_CHUNK == 0 && NCH >= 3, "a chunk is one dwordx4 of a row");
    double sum[16];
    f32x16 prev;
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = 0.0, prev[r] = 0.f;
    float4 a0 = wa_ld4(arow, 0), b0 = wa_ld4(brow, 0), a1 = wa_ld4(arow, 1), b1 = wa_ld4(brow, 1), a2 = wa_ld4(arow, 2), b2 = wa_ld4(brow, 2);
#pragma unroll 1
    for (int c = 0; c < NCH; ++c) {
        const bool more = c + 3 < NCH;
        const float4 a3 = wa_ld4(more ? arow : nullptr, c + 3), b3 = wa_ld4(more ? brow : nullptr, c + 3);
        const f32x16 t = wa_chunk(a0, b0, 0.f);
#pragma unroll
        for (int r = 0; r < 16; ++r) sum[r] += (double)prev[r];      // chunk c - 1 (zeros at c = 0), under the MFMAs of chunk c
        prev = t;
        a0 = a1; b0 = b1; a1 = a2; b1 = b2; a2 = a3; b2 = b3;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] += (double)prev[r];
    return wa_round(sum, mul);
}

// block decomposition shared by the three kernels: owner block ob of window (wy, wx) of batch element b
struct WABlock { int ob, b, wy, wx; };
__device__ __forceinline__ WABlock wa_block(const WAArgs& a, int owner_rows) {
    const int oblocks = (owner_rows + WA_ROWS - 1) / WA_ROWS;
    int blk = blockIdx.x;
    WABlock w;
    w.ob = blk % oblocks; blk /= oblocks;
    const int win = blk % (a.K * a.K);
    w.b = blk / (a.K * a.K);
    w.wy = win / a.K; w.wx = win - w.wy * a.K;
    return w;
}

// Forward.  Owner: queries.  Walks the window's key tiles with a running maximum (float32: it is one of the scores) and a
// running sum (float64).
template <int NCB>
__global__ __launch_bounds__(S360_BLOCK) void k_wa_forward(WAArgs a, float* __restrict__ out, double* __restrict__ lse) {
    constexpr int HC = 16 * NCB;
    __shared__ int s_row[2][WA_T], s_reg[2][WA_T];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const WABlock w = wa_block(a, a.Lw);
    const int qp = w.ob * WA_ROWS + wave * WA_T + l31;
    const bool qvalid = qp < a.Lw;
    int qtok = 0, qreg = 0;
    if (qvalid) wa_token(a, w.wy, w.wx, qp, qtok, qreg);
    const size_t qrow = (size_t)w.b * a.L + qtok;
    float qB[HC];
    wa_load<HC / 4>(qvalid ? a.q + qrow * a.C + hf * HC : nullptr, qB);
    f32x16 o[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[cb][r] = 0.f;
    float m = -INFINITY;
    double lsum = 0.0;
    const int ntiles = (a.Lk + WA_T - 1) / WA_T;
    for (int t = 0; t < ntiles; ++t) {
        if (tid < WA_T) {
            const int j = t * WA_T + tid;
            int row = -1, reg = 0;
            if (j < a.Lk) wa_key(a, w.b, w.wy, w.wx, j, row, reg);
            s_row[t & 1][tid] = row;
            s_reg[t & 1][tid] = reg;
        }
        __syncthreads();                                      // one barrier per tile: the table is double-buffered
        const int* srow = s_row[t & 1];
        const int* sreg = s_reg[t & 1];
        const int kr31 = srow[l31];
        const f32x16 s = wa_dot<HC>(kr31 >= 0 ? a.k + (size_t)kr31 * a.C + hf * HC : nullptr, qB, a.inv_scale);  // S^T / sqrt(C): rows = keys, lane = query
        float p[16];
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kk = mfma_acc_row(r, hf);
            float x = s[r];
            if (a.shift && sreg[kk] != qreg) x += -100.0f;
            if (srow[kk] < 0) x = -INFINITY;
            p[r] = x;
            tmax = fmaxf(tmax, x);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mnew = fmaxf(m, tmax);                    // finite: key 0 of every tile exists
        const float alpha = expf(m - mnew);                   // 0 at the first tile
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
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[cb][r] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {                        // O^T += V^T P^T, two keys (one per lane half) a step
            const int kr = srow[mfma_acc_row(r, hf)];
            float vv[NCB];
            wa_load_c<NCB>(kr >= 0 ? a.v + (size_t)kr * a.C + NCB * l31 : nullptr, vv);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) o[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv[cb], p[r], o[cb], 0, 0, 0);
        }
    }
    if (!qvalid) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float x[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) x[cb] = (float)((double)o[cb][r] / lsum);
        wa_store_c<NCB>(out + qrow * a.C + NCB * mfma_acc_row(r, hf), x);
    }
    if (hf == 0) lse[qrow] = (double)m + log(lsum);
}

// Backward, Delta and g_q.  Owner: queries (as the forward).  First sweep over the key tiles: Delta = sum_k P dP per query, float64,
// written to delta[] for the key-owned pass; second sweep (WANT_Q): dS^T = P (dP - Delta), g_q^T += K^T dS^T.  Delta is formed
// from the very dP values dS subtracts it from (the same fma chains in both sweeps and in the key-owned pass), as torch's
// softmax backward forms it: at a row with few effective keys the rounding of dP then cancels in dP - Delta.  rowsum(g_out out),
// the cheaper form, does not have that property and misses the accuracy rule of the tests at such rows.
template <int NCB, bool WANT_Q>
__global__ __launch_bounds__(S360_BLOCK) void k_wa_backward_q(WAArgs a, const double* __restrict__ lse, const float* __restrict__ g_out,
                                                              double* __restrict__ delta, float* __restrict__ g_q) {
    constexpr int HC = 16 * NCB;
    __shared__ int s_row[2][WA_T], s_reg[2][WA_T];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const WABlock w = wa_block(a, a.Lw);
    const int qp = w.ob * WA_ROWS + wave * WA_T + l31;
    const bool qvalid = qp < a.Lw;
    int qtok = 0, qreg = 0;
    if (qvalid) wa_token(a, w.wy, w.wx, qp, qtok, qreg);
    const size_t qrow = (size_t)w.b * a.L + qtok;
    const float* qB = qvalid ? a.q + qrow * a.C + hf * HC : nullptr;            // the owner's two rows (read per chunk by wa_dot_mem)
    const float* gB = qvalid ? g_out + qrow * a.C + hf * HC : nullptr;
    const double lq = qvalid ? lse[qrow] : 0.0;
    double dsum = 0.0;
    f32x16 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
    const int ntiles = (a.Lk + WA_T - 1) / WA_T;
    int it = 0;                                               // parity of the double-buffered table, across both sweeps
    // The two sweeps are two loops in the code (unrolled: `sweep` is a constant in each).  As one loop over a run-time `sweep`
    // the compiler kept both bodies in one tile loop and moved the g_q accumulator between two register tiles after every
    // MFMA; at C = 32 it then read the tile back at the head of the next key tile 7 wait states after the last MFMA of the
    // previous one (a 16-pass MFMA needs 18), and register 15 — channels 27 and 31 of g_q — came back stale whenever a window
    // had more than one key tile (tests/test_gpu_window_attention_float64.py, cases "edge" and "m5").
#pragma unroll
    for (int sweep = 0; sweep < (WANT_Q ? 2 : 1); ++sweep) {
        for (int t = 0; t < ntiles; ++t, ++it) {
            if (tid < WA_T) {
                const int j = t * WA_T + tid;
                int row = -1, reg = 0;
                if (j < a.Lk) wa_key(a, w.b, w.wy, w.wx, j, row, reg);
                s_row[it & 1][tid] = row;
                s_reg[it & 1][tid] = reg;
            }
            __syncthreads();
            const int* srow = s_row[it & 1];
            const int* sreg = s_reg[it & 1];
            f32x16 s, dp;
            {
                const int kr = srow[l31];
                s = wa_dot_mem<HC>(kr >= 0 ? a.k + (size_t)kr * a.C + hf * HC : nullptr, qB, a.inv_scale);      // S^T / sqrt(C)
                dp = wa_dot_mem<HC>(kr >= 0 ? a.v + (size_t)kr * a.C + hf * HC : nullptr, gB, 1.0);             // dP^T = V dO^T
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kk = mfma_acc_row(r, hf);
                const int kr = srow[kk];
                float x = s[r];
                if (a.shift && sreg[kk] != qreg) x += -100.0f;
                const float p = (kr >= 0 && qvalid) ? expf((float)((double)x - lq)) : 0.f;
                if (sweep == 0) {
                    dsum += (double)p * (double)dp[r];
                } else {
                    const float ds = p * (float)((double)dp[r] - dsum);
                    float kv[NCB];
                    wa_load_c<NCB>(kr >= 0 ? a.k + (size_t)kr * a.C + NCB * l31 : nullptr, kv);
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[cb], ds, acc[cb], 0, 0, 0);
                }
            }
        }
        if (sweep == 0) {
            dsum += __shfl_xor(dsum, 32);
            if (qvalid && hf == 0) delta[qrow] = dsum;
        }
    }
    if (!qvalid || !WANT_Q) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float x[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) x[cb] = acc[cb][r] / a.scale;
        wa_store_c<NCB>(g_q + qrow * a.C + NCB * mfma_acc_row(r, hf), x);
    }
}

// Backward, g_k and / or g_v.  Owner: keys; walks the window's query tiles.  S = Q K^T (rows = queries, lane = key),
// g_v^T += dO^T P, g_k^T += Q^T dS.
template <int NCB, bool WANT_K, bool WANT_V>
__global__ __launch_bounds__(S360_BLOCK) void k_wa_backward_kv(WAArgs a, const double* __restrict__ lse, const double* __restrict__ delta,
                                                               const float* __restrict__ g_out, float* __restrict__ g_k,
                                                               float* __restrict__ g_v) {
    constexpr int HC = 16 * NCB;
    __shared__ int s_row[2][WA_T], s_reg[2][WA_T];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const WABlock w = wa_block(a, a.Lk);
    const int kj = w.ob * WA_ROWS + wave * WA_T + l31;
    const bool kvalid = kj < a.Lk;
    int krow_i = 0, kreg = 0;
    if (kvalid) wa_key(a, w.b, w.wy, w.wx, kj, krow_i, kreg);
    const size_t krow = (size_t)krow_i;
    const float* kB = kvalid ? a.k + krow * a.C + hf * HC : nullptr;             // the owner's two rows (read per chunk by wa_dot_mem)
    const float* vB = kvalid ? a.v + krow * a.C + hf * HC : nullptr;
    f32x16 dk[NCB], dv[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[cb][r] = dv[cb][r] = 0.f;
    const int ntiles = (a.Lw + WA_T - 1) / WA_T;
    for (int t = 0; t < ntiles; ++t) {
        if (tid < WA_T) {
            const int p = t * WA_T + tid;
            int row = -1, reg = 0;
            if (p < a.Lw) {
                int tok;
                wa_token(a, w.wy, w.wx, p, tok, reg);
                row = w.b * a.L + tok;
            }
            s_row[t & 1][tid] = row;
            s_reg[t & 1][tid] = reg;
        }
        __syncthreads();
        const int* srow = s_row[t & 1];
        const int* sreg = s_reg[t & 1];
        f32x16 s, dp;
        {
            const int qr = srow[l31];
            s = wa_dot_mem<HC>(qr >= 0 ? a.q + (size_t)qr * a.C + hf * HC : nullptr, kB, a.inv_scale);              // S / sqrt(C): rows = queries, lane = key; the forward's chain, bit for bit
            if constexpr (WANT_K) {
                dp = wa_dot_mem<HC>(qr >= 0 ? g_out + (size_t)qr * a.C + hf * HC : nullptr, vB, 1.0);                 // dP = dO V^T
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = mfma_acc_row(r, hf);
            const int qr = srow[qq];
            float x = s[r];
            if (a.shift && sreg[qq] != kreg) x += -100.0f;
            float p = 0.f;
            if (qr >= 0 && kvalid) p = expf((float)((double)x - lse[qr]));
            if constexpr (WANT_V) {
                float gv[NCB];
                wa_load_c<NCB>(qr >= 0 ? g_out + (size_t)qr * a.C + NCB * l31 : nullptr, gv);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) dv[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[cb], p, dv[cb], 0, 0, 0);
            }
            if constexpr (WANT_K) {
                const float ds = p * (float)((double)dp[r] - (qr >= 0 ? delta[qr] : 0.0));
                float qv[NCB];
                wa_load_c<NCB>(qr >= 0 ? a.q + (size_t)qr * a.C + NCB * l31 : nullptr, qv);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) dk[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[cb], ds, dk[cb], 0, 0, 0);
            }
        }
    }
    if (!kvalid) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float x[NCB];
        if constexpr (WANT_V) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) x[cb] = dv[cb][r];
            wa_store_c<NCB>(g_v + krow * a.C + NCB * mfma_acc_row(r, hf), x);
        }
        if constexpr (WANT_K) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) x[cb] = dk[cb][r] / a.scale;
            wa_store_c<NCB>(g_k + krow * a.C + NCB * mfma_acc_row(r, hf), x);
        }
    }
}

// ---------------------------------------------------------------------------------------------- the "high" mode (bf16 x 3)
// The same function with every product as a bf16x3 product (s360_bf16x3.h: the split, the three terms and their order, the
// B-operand register rule), accumulated by the MFMA over all channels.  Roll, split and merge, the mask, the scaling, the
// softmax with its running maximum, lse and Delta are those of the kernels above, and so is the orientation: the walked index
// on the accumulator's rows, the owner on the lanes, so the P or dS tile is the B operand of the second product register by
// register.
// A pre-pass (k_wah_split, one launch per operand) splits once per call and writes bf16 planes IN WINDOW ORDER into the caller's
// scratch: "rows" [B K^2 rows, C] for the first products (a lane reads 8 consecutive channels of its row, 16 bytes), and
// "transposed" [B K^2, C, pad4(rows)] for the second products (a lane reads 2 x 4 consecutive walked indices of its channel;
// rows are padded to a multiple of 4 with zeros so that these 8-byte reads are aligned and a group is inside or outside).
// The loops then have no gathered addressing and no split of an input.  Output channel of accumulator block cb, row r is
// 32 cb + r: registers 4 g .. 4 g + 3 of a lane are channels 32 cb + 8 g + 4 hf + (0 .. 3), one 16-byte store.
// The terms of a score are in (q, k) order — (qh, kh), (ql, kh), (qh, kl) — and those of dP in (g, v) order, whichever side is
// walked, so the backward's recomputed tiles are the forward's bit for bit.

struct WAHPlanes {                                            // hi and lo planes of the operands; null where a call has none
    __bf16 *q_rh, *q_rl, *q_th, *q_tl;
    __bf16 *k_rh, *k_rl, *k_th, *k_tl;
    __bf16 *v_rh, *v_rl, *v_th, *v_tl;
    __bf16 *g_rh, *g_rl, *g_th, *g_tl;
};

__host__ __device__ __forceinline__ int wah_pad4(int n) { return (n + 3) & ~3; }

// the lane's 8 channels of k-step s of a row (p: the row at channel 8 hf; null: zeros)
__device__ __forceinline__ bf16x8 wah_frag(const __bf16* p, int s) { return bx3_ld8_or_zero(p ? p + 16 * s : nullptr); }

// tile = sum over all C channels of walked row x owner row, NS = C / 16 k-steps, the walked fragments as A, the owner's as B;
// the pointers are the lane's row at channel 8 hf (null: zeros).  wah_dot: the owner's fragments are held in registers (the
// forward); wah_dot_mem: read per step (the backward passes, whose two owners and two or more output tiles would not fit
// beside them; the reads stay in cache).
template <int NS, bool SWAP>
__device__ __forceinline__ f32x16 wah_dot(const __bf16* wh, const __bf16* wl, const bf16x8* oh, const bf16x8* ol) {
    f32x16 acc = bx3_zero();
#pragma unroll
    for (int s = 0; s < NS; ++s) acc = bx3_mfma3<SWAP>(wah_frag(wh, s), wah_frag(wl, s), oh[s], ol[s], acc);
    return acc;
}

template <int NS, bool SWAP>
__device__ __forceinline__ f32x16 wah_dot_mem(const __bf16* wh, const __bf16* wl, const __bf16* oh, const __bf16* ol) {
    f32x16 acc = bx3_zero();
#pragma unroll
    for (int s = 0; s < NS; ++s) acc = bx3_mfma3<SWAP>(wah_frag(wh, s), wah_frag(wl, s), wah_frag(oh, s), wah_frag(ol, s), acc);
    return acc;
}

// acc[cb]^T += T^T x for the NCB channel blocks: x[16] is the lane's column of a 32 x 32 tile whose rows are the walked indices
// first - 4 hf .. + 31 (split here, register by register); th / tl: the lane's channel row (channel l31 of block 0) of the
// window's transposed planes, block cb another 32 lpad elements on; `first` = the tile's first walked index + 4 hf.
template <int NCB>
__device__ __forceinline__ void wah_accumulate(f32x16* acc, const __bf16* th, const __bf16* tl, int first, int lpad, const float* x) {
    bf16x8 xh[2], xl[2];
    bx3_split_tile(x, xh, xl);
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const size_t off = (size_t)cb * 32 * lpad;
            const bf16x8 ah = bx3_ld44(th + off, first + 16 * s, lpad), al = bx3_ld44(tl + off, first + 16 * s, lpad);
            // bx3_mfma3<false>(ah, al, xh[s], xl[s], acc[cb]), written out: behind any function boundary the register
            // allocation of k_wah_forward<1> exchanges two VGPRs (nothing else moves), and its code is held as it was
            acc[cb] = bx3_mfma(ah, xh[s], acc[cb]);
            acc[cb] = bx3_mfma(ah, xl[s], acc[cb]);
            acc[cb] = bx3_mfma(al, xh[s], acc[cb]);
        }
}

// registers 4 g .. 4 g + 3 of the NCB tiles, times mul, to channels 32 cb + 8 g + 4 hf + (0 .. 3) of row p
template <int NCB, typename F>
__device__ __forceinline__ void wah_store(float* p, const f32x16* acc, int hf, F f) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(p + 32 * cb + 8 * g + 4 * hf) =
                make_float4(f(acc[cb][4 * g]), f(acc[cb][4 * g + 1]), f(acc[cb][4 * g + 2]), f(acc[cb][4 * g + 3]));
}

// The pre-pass: one operand (queries' side: q, g_out; keys' side: k, v) into its planes.  Thread i takes 8 channels of one
// window row, the row index fastest (the transposed plane's 2-byte stores of a wave are then consecutive); rows from `rows` to
// pad4(rows) exist in the transposed plane only and are zeros.  rh / rl or th / tl may be null.
__global__ __launch_bounds__(S360_BLOCK) void k_wah_split(WAArgs a, const float* __restrict__ src, int keys, __bf16* __restrict__ rh,
                                                          __bf16* __restrict__ rl, __bf16* __restrict__ th, __bf16* __restrict__ tl) {
    const int rows = keys ? a.Lk : a.Lw, lpad = wah_pad4(rows), cgs = a.C / 8;
    const size_t i = (size_t)blockIdx.x * S360_BLOCK + threadIdx.x;
    const size_t per_win = (size_t)lpad * cgs, nwin = (size_t)a.B * a.K * a.K;
    if (i >= nwin * per_win) return;
    const size_t win = i / per_win;
    const int rem = (int)(i - win * per_win), cg = rem / lpad, p = rem - cg * lpad;
    const int b = (int)(win / (a.K * a.K)), wi = (int)(win - (size_t)b * a.K * a.K), wy = wi / a.K, wx = wi - wy * a.K;
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = 0.f;
    if (p < rows) {
        int row, reg;
        if (keys) {
            wa_key(a, b, wy, wx, p, row, reg);
        } else {
            wa_token(a, wy, wx, p, row, reg);
            row += b * a.L;
        }
        wa_load<2>(src + (size_t)row * a.C + 8 * cg, x);
    }
    bf16x8 hi, lo;
    bx3_split8(x, hi, lo);
    if (rh && p < rows) bx3_st8(rh, rl, (win * rows + p) * a.C + 8 * cg, hi, lo);
    if (th) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const size_t o = (win * a.C + 8 * cg + j) * lpad + p;
            th[o] = hi[j];
            tl[o] = lo[j];
        }
    }
}

// Forward.  Owner: queries, their split rows in registers; as k_wa_forward otherwise.
template <int NCB>
__global__ __launch_bounds__(S360_BLOCK) void k_wah_forward(WAArgs a, WAHPlanes pl, float* __restrict__ out, double* __restrict__ lse) {
    constexpr int NS = 2 * NCB;
    __shared__ int s_reg[2][WA_T];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const WABlock w = wa_block(a, a.Lw);
    const size_t win = ((size_t)w.b * a.K + w.wy) * a.K + w.wx;
    const int qp = w.ob * WA_ROWS + wave * WA_T + l31;
    const bool qvalid = qp < a.Lw;
    int qtok = 0, qreg = 0;
    if (qvalid) wa_token(a, w.wy, w.wx, qp, qtok, qreg);
    const size_t qrow = (size_t)w.b * a.L + qtok;
    bf16x8 qh[NS], ql[NS];
    {
        const size_t o = (win * a.Lw + qp) * a.C + 8 * hf;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            qh[s] = bx3_ld8_or_zero(qvalid ? pl.q_rh + o + 16 * s : nullptr);
            ql[s] = bx3_ld8_or_zero(qvalid ? pl.q_rl + o + 16 * s : nullptr);
        }
    }
    const int lkpad = wah_pad4(a.Lk);
    const __bf16* vth = pl.v_th + (win * a.C + l31) * lkpad;
    const __bf16* vtl = pl.v_tl + (win * a.C + l31) * lkpad;
    f32x16 o[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[cb][r] = 0.f;
    float m = -INFINITY;
    double lsum = 0.0;
    const int ntiles = (a.Lk + WA_T - 1) / WA_T;
    for (int t = 0; t < ntiles; ++t) {
        if (tid < WA_T) {
            const int j = t * WA_T + tid;
            int row = -1, reg = 0;
            if (j < a.Lk) wa_key(a, w.b, w.wy, w.wx, j, row, reg);
            s_reg[t & 1][tid] = reg;
        }
        __syncthreads();                                      // one barrier per tile: the table is double-buffered
        const int* sreg = s_reg[t & 1];
        const int j31 = t * WA_T + l31;
        const size_t ko = (win * a.Lk + j31) * a.C + 8 * hf;
        const f32x16 s = wah_dot<NS, false>(j31 < a.Lk ? pl.k_rh + ko : nullptr, j31 < a.Lk ? pl.k_rl + ko : nullptr, qh, ql);  // S^T: rows = keys, lane = query
        float p[16];
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kk = mfma_acc_row(r, hf);
            float x = (float)((double)s[r] * a.inv_scale);
            if (a.shift && sreg[kk] != qreg) x += -100.0f;
            if (t * WA_T + kk >= a.Lk) x = -INFINITY;
            p[r] = x;
            tmax = fmaxf(tmax, x);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mnew = fmaxf(m, tmax);                    // finite: key 0 of every tile exists
        const float alpha = expf(m - mnew);                   // 0 at the first tile
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
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[cb][r] *= alpha;
        wah_accumulate<NCB>(o, vth, vtl, t * WA_T + 4 * hf, lkpad, p);                      // O^T += V^T P^T
    }
    if (!qvalid) return;
    wah_store<NCB>(out + qrow * a.C, o, hf, [lsum](float x) { return (float)((double)x / lsum); });
    if (hf == 0) lse[qrow] = (double)m + log(lsum);
}

// Backward, Delta and g_q.  Owner: queries; two sweeps, as k_wa_backward_q.
template <int NCB, bool WANT_Q>
__global__ __launch_bounds__(S360_BLOCK) void k_wah_backward_q(WAArgs a, WAHPlanes pl, const double* __restrict__ lse,
                                                               double* __restrict__ delta, float* __restrict__ g_q) {
    constexpr int NS = 2 * NCB;
    __shared__ int s_reg[2][WA_T];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const WABlock w = wa_block(a, a.Lw);
    const size_t win = ((size_t)w.b * a.K + w.wy) * a.K + w.wx;
    const int qp = w.ob * WA_ROWS + wave * WA_T + l31;
    const bool qvalid = qp < a.Lw;
    int qtok = 0, qreg = 0;
    if (qvalid) wa_token(a, w.wy, w.wx, qp, qtok, qreg);
    const size_t qrow = (size_t)w.b * a.L + qtok;
    const size_t oo = (win * a.Lw + qp) * a.C + 8 * hf;
    const __bf16* oqh = qvalid ? pl.q_rh + oo : nullptr;                        // the owner's rows (read per step by wah_dot_mem)
    const __bf16* oql = qvalid ? pl.q_rl + oo : nullptr;
    const __bf16* ogh = qvalid ? pl.g_rh + oo : nullptr;
    const __bf16* ogl = qvalid ? pl.g_rl + oo : nullptr;
    const int lkpad = wah_pad4(a.Lk);
    const __bf16* kth = WANT_Q ? pl.k_th + (win * a.C + l31) * lkpad : nullptr;
    const __bf16* ktl = WANT_Q ? pl.k_tl + (win * a.C + l31) * lkpad : nullptr;
    const double lq = qvalid ? lse[qrow] : 0.0;
    double dsum = 0.0;
    f32x16 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
    const int ntiles = (a.Lk + WA_T - 1) / WA_T;
    int it = 0;                                               // parity of the double-buffered table, across both sweeps
#pragma unroll
    for (int sweep = 0; sweep < (WANT_Q ? 2 : 1); ++sweep) {  // two loops in the code, as in k_wa_backward_q
        for (int t = 0; t < ntiles; ++t, ++it) {
            if (tid < WA_T) {
                const int j = t * WA_T + tid;
                int row = -1, reg = 0;
                if (j < a.Lk) wa_key(a, w.b, w.wy, w.wx, j, row, reg);
                s_reg[it & 1][tid] = reg;
            }
            __syncthreads();
            const int* sreg = s_reg[it & 1];
            const int j31 = t * WA_T + l31;
            const bool jv = j31 < a.Lk;
            const size_t ko = (win * a.Lk + j31) * a.C + 8 * hf;
            const f32x16 s = wah_dot_mem<NS, false>(jv ? pl.k_rh + ko : nullptr, jv ? pl.k_rl + ko : nullptr, oqh, oql);   // S^T
            const f32x16 dp = wah_dot_mem<NS, false>(jv ? pl.v_rh + ko : nullptr, jv ? pl.v_rl + ko : nullptr, ogh, ogl);  // dP^T = V dO^T
            float ds[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kk = mfma_acc_row(r, hf);
                float x = (float)((double)s[r] * a.inv_scale);
                if (a.shift && sreg[kk] != qreg) x += -100.0f;
                const float p = (t * WA_T + kk < a.Lk && qvalid) ? expf((float)((double)x - lq)) : 0.f;
                if (sweep == 0) dsum += (double)p * (double)dp[r];
                else ds[r] = p * (float)((double)dp[r] - dsum);
            }
            if (sweep == 1) wah_accumulate<NCB>(acc, kth, ktl, t * WA_T + 4 * hf, lkpad, ds);      // g_q^T += K^T dS^T
        }
        if (sweep == 0) {
            dsum += __shfl_xor(dsum, 32);
            if (qvalid && hf == 0) delta[qrow] = dsum;
        }
    }
    if (!qvalid || !WANT_Q) return;
    const float scale = a.scale;
    wah_store<NCB>(g_q + qrow * a.C, acc, hf, [scale](float x) { return x / scale; });
}

// Backward, g_k and / or g_v.  Owner: keys; walks the window's query tiles, as k_wa_backward_kv.
template <int NCB, bool WANT_K, bool WANT_V>
__global__ __launch_bounds__(S360_BLOCK) void k_wah_backward_kv(WAArgs a, WAHPlanes pl, const double* __restrict__ lse,
                                                                const double* __restrict__ delta, float* __restrict__ g_k,
                                                                float* __restrict__ g_v) {
    constexpr int NS = 2 * NCB;
    __shared__ int s_row[2][WA_T], s_reg[2][WA_T];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const WABlock w = wa_block(a, a.Lk);
    const size_t win = ((size_t)w.b * a.K + w.wy) * a.K + w.wx;
    const int kj = w.ob * WA_ROWS + wave * WA_T + l31;
    const bool kvalid = kj < a.Lk;
    int krow_i = 0, kreg = 0;
    if (kvalid) wa_key(a, w.b, w.wy, w.wx, kj, krow_i, kreg);
    const size_t krow = (size_t)krow_i;
    const size_t oo = (win * a.Lk + kj) * a.C + 8 * hf;
    const __bf16* okh = kvalid ? pl.k_rh + oo : nullptr;                        // the owner's rows (read per step by wah_dot_mem)
    const __bf16* okl = kvalid ? pl.k_rl + oo : nullptr;
    const __bf16* ovh = kvalid ? pl.v_rh + oo : nullptr;
    const __bf16* ovl = kvalid ? pl.v_rl + oo : nullptr;
    const int lwpad = wah_pad4(a.Lw);
    const size_t to = (win * a.C + l31) * lwpad;
    f32x16 dk[NCB], dv[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[cb][r] = dv[cb][r] = 0.f;
    const int ntiles = (a.Lw + WA_T - 1) / WA_T;
    for (int t = 0; t < ntiles; ++t) {
        if (tid < WA_T) {
            const int p = t * WA_T + tid;
            int row = -1, reg = 0;
            if (p < a.Lw) {
                int tok;
                wa_token(a, w.wy, w.wx, p, tok, reg);
                row = w.b * a.L + tok;
            }
            s_row[t & 1][tid] = row;
            s_reg[t & 1][tid] = reg;
        }
        __syncthreads();
        const int* srow = s_row[t & 1];
        const int* sreg = s_reg[t & 1];
        const int p31 = t * WA_T + l31;
        const bool pv = p31 < a.Lw;
        const size_t qo = (win * a.Lw + p31) * a.C + 8 * hf;
        const f32x16 s = wah_dot_mem<NS, true>(pv ? pl.q_rh + qo : nullptr, pv ? pl.q_rl + qo : nullptr, okh, okl);   // S: rows = queries, lane = key
        f32x16 dp;
        if constexpr (WANT_K) dp = wah_dot_mem<NS, true>(pv ? pl.g_rh + qo : nullptr, pv ? pl.g_rl + qo : nullptr, ovh, ovl);  // dP = dO V^T
        float pp[16], ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = mfma_acc_row(r, hf);
            const int qr = srow[qq];
            float x = (float)((double)s[r] * a.inv_scale);
            if (a.shift && sreg[qq] != kreg) x += -100.0f;
            float p = 0.f;
            if (qr >= 0 && kvalid) p = expf((float)((double)x - lse[qr]));
            pp[r] = p;
            if constexpr (WANT_K) ds[r] = p * (float)((double)dp[r] - (qr >= 0 ? delta[qr] : 0.0));
        }
        if constexpr (WANT_V) wah_accumulate<NCB>(dv, pl.g_th + to, pl.g_tl + to, t * WA_T + 4 * hf, lwpad, pp);  // g_v^T += dO^T P
        if constexpr (WANT_K) wah_accumulate<NCB>(dk, pl.q_th + to, pl.q_tl + to, t * WA_T + 4 * hf, lwpad, ds);  // g_k^T += Q^T dS
    }
    if (!kvalid) return;
    if constexpr (WANT_V) wah_store<NCB>(g_v + krow * a.C, dv, hf, [](float x) { return x; });
    if constexpr (WANT_K) {
        const float scale = a.scale;
        wah_store<NCB>(g_k + krow * a.C, dk, hf, [scale](float x) { return x / scale; });
    }
}

// ---------------------------------------------------------------------------------------------- the entry points, both modes
// The size rules of a call, "high" with the grid of its largest pre-pass launch; fills the size fields of `a`.
static int wa_sizes(int32_t batch, int32_t partners, int32_t height, int32_t width, int32_t channels, int32_t num_splits,
                    int32_t with_shift, int32_t mask_rule, bool high, WAArgs& a) {
    if (batch < 1 || partners < 0 || height < 1 || width < 1 || num_splits < 1) return S360_E_BADARG;
    if (channels < 32 || channels > 128 || channels % 32 != 0) return S360_E_UNSUPPORTED;
    if (height % num_splits != 0 || width % num_splits != 0 || (mask_rule != 0 && mask_rule != 1)) return S360_E_BADARG;
    const int64_t M = partners > 0 ? partners : 1, L = (int64_t)height * width;
    const int64_t Lw = L / ((int64_t)num_splits * num_splits);
    if (batch * M * L >= (int64_t)1 << 31 || Lw * M >= (int64_t)1 << 31) return S360_E_BADARG;
    const int64_t wins = (int64_t)batch * num_splits * num_splits;
    if (wins * ((Lw * M + WA_ROWS - 1) / WA_ROWS) >= (int64_t)1 << 31) return S360_E_BADARG;
    a.B = batch; a.M = (int)M; a.H = height; a.W = width; a.C = channels; a.K = num_splits;
    a.wh = height / num_splits; a.ww = width / num_splits;
    a.shift = with_shift ? 1 : 0;
    a.sh = a.shift ? a.wh / 2 : 0; a.sw = a.shift ? a.ww / 2 : 0;
    a.Lw = (int)Lw; a.Lk = (int)(Lw * M); a.L = (int)L;
    a.aligned = mask_rule;
    a.scale = (float)sqrt((double)channels);
    a.inv_scale = 1.0 / sqrt((double)channels);
    if (high && !s360_grid_fits((long long)(((size_t)wins * wah_pad4(a.Lk) * (a.C / 8) + S360_BLOCK - 1) / S360_BLOCK))) return S360_E_BADARG;
    return S360_OK;
}

// The scratch of a "high" call: the planes in the order q, k, v, g (rows, then transposed; hi, then lo), each a multiple of 64
// bytes.  Forward: rows of q and k, transposed v.  Backward: rows of all four, transposed q, k and g.
static size_t wah_layout(const WAArgs& a, bool backward, char* base, WAHPlanes* pl) {
    const size_t nwin = (size_t)a.B * a.K * a.K;
    const size_t nq = nwin * a.Lw * a.C, nk = nwin * a.Lk * a.C;
    const size_t tq = nwin * a.C * wah_pad4(a.Lw), tk = nwin * a.C * wah_pad4(a.Lk);
    Bx3Carver c{base};
    WAHPlanes none = {};
    if (pl) *pl = none;
    WAHPlanes* p = pl ? pl : &none;
    c.take(nq, &p->q_rh, &p->q_rl);
    c.take(nk, &p->k_rh, &p->k_rl);
    if (!backward) {
        c.take(tk, &p->v_th, &p->v_tl);
        return c.off;
    }
    c.take(nk, &p->v_rh, &p->v_rl);
    c.take(nq, &p->g_rh, &p->g_rl);
    c.take(tq, &p->q_th, &p->q_tl);
    c.take(tk, &p->k_th, &p->k_tl);
    c.take(tq, &p->g_th, &p->g_tl);
    return c.off;
}

// What every launch entry starts with, in the order of include/s360.h's refusals: the pointer rule (the gradients may be null, and
// so may the scratch, which only a "high" call must have), the sizes, the scratch size.  Completes `a` (the caller has set its
// pointers) with the sizes.
template <bool HIGH, size_t NI, size_t NO>
static int wa_setup(const void* const (&in)[NI], const void* const (&outs)[NO], const void* g_q, const void* g_k, const void* g_v,
                    const void* scratch, size_t scratch_bytes, bool backward, int32_t batch, int32_t partners, int32_t height, int32_t width,
                    int32_t channels, int32_t num_splits, int32_t with_shift, int32_t mask_rule, WAArgs& a) {
    const void* const opt[] = {g_q, g_k, g_v, scratch};
    if ((HIGH && !scratch) || !s360_pointers_ok(in, outs, opt)) return S360_E_BADARG;
    const int rc = wa_sizes(batch, partners, height, width, channels, num_splits, with_shift, mask_rule, HIGH, a);
    if (rc != S360_OK) return rc;
    return HIGH && scratch_bytes < wah_layout(a, backward, nullptr, nullptr) ? S360_E_WORKSPACE : S360_OK;
}

static unsigned wa_grid(const WAArgs& a, int owner_rows) {
    return (unsigned)((int64_t)a.B * a.K * a.K * ((owner_rows + WA_ROWS - 1) / WA_ROWS));
}

// f(std::integral_constant<int, NCB>()) with NCB = channels / 32 channel blocks (1 .. 4: wa_sizes has checked the channels):
// the one place where a call's channel count becomes the kernels' template argument, in both modes
template <typename F>
static void wa_with_ncb(int channels, F f) {
    switch (channels / 32) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        default: f(std::integral_constant<int, 4>()); break;
    }
}

// launches k_wah_split for one operand (wa_sizes has checked that the grid fits)
static void wah_split_launch(const WAArgs& a, const float* src, int keys, __bf16* rh, __bf16* rl, __bf16* th, __bf16* tl, hipStream_t st) {
    const size_t n = (size_t)a.B * a.K * a.K * wah_pad4(keys ? a.Lk : a.Lw) * (a.C / 8);
    hipLaunchKernelGGL(k_wah_split, dim3((unsigned)((n + S360_BLOCK - 1) / S360_BLOCK)), dim3(S360_BLOCK), 0, st, a, src, keys, rh, rl, th, tl);
}

// the backward's query-owned and key-owned pass, with the gradients asked for as template arguments; `pl` serves "high" alone
template <bool HIGH, int NCB>
static void wa_launch_q(const WAArgs& a, const WAHPlanes& pl, const double* lse, const float* g_out, double* delta, float* g_q, hipStream_t st) {
    const dim3 grid(wa_grid(a, a.Lw)), block(S360_BLOCK);
    auto launch = [&](auto want_q) {
        constexpr bool Q = decltype(want_q)::value;
        if constexpr (HIGH) hipLaunchKernelGGL((k_wah_backward_q<NCB, Q>), grid, block, 0, st, a, pl, lse, delta, g_q);
        else hipLaunchKernelGGL((k_wa_backward_q<NCB, Q>), grid, block, 0, st, a, lse, g_out, delta, g_q);
    };
    if (g_q) launch(std::true_type());
    else launch(std::false_type());
}

template <bool HIGH, int NCB>
static void wa_launch_kv(const WAArgs& a, const WAHPlanes& pl, const double* lse, const double* delta, const float* g_out, float* g_k,
                         float* g_v, hipStream_t st) {
    const dim3 grid(wa_grid(a, a.Lk)), block(S360_BLOCK);
    auto launch = [&](auto want_k, auto want_v) {
        constexpr bool K = decltype(want_k)::value, V = decltype(want_v)::value;
        if constexpr (HIGH) hipLaunchKernelGGL((k_wah_backward_kv<NCB, K, V>), grid, block, 0, st, a, pl, lse, delta, g_k, g_v);
        else hipLaunchKernelGGL((k_wa_backward_kv<NCB, K, V>), grid, block, 0, st, a, lse, delta, g_out, g_k, g_v);
    };
    if (g_k && g_v) launch(std::true_type(), std::true_type());
    else if (g_k) launch(std::true_type(), std::false_type());
    else launch(std::false_type(), std::true_type());
}

// s360_window_attention_forward (HIGH = false: no scratch) and s360_window_attention_high_forward (true)
template <bool HIGH>
static int wa_forward(WAArgs a, int32_t batch, int32_t partners, int32_t height, int32_t width, int32_t channels, int32_t num_splits,
                      int32_t with_shift, int32_t mask_rule, float* out, double* lse, void* scratch, size_t scratch_bytes, hipStream_t st) {
    const void* const in[] = {a.q, a.k, a.v};
    const void* const outs[] = {out, lse};
    const int rc = wa_setup<HIGH>(in, outs, nullptr, nullptr, nullptr, scratch, scratch_bytes, false, batch, partners, height, width, channels, num_splits,
                                  with_shift, mask_rule, a);
    if (rc != S360_OK) return rc;
    const dim3 grid(wa_grid(a, a.Lw)), block(S360_BLOCK);
    if constexpr (HIGH) {
        WAHPlanes pl;
        wah_layout(a, false, static_cast<char*>(scratch), &pl);
        wah_split_launch(a, a.q, 0, pl.q_rh, pl.q_rl, nullptr, nullptr, st);
        wah_split_launch(a, a.k, 1, pl.k_rh, pl.k_rl, nullptr, nullptr, st);
        wah_split_launch(a, a.v, 1, nullptr, nullptr, pl.v_th, pl.v_tl, st);
        S360_CHECK_LAUNCH();
        wa_with_ncb(channels, [&](auto ncb) { hipLaunchKernelGGL((k_wah_forward<decltype(ncb)::value>), grid, block, 0, st, a, pl, out, lse); });
    } else {
        wa_with_ncb(channels, [&](auto ncb) { hipLaunchKernelGGL((k_wa_forward<decltype(ncb)::value>), grid, block, 0, st, a, out, lse); });
    }
    return s360_launch_status();
}

// s360_window_attention_backward (HIGH = false: no scratch) and s360_window_attention_high_backward (true)
template <bool HIGH>
static int wa_backward(WAArgs a, const double* lse, const float* g_out, int32_t batch, int32_t partners, int32_t height, int32_t width,
                       int32_t channels, int32_t num_splits, int32_t with_shift, int32_t mask_rule, double* delta, float* g_q, float* g_k,
                       float* g_v, void* scratch, size_t scratch_bytes, hipStream_t st) {
    const void* const in[] = {a.q, a.k, a.v, lse, g_out};
    const void* const outs[] = {delta};
    const int rc = wa_setup<HIGH>(in, outs, g_q, g_k, g_v, scratch, scratch_bytes, true, batch, partners, height, width, channels, num_splits,
                                  with_shift, mask_rule, a);
    if (rc != S360_OK) return rc;
    if (!g_q && !g_k && !g_v) return S360_OK;
    WAHPlanes pl = {};
    if constexpr (HIGH) {
        wah_layout(a, true, static_cast<char*>(scratch), &pl);
        wah_split_launch(a, a.q, 0, pl.q_rh, pl.q_rl, pl.q_th, pl.q_tl, st);
        wah_split_launch(a, a.k, 1, pl.k_rh, pl.k_rl, pl.k_th, pl.k_tl, st);
        wah_split_launch(a, a.v, 1, pl.v_rh, pl.v_rl, nullptr, nullptr, st);
        wah_split_launch(a, g_out, 0, pl.g_rh, pl.g_rl, pl.g_th, pl.g_tl, st);
        S360_CHECK_LAUNCH();
    }
    if (g_q || g_k) {                                         // the query-owned pass first: it writes Delta for the key-owned one
        wa_with_ncb(channels, [&](auto ncb) { wa_launch_q<HIGH, decltype(ncb)::value>(a, pl, lse, g_out, delta, g_q, st); });
        S360_CHECK_LAUNCH();
    }
    if (g_k || g_v) {
        wa_with_ncb(channels, [&](auto ncb) { wa_launch_kv<HIGH, decltype(ncb)::value>(a, pl, lse, delta, g_out, g_k, g_v, st); });
        S360_CHECK_LAUNCH();
    }
    return S360_OK;
}

}  // namespace s360

using namespace s360;

extern "C" int s360_window_attention_forward(const float* q, const float* k, const float* v, int32_t batch, int32_t partners,
                                             int32_t height, int32_t width, int32_t channels, int32_t num_splits, int32_t with_shift,
                                             int32_t mask_rule, float* out, double* lse, void* stream) {
    return wa_forward<false>({q, k, v}, batch, partners, height, width, channels, num_splits, with_shift, mask_rule, out, lse, nullptr, 0,
                             (hipStream_t)stream);
}

extern "C" int s360_window_attention_backward(const float* q, const float* k, const float* v, const double* lse, const float* g_out,
                                              int32_t batch, int32_t partners, int32_t height, int32_t width, int32_t channels,
                                              int32_t num_splits, int32_t with_shift, int32_t mask_rule, double* delta, float* g_q,
                                              float* g_k, float* g_v, void* stream) {
    return wa_backward<false>({q, k, v}, lse, g_out, batch, partners, height, width, channels, num_splits, with_shift, mask_rule, delta,
                              g_q, g_k, g_v, nullptr, 0, (hipStream_t)stream);
}

extern "C" size_t s360_window_attention_high_scratch_bytes(int32_t batch, int32_t partners, int32_t height, int32_t width,
                                                           int32_t channels, int32_t num_splits, int32_t backward) {
    WAArgs a;
    if (wa_sizes(batch, partners, height, width, channels, num_splits, 0, 0, true, a) != S360_OK) return 0;
    return wah_layout(a, backward != 0, nullptr, nullptr);
}

extern "C" int s360_window_attention_high_forward(const float* q, const float* k, const float* v, int32_t batch, int32_t partners,
                                                  int32_t height, int32_t width, int32_t channels, int32_t num_splits,
                                                  int32_t with_shift, int32_t mask_rule, float* out, double* lse, void* scratch,
                                                  size_t scratch_bytes, void* stream) {
    return wa_forward<true>({q, k, v}, batch, partners, height, width, channels, num_splits, with_shift, mask_rule, out, lse, scratch,
                            scratch_bytes, (hipStream_t)stream);
}

extern "C" int s360_window_attention_high_backward(const float* q, const float* k, const float* v, const double* lse,
                                                   const float* g_out, int32_t batch, int32_t partners, int32_t height, int32_t width,
                                                   int32_t channels, int32_t num_splits, int32_t with_shift, int32_t mask_rule,
                                                   double* delta, float* g_q, float* g_k, float* g_v, void* scratch,
                                                   size_t scratch_bytes, void* stream) {
    return wa_backward<true>({q, k, v}, lse, g_out, batch, partners, height, width, channels, num_splits, with_shift, mask_rule, delta, g_q,
                             g_k, g_v, scratch, scratch_bytes, (hipStream_t)stream);
}
