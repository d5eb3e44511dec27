// s360_eval_scores.hip — the weight-free scores of the evaluation step besides SSIM, on the GPU.  gfx950 only.
//
//   s360_depth_metrics   compute_depth_metrics_batched (the reference's src/scripts/compute_depth_metrics.py:47-116, called at
//                        src/model/model_wrapper_erp.py:526-531) and, optionally, the step's reduction over faces (:532-541)
//   s360_psnr            compute_psnr (src/evaluation/metrics.py:11-21; called by the evaluation step at model_wrapper_erp.py:485-487
//                        and by every training step at :234-238)
//
// tests/depth_metrics_reference.py is the numpy statement the tests compare against.
//
// Depth metrics, per row and per VALID element (valid plane != 0, or gt > threshold), float32 IEEE operations as torch does them:
//   d = gt - pred;   |d|,  |d| / gt,  (d d) / gt,  d d,  (log gt - log pred)^2;   q1 = gt / pred,  q2 = pred / gt.
// Each of the five terms is summed (float64) and counted over the valid elements where that term is not NaN — the reference
// writes NaN into invalid elements and takes nanmean, so a NaN term of a valid element drops out of its own metric as well.
// max(q1, q2) < t with a NaN-propagating max is (q1 < t) && (q2 < t): counted (integers) for the five float32 thresholds
// and divided by the number of valid elements.
//
// Determinism: thread t of a workgroup handles the quads (i * 256 + t) * 4 .. + 3 of the workgroup's 4096 elements, i = 0..3, in
// that order, whether they are fetched as one 16-byte load or (unaligned / strided rows, the nearest lookup, the row's tail)
// one by one; wave and workgroup sums run in a fixed order (block_sum's) into the workgroup's own workspace slot, and the
// second stage sums a row's slots in a fixed order (block_tree_sum).  No atomics: results are bit-identical from call to call,
// independent of the other rows of the call and of the alignment of the inputs.
#include "s360_device.h"

namespace s360 {

constexpr int ES_QUADS = 4;                                  // quads of 4 elements per thread
constexpr int ES_CHUNK = S360_BLOCK * 4 * ES_QUADS;          // elements per workgroup: 4096
constexpr int DM_TERMS = 5;                                  // abs_diff, abs_rel, sq_rel, rmse, rmse_log
constexpr int DM_THRESH = 5;                                 // 1.05, 1.10, 1.25, 1.25^2, 1.25^3
constexpr int DM_COUNTS = DM_TERMS + DM_THRESH + 1;          // per-term non-NaN counts, threshold hits, valid
constexpr int DM_OUT = 12;

struct DmPartial {                                           // one workgroup's sums: 88 bytes, 8-byte aligned
    double sum[DM_TERMS];
    unsigned cnt[DM_COUNTS + 1];
};

struct DmAcc {
    double sum[DM_TERMS];
    unsigned cnt[DM_COUNTS];
};

struct DmArgs {
    const float* gt;
    const float* pred;
    const unsigned char* valid;                              // NULL: gt > threshold
    int n, blocks_per_row, rows_per_group;
    size_t gt_row_stride, pred_row_stride, valid_row_stride, gt_group_stride, pred_group_stride;
    float threshold;
    int gt_w, pred_h, pred_w;                                // nearest lookup (LOOKUP only)
    float scale_h, scale_w;
};

__device__ __forceinline__ void dm_element(DmAcc& a, float g, float p) {
    const float d = g - p;
    const float ad = fabsf(d), dd = d * d;
    const float lg = logf(g) - logf(p);
    const float term[DM_TERMS] = {ad, ad / g, dd / g, dd, lg * lg};
#pragma unroll
    for (int k = 0; k < DM_TERMS; ++k) {
        if (term[k] == term[k]) {                            // not NaN (an infinite term is summed: the mean is then infinite)
            a.sum[k] += (double)term[k];
            a.cnt[k] += 1u;
        }
    }
    const float q1 = g / p, q2 = p / g;
    const float thr[DM_THRESH] = {1.05f, 1.10f, 1.25f, 1.5625f, 1.953125f};
#pragma unroll
    for (int k = 0; k < DM_THRESH; ++k) a.cnt[DM_TERMS + k] += (q1 < thr[k] && q2 < thr[k]) ? 1u : 0u;
    a.cnt[DM_TERMS + DM_THRESH] += 1u;
}

// nearest-neighbour source index of F.interpolate(mode="nearest"): min(floor(float(dst) * scale), size - 1)
__device__ __forceinline__ int nearest_src(int dst, float scale, int size) {
    const int s = (int)floorf((float)dst * scale);
    return s < size - 1 ? s : size - 1;
}

template <bool VEC, bool LOOKUP>
__global__ __launch_bounds__(S360_BLOCK) void k_depth_metrics_partials(DmArgs A, DmPartial* __restrict__ partials) {
    __shared__ DmAcc wacc[S360_BLOCK / S360_WAVE];
    const int tid = threadIdx.x;
    const int row = blockIdx.x / A.blocks_per_row, blk = blockIdx.x - row * A.blocks_per_row;
    const int grp = row / A.rows_per_group, in_grp = row - grp * A.rows_per_group;
    const float* g = A.gt + (size_t)grp * A.gt_group_stride + (size_t)in_grp * A.gt_row_stride;
    const float* p = A.pred + (size_t)grp * A.pred_group_stride + (size_t)in_grp * A.pred_row_stride;
    const unsigned char* v = A.valid ? A.valid + (size_t)row * A.valid_row_stride : nullptr;

    DmAcc acc;
#pragma unroll
    for (int k = 0; k < DM_TERMS; ++k) acc.sum[k] = 0.0;
#pragma unroll
    for (int k = 0; k < DM_COUNTS; ++k) acc.cnt[k] = 0u;

    const long long base = (long long)blk * ES_CHUNK;
#pragma unroll
    for (int i = 0; i < ES_QUADS; ++i) {
        const long long e0 = base + ((long long)i * S360_BLOCK + tid) * 4;
        if (e0 >= A.n) break;
        float gv[4], pv[4];
        bool ok[4];
        const bool full = e0 + 4 <= A.n;
        if (VEC && full) {
            const float4 g4 = *reinterpret_cast<const float4*>(g + e0);
            gv[0] = g4.x, gv[1] = g4.y, gv[2] = g4.z, gv[3] = g4.w;
            if (!LOOKUP) {
                const float4 p4 = *reinterpret_cast<const float4*>(p + e0);
                pv[0] = p4.x, pv[1] = p4.y, pv[2] = p4.z, pv[3] = p4.w;
            }
            if (v) {
                const uchar4 v4 = *reinterpret_cast<const uchar4*>(v + e0);
                ok[0] = v4.x != 0, ok[1] = v4.y != 0, ok[2] = v4.z != 0, ok[3] = v4.w != 0;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = e0 + j < A.n;
                gv[j] = in ? g[e0 + j] : 0.f;
                if (!LOOKUP) pv[j] = in ? p[e0 + j] : 0.f;
                if (v) ok[j] = in && v[e0 + j] != 0;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = full || e0 + j < A.n;
            if (!v) ok[j] = in && gv[j] > A.threshold;
            if (LOOKUP) {
                pv[j] = 0.f;
                if (ok[j]) {                                 // ok implies e0 + j < n = gt_h * gt_w
                    const int e = (int)(e0 + j), y = e / A.gt_w, x = e - y * A.gt_w;
                    pv[j] = p[(size_t)nearest_src(y, A.scale_h, A.pred_h) * A.pred_w + nearest_src(x, A.scale_w, A.pred_w)];
                }
            }
            if (ok[j]) dm_element(acc, gv[j], pv[j]);
        }
    }

    // block_sum's order, written out: the per-wave scratch is one DmAcc per wave (sums and counts behind the one barrier);
    // as two block_sum arrays the kernel's registers and LDS moved
#pragma unroll
    for (int off = S360_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < DM_TERMS; ++k) acc.sum[k] += __shfl_down(acc.sum[k], off, S360_WAVE);
#pragma unroll
        for (int k = 0; k < DM_COUNTS; ++k) acc.cnt[k] += __shfl_down(acc.cnt[k], off, S360_WAVE);
    }
    if ((tid & (S360_WAVE - 1)) == 0) wacc[tid / S360_WAVE] = acc;
    __syncthreads();
    if (tid == 0) {
        DmPartial out;
#pragma unroll
        for (int k = 0; k < DM_TERMS; ++k) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < S360_BLOCK / S360_WAVE; ++w) t += wacc[w].sum[k];
            out.sum[k] = t;
        }
#pragma unroll
        for (int k = 0; k < DM_COUNTS; ++k) {
            unsigned t = 0u;
#pragma unroll
            for (int w = 0; w < S360_BLOCK / S360_WAVE; ++w) t += wacc[w].cnt[k];
            out.cnt[k] = t;
        }
        out.cnt[DM_COUNTS] = 0u;
        partials[blockIdx.x] = out;
    }
}

// One workgroup per row: thread t sums slots t, t + 256, ... in order, then a fixed tree; thread 0 forms the twelve numbers.
// metrics_out[12, n_rows]: abs_diff, abs_rel, sq_rel, rmse, rmse_log, a5, a10, a25, a0, a1, a2, a3.
__global__ __launch_bounds__(S360_BLOCK) void k_depth_metrics_rows(const DmPartial* __restrict__ partials, int blocks_per_row, int n_rows,
                                                                    float a_scale, float* __restrict__ metrics_out,
                                                                    int* __restrict__ valid_count) {
    __shared__ double rsum[DM_TERMS][S360_BLOCK];
    __shared__ unsigned long long rcnt[DM_COUNTS][S360_BLOCK];
    const int tid = threadIdx.x, row = blockIdx.x;
    const DmPartial* p = partials + (size_t)row * blocks_per_row;
    double s[DM_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    unsigned long long c[DM_COUNTS];
#pragma unroll
    for (int k = 0; k < DM_COUNTS; ++k) c[k] = 0ull;
    for (int j = tid; j < blocks_per_row; j += S360_BLOCK) {
#pragma unroll
        for (int k = 0; k < DM_TERMS; ++k) s[k] += p[j].sum[k];
#pragma unroll
        for (int k = 0; k < DM_COUNTS; ++k) c[k] += p[j].cnt[k];
    }
    block_tree_sum(s, rsum, c, rcnt);
    if (tid == 0) {
        const unsigned long long nv = rcnt[DM_TERMS + DM_THRESH][0];
        for (int k = 0; k < DM_TERMS; ++k) {
            float m = (float)(rsum[k][0] / (double)rcnt[k][0]);     // 0 / 0: NaN, as nanmean of nothing
            if (k >= 3) m = sqrtf(m);
            metrics_out[(size_t)k * n_rows + row] = m;
        }
        const int a_of[7] = {0, 1, 2, 1, 2, 3, 4};                   // a5, a10, a25, a0 (= a10), a1 (= a25), a2, a3
        for (int k = 0; k < 7; ++k) {
            const float a = (float)rcnt[DM_TERMS + a_of[k]][0] / (float)nv;
            metrics_out[(size_t)(DM_TERMS + k) * n_rows + row] = a_scale == 1.0f ? a : a * a_scale;
        }
        valid_count[row] = (int)(nv > 0x7fffffffull ? 0x7fffffffull : nv);
    }
}

// The evaluation step's reduction (model_wrapper_erp.py:537-541): a row without a valid element counts 0, the sum over rows is
// divided by the number of rows that have one.  Thread k handles metric k; rows in order, float64.
__global__ void k_depth_metrics_scores(const float* __restrict__ metrics, const int* __restrict__ valid_count, int n_rows,
                                       float* __restrict__ scores_out) {
    const int k = threadIdx.x;
    if (k >= DM_OUT) return;
    double s = 0.0;
    int rows = 0;
    for (int r = 0; r < n_rows; ++r) {
        if (valid_count[r] > 0) {
            s += (double)metrics[(size_t)k * n_rows + r];
            ++rows;
        }
    }
    scores_out[k] = (float)(s / (double)rows);
}

__device__ __forceinline__ float clip01(float x) {           // NaN stays NaN (torch.clip)
    return x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
}

template <bool VEC>
__global__ __launch_bounds__(S360_BLOCK) void k_psnr_partials(const float* __restrict__ pred, const float* __restrict__ gt, long long m,
                                                              int blocks_per_image, double* __restrict__ partials) {
    __shared__ double wsum[1][BLOCK_WAVES];
    const int tid = threadIdx.x;
    const int img = blockIdx.x / blocks_per_image, blk = blockIdx.x - img * blocks_per_image;
    const float* a = pred + (size_t)img * m;
    const float* b = gt + (size_t)img * m;
    const long long base = (long long)blk * ES_CHUNK;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < ES_QUADS; ++i) {
        const long long e0 = base + ((long long)i * S360_BLOCK + tid) * 4;
        if (e0 >= m) break;
        float av[4], bv[4];
        if (VEC && e0 + 4 <= m) {
            const float4 a4 = *reinterpret_cast<const float4*>(a + e0), b4 = *reinterpret_cast<const float4*>(b + e0);
            av[0] = a4.x, av[1] = a4.y, av[2] = a4.z, av[3] = a4.w;
            bv[0] = b4.x, bv[1] = b4.y, bv[2] = b4.z, bv[3] = b4.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = e0 + j < m;
                av[j] = in ? a[e0 + j] : 0.f;                // 0 - 0: adds nothing
                bv[j] = in ? b[e0 + j] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = clip01(bv[j]) - clip01(av[j]);
            acc += (double)(d * d);
        }
    }
    double s[1] = {acc};
    block_sum<false>(s, wsum);
    if (tid == 0) partials[blockIdx.x] = s[0];
}

// One workgroup per image: the mean (float64 -> float32), 0 -> 1e-10, -10 log10.
__global__ __launch_bounds__(S360_BLOCK) void k_psnr_reduce(const double* __restrict__ partials, int blocks_per_image, double count,
                                                            float* __restrict__ out) {
    __shared__ double red[1][S360_BLOCK];
    const int tid = threadIdx.x, img = blockIdx.x;
    const double* p = partials + (size_t)img * blocks_per_image;
    double t[1] = {0.0};
    for (int j = tid; j < blocks_per_image; j += S360_BLOCK) t[0] += p[j];
    block_tree_sum(t, red);
    if (tid == 0) {
        float mse = (float)(red[0][0] / count);
        if (mse == 0.0f) mse = 1e-10f;
        out[img] = (float)(-10.0 * log10((double)mse));
    }
}

}  // namespace s360

using namespace s360;

extern "C" int s360_depth_metrics(const float* gt, const float* pred, const uint8_t* valid, int32_t n_rows, int32_t n,
                                  size_t gt_row_stride, size_t pred_row_stride, size_t valid_row_stride, int32_t rows_per_group,
                                  size_t gt_group_stride, size_t pred_group_stride, float threshold, int32_t gt_height,
                                  int32_t gt_width, int32_t pred_height, int32_t pred_width, int32_t mult_a, float* metrics_out,
                                  int32_t* valid_count, float* scores_out, void* workspace, size_t* workspace_bytes, void* stream) {
    if (!workspace_bytes || n_rows < 1 || n < 1 || rows_per_group < 1) return S360_E_BADARG;
    const bool lookup = pred_height > 0 || pred_width > 0;
    if (lookup && (gt_height < 1 || gt_width < 1 || pred_height < 1 || pred_width < 1 || (long long)gt_height * gt_width != n))
        return S360_E_BADARG;
    const long long bpr = ((long long)n + ES_CHUNK - 1) / ES_CHUNK;
    const long long blocks = bpr * n_rows;
    if (!s360_grid_fits(blocks)) return S360_E_BADARG;
    const int ws = s360_workspace(workspace, workspace_bytes, (size_t)blocks * sizeof(DmPartial), 8, gt && pred && metrics_out && valid_count);
    if (ws != S360_WS_READY) return ws;
    DmArgs A;
    A.gt = gt, A.pred = pred, A.valid = valid;
    A.n = n, A.blocks_per_row = (int)bpr, A.rows_per_group = rows_per_group;
    A.gt_row_stride = gt_row_stride, A.pred_row_stride = pred_row_stride, A.valid_row_stride = valid_row_stride;
    A.gt_group_stride = gt_group_stride, A.pred_group_stride = pred_group_stride;
    A.threshold = threshold;
    A.gt_w = lookup ? gt_width : 1, A.pred_h = pred_height, A.pred_w = pred_width;
    A.scale_h = lookup ? (float)pred_height / (float)gt_height : 1.f;
    A.scale_w = lookup ? (float)pred_width / (float)gt_width : 1.f;
    // 16-byte loads need every row to start on a 16-byte boundary (4-byte for the validity plane)
    bool vec = s360_aligned(gt, 16) && gt_row_stride % 4 == 0 && gt_group_stride % 4 == 0;
    if (!lookup) vec = vec && s360_aligned(pred, 16) && pred_row_stride % 4 == 0 && pred_group_stride % 4 == 0;
    if (valid) vec = vec && s360_aligned(valid, 4) && valid_row_stride % 4 == 0;
    DmPartial* partials = (DmPartial*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(S360_BLOCK);
    if (lookup) {
        if (vec) hipLaunchKernelGGL((k_depth_metrics_partials<true, true>), grid, block, 0, st, A, partials);
        else hipLaunchKernelGGL((k_depth_metrics_partials<false, true>), grid, block, 0, st, A, partials);
    } else {
        if (vec) hipLaunchKernelGGL((k_depth_metrics_partials<true, false>), grid, block, 0, st, A, partials);
        else hipLaunchKernelGGL((k_depth_metrics_partials<false, false>), grid, block, 0, st, A, partials);
    }
    S360_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_depth_metrics_rows, dim3((unsigned)n_rows), block, 0, st, (const DmPartial*)partials, (int)bpr, (int)n_rows,
                       mult_a ? 100.0f : 1.0f, metrics_out, valid_count);
    S360_CHECK_LAUNCH();
    if (scores_out) {
        hipLaunchKernelGGL(k_depth_metrics_scores, dim3(1), dim3(S360_WAVE), 0, st, (const float*)metrics_out, (const int*)valid_count,
                           (int)n_rows, scores_out);
        S360_CHECK_LAUNCH();
    }
    return S360_OK;
}

extern "C" int s360_psnr(const float* pred, const float* gt, int32_t n_images, int32_t channels, int32_t height, int32_t width,
                         float* psnr_out, void* workspace, size_t* workspace_bytes, void* stream) {
    if (!workspace_bytes || n_images < 1 || channels < 1 || height < 1 || width < 1) return S360_E_BADARG;
    const long long m = (long long)channels * height * width;
    const long long bpi = (m + ES_CHUNK - 1) / ES_CHUNK;
    const long long blocks = bpi * n_images;
    if (!s360_grid_fits(blocks)) return S360_E_BADARG;
    const int ws = s360_workspace(workspace, workspace_bytes, (size_t)blocks * sizeof(double), 8, pred && gt && psnr_out);
    if (ws != S360_WS_READY) return ws;
    double* partials = (double*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(S360_BLOCK);
    if (s360_aligned(pred, 16) && s360_aligned(gt, 16) && m % 4 == 0)
        hipLaunchKernelGGL((k_psnr_partials<true>), grid, block, 0, st, pred, gt, m, (int)bpi, partials);
    else
        hipLaunchKernelGGL((k_psnr_partials<false>), grid, block, 0, st, pred, gt, m, (int)bpi, partials);
    S360_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_psnr_reduce, dim3((unsigned)n_images), block, 0, st, (const double*)partials, (int)bpi, (double)m, psnr_out);
    return s360_launch_status();
}
