// s360_visualize.hip — the pictures of the evaluation step on the GPU: depth colour maps, colour tables, 8-bit frames and error
// maps.  gfx950 only.
//
//   s360_depth_colormap  depth_map (the reference's src/model/model_wrapper_erp.py:122-133) + apply_color_map_to_image
//                        (src/visualization/color_map.py:9-27) + optionally prep_image (src/misc/image_io.py:38-54), N maps a call
//   s360_colorize        apply_color_map (color_map.py:9-19)
//   s360_prep_image      prep_image (image_io.py:38-54)
//   s360_error_map       |a - b|.mean(0) -> convert_single_colormap / get_colormap (model_wrapper_erp.py:369-371, :88-92, :109-120)
//
// tests/depth_vis_reference.py is the numpy statement the tests compare against.
//
// The two quantiles of a depth map are an exact SELECTION, not a sort: a radix select over the order-preserving 32-bit key of the
// float (sign bit flipped for positives, all bits for negatives), digits of 11, 11 and 10 bits.  Four ranks are followed through
// the same three passes: floor and ceil of the 0.01 rank among the positive elements and of the 0.99 rank among all of them.  The
// positives need no compaction: they are the keys above key(+0) up to key(+inf), so a rank r among them is the rank
// (n - n_pos - n_positive_NaN) + r among all keys.  Each rank is an independent order statistic, so duplicates (also ones that
// straddle a digit boundary of a neighbouring rank) cannot go wrong: ranks that share the digits found so far share a histogram,
// the others get one of their own (at most four).
//
// A map is shared by up to VS_MAX_WGS workgroups.  Each counts its elements into integer histograms in LDS (integer LDS atomics:
// the counts do not depend on their order) and stores them as ITS partial histograms in the workspace; the next launch sums a
// map's partials in a fixed order, finds each rank's digit and counts the next one.  No float atomics, no global atomics, no
// waiting between workgroups, no host read: the result is bit-identical from call to call and a map does not depend on its
// neighbours.  Launches: digit 1, digit 2, digit 3, the per-map record, the colouring — five for any N.
#include "s360_device.h"
#include "s360_colormap_tables.h"

namespace s360 {

constexpr int VS_BINS = 2048;                                // digits 1 and 2: 11 bits; digit 3: 10 bits (1024 bins)
constexpr int VS_RANKS = 4;                                  // near lo, near hi, far lo, far hi
constexpr int VS_CHUNK = 16384;                              // least elements per workgroup before a map is shared
constexpr int VS_MAX_WGS = 32;                               // workgroups per map, at most
constexpr long long VS_MAX_ELEMENTS = 16000000;              // per map (torch.quantile's own limit; the reference truncates)
constexpr int VS_BATCH = 8;                                  // elements a thread loads before it counts them
static_assert(VS_MAX_WGS <= S360_WAVE, "one lane per workgroup sums a map's counts");
constexpr int VS_BAD = 256;                                  // table row of NaN

struct VsCounts {                                            // one workgroup's share of a map
    unsigned n_pos, n_pnan, n_nan, min_key, max_key, pad[3];
};

struct VsState {                                             // one map, after a digit
    unsigned prefix[VS_RANKS];                               // the key bits found so far (in place, low bits 0)
    unsigned rem[VS_RANKS];                                  // the rank among the keys that share them
    unsigned slot[VS_RANKS];                                 // which of the next launch's histograms holds rank j
    unsigned slot_prefix[VS_RANKS];
    unsigned n_slots, active, n_pos, n_pnan, n_nan, min_key, max_key, pad;
};

struct VsRecord {                                            // one map, for the colouring
    float near_q, far_q, log_near, log_far;
    int fallback, pad[3];
};

__device__ __forceinline__ unsigned vs_key(float v) {
    const unsigned b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float vs_unkey(unsigned k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// ATen's linear quantile: rank = float32(q) * float32(n - 1) as a float32 product
__device__ __forceinline__ void vs_rank(float q, unsigned n, unsigned& lo, unsigned& hi, float& w) {
    const float rank = q * (float)(n - 1u);
    const float fl = floorf(rank);
    lo = (unsigned)fl, hi = (unsigned)ceilf(rank);
    w = rank - fl;
}

__device__ __forceinline__ float vs_lerp(float a, float b, float w) {
    const double da = (double)a, db = (double)b, dw = (double)w;
    return (float)(w < 0.5f ? da + dw * (db - da) : db - (db - da) * (1.0 - dw));
}

// The bin of `tot[0 .. BINS)` that holds rank `rem` (counting from 0), and the rank inside that bin: every thread of the
// workgroup calls it; the answer is in res[0], res[1] after it returns.  A rank beyond the total leaves (0, 0).
template <int BINS>
__device__ void vs_select(const unsigned* tot, unsigned rem, unsigned* wsum, unsigned* res) {
    constexpr int PER = BINS / S360_BLOCK;
    const int tid = threadIdx.x, lane = tid & (S360_WAVE - 1), wave = tid / S360_WAVE;
    unsigned local = 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i) local += tot[tid * PER + i];
    unsigned inc = local;
#pragma unroll
    for (int off = 1; off < S360_WAVE; off <<= 1) {
        const unsigned t = __shfl_up(inc, off, S360_WAVE);
        if (lane >= off) inc += t;
    }
    if (tid == 0) res[0] = 0u, res[1] = 0u;
    if (lane == S360_WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    unsigned excl = inc - local;
    for (int w = 0; w < wave; ++w) excl += wsum[w];
    if (rem >= excl && rem - excl < local) {                 // one thread at most
        unsigned c = excl;
        for (int i = 0; i < PER; ++i) {
            const unsigned v = tot[tid * PER + i];
            if (rem - c < v) {
                res[0] = (unsigned)(tid * PER + i), res[1] = rem - c;
                break;
            }
            c += v;
        }
    }
    __syncthreads();
}

struct VsMapArgs {
    const float* depth;
    size_t map_stride;
    unsigned n;                                              // elements per map
    int wgs, per;                                            // workgroups per map, elements per workgroup
};

// digit 1: the histogram of key >> 21 and the counts of this workgroup's elements
__global__ __launch_bounds__(S360_BLOCK) void k_vs_digit1(VsMapArgs A, VsCounts* __restrict__ counts, unsigned* __restrict__ part1) {
    __shared__ unsigned hist[VS_BINS];
    __shared__ unsigned cnt[5];
    const int tid = threadIdx.x;
    const int map = blockIdx.x / A.wgs, blk = blockIdx.x - map * A.wgs;
    for (int b = tid; b < VS_BINS; b += S360_BLOCK) hist[b] = 0u;
    if (tid == 0) cnt[0] = 0u, cnt[1] = 0u, cnt[2] = 0u, cnt[3] = 0xffffffffu, cnt[4] = 0u;
    __syncthreads();
    const float* d = A.depth + (size_t)map * A.map_stride;
    const unsigned begin = (unsigned)blk * (unsigned)A.per;
    const unsigned end = begin + (unsigned)A.per < A.n ? begin + (unsigned)A.per : A.n;
    unsigned n_pos = 0u, n_pnan = 0u, n_nan = 0u, mn = 0xffffffffu, mx = 0u;
    for (unsigned i0 = begin + tid; i0 < end; i0 += S360_BLOCK * VS_BATCH) {     // VS_BATCH loads in flight, then the atomics
        float v[VS_BATCH];
#pragma unroll
        for (int u = 0; u < VS_BATCH; ++u) {
            const unsigned i = i0 + (unsigned)u * S360_BLOCK;
            v[u] = i < end ? d[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < VS_BATCH; ++u) {
            if (i0 + (unsigned)u * S360_BLOCK >= end) break;
            const unsigned k = vs_key(v[u]);
            atomicAdd(&hist[k >> 21], 1u);
            const bool nan = v[u] != v[u];
            n_pos += v[u] > 0.f ? 1u : 0u;
            n_nan += nan ? 1u : 0u;
            n_pnan += (nan && (k >> 31)) ? 1u : 0u;
            mn = k < mn ? k : mn;
            mx = k > mx ? k : mx;
        }
    }
    atomicAdd(&cnt[0], n_pos);
    atomicAdd(&cnt[1], n_pnan);
    atomicAdd(&cnt[2], n_nan);
    atomicMin(&cnt[3], mn);
    atomicMax(&cnt[4], mx);
    __syncthreads();
    unsigned* out = part1 + (size_t)blockIdx.x * VS_BINS;
    for (int b = tid; b < VS_BINS; b += S360_BLOCK) out[b] = hist[b];
    if (tid == 0) {
        VsCounts c;
        c.n_pos = cnt[0], c.n_pnan = cnt[1], c.n_nan = cnt[2], c.min_key = cnt[3], c.max_key = cnt[4];
        c.pad[0] = c.pad[1] = c.pad[2] = 0u;
        counts[blockIdx.x] = c;
    }
}

// Digits 2 (PASS 2: shift 10, 2048 bins, reads the counts and the digit-1 partials) and 3 (PASS 3: shift 0, 1024 bins, reads the
// state and the partials of digit 2).  Every workgroup of a map repeats the same scan of the map's summed partials, then counts
// its own elements; workgroup 0 of the map stores the state for the next launch (state_out is not state_in).
template <int PASS>
__global__ __launch_bounds__(S360_BLOCK) void k_vs_digit(VsMapArgs A, const VsCounts* __restrict__ counts, const VsState* __restrict__ state_in,
                                                        const unsigned* __restrict__ part_in, VsState* __restrict__ state_out,
                                                        unsigned* __restrict__ part_out) {
    constexpr int IN_BINS = VS_BINS;                                     // both read 2048-bin partials
    constexpr int IN_SLOTS = PASS == 2 ? 1 : VS_RANKS;                   // histograms per workgroup in part_in
    constexpr int OUT_BINS = PASS == 2 ? VS_BINS : VS_BINS / 2;
    constexpr int IN_SHIFT = PASS == 2 ? 21 : 10;                        // where the digit scanned here sits in the key
    constexpr int OUT_SHIFT = PASS == 2 ? 10 : 0;                        // where the digit counted here sits
    __shared__ unsigned hist[VS_RANKS][OUT_BINS];
    __shared__ unsigned tot[IN_BINS];
    __shared__ unsigned wsum[S360_BLOCK / S360_WAVE], res[2];
    __shared__ VsState st;
    const int tid = threadIdx.x;
    const int map = blockIdx.x / A.wgs, blk = blockIdx.x - map * A.wgs;

    if (PASS == 2) {
        if (tid < S360_WAVE) {                                           // wgs <= VS_MAX_WGS <= 64: one lane per workgroup's counts
            VsState s;
            s.n_pos = 0u, s.n_pnan = 0u, s.n_nan = 0u, s.min_key = 0xffffffffu, s.max_key = 0u, s.pad = 0u;
            if (tid < A.wgs) {
                const VsCounts c = counts[(size_t)map * A.wgs + tid];
                s.n_pos = c.n_pos, s.n_pnan = c.n_pnan, s.n_nan = c.n_nan, s.min_key = c.min_key, s.max_key = c.max_key;
            }
#pragma unroll
            for (int off = S360_WAVE / 2; off > 0; off >>= 1) {
                s.n_pos += __shfl_down(s.n_pos, off, S360_WAVE);
                s.n_pnan += __shfl_down(s.n_pnan, off, S360_WAVE);
                s.n_nan += __shfl_down(s.n_nan, off, S360_WAVE);
                const unsigned mn = __shfl_down(s.min_key, off, S360_WAVE), mx = __shfl_down(s.max_key, off, S360_WAVE);
                s.min_key = mn < s.min_key ? mn : s.min_key;
                s.max_key = mx > s.max_key ? mx : s.max_key;
            }
            if (tid == 0) {
                s.active = s.n_pos > 0u ? 1u : 0u;
                s.n_slots = s.active;
                for (int j = 0; j < VS_RANKS; ++j) s.prefix[j] = 0u, s.rem[j] = 0u, s.slot[j] = 0u, s.slot_prefix[j] = 0xffffffffu;
                if (s.active) {
                    unsigned lo, hi;
                    float w;
                    vs_rank(0.01f, s.n_pos, lo, hi, w);
                    const unsigned base = A.n - s.n_pos - s.n_pnan;      // keys up to key(+0), negative NaNs among them
                    s.rem[0] = base + lo, s.rem[1] = base + hi;
                    vs_rank(0.99f, A.n, lo, hi, w);
                    s.rem[2] = lo, s.rem[3] = hi;
                }
                st = s;
            }
        }
    } else if (tid == 0) {
        st = state_in[map];
    }
    __syncthreads();
    if (!st.active) {                                                    // no positive element: min / max, nothing to select
        if (blk == 0 && tid == 0) state_out[map] = st;
        return;
    }

    // the digit at IN_SHIFT of every rank, from the map's summed partials
    const unsigned n_in = st.n_slots;
    unsigned digit[VS_RANKS], rem[VS_RANKS];
    for (unsigned s = 0; s < n_in; ++s) {
        for (int b = tid; b < IN_BINS; b += S360_BLOCK) {
            unsigned t = 0u;
#pragma unroll 8
            for (int w = 0; w < A.wgs; ++w) t += part_in[(((size_t)map * A.wgs + w) * IN_SLOTS + s) * IN_BINS + b];
            tot[b] = t;
        }
        __syncthreads();
        for (int j = 0; j < VS_RANKS; ++j) {
            if (st.slot[j] != s) continue;                               // uniform over the workgroup
            vs_select<IN_BINS>(tot, st.rem[j], wsum, res);
            digit[j] = res[0], rem[j] = res[1];
            __syncthreads();
        }
    }
    if (tid == 0) {
        unsigned ns = 0u;
        for (int j = 0; j < VS_RANKS; ++j) {
            st.prefix[j] |= digit[j] << IN_SHIFT;
            st.rem[j] = rem[j];
            int s = -1;
            for (int i = 0; i < j; ++i)
                if (st.prefix[i] == st.prefix[j]) {
                    s = (int)st.slot[i];
                    break;
                }
            if (s < 0) {
                s = (int)ns++;
                st.slot_prefix[s] = st.prefix[j] >> IN_SHIFT;
            }
            st.slot[j] = (unsigned)s;
        }
        for (unsigned s = ns; s < VS_RANKS; ++s) st.slot_prefix[s] = 0xffffffffu;   // a prefix of at most 22 bits never equals it
        st.n_slots = ns;
    }
    for (int b = tid; b < VS_RANKS * OUT_BINS; b += S360_BLOCK) (&hist[0][0])[b] = 0u;
    __syncthreads();
    if (blk == 0 && tid == 0) state_out[map] = st;

    const unsigned p0 = st.slot_prefix[0], p1 = st.slot_prefix[1], p2 = st.slot_prefix[2], p3 = st.slot_prefix[3];
    const float* d = A.depth + (size_t)map * A.map_stride;
    const unsigned begin = (unsigned)blk * (unsigned)A.per;
    const unsigned end = begin + (unsigned)A.per < A.n ? begin + (unsigned)A.per : A.n;
    for (unsigned i0 = begin + tid; i0 < end; i0 += S360_BLOCK * VS_BATCH) {
        float v[VS_BATCH];
#pragma unroll
        for (int u = 0; u < VS_BATCH; ++u) {
            const unsigned i = i0 + (unsigned)u * S360_BLOCK;
            v[u] = i < end ? d[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < VS_BATCH; ++u) {
            if (i0 + (unsigned)u * S360_BLOCK >= end) break;
            const unsigned k = vs_key(v[u]);
            const unsigned p = k >> IN_SHIFT, b = (k >> OUT_SHIFT) & (unsigned)(OUT_BINS - 1);
            if (p == p0) atomicAdd(&hist[0][b], 1u);
            if (p == p1) atomicAdd(&hist[1][b], 1u);
            if (p == p2) atomicAdd(&hist[2][b], 1u);
            if (p == p3) atomicAdd(&hist[3][b], 1u);
        }
    }
    __syncthreads();
    const unsigned n_out = st.n_slots;
    unsigned* out = part_out + (size_t)blockIdx.x * VS_RANKS * OUT_BINS;
    for (unsigned s = 0; s < n_out; ++s)
        for (int b = tid; b < OUT_BINS; b += S360_BLOCK) out[s * OUT_BINS + b] = hist[s][b];
}

// One workgroup per map: the last digit from the digit-3 partials, the four values, the two quantiles and their logarithms.
__global__ __launch_bounds__(S360_BLOCK) void k_vs_record(int wgs, unsigned n, const VsState* __restrict__ state_in,
                                                         const unsigned* __restrict__ part_in, VsRecord* __restrict__ records,
                                                         float* __restrict__ range_out) {
    constexpr int BINS = VS_BINS / 2;
    __shared__ unsigned tot[BINS];
    __shared__ unsigned wsum[S360_BLOCK / S360_WAVE], res[2];
    __shared__ VsState st;
    const int tid = threadIdx.x, map = blockIdx.x;
    if (tid == 0) st = state_in[map];
    __syncthreads();
    VsRecord r;
    r.pad[0] = r.pad[1] = r.pad[2] = 0;
    const float nan = __uint_as_float(0x7fc00000u);
    if (!st.active) {
        r.fallback = 1;
        r.near_q = st.n_nan ? nan : vs_unkey(st.min_key);
        r.far_q = st.n_nan ? nan : vs_unkey(st.max_key);
        r.log_near = nan, r.log_far = nan;
    } else {
        unsigned key[VS_RANKS];
        for (unsigned s = 0; s < st.n_slots; ++s) {
            for (int b = tid; b < BINS; b += S360_BLOCK) {
                unsigned t = 0u;
#pragma unroll 8
                for (int w = 0; w < wgs; ++w) t += part_in[(((size_t)map * wgs + w) * VS_RANKS + s) * BINS + b];
                tot[b] = t;
            }
            __syncthreads();
            for (int j = 0; j < VS_RANKS; ++j) {
                if (st.slot[j] != s) continue;
                vs_select<BINS>(tot, st.rem[j], wsum, res);
                key[j] = st.prefix[j] | res[0];
                __syncthreads();
            }
        }
        unsigned lo, hi;
        float wn, wf;
        vs_rank(0.01f, st.n_pos, lo, hi, wn);
        vs_rank(0.99f, n, lo, hi, wf);
        r.fallback = 0;
        r.near_q = vs_lerp(vs_unkey(key[0]), vs_unkey(key[1]), wn);
        r.far_q = st.n_nan ? nan : vs_lerp(vs_unkey(key[2]), vs_unkey(key[3]), wf);
        r.log_near = (float)log((double)r.near_q);
        r.log_far = (float)log((double)r.far_q);
    }
    if (tid == 0) {
        records[map] = r;
        if (range_out) {
            range_out[(size_t)map * 4 + 0] = r.near_q, range_out[(size_t)map * 4 + 1] = r.far_q;
            range_out[(size_t)map * 4 + 2] = r.log_near, range_out[(size_t)map * 4 + 3] = r.log_far;
        }
    }
}

// matplotlib's index of a float32 x among 256 colours: NaN -> the "bad" row, else min(floor(clip(x, 0, 1) * 256), 255)
__device__ __forceinline__ int vs_index(float x) {
    if (x != x) return VS_BAD;
    const float c = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
    const int i = (int)(c * 256.f);
    return i < 255 ? i : 255;
}

struct VsOut {
    float* f32;                                              // may be NULL
    unsigned char* u8;                                       // may be NULL
    int map_id, byte_rule;                                   // byte_rule 0: kCmapPrep, 1: kCmapByte
    int f32_first, u8_first;                                 // channel-first [.., 3, plane] or channel-last [.., 3]
    long long plane;                                         // elements per plane (channel-first only)
};

// The colours of the elements g0 .. g0 + cnt (cnt <= 4) with table rows idx[]: channel-last bytes of a full quad go out as three
// dwords when the base is 4-byte aligned (12 g0 then is), everything else element by element.
__device__ __forceinline__ void vs_write4(const VsOut& o, long long g0, int cnt, const int idx[4]) {
    const unsigned char(*tb)[3] = o.byte_rule ? kCmapByte[o.map_id] : kCmapPrep[o.map_id];
    if (o.u8) {
        if (!o.u8_first && cnt == 4 && ((uintptr_t)o.u8 & 3) == 0) {
            unsigned char b[12];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) b[j * 3 + c] = tb[idx[j]][c];
            unsigned* dst = reinterpret_cast<unsigned*>(o.u8 + (size_t)g0 * 3);
#pragma unroll
            for (int q = 0; q < 3; ++q)
                dst[q] = (unsigned)b[q * 4] | ((unsigned)b[q * 4 + 1] << 8) | ((unsigned)b[q * 4 + 2] << 16) | ((unsigned)b[q * 4 + 3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= cnt) break;
                const long long g = g0 + j;
                for (int c = 0; c < 3; ++c) {
                    const size_t at = o.u8_first ? ((size_t)(g / o.plane) * 3 + c) * (size_t)o.plane + (size_t)(g % o.plane) : (size_t)g * 3 + c;
                    o.u8[at] = tb[idx[j]][c];
                }
            }
        }
    }
    if (o.f32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= cnt) break;
            const long long g = g0 + j;
            for (int c = 0; c < 3; ++c) {
                const size_t at = o.f32_first ? ((size_t)(g / o.plane) * 3 + c) * (size_t)o.plane + (size_t)(g % o.plane) : (size_t)g * 3 + c;
                o.f32[at] = kCmapF32[o.map_id][idx[j]][c];
            }
        }
    }
}

// Four consecutive pixels of the N maps laid end to end per thread.
__global__ __launch_bounds__(S360_BLOCK) void k_vs_depth_colour(const float* __restrict__ depth, size_t map_stride, long long hw, long long total,
                                                               const VsRecord* __restrict__ records, VsOut o) {
    const long long g0 = ((long long)blockIdx.x * S360_BLOCK + threadIdx.x) * 4;
    if (g0 >= total) return;
    const int cnt = total - g0 < 4 ? (int)(total - g0) : 4;
    int idx[4] = {0, 0, 0, 0};
    long long map = g0 / hw, p = g0 - map * hw;
    VsRecord r = records[map];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= cnt) break;
        if (p == hw) {
            p = 0, ++map;
            r = records[map];
        }
        const double d = (double)depth[(size_t)map * map_stride + (size_t)p];
        float x;
        if (r.fallback) {
            x = (float)(1.0 - (d - (double)r.near_q) / ((double)r.far_q - (double)r.near_q));
        } else {
            const float L = (float)log(d);                   // rounded: a constant map then gives 0 / 0 = NaN, as in the reference
            x = (float)(1.0 - ((double)L - (double)r.log_near) / ((double)r.log_far - (double)r.log_near));
        }
        idx[j] = vs_index(x);
        ++p;
    }
    vs_write4(o, g0, cnt, idx);
}

__global__ __launch_bounds__(S360_BLOCK) void k_vs_colorize(const float* __restrict__ x, long long total, VsOut o) {
    const long long g0 = ((long long)blockIdx.x * S360_BLOCK + threadIdx.x) * 4;
    if (g0 >= total) return;
    const int cnt = total - g0 < 4 ? (int)(total - g0) : 4;
    int idx[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < cnt) idx[j] = vs_index(x[g0 + j]);
    vs_write4(o, g0, cnt, idx);
}

__global__ __launch_bounds__(S360_BLOCK) void k_vs_error_map(const float* __restrict__ a, const float* __restrict__ b, long long hw, VsOut o) {
    const long long g0 = ((long long)blockIdx.x * S360_BLOCK + threadIdx.x) * 4;
    if (g0 >= hw) return;
    const int cnt = hw - g0 < 4 ? (int)(hw - g0) : 4;
    int idx[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= cnt) break;
        const long long g = g0 + j;
        const double e0 = fabs((double)a[g] - (double)b[g]);
        const double e1 = fabs((double)a[hw + g] - (double)b[hw + g]);
        const double e2 = fabs((double)a[2 * hw + g] - (double)b[2 * hw + g]);
        idx[j] = vs_index((float)(((e0 + e1) + e2) / 3.0));
    }
    vs_write4(o, g0, cnt, idx);
}

__device__ __forceinline__ unsigned char vs_byte(float v) {  // trunc(clip(v, 0, 1) * 255); NaN -> 0
    const float c = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    return c == c ? (unsigned char)(int)(c * 255.f) : (unsigned char)0;
}

// image[b, c, h, w] -> out[h, b w, C]: four consecutive output pixels per thread, 4 C bytes that go out as dwords when the base
// is 4-byte aligned.  c == 1 is replicated to three channels.
template <int C>
__global__ __launch_bounds__(S360_BLOCK) void k_vs_prep_image(const float* __restrict__ image, int batch, int channels, int h, int w,
                                                             unsigned char* __restrict__ out) {
    const long long total = (long long)h * batch * w;
    const long long g0 = ((long long)blockIdx.x * S360_BLOCK + threadIdx.x) * 4;
    if (g0 >= total) return;
    const int cnt = total - g0 < 4 ? (int)(total - g0) : 4;
    const long long row = (long long)batch * w, plane = (long long)h * w;
    unsigned char bytes[4 * C];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long g = g0 + (j < cnt ? j : 0);
        const long long y = g / row, bx = g - y * row;
        const long long bi = bx / w, x = bx - bi * w;
        const float* src = image + ((size_t)bi * channels) * plane + (size_t)y * w + (size_t)x;
#pragma unroll
        for (int c = 0; c < C; ++c) bytes[j * C + c] = vs_byte(src[channels == 1 ? 0 : (size_t)c * plane]);
    }
    unsigned char* dst = out + (size_t)g0 * C;
    if (cnt == 4 && ((uintptr_t)out & 3) == 0) {
#pragma unroll
        for (int q = 0; q < C; ++q)
            reinterpret_cast<unsigned*>(dst)[q] = (unsigned)bytes[q * 4] | ((unsigned)bytes[q * 4 + 1] << 8) | ((unsigned)bytes[q * 4 + 2] << 16) |
                                                  ((unsigned)bytes[q * 4 + 3] << 24);
    } else {
#pragma unroll
        for (int q = 0; q < 4 * C; ++q)
            if (q < cnt * C) dst[q] = bytes[q];
    }
}

static size_t vs_align(size_t x) {
    return (x + 255) & ~(size_t)255;
}

static bool vs_grid(long long total, unsigned& blocks) {     // a thread per 4 elements
    const long long b = (total + 4LL * S360_BLOCK - 1) / (4LL * S360_BLOCK);
    if (b < 1 || !s360_grid_fits(b)) return false;
    blocks = (unsigned)b;
    return true;
}

}  // namespace s360

using namespace s360;

extern "C" int s360_depth_colormap(const float* depth, int32_t n_maps, int32_t height, int32_t width, size_t map_stride, float* rgb_out,
                                   uint8_t* bytes_out, float* range_out, void* workspace, size_t* workspace_bytes, void* stream) {
    if (!workspace_bytes || n_maps < 1 || height < 1 || width < 1) return S360_E_BADARG;
    const long long hw = (long long)height * width;
    if (hw > VS_MAX_ELEMENTS) return S360_E_UNSUPPORTED;
    if (map_stride < (size_t)hw) return S360_E_BADARG;
    const long long total = hw * n_maps;
    unsigned colour_blocks;
    if (!vs_grid(total, colour_blocks)) return S360_E_BADARG;
    long long wgs = (hw + VS_CHUNK - 1) / VS_CHUNK;
    wgs = wgs > VS_MAX_WGS ? VS_MAX_WGS : wgs;
    const long long per = (hw + wgs - 1) / wgs;
    const long long blocks = wgs * n_maps;
    if (!s360_grid_fits(blocks)) return S360_E_BADARG;
    // workspace: counts | state after digit 1 | state after digit 2 | records | partials of digit 1 | digit 2 | digit 3
    const size_t o_counts = 0;
    const size_t o_state1 = o_counts + vs_align((size_t)blocks * sizeof(VsCounts));
    const size_t o_state2 = o_state1 + vs_align((size_t)n_maps * sizeof(VsState));
    const size_t o_records = o_state2 + vs_align((size_t)n_maps * sizeof(VsState));
    const size_t o_part1 = o_records + vs_align((size_t)n_maps * sizeof(VsRecord));
    const size_t o_part2 = o_part1 + vs_align((size_t)blocks * VS_BINS * sizeof(unsigned));
    const size_t o_part3 = o_part2 + vs_align((size_t)blocks * VS_RANKS * VS_BINS * sizeof(unsigned));
    const size_t need = o_part3 + vs_align((size_t)blocks * VS_RANKS * (VS_BINS / 2) * sizeof(unsigned));
    const int wsr = s360_workspace(workspace, workspace_bytes, need, 16, depth && (rgb_out || bytes_out || range_out));
    if (wsr != S360_WS_READY) return wsr;
    char* ws = (char*)workspace;
    VsCounts* counts = (VsCounts*)(ws + o_counts);
    VsState* state1 = (VsState*)(ws + o_state1);
    VsState* state2 = (VsState*)(ws + o_state2);
    VsRecord* records = (VsRecord*)(ws + o_records);
    unsigned* part1 = (unsigned*)(ws + o_part1);
    unsigned* part2 = (unsigned*)(ws + o_part2);
    unsigned* part3 = (unsigned*)(ws + o_part3);
    VsMapArgs A;
    A.depth = depth, A.map_stride = map_stride, A.n = (unsigned)hw, A.wgs = (int)wgs, A.per = (int)per;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(S360_BLOCK);
    hipLaunchKernelGGL(k_vs_digit1, grid, block, 0, st, A, counts, part1);
    S360_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_vs_digit<2>), grid, block, 0, st, A, (const VsCounts*)counts, (const VsState*)nullptr, (const unsigned*)part1, state1, part2);
    S360_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_vs_digit<3>), grid, block, 0, st, A, (const VsCounts*)counts, (const VsState*)state1, (const unsigned*)part2, state2, part3);
    S360_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vs_record, dim3((unsigned)n_maps), block, 0, st, (int)wgs, (unsigned)hw, (const VsState*)state2, (const unsigned*)part3,
                       records, range_out);
    S360_CHECK_LAUNCH();
    if (rgb_out || bytes_out) {
        VsOut o;
        o.f32 = rgb_out, o.u8 = bytes_out, o.map_id = 0, o.byte_rule = 0, o.f32_first = 1, o.u8_first = 0, o.plane = hw;
        hipLaunchKernelGGL(k_vs_depth_colour, dim3(colour_blocks), block, 0, st, depth, map_stride, hw, total, (const VsRecord*)records, o);
        S360_CHECK_LAUNCH();
    }
    return S360_OK;
}

extern "C" int s360_colorize(const float* x, size_t count, size_t plane, int32_t color_map, int32_t channels_first, float* rgb_out,
                             uint8_t* bytes_out, void* stream) {
    if (!x || (!rgb_out && !bytes_out) || count < 1 || color_map < 0 || color_map > 2) return S360_E_BADARG;
    if (channels_first && (plane < 1 || count % plane != 0)) return S360_E_BADARG;
    unsigned blocks;
    if (count > (size_t)0x7fffffffffffLL || !vs_grid((long long)count, blocks)) return S360_E_BADARG;
    VsOut o;
    o.f32 = rgb_out, o.u8 = bytes_out, o.map_id = color_map, o.byte_rule = 0;
    o.f32_first = o.u8_first = channels_first ? 1 : 0, o.plane = channels_first ? (long long)plane : 1;
    hipLaunchKernelGGL(k_vs_colorize, dim3(blocks), dim3(S360_BLOCK), 0, (hipStream_t)stream, x, (long long)count, o);
    return s360_launch_status();
}

extern "C" int s360_prep_image(const float* image, int32_t batch, int32_t channels, int32_t height, int32_t width, uint8_t* bytes_out,
                               void* stream) {
    if (!image || !bytes_out || batch < 1 || height < 1 || width < 1) return S360_E_BADARG;
    if (channels != 1 && channels != 3 && channels != 4) return S360_E_BADARG;
    unsigned blocks;
    if (!vs_grid((long long)height * batch * width, blocks)) return S360_E_BADARG;
    const hipStream_t st = (hipStream_t)stream;
    if (channels == 4)
        hipLaunchKernelGGL((k_vs_prep_image<4>), dim3(blocks), dim3(S360_BLOCK), 0, st, image, (int)batch, (int)channels, (int)height, (int)width, bytes_out);
    else
        hipLaunchKernelGGL((k_vs_prep_image<3>), dim3(blocks), dim3(S360_BLOCK), 0, st, image, (int)batch, (int)channels, (int)height, (int)width, bytes_out);
    return s360_launch_status();
}

extern "C" int s360_error_map(const float* a, const float* b, int32_t height, int32_t width, uint8_t* bytes_out, void* stream) {
    if (!a || !b || !bytes_out || height < 1 || width < 1) return S360_E_BADARG;
    unsigned blocks;
    const long long hw = (long long)height * width;
    if (!vs_grid(hw, blocks)) return S360_E_BADARG;
    VsOut o;
    o.f32 = nullptr, o.u8 = bytes_out, o.map_id = 1, o.byte_rule = 1, o.f32_first = 0, o.u8_first = 0, o.plane = 1;
    hipLaunchKernelGGL(k_vs_error_map, dim3(blocks), dim3(S360_BLOCK), 0, (hipStream_t)stream, a, b, hw, o);
    return s360_launch_status();
}
