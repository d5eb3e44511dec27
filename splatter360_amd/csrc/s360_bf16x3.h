// s360_bf16x3.h — the one vocabulary of the "high" precision modes: a float32 product as three bf16 products on
// v_mfma_f32_32x32x16_bf16.  Included after s360_device.h by every file that has a "high" mode; a new one includes it and adds
// no arithmetic of its own.
//
// Split.  split(x) = (hi, lo): hi = bf16(x), round-to-nearest-even; lo = bf16(x - float32(hi)).  hi + lo carries 16 bits of x's
// significand; what is dropped is 2^-16 |x| at the most.
// Product.  A B = Ah Bh + Ah Bl + Al Bh, accumulated in float32 by the MFMA over the whole k range.  Al Bl (2^-16 of the
// product) is left out, and no float64 chunk sums are taken: the split's own error is far above a float32 chain's.
// Order.  bx3_mfma3 issues a k-step's three terms as (h, h), (h, l), (l, h) of its (A, B) operands — or, with SWAP, as (h, h),
// (l, h), (h, l).  A kernel that holds a product's operands on the other sides of the MFMA than the forward does (the owner
// that was B is now walked as A) says SWAP, and the terms are then added in one order of the pair as the operator names it —
// (q, k), (g, v), (weight, token side) — whichever side is walked.  float32 addition does not associate, so this order is why
// a backward pass that recomputes a forward's tile, with the operands' roles exchanged, gets it bit for bit — and why the
// order is written here (s360_window_attention.hip's wah_accumulate spells bx3_mfma3<false> out, for the reason it states).
// The B-operand register rule.  The walked index sits on the accumulator's rows and the owner on the lanes, so a score-shaped
// tile is, register by register, the B operand of the next product: registers 8 s .. 8 s + 7 of a lane are k-step s (bx3_split_tile),
// and element j of lane half h is tile row 16 s + 8 (j / 4) + 4 h + j % 4 (mfma_acc_row, s360_device.h).  The A operand's
// elements are read in that order: 4 + 4 consecutive walked indices, 8 apart (bx3_ld44), or 8 consecutive ones of a plane stored in
// that permutation.
#pragma once
#include "s360_device.h"

namespace s360 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void bx3_split(float x, __bf16& hi, __bf16& lo) {
    hi = (__bf16)x;
    lo = (__bf16)(x - (float)hi);
}

__device__ __forceinline__ void bx3_split8(const float* x, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        __bf16 h, l;
        bx3_split(x[j], h, l);
        hi[j] = h;
        lo[j] = l;
    }
}

// the lane's column of a 32 x 32 accumulator tile as the B operand of the next product: two k-steps of 16, split here
__device__ __forceinline__ void bx3_split_tile(const float* t, bf16x8* hi, bf16x8* lo) {
    bx3_split8(t, hi[0], lo[0]);
    bx3_split8(t + 8, hi[1], lo[1]);
}

// 8 consecutive bf16 (p 16-byte aligned)
__device__ __forceinline__ bf16x8 bx3_ld8(const __bf16* p) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p)); }

// the same, or zeros for p == null
__device__ __forceinline__ bf16x8 bx3_ld8_or_zero(const __bf16* p) {
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (p) u = *reinterpret_cast<const uint4*>(p);
    return __builtin_bit_cast(bf16x8, u);
}

// p[0 .. 3] and p[8 .. 11] (p 8-byte aligned): the A fragment that goes with registers 8 s .. 8 s + 7 of an accumulator tile as
// the B operand, p at tile row 16 s + 4 hf
__device__ __forceinline__ bf16x8 bx3_ld44(const __bf16* p) {
    const uint2 u0 = *reinterpret_cast<const uint2*>(p), u1 = *reinterpret_cast<const uint2*>(p + 8);
    return __builtin_bit_cast(bf16x8, make_uint4(u0.x, u0.y, u1.x, u1.y));
}

// the same of a row of n elements (n and g multiples of 4), p = row + g: zeros from n on
__device__ __forceinline__ bf16x8 bx3_ld44(const __bf16* row, int g, int n) {
    uint2 u0 = make_uint2(0u, 0u), u1 = make_uint2(0u, 0u);
    if (g < n) u0 = *reinterpret_cast<const uint2*>(row + g);
    if (g + 8 < n) u1 = *reinterpret_cast<const uint2*>(row + g + 8);
    return __builtin_bit_cast(bf16x8, make_uint4(u0.x, u0.y, u1.x, u1.y));
}

// 8 bf16 to p (16-byte aligned), and a (hi, lo) pair to the same offset o of the two planes of an operand
__device__ __forceinline__ void bx3_st8(__bf16* p, bf16x8 x) { *reinterpret_cast<uint4*>(p) = __builtin_bit_cast(uint4, x); }
__device__ __forceinline__ void bx3_st8(__bf16* hi_plane, __bf16* lo_plane, size_t o, bf16x8 hi, bf16x8 lo) {
    bx3_st8(hi_plane + o, hi);
    bx3_st8(lo_plane + o, lo);
}

__device__ __forceinline__ f32x16 bx3_mfma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

// one k-step of 16: acc += A B in three terms, in THE order (above)
template <bool SWAP>
__device__ __forceinline__ f32x16 bx3_mfma3(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x16 acc) {
    acc = bx3_mfma(ah, bh, acc);
    if constexpr (SWAP) {
        acc = bx3_mfma(al, bh, acc);
        acc = bx3_mfma(ah, bl, acc);
    } else {
        acc = bx3_mfma(ah, bl, acc);
        acc = bx3_mfma(al, bh, acc);
    }
    return acc;
}

__device__ __forceinline__ f32x16 bx3_zero() {
    f32x16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.f;
    return t;
}

// Host: carves the (hi, lo) plane pairs of a call out of its scratch, in the order they are taken.  With a null base nothing is
// written and `off` ends as the bytes the planes need.
struct Bx3Carver {
    char* base;
    size_t off = 0;
    // the next n elements as a hi plane and n as its lo plane: 4 n bytes
    void take(size_t n, __bf16** hi, __bf16** lo) {
        if (base) {
            *hi = reinterpret_cast<__bf16*>(base + off);
            *lo = reinterpret_cast<__bf16*>(base + off + 2 * n);
        }
        off += 4 * n;
    }
};

}  // namespace s360
