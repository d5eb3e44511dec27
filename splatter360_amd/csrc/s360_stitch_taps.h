// s360_stitch_taps.h — the float32 expressions of the cube -> equirectangular stitch's sampling position, shared by
// s360_stitch.hip (the stand-alone stitch and its adjoint) and s360_mono_fusion.hip (the stitch fused into the mono-feature
// fusion), so that every kernel that takes a tap forms the same corner and the same weights, bit for bit.
#pragma once
#include "s360_device.h"

namespace s360 {

__device__ __forceinline__ float unnorm_clip(float g, int size) {
    float i = ((g + 1.0f) / 2.0f) * (float)(size - 1);
    return fminf((float)(size - 1), fmaxf(i, 0.0f));
}

// Corner (x0, y0, z0) and the per-axis weights of pixel i: shared by both kernels so the adjoint's weights are the forward's bits.
struct StitchFrac {
    int x0, y0, z0;
    float wx[2], wy[2], wz[2];
};

__device__ __forceinline__ StitchFrac stitch_frac(const float* __restrict__ grid, size_t i, int fw) {
    const float ix = unnorm_clip(grid[3 * i], fw), iy = unnorm_clip(grid[3 * i + 1], fw), iz = unnorm_clip(grid[3 * i + 2], 6);
    const float x0f = floorf(ix), y0f = floorf(iy), z0f = floorf(iz);
    const float fx = ix - x0f, fy = iy - y0f, fz = iz - z0f;
    StitchFrac f;
    f.x0 = (int)x0f;
    f.y0 = (int)y0f;
    f.z0 = (int)z0f;
    f.wx[0] = 1.0f - fx;
    f.wx[1] = fx;
    f.wy[0] = 1.0f - fy;
    f.wy[1] = fy;
    f.wz[0] = 1.0f - fz;
    f.wz[1] = fz;
    return f;
}

}  // namespace s360
