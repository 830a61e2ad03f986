// rtr_voxel_key.h -- the cell of a point in a regular grid (rtr_select_voxel_grid, rtr.h section 6g), shared by the key
// kernel and the host (plain C++ apart from the qualifiers: tests/cpp/voxel_key_check.cpp compiles it with g++).
// The arithmetic contract: per axis t = (p - origin) * inv with the difference and the product each rounded to fp32 on
// its own (-ffp-contract=off), inv = 1.0f / cell computed once on the host.  numpy float32 in that order is exact.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RTR_VOXEL_HD __host__ __device__ inline
#else
#define RTR_VOXEL_HD inline
#endif

namespace rtr {

constexpr uint64_t kVoxelOut = 1ull << 63;  // the point lies in no cell of the grid
constexpr float kVoxelSpan = 1048576.0f;    // 2^20: cells -2^20 .. 2^20 - 1 per axis, 21 bits

// One axis: the cell index + 2^20 (0 .. 2^21 - 1), or a negative number when the point is out of the grid on this axis.
// NaN and +-inf fail both comparisons, as does a difference or a product that overflowed.
RTR_VOXEL_HD int32_t voxel_axis(float p, float origin, float inv) {
    const float d = p - origin;
    const float t = d * inv;
    if (!(t >= -kVoxelSpan && t < kVoxelSpan)) return -1;
    return (int32_t)__builtin_floorf(t) + (1 << 20);  // (floor of -2^20 <= t < 2^20 is exact and fits)
}

// The 63-bit key qx << 42 | qy << 21 | qz of an in-grid point (q = floor(t) + 2^20), or kVoxelOut.  t is monotone
// non-decreasing in the coordinate (a rounded subtraction and a rounded product by a positive number are), so the key's
// fields are too.
RTR_VOXEL_HD uint64_t voxel_key(float x, float y, float z, const float origin[3], const float inv[3]) {
    const int32_t qx = voxel_axis(x, origin[0], inv[0]);
    const int32_t qy = voxel_axis(y, origin[1], inv[1]);
    const int32_t qz = voxel_axis(z, origin[2], inv[2]);
    if ((qx | qy | qz) < 0) return kVoxelOut;
    return ((uint64_t)(uint32_t)qx << 42) | ((uint64_t)(uint32_t)qy << 21) | (uint64_t)(uint32_t)qz;
}

}  // namespace rtr
