// rtr_lane_test.h -- the constants of the point kernel's lane test, computed on the host per frame and per view (plain
// C++: tests/cpp/frustum_general_check.cpp compiles it with g++).  The argument for them stands with the kernel that
// uses them: "LANE TEST" in rtr_kernels.hip.
#pragma once

namespace rtr {

struct LaneTest {
    float lz, lall, zsafe, zfront;
};
// m: rows 0..2 of the row-major camera matrix (Proj::m); absmax: the largest |x|, |y|, |z| of the resident cloud
inline LaneTest lane_test_consts(const float m[12], int W, int H, const float absmax[3]) {
    LaneTest t;
    const float l1x = __builtin_fabsf(m[0]) + __builtin_fabsf(m[1]) + __builtin_fabsf(m[2]), l1y = __builtin_fabsf(m[4]) + __builtin_fabsf(m[5]) + __builtin_fabsf(m[6]);
    const float l1z = __builtin_fabsf(m[8]) + __builtin_fabsf(m[9]) + __builtin_fabsf(m[10]);
    const float hi = (float)(W > H ? W : H) + 0.25f;
    t.lz = l1z * 1.001f;
    t.lall = ((l1x > l1y ? l1x : l1y) + hi * l1z) * 1.001f;
    auto mag = [&](int r) { return __builtin_fabsf(m[4 * r]) * absmax[0] + __builtin_fabsf(m[4 * r + 1]) * absmax[1] + __builtin_fabsf(m[4 * r + 2]) * absmax[2] + __builtin_fabsf(m[4 * r + 3]); };
    const float rx = mag(0), ry = mag(1), rz = mag(2);
    t.zsafe = 0x1p-18f * ((rx > ry ? rx : ry) + hi * rz);
    t.zfront = 0x1p-20f * rz;
    if (!(t.zsafe >= 1e-30f)) t.zsafe = __builtin_inff();  // (NaN / no finite box: the margin step never applies)
    if (!(t.zfront < 3e38f)) t.zfront = __builtin_inff();  // (... nor does the front step)
    if (!(t.lz < 3e38f) || !(t.lall < 3e38f)) t.zsafe = t.zfront = __builtin_inff(), t.lz = t.lall = 3e38f;
    return t;
}

}  // namespace rtr
