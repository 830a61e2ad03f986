// rtr_segment_rule.h -- the edge rule of rtr_select_segments (include/rtr_segments.h section 6q) beyond the distance
// test, free of HIP apart from the qualifiers: the kernels (rtr_segments.hip: k_sg_gather, k_sg_link) call it, and
// tests/cpp/segment_rule_check.cpp calls it over plain arrays with g++ (-ffp-contract=off -fno-fast-math, as the device
// build).  Everything is fp32, every product and sum rounded on its own.
//   segment_usable  one compare: curvature <= max_curvature.  A NaN curvature fails; +inf fails any finite limit.
//   segment_dot     (ax * bx + ay * by) + az * bz.  fp32 products commute and the sums pair the same terms from either
//                   end, so the value -- and with it the relation -- is symmetric bit for bit.
//   segment_joined  |dot| >= cos_angle, or with `oriented` dot >= cos_angle.  A NaN dot fails either compare.
// THE ZERO NORMAL.  k_sg_gather replaces the normal of a point that is not usable by (+0, +0, +0) and k_sg_link then
// tests normals alone.  That gives exactly the edges of "both usable and joined", because cos_angle > 0 (the call
// rejects anything else): with one normal zero every product is +-0 or -- against an infinite or NaN component -- NaN,
// so dot is +-0 or NaN; |+-0| = +0 < cos_angle and NaN fails: the pair is not joined, which is what an unusable end asks
// for.  With both ends usable both normals are the caller's and the test is the contract's.  For the same reason a
// point whose normal is section 6o's (+0, +0, +0) joins nothing.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RTR_SEG_HD __host__ __device__ __forceinline__
#else
#define RTR_SEG_HD inline
#endif

namespace rtr {

RTR_SEG_HD bool segment_usable(float curvature, float max_curvature) { return curvature <= max_curvature; }

RTR_SEG_HD float segment_dot(float ax, float ay, float az, float bx, float by, float bz) {
    const float xx = ax * bx, yy = ay * by, zz = az * bz;
    const float xy = xx + yy;
    return xy + zz;
}

RTR_SEG_HD bool segment_joined(float ax, float ay, float az, float bx, float by, float bz, float cos_angle, bool oriented) {
    const float dot = segment_dot(ax, ay, az, bx, by, bz);
    return (oriented ? dot : fabsf(dot)) >= cos_angle;
}

}  // namespace rtr
