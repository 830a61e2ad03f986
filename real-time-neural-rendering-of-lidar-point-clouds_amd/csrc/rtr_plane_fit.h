// rtr_plane_fit.h -- the host side of rtr_fit_plane (rtr.h section 6j): the sampler, the candidate plane of three points
// and its band.  Plain C++, free of HIP (tests/cpp/plane_fit_check.cpp compiles it with g++); like rtr_voxel_key.h it is
// compiled with -ffp-contract=off -fno-fast-math everywhere, so every product, sum, division and square root below is one
// IEEE operation of its type.  A numpy float64 / uint64 program in the same order is an exact reference
// (tests/planes_ref.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RTR_PLANE_HD __host__ __device__ inline
#else
#define RTR_PLANE_HD inline
#endif

namespace rtr {

// Draw t (t = 3 c + j: candidate c, its point j = 0..2) of the stream `seed`: splitmix64's output function over the state
// seed + (t + 1) * 0x9E3779B97F4A7C15 (all arithmetic modulo 2^64).  The draw's rank in a population of m is z % m.
RTR_PLANE_HD uint64_t plane_draw(uint64_t seed, uint64_t t) {
    uint64_t z = seed + (t + 1u) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

RTR_PLANE_HD bool plane_finite(double v) { return v - v == 0.0; }  // (NaN and +-inf fail)

// The candidate of the sample p0, p1, p2 (fp32 coordinates) with ranks r[0..2]: false = DEGENERATE (two ranks coincide,
// a coordinate is not finite, the normal's length is not finite and > 0, or the offset leaves fp32's range); else plane = {a, b, c, d}, the unit normal
// of the triangle, oriented so that (c, b, a) is lexicographically positive, and the offset through p0, all computed in
// double in the order written here and rounded to fp32 once at the end.
RTR_PLANE_HD bool plane_candidate(const float p0[3], const float p1[3], const float p2[3], const uint64_t r[3], float plane[4]) {
    if (r[0] == r[1] || r[0] == r[2] || r[1] == r[2]) return false;
    for (int k = 0; k < 3; ++k)
        if (!plane_finite((double)p0[k]) || !plane_finite((double)p1[k]) || !plane_finite((double)p2[k])) return false;
    const double x0 = (double)p0[0], y0 = (double)p0[1], z0 = (double)p0[2];
    const double e1x = (double)p1[0] - x0, e1y = (double)p1[1] - y0, e1z = (double)p1[2] - z0;
    const double e2x = (double)p2[0] - x0, e2y = (double)p2[1] - y0, e2z = (double)p2[2] - z0;
    const double ax = e1y * e2z, bx = e1z * e2y, nx = ax - bx;
    const double ay = e1z * e2x, by = e1x * e2z, ny = ay - by;
    const double az = e1x * e2y, bz = e1y * e2x, nz = az - bz;
    const double sx = nx * nx, sy = ny * ny, sxy = sx + sy, sz = nz * nz, s = sxy + sz;
    const double len = __builtin_sqrt(s);
    if (!(plane_finite(len) && len > 0.0)) return false;
    double A[3] = {nx / len, ny / len, nz / len};
    const bool flip = A[2] < 0.0 || (A[2] == 0.0 && (A[1] < 0.0 || (A[1] == 0.0 && A[0] < 0.0)));
    if (flip) A[0] = -A[0], A[1] = -A[1], A[2] = -A[2];
    const double tx = A[0] * x0, ty = A[1] * y0, txy = tx + ty, tz = A[2] * z0, t = txy + tz;
    const double D = -t;
    plane[0] = (float)A[0], plane[1] = (float)A[1], plane[2] = (float)A[2], plane[3] = (float)D;
    return plane_finite((double)plane[3]);  // (an offset beyond fp32's range: no band can be formed, DEGENERATE too)
}

// The band {a, b, c, d_lo, d_hi} of `plane` at distance dist (rtr_count_in_bands): d_lo = d + dist and d_hi = dist - d,
// each one fp32 operation.  rtr_fit_plane counts it, and the facades' selectPlane builds its two section 6d planes
// {a, b, c, d_lo} and {-a, -b, -c, d_hi} from the same two sums.
RTR_PLANE_HD void plane_band(const float plane[4], float dist, float band[5]) {
    band[0] = plane[0], band[1] = plane[1], band[2] = plane[2];
    const float lo = plane[3] + dist, hi = dist - plane[3];
    band[3] = lo, band[4] = hi;
}

}  // namespace rtr
