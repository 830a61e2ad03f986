// Host-side check of rtr::clip_box_outside (csrc/rtr_chunk_box.h, the chunk-level rejection of the clip planes) against
// the exact point test rtr::clip_keep: for random planes and boxes -- coefficients and coordinates from 1e-38 to 1e30,
// subnormals, boxes that touch a plane to the last bit, and the boxes rtr::chunk_box gives for random packed headers --
// a box the helper rejects must hold no corner and no sampled point that clip_keep keeps.  Also checks that clip_keep
// of an axis box's six unit-normal planes is exactly lo <= p <= hi.  Prints "ok <boxes> <rejected> <points>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "rtr_chunk_box.h"

static float as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

int main() {
    std::mt19937_64 rng(0xC11Bu);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    auto mag = [&]() -> float {  // a random magnitude 1e-38 .. 1e30 (sometimes subnormal, sometimes 0)
        const int m = (int)(rng() % 16);
        if (m == 0) return 0.f;
        if (m == 1) return as_float((uint32_t)(rng() % 0x00800000u));  // subnormal
        return (float)std::pow(10.0, -38.0 + 68.0 * u01(rng));
    };
    auto sgn = [&](float v) { return (rng() & 1) ? -v : v; };
    long boxes = 0, rejected = 0, points = 0;
    for (int t = 0; t < 400000; ++t) {
        rtr::Clip c{};
        c.count = 1 + (int)(rng() % 3);
        const int scale = (int)(rng() % 4);  // 0: mixed, 1: tiny, 2: huge, 3: unit
        for (int j = 0; j < c.count; ++j) {
            for (int k = 0; k < 3; ++k) {
                float v = scale == 3 ? (float)(2.0 * u01(rng) - 1.0) : mag();
                if (scale == 1) v = (float)(1e-30 * u01(rng));
                if (scale == 2) v = (float)(1e15 * u01(rng));
                c.p[j][k] = sgn(v);
            }
            if (c.p[j][0] == 0.f && c.p[j][1] == 0.f && c.p[j][2] == 0.f) c.p[j][0] = 1.f;
            c.p[j][3] = sgn(mag());
        }
        float lo[3], hi[3];
        const int kind = (int)(rng() % 4);
        if (kind == 3) {  // the box of a random packed chunk header (as the point kernel tests it)
            uint32_t base[3], w[3];
            for (int a = 0; a < 3; ++a) {
                w[a] = (uint32_t)(rng() % 26);
                base[a] = ((uint32_t)rng() & 0xBFFFFFFFu) >> w[a] << w[a];  // (finite: exponent < 0xFF)
            }
            if (!rtr::chunk_box(base[0], base[1], base[2], w[0] | (w[1] << 6) | (w[2] << 12), lo, hi)) continue;
        } else {
            for (int a = 0; a < 3; ++a) {
                float x0 = sgn(mag()), x1 = kind == 0 ? x0 : sgn(mag());
                if (kind == 2) x1 = std::nextafter(x0, (rng() & 1) ? INFINITY : -INFINITY);
                lo[a] = x0 < x1 ? x0 : x1;
                hi[a] = x0 < x1 ? x1 : x0;
            }
            if (kind == 2 && c.count == 1) {  // a plane through (about) a corner of the box: decided by rounding
                const float a = c.p[0][0] * lo[0], b = c.p[0][1] * lo[1], s = a + b, cz = c.p[0][2] * lo[2], v = s + cz;
                c.p[0][3] = -v;
                if (!std::isfinite(c.p[0][3])) continue;
            }
        }
        ++boxes;
        if (!rtr::clip_box_outside(c, lo, hi)) continue;
        ++rejected;
        for (int s = 0; s < 8 + 24; ++s) {
            float p[3];
            for (int a = 0; a < 3; ++a) {
                if (s < 8) p[a] = ((s >> a) & 1) ? hi[a] : lo[a];
                else {
                    p[a] = (float)((double)lo[a] + ((double)hi[a] - (double)lo[a]) * u01(rng));
                    if (p[a] < lo[a]) p[a] = lo[a];
                    if (p[a] > hi[a]) p[a] = hi[a];
                }
            }
            ++points;
            if (rtr::clip_keep(c, p[0], p[1], p[2])) {
                std::printf("FAIL case %d: box [%a %a %a]-[%a %a %a] rejected, point (%a %a %a) kept\n", t, lo[0], lo[1], lo[2],
                            hi[0], hi[1], hi[2], p[0], p[1], p[2]);
                return 1;
            }
        }
    }
    // axis box: the six unit-normal planes keep exactly lo <= p <= hi (faces, +-0, subnormals, NaN, inf)
    const float vals[] = {0.f, -0.f, 1.f, -1.f, 0.5f, 2.f, as_float(1u), as_float(0x80000001u), as_float(0x007FFFFFu),
                          1e30f, -1e30f, 3.4e38f, -3.4e38f, INFINITY, -INFINITY, NAN, 1.0000001f, 0.99999994f};
    const int nv = (int)(sizeof(vals) / sizeof(vals[0]));
    for (int i = 0; i < 200000; ++i) {
        float lo[3], hi[3], p[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = vals[rng() % 13], hi[a] = vals[rng() % 13];
            if (lo[a] > hi[a]) std::swap(lo[a], hi[a]);
            p[a] = (rng() % 3) ? vals[rng() % nv] : ((rng() & 1) ? lo[a] : hi[a]);
        }
        rtr::Clip c{};
        c.count = 6;
        for (int a = 0; a < 3; ++a) {
            c.p[2 * a][a] = 1.f, c.p[2 * a][3] = -lo[a];
            c.p[2 * a + 1][a] = -1.f, c.p[2 * a + 1][3] = hi[a];
        }
        const bool want = lo[0] <= p[0] && p[0] <= hi[0] && lo[1] <= p[1] && p[1] <= hi[1] && lo[2] <= p[2] && p[2] <= hi[2];
        if (rtr::clip_keep(c, p[0], p[1], p[2]) != want) {
            std::printf("FAIL axis box: p (%a %a %a) box [%a %a %a]-[%a %a %a]\n", p[0], p[1], p[2], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
            return 1;
        }
    }
    std::printf("ok %ld %ld %ld\n", boxes, rejected, points);
    return 0;
}
