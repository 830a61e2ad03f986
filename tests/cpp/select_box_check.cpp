// Host-side check of the two chunk-level decisions rtr_select_points adds (csrc/rtr_chunk_box.h), built with g++
// -ffp-contract=off and linked against the oracle's shared library:
//   1. rtr::clip_box_inside against the exact point test rtr::clip_keep: for random plane sets (axis planes among them),
//      boxes and points of the box -- corners, faces, interior; magnitudes from subnormal to 1e30; planes through a face
//      or a corner of the box to the last bit; the boxes rtr::chunk_box gives for random packed headers -- a box the
//      helper calls inside must hold no point that clip_keep drops;
//   2. rtr::rect_planes + rtr::box_outside against the oracle's projection (orc_project_point): no box they reject holds
//      a corner or a sampled point that the oracle projects onto a pixel of the rectangle;
//   3. rect_planes(m, 0, 0, W, H) equals frustum_planes(m, W, H) bit for bit.
// Prints "ok <cases> <inside boxes> <rect boxes> <rect rejected> <rect points in the rectangle>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "rtr_chunk_box.h"

extern "C" int64_t orc_project_point(const float P[16], float x, float y, float z, int W, int H, uint32_t* depth_bits);

static float as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

int main() {
    std::mt19937_64 rng(0x5E1EC7u);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    auto mag = [&]() -> float {  // a random magnitude 1e-38 .. 1e30 (sometimes subnormal, sometimes 0)
        const int m = (int)(rng() % 16);
        if (m == 0) return 0.f;
        if (m == 1) return as_float((uint32_t)(rng() % 0x00800000u));  // subnormal
        if (m == 2) return 1e30f;
        return (float)std::pow(10.0, -38.0 + 68.0 * u01(rng));
    };
    auto sgn = [&](float v) { return (rng() & 1) ? -v : v; };
    long cases = 0, inside = 0;
    for (int t = 0; t < 1500000; ++t) {
        rtr::Clip c{};
        c.count = 1 + (int)(rng() % 3);
        const int scale = (int)(rng() % 4);  // 0: mixed, 1: tiny, 2: huge, 3: unit
        for (int j = 0; j < c.count; ++j) {
            if (rng() % 5 < 2) {  // an axis plane (the faces of selectBox)
                c.p[j][rng() % 3] = (rng() & 1) ? 1.f : -1.f;
            } else {
                for (int k = 0; k < 3; ++k) {
                    float v = scale == 3 ? (float)(2.0 * u01(rng) - 1.0) : mag();
                    if (scale == 1) v = (float)(1e-30 * u01(rng));
                    if (scale == 2) v = (float)(1e15 * u01(rng));
                    c.p[j][k] = sgn(v);
                }
                if (c.p[j][0] == 0.f && c.p[j][1] == 0.f && c.p[j][2] == 0.f) c.p[j][0] = 1.f;
            }
            c.p[j][3] = scale == 3 ? (float)(8.0 * u01(rng) - 2.0) : sgn(mag());
        }
        float lo[3], hi[3];
        const int kind = (int)(rng() % 5);
        if (kind == 3) {  // the box of a random packed chunk header
            uint32_t base[3], w[3];
            for (int a = 0; a < 3; ++a) {
                w[a] = (uint32_t)(rng() % 26);
                base[a] = ((uint32_t)rng() & 0xBFFFFFFFu) >> w[a] << w[a];
            }
            if (!rtr::chunk_box(base[0], base[1], base[2], w[0] | (w[1] << 6) | (w[2] << 12), lo, hi)) continue;
        } else {
            for (int a = 0; a < 3; ++a) {
                float x0 = scale == 3 ? (float)(4.0 * u01(rng) - 2.0) : sgn(mag());
                float x1 = kind == 0 ? x0 : (scale == 3 ? x0 + (float)(0.5 * u01(rng)) : sgn(mag()));
                if (kind == 2) x1 = std::nextafter(x0, (rng() & 1) ? INFINITY : -INFINITY);
                lo[a] = x0 < x1 ? x0 : x1;
                hi[a] = x0 < x1 ? x1 : x0;
            }
            if (kind == 4 || (kind == 2 && c.count == 1)) {  // plane 0 through a corner / a face of the box: decided by rounding
                float q[3];
                for (int a = 0; a < 3; ++a) q[a] = (rng() & 1) ? lo[a] : hi[a];
                const float a = c.p[0][0] * q[0], b = c.p[0][1] * q[1], s = a + b, cz = c.p[0][2] * q[2], v = s + cz;
                c.p[0][3] = -v;
                if (!std::isfinite(c.p[0][3])) continue;
                if (rng() & 1) c.p[0][3] = std::nextafter(c.p[0][3], (rng() & 1) ? INFINITY : -INFINITY);
            }
        }
        ++cases;
        if (!rtr::clip_box_inside(c, lo, hi)) continue;
        ++inside;
        if (rtr::clip_box_outside(c, lo, hi)) { std::printf("FAIL case %d: inside and outside\n", t); return 1; }
        for (int s = 0; s < 8 + 16; ++s) {
            float p[3];
            for (int a = 0; a < 3; ++a) {
                if (s < 8) p[a] = ((s >> a) & 1) ? hi[a] : lo[a];
                else if (rng() % 4 == 0) p[a] = (rng() & 1) ? lo[a] : hi[a];  // on a face
                else {
                    p[a] = (float)((double)lo[a] + ((double)hi[a] - (double)lo[a]) * u01(rng));
                    if (p[a] < lo[a]) p[a] = lo[a];
                    if (p[a] > hi[a]) p[a] = hi[a];
                }
            }
            if (!rtr::clip_keep(c, p[0], p[1], p[2])) {
                std::printf("FAIL case %d: box [%a %a %a]-[%a %a %a] inside, point (%a %a %a) dropped\n", t, lo[0], lo[1], lo[2],
                            hi[0], hi[1], hi[2], p[0], p[1], p[2]);
                return 1;
            }
        }
    }
    // no plane: every box is inside, also one with NaN ends
    {
        rtr::Clip none{};
        const float l[3] = {NAN, 0.f, -INFINITY}, h[3] = {NAN, 1.f, INFINITY};
        if (!rtr::clip_box_inside(none, l, h) || rtr::clip_box_outside(none, l, h)) { std::printf("FAIL no plane\n"); return 1; }
        rtr::Clip one{};
        one.count = 1, one.p[0][0] = 1.f, one.p[0][3] = 100.f;
        if (rtr::clip_box_inside(one, l, h)) { std::printf("FAIL NaN / inf box called inside\n"); return 1; }
    }

    // 2. + 3.: the rectangle's half-spaces against the oracle's projection
    long rboxes = 0, rrej = 0, rin = 0;
    for (int t = 0; t < 60000; ++t) {
        const int W = (rng() & 1) ? 64 : 1920, H = W == 64 ? 48 : 1080;
        // a camera: focal length 0.8 W, principal point at the centre, a random rotation about y and x, a random position
        const double f = 0.8 * W, ay = 6.2831853 * u01(rng), ax = 0.6 * (u01(rng) - 0.5);
        const double R[3][3] = {{std::cos(ay), 0, std::sin(ay)},
                                {std::sin(ax) * std::sin(ay), std::cos(ax), -std::sin(ax) * std::cos(ay)},
                                {-std::cos(ax) * std::sin(ay), std::sin(ax), std::cos(ax) * std::cos(ay)}};
        const double cpos[3] = {6 * (u01(rng) - 0.5), 3 * (u01(rng) - 0.5), 6 * (u01(rng) - 0.5)};
        float P[16] = {0};
        for (int j = 0; j < 3; ++j) {
            P[j] = (float)(f * R[0][j] + 0.5 * W * R[2][j]);
            P[4 + j] = (float)(f * R[1][j] + 0.5 * H * R[2][j]);
            P[8 + j] = (float)R[2][j];
        }
        const double t0 = -(R[0][0] * cpos[0] + R[0][1] * cpos[1] + R[0][2] * cpos[2]);
        const double t1 = -(R[1][0] * cpos[0] + R[1][1] * cpos[1] + R[1][2] * cpos[2]);
        const double t2 = -(R[2][0] * cpos[0] + R[2][1] * cpos[1] + R[2][2] * cpos[2]);
        P[3] = (float)(f * t0 + 0.5 * W * t2), P[7] = (float)(f * t1 + 0.5 * H * t2), P[11] = (float)t2, P[15] = 1.f;
        if (t % 1000 == 0) {  // 3.
            const rtr::FrustumPlanes a = rtr::frustum_planes(P, (float)W, (float)H), b = rtr::rect_planes(P, 0.f, 0.f, (float)W, (float)H);
            if (std::memcmp(&a, &b, sizeof a) != 0) { std::printf("FAIL rect_planes(0, 0, W, H) != frustum_planes\n"); return 1; }
        }
        int x0 = (int)(rng() % W), x1 = (int)(rng() % W), y0 = (int)(rng() % H), y1 = (int)(rng() % H);
        if (x0 > x1) std::swap(x0, x1);
        if (y0 > y1) std::swap(y0, y1);
        ++x1, ++y1;
        if (rng() % 8 == 0) x0 = 0, y0 = 0, x1 = W, y1 = H;
        const rtr::FrustumPlanes rp = rtr::rect_planes(P, (float)x0, (float)y0, (float)x1, (float)y1);
        for (int b = 0; b < 8; ++b) {
            float lo[3], hi[3];
            const double size = std::pow(10.0, -3.0 + 3.5 * u01(rng));
            for (int a = 0; a < 3; ++a) {
                lo[a] = (float)(12.0 * (u01(rng) - 0.5));
                hi[a] = lo[a] + (float)(size * u01(rng));
            }
            ++rboxes;
            const bool rej = rtr::box_outside(rp, lo, hi);
            rrej += rej;
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
                const int64_t pix = orc_project_point(P, p[0], p[1], p[2], W, H, nullptr);
                const bool in = pix >= 0 && pix % W >= x0 && pix % W < x1 && pix / W >= y0 && pix / W < y1;
                rin += in;
                if (rej && in) {
                    std::printf("FAIL rect case %d: box [%a %a %a]-[%a %a %a] rejected for [%d %d %d %d], point (%a %a %a) lands on %lld\n",
                                t, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], x0, y0, x1, y1, p[0], p[1], p[2], (long long)pix);
                    return 1;
                }
            }
        }
    }
    std::printf("ok %ld %ld %ld %ld %ld\n", cases, inside, rboxes, rrej, rin);
    return 0;
}
