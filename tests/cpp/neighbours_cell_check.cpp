// neighbours_cell_check.cpp -- csrc/rtr_neighbour_cell.h compiled by plain g++ (-ffp-contract=off -fno-fast-math) as a
// stand-alone program: a few million random and adversarial pairs of points, at magnitudes from 1e-3 to the end of the
// grid's span, and for every pair that the fp32 neighbour relation of rtr.h section 6h accepts the two cells differ by at
// most 1 on every axis and the second point's key lies in one of the 9 key ranges of the first point's cell.
// Prints "ok <pairs> <accepted> <accepted in different cells> <accepted at the relation's edge>" or the failing pair.
#include "rtr_neighbour_cell.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)

float step(float v, int ulps) {
    for (int k = 0; k < (ulps < 0 ? -ulps : ulps); ++k) v = std::nextafterf(v, ulps < 0 ? -INFINITY : INFINITY);
    return v;
}

bool accepted(const float p[3], const float q[3], float r2) {
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 <= r2;
}

struct Tally {
    uint64_t pairs = 0, accepted = 0, apart = 0, edge = 0, out = 0;
};

// 0: fine or not a pair to judge; 1: failed (printed)
int judge(const float p[3], const float q[3], float radius, Tally& t) {
    const float r2 = radius * radius;
    const double h = rtr::neighbour_cell_edge(radius);
    ++t.pairs;
    int kp, kq;
    const uint64_t a = rtr::neighbour_key(p[0], p[1], p[2], h, &kp), b = rtr::neighbour_key(q[0], q[1], q[2], h, &kq);
    if (kp || kq) {
        ++t.out;
        return 0;
    }
    if (!accepted(p, q, r2)) return 0;
    if (accepted(q, p, r2) != true) {
        printf("FAIL the relation is not symmetric\n");
        return 1;
    }
    ++t.accepted;
    bool differ = false;
    for (int k = 0; k < 3; ++k) {
        const int64_t ca = (int64_t)((a >> (21 * (2 - k))) & 0x1FFFFF), cb = (int64_t)((b >> (21 * (2 - k))) & 0x1FFFFF);
        differ |= ca != cb;
        if (ca - cb > 1 || cb - ca > 1 || ca != rtr::neighbour_axis(p[k], h) || ca < 1 || ca > (1 << 21) - 2) {
            printf("FAIL radius %.9g axis %d: %.9g in cell %lld, %.9g in cell %lld\n", radius, k, p[k], (long long)ca - (1 << 20), q[k],
                   (long long)cb - (1 << 20));
            return 1;
        }
    }
    t.apart += differ;
    bool in_range = false;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            in_range |= b >= rtr::neighbour_key_offset(a, dx, dy, -1) && b <= rtr::neighbour_key_offset(a, dx, dy, 1);
    if (!in_range) {
        printf("FAIL radius %.9g: key %llx lies in none of the 9 ranges of key %llx\n", radius, (unsigned long long)b, (unsigned long long)a);
        return 1;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t per_kind = argc > 1 ? strtoull(argv[1], nullptr, 10) : 60000;
    const float radii[] = {1e-3f, 0.02f, 0.05f, 0.3f, 1.0f, 37.5f, 1e4f, 3e-12f, 1.5e18f};
    Tally t;
    for (float radius : radii) {
        const double h = rtr::neighbour_cell_edge(radius);
        const double span = (double)radius * 1048576.0;  // the span the header promises: +-2^20 radius
        const float far = step((float)span, -1);
        for (int kind = 0; kind < 6; ++kind) {
            for (uint64_t it = 0; it < per_kind; ++it) {
                // a base point: magnitudes log-uniform from 1e-3 radius (and 1e-3 absolute for radius 1) to the span
                float p[3], q[3];
                for (int k = 0; k < 3; ++k) {
                    const double mag = std::exp(std::log(1e-3 * radius) + uni() * (std::log(span) - std::log(1e-3 * radius)));
                    p[k] = (float)((rnd() & 1) ? -mag : mag);
                    if ((rnd() & 63) == 0) p[k] = (rnd() & 1) ? far : -far;  // the last floats of the span
                    if ((rnd() & 63) == 1) p[k] = (rnd() & 1) ? 0.f : -0.f;
                }
                const int axis = (int)(rnd() % 3);
                if (kind >= 3) {  // straddling a multiple of h, across 0 included: p a few ulp off m h
                    const int64_t m = (int64_t)(uni() * uni() * 2097100.0) - (kind == 5 ? 3 : 1048550);
                    p[axis] = step((float)((double)m * h), (int)(rnd() % 9) - 4);
                }
                memcpy(q, p, sizeof q);
                const float sign = (rnd() & 1) ? 1.f : -1.f;
                switch (kind) {
                case 0:  // anywhere within 1.2 radius on every axis
                    for (int k = 0; k < 3; ++k) q[k] = p[k] + (float)((uni() * 2.4 - 1.2) * radius);
                    break;
                case 1:  // exactly radius apart on one axis (as far as fp32 can say), the others equal or a whisker off
                    q[axis] = p[axis] + sign * radius;
                    if (rnd() & 1) q[(axis + 1) % 3] = step(p[(axis + 1) % 3], (int)(rnd() % 3) - 1);
                    break;
                case 2:  // 1 .. 4 ulp on either side of that
                    q[axis] = step(p[axis] + sign * radius, (int)(rnd() % 9) - 4);
                    break;
                case 3:
                case 5:  // the partner up to radius away on the straddled axis, +- a few ulp
                    q[axis] = step(p[axis] + sign * (float)(uni() * radius), (int)(rnd() % 5) - 2);
                    if (rnd() & 1) q[axis] = step(p[axis] + sign * radius, (int)(rnd() % 5) - 2);
                    break;
                case 4:  // a diagonal of length about radius
                {
                    double d[3] = {uni() - 0.5, uni() - 0.5, uni() - 0.5};
                    const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-30;
                    for (int k = 0; k < 3; ++k) q[k] = p[k] + (float)(d[k] / len * radius * (1.0 + (uni() - 0.5) * 1e-6));
                    break;
                }
                }
                const uint64_t before = t.accepted;
                if (judge(p, q, radius, t)) return 1;
                if (t.accepted != before && kind != 0) ++t.edge;
            }
        }
    }
    // the documented ends of the span, and what lies beyond
    const double h1 = rtr::neighbour_cell_edge(1.0f);
    if (rtr::neighbour_axis(1048576.0f, h1) < 0 || rtr::neighbour_axis(-1048576.0f, h1) < 0 || rtr::neighbour_axis(1.0497e6f, h1) != -1 ||
        rtr::neighbour_axis(-1.0497e6f, h1) != -1 || rtr::neighbour_axis(3.4e38f, h1) != -1 || rtr::neighbour_axis(INFINITY, h1) != -2 ||
        rtr::neighbour_axis(-INFINITY, h1) != -2 || rtr::neighbour_axis(NAN, h1) != -2 || rtr::neighbour_axis(0.f, h1) != (1 << 20) ||
        rtr::neighbour_axis(-0.f, h1) != (1 << 20) || rtr::neighbour_axis(-1e-30f, h1) != (1 << 20) - 1) {
        printf("FAIL the ends of the span\n");
        return 1;
    }
    int kind = 0;
    if (rtr::neighbour_key(0.f, NAN, 3e38f, h1, &kind) != rtr::kNbOut || kind != 2 || rtr::neighbour_key(0.f, 1.f, 3e38f, h1, &kind) != rtr::kNbOut ||
        kind != 1) {
        printf("FAIL the kinds\n");
        return 1;
    }
    printf("ok %llu %llu %llu %llu %llu\n", (unsigned long long)t.pairs, (unsigned long long)t.accepted, (unsigned long long)t.apart,
           (unsigned long long)t.edge, (unsigned long long)t.out);
    return 0;
}
