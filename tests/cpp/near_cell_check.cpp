// csrc/rtr_neighbour_cell.h across the edge of the span (rtr.h section 6k), built with plain g++ -ffp-contract=off:
// rtr_select_near asks a cell of the GIVEN point of a pair only, the resident point may lie beyond the span.  Pairs with
// the given end in the last or the first in-span cell of an axis and the resident end up to 3 cells beyond, at several
// radii: every pair the fp32 relation accepts has cells -- the resident one taken by the header's arithmetic without its
// span check -- at most 1 apart on every axis, so a resident point more than one cell out is near nothing, and the cells
// around any other, cut to the span BY CELL INDEX, hold every given point near it.
// Prints "ok <pairs> <accepted> <accepted with the resident end beyond the span> <resident ends more than one cell out>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "rtr_neighbour_cell.h"

using namespace rtr;

static bool accepts(const float a[3], const float g[3], float r2) {
    const float dx = a[0] - g[0], dy = a[1] - g[1], dz = a[2] - g[2];
    const float xx = dx * dx, yy = dy * dy, s = xx + yy, zz = dz * dz, d2 = s + zz;
    return d2 <= r2;
}
// the header's quotient and floor, without the span check
static double cell_of(float p, double h) { return std::floor((double)p / h); }

int main() {
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    const float radii[] = {0.02f, 0.05f, 0.37f, 1.0f, 1.5f, 3e-3f, 250.0f};
    unsigned long long pairs = 0, accepted = 0, accepted_beyond = 0, far_out = 0;
    for (float radius : radii) {
        const double h = neighbour_cell_edge(radius);
        const float r2 = radius * radius;
        for (int side = 0; side < 2; ++side) {
            const double edge = side ? -(double)((1 << 20) - 1) * h : (double)((1 << 20) - 1) * h, sign = side ? -1.0 : 1.0;
            for (int axis = 0; axis < 3; ++axis) {
                for (int it = 0; it < 60000; ++it) {
                    float g[3], a[3];
                    for (int k = 0; k < 3; ++k) g[k] = (float)((u01(rng) - 0.5) * 40.0 * h);
                    g[axis] = (float)(edge - sign * u01(rng) * h);  // the last (first) in-span cell, or just across its faces
                    int kind;
                    if (neighbour_key(g[0], g[1], g[2], h, &kind) == kNbOut) continue;  // (rounded across the edge: no given point)
                    // the resident end: within about a radius of g off the axis, from one cell inside to three beyond on it
                    for (int k = 0; k < 3; ++k) a[k] = (float)((double)g[k] + (u01(rng) - 0.5) * 1.2 * (double)radius);
                    const int mode = it % 4;
                    if (mode == 0) a[axis] = (float)(edge + sign * (u01(rng) * 4.0 - 1.0) * h);
                    else if (mode == 1) a[axis] = (float)((double)g[axis] + sign * (double)radius * (1.0 + (u01(rng) - 0.5) * 1e-6));
                    else if (mode == 2) a[axis] = std::nextafter((float)((double)g[axis] + sign * (double)radius), sign > 0 ? INFINITY : -INFINITY);
                    else a[axis] = (float)((double)g[axis] + sign * u01(rng) * (double)radius);
                    if (mode != 0 && it % 8 < 4) a[(axis + 1) % 3] = g[(axis + 1) % 3], a[(axis + 2) % 3] = g[(axis + 2) % 3];
                    ++pairs;
                    bool beyond = false, far = false;
                    double apart = 0.0;
                    for (int k = 0; k < 3; ++k) {
                        const double qa = cell_of(a[k], h), qg = cell_of(g[k], h);
                        beyond = beyond || qa < (double)kNbCellMin || qa > (double)kNbCellMax;
                        far = far || qa < (double)kNbCellMin - 1.0 || qa > (double)kNbCellMax + 1.0;
                        apart = std::fmax(apart, std::fabs(qa - qg));
                    }
                    far_out += far;
                    if (!accepts(a, g, r2)) continue;
                    ++accepted;
                    accepted_beyond += beyond;
                    if (apart > 1.0 || far) {
                        printf("FAIL radius %a: resident (%a %a %a) given (%a %a %a) accepted with cells %g apart\n", radius, a[0], a[1], a[2],
                               g[0], g[1], g[2], apart);
                        return 1;
                    }
                    if (accepts(g, a, r2) != true) {  // (the direction of the subtraction does not matter)
                        printf("FAIL: the relation is not symmetric\n");
                        return 1;
                    }
                }
            }
        }
    }
    printf("ok %llu %llu %llu %llu\n", pairs, accepted, accepted_beyond, far_out);
    return 0;
}
