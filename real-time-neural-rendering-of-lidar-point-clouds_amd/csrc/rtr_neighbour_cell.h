// rtr_neighbour_cell.h -- the cell of a point in the internal grid of rtr_select_neighbours (rtr.h section 6h), shared by
// the key kernel and the host (plain C++ apart from the qualifiers: tests/cpp/neighbours_cell_check.cpp compiles it with
// g++).  The grid is cubic, anchored at the world origin, of edge h = radius * (1 + 2^-10) computed in fp64 (exact: a
// 24-bit by an 11-bit significand), and a coordinate's cell is q = floor(fl64((double)p / h)).
//
// Why two neighbours never lie more than one cell apart on an axis.  The relation of section 6h accepts the pair iff
// fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) <= r2, all in fp32, r2 = fl(radius radius) a normal number.  Rounding is
// monotone and every term is >= 0, so the sum is >= fl(dx dx), hence fl(dx dx) <= r2 <= radius^2 (1 + 2^-24), and with
// the product's own rounding (relative 2^-24, or absolute 2^-150 <= 2^-24 r2 where it is subnormal) and the
// subtraction's (relative 2^-24; exact where subnormal)  |x_i - x_j| <= radius (1 + 2^-22) = h (1 + 2^-22) / (1 + 2^-10)
// < h (1 - 2^-11).  One correctly rounded fp64 division moves each quotient by at most 2^-53 |t| <= 2^-33 inside the
// span, so the two computed quotients differ by less than 1 - 2^-11 + 2^-32 < 1, and the floors of two numbers less
// than 1 apart differ by at most 1.  The same holds for y and z.  (The 6g arithmetic, t = fl32(fl32(p - origin) inv), is
// off by up to 2^20 2^-23 cells and more near the end of the span: not safe here.)
//
// Across the span's edge (rtr_select_near, section 6k: only the GIVEN point of a pair must have a cell).  The argument
// above asks nothing of the span but the size of the quotients: a resident point near a given one has |t| <= 2^20 + 1, so
// the division still moves it by at most 2^-53 |t| < 2^-32, far below the 2^-11 margin, and its floor -- taken without the
// span check -- differs from the given point's cell by at most 1.  A resident point whose floor lies more than one cell
// beyond the span is therefore near no given point, and the cells to look at around any other are q - 1 .. q + 1 cut to
// kNbCellMin .. kNbCellMax BY CELL INDEX: neighbour_key_offset must not be used there, a key field has no room for
// a cell beyond the span.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RTR_NB_HD __host__ __device__ inline
#else
#define RTR_NB_HD inline
#endif

namespace rtr {

constexpr uint64_t kNbOut = 1ull << 63;  // the point has no cell: not finite, or beyond the span
constexpr int32_t kNbBias = 1 << 20;     // a key field is q + 2^20
// the cells of the span: -(2^20 - 1) .. 2^20 - 2 per axis, so that q - 1 and q + 1 still fit a 21-bit field.  Every
// coordinate with |p| <= 2^20 radius lies inside: |p| / h <= 2^20 / (1 + 2^-10) < 2^20 - 1023.
constexpr int32_t kNbCellMin = -(1 << 20) + 1, kNbCellMax = (1 << 20) - 2;

// h of a radius (radius finite and > 0)
RTR_NB_HD double neighbour_cell_edge(float radius) { return (double)radius * (1.0 + 1.0 / 1024.0); }

// One axis: the cell index + 2^20 (1 .. 2^21 - 2), -1 when the coordinate is finite but beyond the span, -2 when it is
// NaN or infinite.
RTR_NB_HD int32_t neighbour_axis(float p, double h) {
    if (!(p - p == 0.0f)) return -2;
    const double t = (double)p / h;
    const double q = __builtin_floor(t);
    if (!(q >= (double)kNbCellMin && q <= (double)kNbCellMax)) return -1;
    return (int32_t)q + kNbBias;
}

// The 63-bit key qx << 42 | qy << 21 | qz of a point with a cell (z in the lowest field: the cells z - 1 .. z + 1 of one
// (x, y) column are one contiguous key range), or kNbOut.  *kind: 0 in the grid, 1 finite and beyond the span on some
// axis, 2 not finite (a non-finite coordinate wins over an axis beyond the span).
RTR_NB_HD uint64_t neighbour_key(float x, float y, float z, double h, int *kind) {
    const int32_t qx = neighbour_axis(x, h), qy = neighbour_axis(y, h), qz = neighbour_axis(z, h);
    if ((qx | qy | qz) < 0) {
        *kind = (qx == -2 || qy == -2 || qz == -2) ? 2 : 1;
        return kNbOut;
    }
    *kind = 0;
    return ((uint64_t)(uint32_t)qx << 42) | ((uint64_t)(uint32_t)qy << 21) | (uint64_t)(uint32_t)qz;
}

// the key of the cell (qx + dx, qy + dy, qz + dz) next to key's cell, |d| <= 1 (the span leaves the room)
RTR_NB_HD uint64_t neighbour_key_offset(uint64_t key, int dx, int dy, int dz) {
    return key + (uint64_t)((int64_t)dx * (1ll << 42) + (int64_t)dy * (1ll << 21) + (int64_t)dz);
}

}  // namespace rtr
