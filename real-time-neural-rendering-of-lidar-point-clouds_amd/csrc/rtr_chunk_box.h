// rtr_chunk_box.h -- the frustum half-spaces and the box of a packed chunk, shared by the point kernel and the host
// (plain C++ apart from the qualifiers: tests/cpp/chunk_box_check.cpp compiles it with g++).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RTR_HD __host__ __device__ inline
#else
#define RTR_HD inline
#endif

namespace rtr {

constexpr uint32_t kPackWideFlag = 1u << 18;  // header widths word: some axis of the chunk needs all 32 bits

// The five half-spaces r.z >= 0, r.x + r.z >= 0, W r.z - r.x >= 0, r.y + r.z >= 0, H r.z - r.y >= 0 (r = the matrix
// rows, m row-major 3 x 4): coefficients pl, |coefficient| row sums plm, |offset| sums pld.
struct FrustumPlanes {
    float pl[5][4], plm[5][3], pld[5];
};
RTR_HD FrustumPlanes frustum_planes(const float m[12], float fW, float fH) {
    FrustumPlanes f;
    const float comb[5][3] = {{0.f, 0.f, 1.f}, {1.f, 0.f, 1.f}, {-1.f, 0.f, fW}, {0.f, 1.f, 1.f}, {0.f, -1.f, fH}};
    for (int q = 0; q < 5; ++q) {
        for (int k = 0; k < 4; ++k) f.pl[q][k] = comb[q][0] * m[k] + comb[q][1] * m[4 + k] + comb[q][2] * m[8 + k];
        for (int k = 0; k < 3; ++k) f.plm[q][k] = __builtin_fabsf(comb[q][0] * m[k]) + __builtin_fabsf(comb[q][1] * m[4 + k]) + __builtin_fabsf(comb[q][2] * m[8 + k]);
        f.pld[q] = __builtin_fabsf(comb[q][0] * m[3]) + __builtin_fabsf(comb[q][1] * m[7]) + __builtin_fabsf(comb[q][2] * m[11]);
    }
    return f;
}
// The same five half-spaces for the pixels of a screen rectangle x0 <= px < x1, y0 <= py < y1 (rtr_select_points): r.z >= 0,
// r.x - (x0 - 1) r.z >= 0, x1 r.z - r.x >= 0 and the same in y -- one pixel of slack on each side, as above (a point
// that lands in column px >= x0 has a quotient >= x0 - 1/2 before rintf).  frustum_planes(m, W, H) is rect_planes(m, 0,
// 0, W, H) bit for bit: 1 - 0 is the 1 of its table.
RTR_HD FrustumPlanes rect_planes(const float m[12], float x0, float y0, float x1, float y1) {
    FrustumPlanes f;
    const float comb[5][3] = {{0.f, 0.f, 1.f}, {1.f, 0.f, 1.f - x0}, {-1.f, 0.f, x1}, {0.f, 1.f, 1.f - y0}, {0.f, -1.f, y1}};
    for (int q = 0; q < 5; ++q) {
        for (int k = 0; k < 4; ++k) f.pl[q][k] = comb[q][0] * m[k] + comb[q][1] * m[4 + k] + comb[q][2] * m[8 + k];
        for (int k = 0; k < 3; ++k) f.plm[q][k] = __builtin_fabsf(comb[q][0] * m[k]) + __builtin_fabsf(comb[q][1] * m[4 + k]) + __builtin_fabsf(comb[q][2] * m[8 + k]);
        f.pld[q] = __builtin_fabsf(comb[q][0] * m[3]) + __builtin_fabsf(comb[q][1] * m[7]) + __builtin_fabsf(comb[q][2] * m[11]);
    }
    return f;
}
// The box [lo, hi] lies entirely on the wrong side of one half-space by more than kBoxSlack x the magnitude of the terms
// involved: no point in it can pass the exact test (see "CULL" in rtr_kernels.hip).  NaN / inf boxes never do.
//   Error argument (u = 2^-24; p a point of the box that the exact test keeps; T the sum of the term magnitudes of the
// rows involved at p, weighted as the half-space weights them; M the real value of m, >= T and >= sum |pl_k p_k| + |pl_3|):
//   - the exact test: each row is one product, two fused multiply-adds and one sum, four roundings of at most u of the
//     row's term magnitudes; a kept point has r.z > 0 and a rounded quotient in [-0.5, W - 0.5] (1 + 3u) on those rows, which
//     lies half a pixel inside the half-spaces' -1 and W: the half-space's real value at p is >= -4.01 u T;
//   - the coefficients pl are sums of up to two rounded terms: <= 2 u of plm each, 2 u M in all;
//   - the box arithmetic: its products round the real ones monotonically, so max(fl(pl lo), fl(pl hi)) >= pl p_k - u |pl p_k|,
//     and the three sums of those maxima err by <= 3.01 u M: v >= -10.1 u M (6.0e-7 M), the computed m >= M (1 - 8 u);
//   - rejection needs v < -2e-6 m, 3.3 times that distance.  The factor is small on purpose: m is the size of the
//     coordinates times the row, so for a cloud kilometres from the origin every further factor in the slack is that many
//     scene units through which the test rejects nothing (tests/README_cameras.md has the counts).  Whoever adds a
//     rounding to the exact test or to the lines below has to add it to this sum.
//   - not covered: a product in the subnormal range carries 2^-150 of absolute error that no multiple of m pays for;
//     it counts where m itself is below ~2^-131 (4e-40).  No matrix and cloud that the tests run come near it.
constexpr float kBoxSlack = 2e-6f;
RTR_HD bool box_outside(const FrustumPlanes &f, const float lo[3], const float hi[3]) {
    bool culled = false;
    for (int q = 0; q < 5; ++q) {
        float v = f.pl[q][3], m = f.pld[q];
        for (int k = 0; k < 3; ++k) {
            const float t0 = f.pl[q][k] * lo[k], t1 = f.pl[q][k] * hi[k];
            v += t0 > t1 ? t0 : t1;
            const float e0 = __builtin_fabsf(lo[k]), e1 = __builtin_fabsf(hi[k]);
            m += f.plm[q][k] * (e0 > e1 ? e0 : e1);
        }
        culled = culled || (v < -kBoxSlack * m);
    }
    return culled;
}
// The box of a packed chunk from its header word {base x, base y, base z, widths} (rtr_kernels.h, PackedXyz).  An axis
// of b <= 25 bits has every value's bit pattern in [base, base | (2^b - 1)]; the sign bit is part of the common prefix,
// so the values lie between the floats of the two ends (swapped when the sign is negative; b = 0: one value).  Lanes
// past the cloud's end hold copies of its last quad, inside the box.  Returns false -- no box: keep the chunk -- for a
// wide chunk (some axis needs 32 bits: mixed signs, NaNs, -0 next to +0) or when an end is inf / NaN (base | mask can
// reach exponent 0xFF; the base then has a smaller one or the same).
RTR_HD bool chunk_box(uint32_t bx, uint32_t by, uint32_t bz, uint32_t widths, float lo[3], float hi[3]) {
    const uint32_t base[3] = {bx, by, bz};
    bool ok = (widths & kPackWideFlag) == 0u;
    for (int a = 0; a < 3; ++a) {
        const uint32_t b = (widths >> (6 * a)) & 31u;  // (<= 25 unless wide)
        const uint32_t top = base[a] | ((1u << b) - 1u);
        ok = ok && (top & 0x7F800000u) != 0x7F800000u;
        const float f0 = __builtin_bit_cast(float, base[a]), f1 = __builtin_bit_cast(float, top);
        const bool neg = (base[a] >> 31) != 0u;
        lo[a] = neg ? f1 : f0;
        hi[a] = neg ? f0 : f1;
    }
    return ok;
}
// The box word of a wide chunk, hdr[2 c + 1].w (round 6).  A chunk that straddles a coordinate plane has an axis without
// a usable prefix -- no box above, so the chunk test kept it and the long path decoded it for nothing.  k_pack_measure
// therefore stores, for the chunk's FIRST wide axis, the smallest and the largest of its values below n as two 16-bit
// truncated floats (the top half of the fp32 pattern): lo in the low half, rounded toward -inf, hi in the high half,
// rounded toward +inf.  0 = no box: the chunk holds a NaN or an infinity below n (on any axis), or a rounded end reaches
// exponent 0xFF.  0 is no real box: lo = hi = +0 means every value is +0 (a -0 among them would make lo -0, see
// float_order_key), and such an axis is not wide.
//   Error argument.  Truncating a pattern to its top 16 bits moves the value toward zero and adding one unit to the
// truncated pattern moves it away from zero past the original (patterns of one sign are ordered like their magnitudes,
// denormals included), so lo16 <= min and hi16 >= max EXACTLY: the interval holds every value, and at most 2^-7 of an
// end's magnitude is given away.  box_outside / clip_box_outside ask no more of a box than that it contains the points
// (see there: the slack covers the arithmetic of the test, and is unchanged).
// (total order of the finite patterns as unsigned keys: -max < ... < -0 < +0 < ... < +max)
RTR_HD uint32_t float_order_key(uint32_t bits) { return bits ^ ((bits >> 31) != 0u ? 0xFFFFFFFFu : 0x80000000u); }
RTR_HD uint32_t float_order_bits(uint32_t key) { return key ^ ((key >> 31) != 0u ? 0x80000000u : 0xFFFFFFFFu); }
// min_bits / max_bits: the patterns of the smallest / largest value (by float_order_key), both finite
RTR_HD uint32_t wide_box_word(uint32_t min_bits, uint32_t max_bits) {
    const uint32_t lo_low = min_bits & 0xFFFFu, hi_low = max_bits & 0xFFFFu;
    // away from zero exactly when that is the direction asked for: lo of a negative, hi of a positive value
    const uint32_t lo16 = (min_bits >> 16) + (((min_bits >> 31) != 0u && lo_low != 0u) ? 1u : 0u);
    const uint32_t hi16 = (max_bits >> 16) + (((max_bits >> 31) == 0u && hi_low != 0u) ? 1u : 0u);
    const bool finite = (lo16 & 0x7F80u) != 0x7F80u && (hi16 & 0x7F80u) != 0x7F80u;
    return finite ? (lo16 | (hi16 << 16)) : 0u;
}
// chunk_box with the box word: the same box for a chunk that is not wide (wbox is not looked at), and for a wide chunk
// with a box word: its first wide axis from the word, every other wide axis (two or three planes straddled: one chunk in
// two thousand) unbounded, the other axes from their prefix as above.  Unbounded = [-FLT_MAX, FLT_MAX]: it holds every
// finite value (the word vouches that the chunk holds no other), 0 x FLT_MAX is 0, not NaN, and a term that overflows
// makes v = +inf or NaN and m = inf, which never reject.  Returns false -- keep the chunk -- for wbox = 0 on a wide chunk.
RTR_HD bool chunk_box(uint32_t bx, uint32_t by, uint32_t bz, uint32_t widths, uint32_t wbox, float lo[3], float hi[3]) {
    const uint32_t base[3] = {bx, by, bz};
    bool ok = (widths & kPackWideFlag) == 0u || wbox != 0u;
    bool first = true;
    for (int a = 0; a < 3; ++a) {
        const uint32_t b = (widths >> (6 * a)) & 63u;  // (<= 25, or 32)
        const bool wide = b == 32u;
        const uint32_t top = base[a] | ((1u << (b & 31u)) - 1u);
        const uint32_t p0 = wide ? (first ? wbox << 16 : 0xFF7FFFFFu) : base[a];
        const uint32_t p1 = wide ? (first ? wbox & 0xFFFF0000u : 0x7F7FFFFFu) : top;
        ok = ok && (p0 & 0x7F800000u) != 0x7F800000u && (p1 & 0x7F800000u) != 0x7F800000u;
        const float f0 = __builtin_bit_cast(float, p0), f1 = __builtin_bit_cast(float, p1);
        const bool neg = !wide && (base[a] >> 31) != 0u;
        lo[a] = neg ? f1 : f0;
        hi[a] = neg ? f0 : f1;
        first = first && !wide;
    }
    return ok;
}

// ---- user clip planes (rtr_set_clip_planes) ----------------------------------------------------------------------
// A point (x, y, z) of the uploaded cloud is kept iff ((a x + b y) + c z) + d >= 0 for every plane {a, b, c, d}, each
// product and sum rounded to fp32 on its own (no FMA: this header is compiled with -ffp-contract=off everywhere).  NaN
// is not >= 0.  For the unit normals of an axis-aligned box ({1, 0, 0, -lo}, {-1, 0, 0, hi}, ...) this is exactly
// lo <= x <= hi: 0 x y and 0 x z are +-0, the sums x + +-0 are x (or +0 for x = -0, which still compares as 0), and
// x - lo rounds to >= 0 exactly when x >= lo (round-to-nearest is monotonic and x - lo = 0 only for x = lo).
// Passed BY VALUE to the point kernels (like Proj); count = 0 never reaches a kernel.
constexpr int kMaxClipPlanes = 8;
struct Clip {
    float p[kMaxClipPlanes][4];
    int count;
};
RTR_HD bool clip_keep(const Clip &c, float x, float y, float z) {
    bool keep = true;
    for (int j = 0; j < c.count; ++j) {
        const float a = c.p[j][0] * x, b = c.p[j][1] * y, s = a + b, cz = c.p[j][2] * z, t = s + cz, v = t + c.p[j][3];
        keep = keep && (v >= 0.f);
    }
    return keep;
}
// The box [lo, hi] lies entirely on the wrong side of one clip plane: no point in it can pass clip_keep.  Same form as
// box_outside -- the largest value of a.p + d over the box, v, against a slack (here 1e-4) x the magnitude of its terms, m,
// plus 2^-126 for products that leave the normal range.  Why no box holding a point p that clip_keep keeps is rejected
// (u = 2^-24, T = |a x| + |b y| + |c z| + |d| of the plane at p, all <= m's real value M):
//   - the point test: each of its three products errs by <= u |term| + 2^-150 (2^-150: a product in the subnormal range;
//     sums carry no absolute error there) and each of its three sums by <= u |partial sum|, so its real value
//     a.p + d >= computed - 3.01 u T - 3 x 2^-150 >= -3.01 u M - 2^-148 (computed >= 0);
//   - the box arithmetic: its products round the real ones monotonically, so max(fl(a lo), fl(a hi)) >= fl(a p_k) >=
//     a p_k - u |a p_k| - 2^-150; the three sums of those maxima err by <= 3.01 u M more, hence
//     v >= a.p + d - 4.02 u M - 2^-148 >= -7.1 u M - 2^-147 (~ -4.3e-7 M), and the computed m is >= M (1 - 7.1 u);
//   - rejection needs v < -1e-4 m - 2^-126, more than 200 times that distance: it never happens.
// NaN (0 x inf, a NaN coefficient) compares false and an infinite box end makes m infinite: neither is ever rejected.
RTR_HD bool clip_box_outside(const Clip &c, const float lo[3], const float hi[3]) {
    bool culled = false;
    for (int j = 0; j < c.count; ++j) {
        float v = c.p[j][3], m = __builtin_fabsf(c.p[j][3]);
        for (int k = 0; k < 3; ++k) {
            const float t0 = c.p[j][k] * lo[k], t1 = c.p[j][k] * hi[k];
            v += t0 > t1 ? t0 : t1;
            const float e0 = __builtin_fabsf(lo[k]), e1 = __builtin_fabsf(hi[k]);
            m += __builtin_fabsf(c.p[j][k]) * (e0 > e1 ? e0 : e1);
        }
        culled = culled || (v < -1e-4f * m - 0x1p-126f);
    }
    return culled;
}
// The box [lo, hi] lies entirely on the kept side of EVERY clip plane: clip_keep keeps each point in it (rtr_select_points
// sets a chunk's 256 bits without reading its coordinates; a frame could skip the per-point test the same way).  The
// mirror image of clip_box_outside -- the SMALLEST value of a.p + d over the box, v = d + sum of min(a_k lo_k, a_k hi_k),
// must exceed the same slack, 1e-4 m + 2^-126.  The error argument above carries over with the signs turned (u = 2^-24,
// M the real value of m, p any point of the box):
//   - the box arithmetic: its products round the real ones monotonically, so min(fl(a lo), fl(a hi)) <= fl(a p_k) <=
//     a p_k + u |a p_k| + 2^-150; the three sums of those minima err by <= 3.01 u M, hence the real a.p + d >=
//     v - 4.02 u M - 2^-148;
//   - the point test: its computed value is >= (a.p + d) - 3.01 u T - 3 x 2^-150 with T <= M, so it is at least
//     v - 7.1 u M - 2^-147, and the computed m is >= M (1 - 7.1 u);
//   - acceptance needs v > 1e-4 m + 2^-126, more than 200 times that distance: the point test's value is > 0, the
//     point is kept.
// Only for boxes whose every point is a number: a packed chunk that has a box (chunk_box) holds no NaN.  NaN (a NaN
// box end) compares false and an infinite end makes m infinite: neither is ever inside.  No plane: every box is inside.
RTR_HD bool clip_box_inside(const Clip &c, const float lo[3], const float hi[3]) {
    bool inside = true;
    for (int j = 0; j < c.count; ++j) {
        float v = c.p[j][3], m = __builtin_fabsf(c.p[j][3]);
        for (int k = 0; k < 3; ++k) {
            const float t0 = c.p[j][k] * lo[k], t1 = c.p[j][k] * hi[k];
            v += t0 < t1 ? t0 : t1;
            const float e0 = __builtin_fabsf(lo[k]), e1 = __builtin_fabsf(hi[k]);
            m += __builtin_fabsf(c.p[j][k]) * (e0 > e1 ? e0 : e1);
        }
        inside = inside && (v > 1e-4f * m + 0x1p-126f);
    }
    return inside;
}

// ---- moving resident points (rtr_transform_points) ---------------------------------------------------------------
// M row-major 3 x 4: a selected point (x, y, z) becomes x' = ((m0 x + m1 y) + m2 z) + m3, y' and z' likewise from rows 1
// and 2, every product and sum rounded to fp32 on its own (no FMA, as clip_keep).  No shortcut for special matrices:
// [I|0] maps -0 to +0 (the last sum adds +0) and an infinite coordinate makes the point's other coordinates NaN (0 x inf),
// exactly what one upload of the moved points computed this way gives.  Passed BY VALUE to the kernel (like Proj).
struct Affine {
    float m[12];
};
RTR_HD void affine_apply(const Affine &a, float &x, float &y, float &z) {
    float o[3];
    for (int r = 0; r < 3; ++r) {
        const float p = a.m[4 * r] * x, q = a.m[4 * r + 1] * y, s = p + q, t = a.m[4 * r + 2] * z, u = s + t;
        o[r] = u + a.m[4 * r + 3];
    }
    x = o[0], y = o[1], z = o[2];
}

// ---- per-point keep mask (rtr_set_point_keep) --------------------------------------------------------------------
// The mask in RESIDENT order: bit r % 32 of words[r / 32] set = resident point r is kept; a 256-point chunk c owns
// words[8 c .. 8 c + 7], and lane l of the wave that holds the chunk (its points 4 l .. 4 l + 3) finds its four bits at
// (l % 8) * 4 .. + 3 of the chunk's word l / 8 (keep_lane_bits).  sum[c] summarises the chunk's points below n: all of
// them hidden (the chunk is rejected with the box tests, before its coordinates are read), all kept (the mask is never
// read for it) or some of each.  Bits at or past n are 0 and do not count.
// Passed BY VALUE to the point kernels (like Clip); words = null never reaches a kernel.
constexpr uint8_t kKeepSome = 0, kKeepNone = 1, kKeepAll = 2;
struct Keep {
    const uint32_t *words;  // [8 x chunks] resident order
    const uint8_t *sum;     // [chunks] kKeepSome / kKeepNone / kKeepAll
};
RTR_HD uint32_t keep_lane_bits(uint32_t word, uint32_t lane) { return (word >> ((lane & 7u) * 4u)) & 15u; }
// the summary of one chunk from its eight words; `valid` = its points below n (1..256)
RTR_HD uint8_t keep_chunk_state(const uint32_t w[8], uint32_t valid) {
    bool any = false, all = true;
    for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t bits = valid >= 32u * (j + 1u) ? 32u : (valid > 32u * j ? valid - 32u * j : 0u);
        if (bits == 0u) break;
        const uint32_t m = bits == 32u ? 0xFFFFFFFFu : (1u << bits) - 1u;
        any = any || (w[j] & m) != 0u;
        all = all && (w[j] & m) == m;
    }
    return !any ? kKeepNone : (all ? kKeepAll : kKeepSome);
}

}  // namespace rtr
