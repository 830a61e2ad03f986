// rtr_normal_fit.h -- what a query point of rtr_estimate_normals does on its own (include/rtr_normals.h section 6o), free
// of HIP apart from the qualifiers: the kernel (rtr_normals.hip, k_nb_normal_rows) runs it over a row in LDS,
// tests/cpp/normal_fit_check.cpp over plain arrays with g++ (-ffp-contract=off -fno-fast-math, as the device build).
//
// 1. The row.  A Row is anything with  float d2(uint32_t slot) const,  uint32_t pos(uint32_t slot) const  and
//    void set(uint32_t slot, float d2, uint32_t pos)  over at least k slots; an entry is a candidate's squared distance
//    (finite, >= +0, never -0 and never NaN: float comparisons order them as their bits do) and its POSITION among the
//    sorted records.  The order is (d2, upload index); the index of a position comes from  uint32_t index_of(pos)  and is
//    asked for only where two d2 are equal.  The row is an unordered set while it is filled:
//      * an entry enters a row that is not full in the next free slot;
//      * a full row takes an entry only when it is SMALLER in that order than the row's worst (largest) entry, in the
//        worst entry's slot, and is then scanned once for its new worst (and once more, by index, where the largest d2
//        occurs in several slots).
//    The worst d2 and its slot live in the state (registers): a candidate that is farther costs one comparison.
//    normal_row_sort puts the row in ascending order (insertion sort: the row is short and one lane's own).
// 2. sqrt_rn: the correctly rounded square root of a double, whatever the builtin's lowering gives within one ulp.
// 3. normal_fit: from the nine sums over the row to the normal, the curvature and whether the viewpoint negated the
//    normal -- section 6o's contract, parts 2 and 3, in fp64 with + - * / and sqrt_rn only, every operation rounded on
//    its own.  tests/normals_ref.py states the same thing in numpy float64.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RTR_NFIT_HD __host__ __device__ __forceinline__
#else
#define RTR_NFIT_HD inline
#endif

// (tests/cpp/normal_fit_check.cpp sees every square root through this: x, the builtin's value, the value returned)
#ifndef RTR_SQRT_RN_HOOK
#define RTR_SQRT_RN_HOOK(x, y0, y)
#endif

namespace rtr {

struct NormalRowState {
    uint32_t count = 0;       // the filled slots: 0 .. k
    uint32_t worst_slot = 0;  // the slot of the largest entry among them
    float worst = 0.f;        // ... and its d2
};

// (d2, pos) of the candidate with upload index u into the row of k (>= 1) slots; true when the row was written
template <class Row, class IndexOf>
RTR_NFIT_HD bool normal_row_insert(Row &row, uint32_t k, NormalRowState &st, const IndexOf &index_of, float d2, uint32_t pos, uint32_t u) {
    if (st.count < k) {
        const bool above = st.count == 0u || d2 > st.worst || (d2 == st.worst && u > index_of(row.pos(st.worst_slot)));
        row.set(st.count, d2, pos);
        if (above) st.worst = d2, st.worst_slot = st.count;
        ++st.count;
        return true;
    }
    if (d2 > st.worst) return false;
    if (d2 == st.worst && u > index_of(row.pos(st.worst_slot))) return false;
    row.set(st.worst_slot, d2, pos);
    // the scan for the new worst: first by d2 alone, without a branch and without the position plane, counting the slots
    // that tie with the largest d2; only a row that has such ties is scanned again, with the indices looked up
    float w = row.d2(0);
    uint32_t ws = 0, ties = 0;
    for (uint32_t s = 1; s < k; ++s) {
        const float v = row.d2(s);
        ties = v > w ? 0u : ties + (v == w ? 1u : 0u);
        ws = v > w ? s : ws;
        w = v > w ? v : w;
    }
    if (ties != 0u) {
        uint32_t wu = index_of(row.pos(ws));  // (ws: the first slot that holds w)
        for (uint32_t s = ws + 1u; s < k; ++s) {
            if (row.d2(s) != w) continue;
            const uint32_t su = index_of(row.pos(s));
            if (su > wu) wu = su, ws = s;
        }
    }
    st.worst = w, st.worst_slot = ws;
    return true;
}

// the first `count` slots into ascending order of (d2, upload index)
template <class Row, class IndexOf> RTR_NFIT_HD void normal_row_sort(Row &row, uint32_t count, const IndexOf &index_of) {
    for (uint32_t i = 1; i < count; ++i) {
        const float v = row.d2(i);
        const uint32_t p = row.pos(i);
        uint32_t j = i;
        for (; j > 0; --j) {
            const float below = row.d2(j - 1);
            if (!(below > v || (below == v && index_of(row.pos(j - 1)) > index_of(p)))) break;
            row.set(j, below, row.pos(j - 1));
        }
        if (j != i) row.set(j, v, p);
    }
}

// The square root of x, correctly rounded.  y is the builtin's value; with y- and y+ its neighbours, the exact root
// lies nearer to y+ than to y iff x - y * y+ > 0 and nearer to y- iff x - y * y- <= 0: both products differ from x by a
// multiple of ulp(y)^2 and the midpoints' squares lie ulp(y)^2 / 4 above them, and the residuals are single fma()s, whose
// sign is exact.  One step: the builtin is taken to be within one ulp.  Zero, infinity and NaN pass through, and so does
// an x below 2^-900, where a residual could underflow (normal_fit's arguments are all >= 1 or squares of unit vectors).
RTR_NFIT_HD double sqrt_rn(double x) {
    const double y0 = sqrt(x);
    double y = y0;
    if (x >= 0x1p-900 && x < (double)INFINITY) {
        uint64_t b;
        memcpy(&b, &y0, sizeof b);
        const uint64_t bu = b + 1u, bd = b - 1u;
        double yu, yd;
        memcpy(&yu, &bu, sizeof yu);
        memcpy(&yd, &bd, sizeof yd);
        if (fma(-y0, yu, x) > 0.0) y = yu;
        else if (fma(-y0, yd, x) <= 0.0) y = yd;
    }
    RTR_SQRT_RN_HOOK(x, y0, y);
    return y;
}

// One rotation of the cyclic Jacobi on the symmetric A (app, aqq, apq and the two entries arp, arq of the third index)
// and the columns p, q of V (three rows each).  Everything is a named scalar: nothing here is indexed at run time, so
// that the device build keeps it all in registers.
RTR_NFIT_HD void normal_fit_mix(double c, double s, double &xp, double &xq) {
    const double np = c * xp - s * xq, nq = s * xp + c * xq;
    xp = np, xq = nq;
}
RTR_NFIT_HD void normal_fit_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &vp0, double &vp1, double &vp2,
                                   double &vq0, double &vq1, double &vq2) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double a = theta < 0.0 ? -theta : theta;
    double t = 1.0 / (a + sqrt_rn(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt_rn(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app = app - h, aqq = aqq + h, apq = 0.0;
    normal_fit_mix(c, s, arp, arq);
    normal_fit_mix(c, s, vp0, vq0);
    normal_fit_mix(c, s, vp1, vq1);
    normal_fit_mix(c, s, vp2, vq2);
}

constexpr int kNormalFitSweeps = 8;

// S: the sums of dx, dy, dz over the row; Q: the sums of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz; m = the row's length
// + 1 (>= 3); p: the point; towards: orient the normal towards view[3] (read only then).  normal[3], *curvature: the
// contract's; returns whether the viewpoint rule negated the normal.
RTR_NFIT_HD bool normal_fit(const double S[3], const double Q[6], uint32_t m, const float p[3], bool towards, const float view[3], float normal[3],
                            float *curvature) {
    const double dm = (double)m;
    const double mx = S[0] / dm, my = S[1] / dm, mz = S[2] / dm;
    double a00 = Q[0] / dm - mx * mx, a01 = Q[1] / dm - mx * my, a02 = Q[2] / dm - mx * mz;
    double a11 = Q[3] / dm - my * my, a12 = Q[4] / dm - my * mz, a22 = Q[5] / dm - mz * mz;
    double v00 = 1.0, v10 = 0.0, v20 = 0.0, v01 = 0.0, v11 = 1.0, v21 = 0.0, v02 = 0.0, v12 = 0.0, v22 = 1.0;  // (v<row><column>)
    for (int sweep = 0; sweep < kNormalFitSweeps; ++sweep) {
        normal_fit_rotate(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);  // (p, q, r) = (0, 1, 2)
        normal_fit_rotate(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);  //             (0, 2, 1)
        normal_fit_rotate(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);  //             (1, 2, 0)
    }
    int a = 0;
    double la = a00;
    if (a11 < la) a = 1, la = a11;
    if (a22 < la) a = 2, la = a22;
    const double w0 = a == 0 ? v00 : a == 1 ? v01 : v02, w1 = a == 0 ? v10 : a == 1 ? v11 : v12, w2 = a == 0 ? v20 : a == 1 ? v21 : v22;
    const double L = sqrt_rn((w0 * w0 + w1 * w1) + w2 * w2);
    double n0 = w0 / L, n1 = w1 / L, n2 = w2 / L;
    const double m0 = n0 < 0.0 ? -n0 : n0, m1 = n1 < 0.0 ? -n1 : n1, m2 = n2 < 0.0 ? -n2 : n2;
    double top = n0, mag = m0;  // (the component of largest magnitude, the lowest axis on ties)
    if (m1 > mag) mag = m1, top = n1;
    if (m2 > mag) mag = m2, top = n2;
    if (top < 0.0) n0 = -n0, n1 = -n1, n2 = -n2;
    bool flipped = false;
    if (towards) {
        const double g = (n0 * ((double)view[0] - (double)p[0]) + n1 * ((double)view[1] - (double)p[1])) + n2 * ((double)view[2] - (double)p[2]);
        if (g < 0.0) n0 = -n0, n1 = -n1, n2 = -n2, flipped = true;
    }
    normal[0] = (float)n0, normal[1] = (float)n1, normal[2] = (float)n2;
    const double l0 = a00 > 0.0 ? a00 : 0.0, l1 = a11 > 0.0 ? a11 : 0.0, l2 = a22 > 0.0 ? a22 : 0.0;
    const double sum = (l0 + l1) + l2, lmin = a == 0 ? l0 : a == 1 ? l1 : l2;
    *curvature = sum == 0.0 ? 0.f : (float)(lmin / sum);
    return flipped;
}

}  // namespace rtr
