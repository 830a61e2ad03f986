// rtr_register_fit.h -- the host half of rtr_register_points (include/rtr_register.h section 6p, part 4): from the sums
// of one call to the rigid step, and the composition of a step with a pose.  Free of HIP apart from the qualifiers:
// rtr_select_api.hip runs it on the host, tests/cpp/register_fit_check.cpp with g++ (-ffp-contract=off -fno-fast-math, as
// the library's build).  fp64 throughout, + - * / and rtr_normal_fit.h's sqrt_rn only, every operation rounded on its
// own, no FMA and no libm trigonometry: tests/register_ref.py states the same thing in numpy float64, bit for bit.
//   register_means      c and the six sums of pass 0 -> moments[0 .. 6]
//   register_fit_point  Horn's quaternion form: the symmetric 4x4 N from the nine cross sums, a fixed cyclic Jacobi,
//                       the eigenvector of the largest diagonal entry, R from the unit quaternion, t = qbar - R pbar
//   register_fit_plane  the 6x6 normal equations by LDL^T without pivoting, R by the Cayley form, t = (pbar - R pbar) + tau
//   register_compose    out = step o pose
//   register_rms        sqrt(residual sum / c)
#pragma once
#include "rtr_normal_fit.h"

#ifndef RTR_REGISTER_MOMENTS
#define RTR_REGISTER_MOMENTS 32
#endif

namespace rtr {

constexpr int kRegisterSweeps = 12;      // the Jacobi's sweeps over the six pairs of the 4x4
constexpr int kRegPointSums = 10;        // pass 1, point-to-point: nine cross sums and the residual
constexpr int kRegPlaneSums = 28;        // pass 1, point-to-plane: 21 + 6 + 1
constexpr int kRegPointResidual = 16;    // moments[] index of sum |p - q|^2
constexpr int kRegPlaneResidual = 31;    // moments[] index of sum b^2

RTR_NFIT_HD void register_identity(double step[12]) {
    for (int i = 0; i < 12; ++i) step[i] = (i % 5 == 0) ? 1.0 : 0.0;  // (3x4 row-major: entries 0, 5, 10)
}

// moments[0] = c, [1 .. 3] = pbar, [4 .. 6] = qbar (all +0 when c == 0); the rest +0.  sums: c, sum p (3), sum q (3)
RTR_NFIT_HD void register_means(const double sums[7], double moments[RTR_REGISTER_MOMENTS]) {
    for (int i = 0; i < RTR_REGISTER_MOMENTS; ++i) moments[i] = 0.0;
    const double c = sums[0];
    moments[0] = c;
    if (c > 0.0)
        for (int a = 0; a < 6; ++a) moments[1 + a] = sums[1 + a] / c;
}

// step o pose: rotation entries ((S_a0 P_0b + S_a1 P_1b) + S_a2 P_2b), translation (that of b = 3) + S_a3
RTR_NFIT_HD void register_compose(const double step[12], const double pose[12], double out[12]) {
    double r[12];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 4; ++b) {
            double v = (step[4 * a] * pose[b] + step[4 * a + 1] * pose[4 + b]) + step[4 * a + 2] * pose[8 + b];
            if (b == 3) v = v + step[4 * a + 3];
            r[4 * a + b] = v;
        }
    for (int i = 0; i < 12; ++i) out[i] = r[i];
}

RTR_NFIT_HD double register_rms(double residual_sum, double c) { return c > 0.0 ? sqrt_rn(residual_sum / c) : (double)INFINITY; }

// t_a = base_a - ((R_a0 p0 + R_a1 p1) + R_a2 p2)
RTR_NFIT_HD void register_put(const double R[9], const double base[3], const double p[3], const double add[3], double step[12]) {
    for (int a = 0; a < 3; ++a) {
        const double rp = (R[3 * a] * p[0] + R[3 * a + 1] * p[1]) + R[3 * a + 2] * p[2];
        step[4 * a] = R[3 * a], step[4 * a + 1] = R[3 * a + 1], step[4 * a + 2] = R[3 * a + 2];
        step[4 * a + 3] = add ? (base[a] - rp) + add[a] : base[a] - rp;
    }
}

// One rotation of the cyclic Jacobi on the symmetric 4x4 A (both triangles kept) and the columns p, q of V: section 6o's
// formula
RTR_NFIT_HD void register_rotate(double A[4][4], double V[4][4], int p, int q) {
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double a = theta < 0.0 ? -theta : theta;
    double t = 1.0 / (a + sqrt_rn(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt_rn(t * t + 1.0), s = t * c;
    const double h = t * apq;
    A[p][p] = A[p][p] - h, A[q][q] = A[q][q] + h, A[p][q] = 0.0, A[q][p] = 0.0;
    for (int r = 0; r < 4; ++r) {
        if (r == p || r == q) continue;
        normal_fit_mix(c, s, A[r][p], A[r][q]);
        A[p][r] = A[r][p], A[q][r] = A[r][q];
    }
    for (int r = 0; r < 4; ++r) normal_fit_mix(c, s, V[r][p], V[r][q]);
}

// A: Horn's N from S (row-major S_ab = sum u_a v_b); runs the sweeps; V: the accumulated rotations
RTR_NFIT_HD void register_horn(const double S[9], double A[4][4], double V[4][4]) {
    const double xx = S[0], xy = S[1], xz = S[2], yx = S[3], yy = S[4], yz = S[5], zx = S[6], zy = S[7], zz = S[8];
    A[0][0] = (xx + yy) + zz, A[0][1] = yz - zy, A[0][2] = zx - xz, A[0][3] = xy - yx;
    A[1][1] = (xx - yy) - zz, A[1][2] = xy + yx, A[1][3] = zx + xz;
    A[2][2] = (yy - xx) - zz, A[2][3] = yz + zy;
    A[3][3] = (zz - xx) - yy;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < i; ++j) A[i][j] = A[j][i];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kRegisterSweeps; ++sweep)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) register_rotate(A, V, p, q);
}

// moments: [0] c, [1 .. 3] pbar, [4 .. 6] qbar, [7 .. 15] S.  Returns true when degenerate (step = the identity)
RTR_NFIT_HD bool register_fit_point(const double moments[RTR_REGISTER_MOMENTS], double step[12]) {
    register_identity(step);
    if (!(moments[0] >= 3.0)) return true;
    double A[4][4], V[4][4];
    register_horn(moments + 7, A, V);
    int k = 0;
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > A[k][k]) k = i;
    double w = V[0][k], x = V[1][k], y = V[2][k], z = V[3][k];
    const double L = sqrt_rn(((w * w + x * x) + y * y) + z * z);
    if (!(L > 0.0) || !(L < (double)INFINITY)) return true;
    w = w / L, x = x / L, y = y / L, z = z / L;
    // sign: w >= 0; with w == 0 the first non-zero of x, y, z is positive
    const bool neg = w < 0.0 || (w == 0.0 && (x < 0.0 || (x == 0.0 && (y < 0.0 || (y == 0.0 && z < 0.0)))));
    if (neg) w = -w, x = -x, y = -y, z = -z;
    const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z),       2.0 * (x * z + w * y),
                         2.0 * (x * y + w * z),       1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                         2.0 * (x * z - w * y),       2.0 * (y * z + w * x),       1.0 - 2.0 * (x * x + y * y)};
    register_put(R, moments + 4, moments + 1, nullptr, step);
    return false;
}

// moments: [0] c, [1 .. 3] pbar, [4 .. 24] the upper triangle of sum a a^T by rows, [25 .. 30] sum a b.  Returns true
// when degenerate
RTR_NFIT_HD bool register_fit_plane(const double moments[RTR_REGISTER_MOMENTS], double step[12]) {
    register_identity(step);
    if (!(moments[0] >= 6.0)) return true;
    double A[6][6], Lm[6][6], W[6][6], d[6], x[6];
    int at = 4;
    for (int r = 0; r < 6; ++r)
        for (int s = r; s < 6; ++s) A[r][s] = A[s][r] = moments[at++];
    for (int j = 0; j < 6; ++j) {  // column by column: W_jk = L_jk d_k, d_j = A_jj - sum_k L_jk W_jk, L_ij = (A_ij - sum_k L_ik W_jk) / d_j
        double v = A[j][j];
        for (int k = 0; k < j; ++k) {
            W[j][k] = Lm[j][k] * d[k];
            v = v - Lm[j][k] * W[j][k];
        }
        if (!(v > 0.0) || !(v < (double)INFINITY)) return true;
        d[j] = v;
        for (int i = j + 1; i < 6; ++i) {
            double u = A[i][j];
            for (int k = 0; k < j; ++k) u = u - Lm[i][k] * W[j][k];
            Lm[i][j] = u / v;
        }
    }
    for (int i = 0; i < 6; ++i) {  // L z = g
        double v = moments[25 + i];
        for (int k = 0; k < i; ++k) v = v - Lm[i][k] * x[k];
        x[i] = v;
    }
    for (int i = 0; i < 6; ++i) x[i] = x[i] / d[i];
    for (int i = 5; i >= 0; --i) {  // L^T x = y
        double v = x[i];
        for (int k = i + 1; k < 6; ++k) v = v - Lm[k][i] * x[k];
        x[i] = v;
    }
    for (int i = 0; i < 6; ++i)
        if (!(x[i] - x[i] == 0.0)) return true;  // (a solution that is not finite)
    const double w0 = x[0] / 2.0, w1 = x[1] / 2.0, w2 = x[2] / 2.0;
    const double m = (w0 * w0 + w1 * w1) + w2 * w2, k = 2.0 / (1.0 + m);
    const double R[9] = {1.0 + k * (w0 * w0 - m), k * (w0 * w1 - w2),       k * (w0 * w2 + w1),
                         k * (w1 * w0 + w2),       1.0 + k * (w1 * w1 - m), k * (w1 * w2 - w0),
                         k * (w2 * w0 - w1),       k * (w2 * w1 + w0),       1.0 + k * (w2 * w2 - m)};
    register_put(R, moments + 1, moments + 1, x + 3, step);
    return false;
}

}  // namespace rtr
