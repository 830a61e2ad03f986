/* rtr_register.h -- registering a scan against the resident cloud, computed by librtr_hip.so on the device.  The header
 * continues section 6 of rtr.h (6f - 6m), of rtr_statistics.h (6n) and of rtr_normals.h (6o) and includes rtr.h; a program
 * that includes this one needs nothing else.  RTR_ABI_VERSION is rtr.h's and unchanged: the call below adds a symbol and
 * changes no struct and no existing signature. */
#ifndef RTR_REGISTER_H
#define RTR_REGISTER_H

#include "rtr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 6p. registration: one ICP step of given points against the resident cloud ---------------------------------------
 * rtr_register_points finds for every GIVEN point, moved by `pose`, the nearest resident point within `radius`, sums the
 * moments of those pairs on the device and returns the rigid STEP that best moves the posed points onto their partners:
 * point-to-point (Horn's closed form) or, with RTR_REGISTER_POINT_TO_PLANE, point-to-plane with the resident points'
 * normals (section 6o writes them where this call reads them).  It is a pure ANALYSIS call like sections 6l and 6o: it
 * reads the uploaded coordinates and changes nothing -- the selection is neither read, created nor written, no frame,
 * frame buffer, tile store, pool, frame statistics, point-pass buffer or keep mask is touched, and an open peer-to-peer
 * exchange stays open.  EVERY resident point counts.  The caller's xyz and normals are never written: a loop keeps one
 * scan in device memory and changes only the twelve doubles of the pose.
 * 1. Posed points.  For given point j, in fp64 with every operation rounded on its own and no FMA, p'_a = ((T_a0 * x +
 * T_a1 * y) + T_a2 * z) + T_a3 with T = pose (3x4 row-major), then p' is rounded to fp32.  The fp32 p'_j is both the
 * query point of the search and the p of the sums.  pose NULL: p' is the given point as it is (its bits).
 * 2. Correspondences.  Section 6l's given side on the p': r2 = radius * radius rounded once to fp32 on the host; a
 * resident point is a candidate iff ((dx*dx + dy*dy) + dz*dz) <= r2, every operation in fp32 on its own (no FMA,
 * denormals kept), inclusive; the smallest d2 wins, ties go to the smallest upload index; non-finite p' match nothing and
 * non-finite resident points are nobody's partner.  q_j is the coordinates of the winner, bit for bit; n_j is normals[3 *
 * winner ..].  In plane mode a pair is dropped when its normal has a non-finite component or is exactly (0, 0, 0) (-0
 * counts as 0): the normal section 6o writes beside the curvature +inf.  The pairs that remain are the pairs USED.
 * 3. Sums.  fp64, every operation rounded on its own, no FMA, over the GIVEN index j in section 6n's fixed shape: blocks
 * of 1024 consecutive indices; thread t adds the terms of j = 1024 c + t, + 256, + 512, + 768 in that order, from +0.0;
 * the 64 lanes fold by a butterfly, then the four waves add in order; the blocks' sums fold the same way, thread t taking
 * block t, t + 256, ... in order.  The shape depends on count alone.  No floating-point atomic anywhere.  A given point
 * without a used pair contributes no term, which is the same bits as a +0.0 term.  Two passes:
 * pass 0: c = the sum of 1.0 per used pair (an exact integer), sum p, sum q; on the host pbar = sum p / c and qbar =
 * sum q / c (all +0 when c == 0, and pass 1 is then all +0).
 * pass 1, point-to-point: u = p - pbar, v = q - qbar; the nine S_ab = sum u_a * v_b; E = sum ((d0*d0 + d1*d1) + d2*d2)
 * with d = p - q.
 * pass 1, point-to-plane: u = p - pbar; a = (u1*n2 - u2*n1, u2*n0 - u0*n2, u0*n1 - u1*n0, n0, n1, n2); b = (n0 * (q0 -
 * p0) + n1 * (q1 - p1)) + n2 * (q2 - p2); the 21 sums a_r * a_s with r <= s, the six a_r * b, and sum b * b.
 * moments, point-to-point: [0] c, [1 .. 3] pbar, [4 .. 6] qbar, [7 + 3 a + b] S_ab, [16] E, [17 .. 31] +0.
 * moments, point-to-plane: [0] c, [1 .. 3] pbar, [4 .. 24] the a_r a_s by rows of the upper triangle ((0,0), (0,1), ..
 * (0,5), (1,1), ..), [25 .. 30] the a_r b, [31] sum b * b; qbar is not returned.  The root mean square residual is
 * sqrt(moments[16] / c), or sqrt(moments[31] / c) in plane mode.
 * The result is the same bits for packed, "pack" 0, sorted and hash-ordered contexts of one cloud, for host and device
 * inputs, and on repeated calls.
 * 4. The step, on the host (csrc/rtr_register_fit.h; tests/register_ref.py restates it in numpy float64): fp64, + - * /
 * and a correctly rounded sqrt only, no FMA, no libm trigonometry.
 * Point-to-point: N = the symmetric 4x4 with N00 = (Sxx + Syy) + Szz, N01 = Syz - Szy, N02 = Szx - Sxz, N03 = Sxy - Syx,
 * N11 = (Sxx - Syy) - Szz, N12 = Sxy + Syx, N13 = Szx + Sxz, N22 = (Syy - Sxx) - Szz, N23 = Syz + Szy, N33 = (Szz - Sxx) -
 * Syy.  A = N, V = I; 12 sweeps over (p, q) = (0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3) with section 6o's rotation
 * (skipped when A_pq == 0; theta = (A_qq - A_pp) / (2 A_pq), t = 1 / (|theta| + sqrt(theta * theta + 1)) negated when
 * theta < 0, c = 1 / sqrt(t * t + 1), s = t * c, h = t * A_pq; A_pp -= h, A_qq += h, A_pq = 0; for the two other indices r
 * (ascending) (A_rp, A_rq) <- (c A_rp - s A_rq, s A_rp + c A_rq); the columns p, q of V get the same update in each of
 * their four rows).  The quaternion is the column of V at the largest diagonal entry of A, the first on ties; L =
 * sqrt(((w*w + x*x) + y*y) + z*z); (w, x, y, z) / L; sign: negated when w < 0, and with w == 0 when the first non-zero of
 * x, y, z is negative.  R00 = 1 - 2 (y*y + z*z), R01 = 2 (x*y - w*z), R02 = 2 (x*z + w*y), R10 = 2 (x*y + w*z), R11 = 1 -
 * 2 (x*x + z*z), R12 = 2 (y*z - w*x), R20 = 2 (x*z - w*y), R21 = 2 (y*z + w*x), R22 = 1 - 2 (x*x + y*y); t_a = qbar_a -
 * ((R_a0 * pbar_0 + R_a1 * pbar_1) + R_a2 * pbar_2).
 * Point-to-plane: the 6x6 normal equations (sum a a^T) x = sum a b by LDL^T without pivoting, column j = 0 .. 5: W_jk =
 * L_jk * d_k, d_j = A_jj - L_j0 * W_j0 - .. (k ascending), L_ij = (A_ij - L_i0 * W_j0 - ..) / d_j; forward z_i = g_i -
 * L_i0 * z_0 - .., then z_i / d_i, then backward x_i = y_i - L_(i+1)i * x_(i+1) - .. (k ascending) from i = 5 down; x =
 * (omega, tau).  R is the Cayley form of w = omega / 2: m = (w0*w0 + w1*w1) + w2*w2, k = 2 / (1 + m), R_aa = 1 + k * (w_a
 * * w_a - m), R_01 = k * (w0*w1 - w2), R_02 = k * (w0*w2 + w1), R_10 = k * (w1*w0 + w2), R_12 = k * (w1*w2 - w0), R_20 = k
 * * (w2*w0 - w1), R_21 = k * (w2*w1 + w0): rational, and orthogonal up to rounding.  The step rotates about pbar: t_a =
 * (pbar_a - ((R_a0 * pbar_0 + R_a1 * pbar_1) + R_a2 * pbar_2)) + tau_a.
 * DEGENERATE cases are not errors: c < 3 (point-to-point) or c < 6 (point-to-plane), a pivot d_j that is not finite and
 * > 0, a solution that is not finite, or a quaternion of length 0: step is the identity, stats[3] = 1, and moments is
 * still returned.  A plane -- every normal parallel -- leaves the in-plane motion free: a pivot is exactly 0.
 * step is the 3x4 row-major that moves the POSED points; the new pose is step o pose: rotation part ((S_a0 * P_0b + S_a1 *
 * P_1b) + S_a2 * P_2b), translation (the same with b = 3) + S_a3.  Both facades compose with one function each and loop:
 * registerPoints stops after `iterations` calls, at a degenerate step, or at the first call whose pair count equals the
 * previous call's and whose rms residual did not fall (that call's step is not applied).
 * stats (may be NULL): [0] pairs used, [1] finite posed points without a used pair (beyond radius or, in plane mode, a
 * dropped normal), [2] non-finite posed points, [3] 1 when degenerate.
 * moments, step and stats may each be NULL; they are written only when the call succeeds.
 * xyz: count records of three floats, xyz_stride_bytes apart, in host or device memory, told apart as section 6i tells
 * labels.  normals: 3 n floats in upload order, host or device memory; plane mode only.
 * The internal grid and its SPAN: section 6h's, over the posed points; a finite posed point beyond the span fails the call
 * before anything is written.  Indices are the point pass's; a cloud sorted by the library needs option "point_ids" = 1.
 * A sharded context registers against its own points.
 * Ordering: as section 6l.  Queued on the context's stream behind everything issued before it; the call ALWAYS waits for
 * its own work before it returns (and twice on the way: for the given points' counters and for pass 0).
 * Memory and cost: the pose kernel, section 6l's keys, sort, gather and sweep, one bit per winner set by an integer
 * atomicOr in scratch words (never the context's selection), their popcount scan, ONE extract of the winners'
 * coordinates -- only the chunks that hold a winner are decoded, no fp32 copy of the cloud is built --, and two launches
 * per pass for the sums.  Scratch for the duration of the call: 16 B per given point for the posed records, section 6l's
 * 64 B per given point, 224 B per 1024 given points for the partial sums, 16 B per distinct winner, 8 B per 32 resident
 * points for the winner words and their scan, a staging copy of xyz when it lies in host memory, and 12 B per resident
 * point for normals that lie in host memory.
 * The call adds no option key: rtr_get_option and the context it reads are the frame path's and stay as they are.
 * Errors, with nothing written (moments, step, stats): section 6l's list -- no cloud, a radius that is not finite and
 * > 0, an r2 that is not a finite normal fp32 number, xyz NULL with count > 0, a stride below 12 or not a multiple of 4,
 * a sorted cloud without point_ids -> RTR_ERR_INVALID; 2^32 points or given points or more, or a finite posed point beyond
 * the span -> RTR_ERR_UNSUPPORTED; a failed allocation -> RTR_ERR_HIP -- and, all RTR_ERR_INVALID: unknown bits in flags;
 * RTR_REGISTER_POINT_TO_PLANE with normals NULL; normals given without the flag; a non-finite pose entry.
 * rtr_last_error names the argument. */
#define RTR_REGISTER_POINT_TO_PLANE 1
#define RTR_REGISTER_MOMENTS 32
int rtr_register_points(rtr_ctx *ctx, const float *xyz, size_t xyz_stride_bytes, uint64_t count, float radius, int flags,
                        const double pose[12],      /* 3x4 row-major, or NULL: identity */
                        const float *normals,       /* 3 n floats, upload order, host or device; plane mode only */
                        double moments[RTR_REGISTER_MOMENTS], double step[12], uint64_t stats[4]);

#ifdef __cplusplus
}
#endif

#endif /* RTR_REGISTER_H */
