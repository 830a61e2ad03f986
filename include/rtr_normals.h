/* rtr_normals.h -- per-point geometric attributes of the resident cloud, computed by librtr_hip.so on the device.  The
 * header continues section 6 of rtr.h (6f - 6m) and of rtr_statistics.h (6n) and includes rtr.h; a program that
 * includes this one needs nothing else.  RTR_ABI_VERSION is rtr.h's and unchanged: the call below adds a symbol and
 * changes no struct and no existing signature. */
#ifndef RTR_NORMALS_H
#define RTR_NORMALS_H

#include "rtr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 6o. normals and curvature: PCA over the k nearest neighbours ---------------------------------------------------
 * rtr_estimate_normals gives every resident point the unit normal of the plane fitted to the point and its k nearest
 * neighbours within `radius`, and the surface variation of that neighbourhood (PCL's NormalEstimation, Open3D's
 * estimate_normals): what point-to-plane registration, region growing, shading and meshing consume.  It is a pure
 * ANALYSIS call like sections 6l and 6m: it reads the uploaded coordinates and changes nothing -- not the selection,
 * which is neither read, created nor written, no frame, frame buffer, tile store, pool, frame statistics, point-pass
 * buffer or keep mask, and an open peer-to-peer exchange stays open.  EVERY resident point counts: the keep mask, the
 * clip planes and the selection are ignored.
 * 1. The neighbourhood.  The candidates of point i are section 6n's: section 6h's relation with the same rounding --
 * r2 = radius * radius rounded once to fp32 on the host; the points j != i (upload indices, not positions) with
 * ((dx*dx + dy*dy) + dz*dz) <= r2, every difference, product and sum rounded to fp32 on its own (no FMA, denormals
 * kept); inclusive; coincident points are candidates of each other at d2 == +0.  Non-finite points have no candidates
 * and are nobody's.  `radius` BOUNDS the search and is the edge of the internal grid.  found[i] = min(k, candidates).
 * The ROW of i is its found[i] candidates that are smallest by (d2 bits, upload index), in that order: section 6m's
 * order.  Unlike section 6n the tie rule by index is needed, because which point sits at the row's end changes the
 * answer.  This is section 6m's row for the point itself with k + 1 asked for and its own index dropped.  The
 * neighbourhood is the point itself plus its row: m = found[i] + 1 points (PCL and Open3D count the query point in).
 * 2. The moments.  Everything from here on is fp64, every operation rounded on its own, no FMA.  For row entry t,
 * e_t = (dx, dy, dz) are the three fp32 differences of the pair test (their sign does not matter: every use is even).
 * In row order, starting from +0.0: S_a += (double)e_a and S_ab += (double)e_a * (double)e_b (the product is exact),
 * for the three a and the six a <= b; the point's own term is zero.  mean_a = S_a / m; C_ab = S_ab / m - mean_a * mean_b.
 * 3. The eigenvector, by a fixed cyclic Jacobi that uses + - * / and sqrt only, all correctly rounded, so that numpy
 * float64 restates it exactly (tests/normals_ref.py).  A = C, V = I; 8 sweeps over (p, q) = (0, 1), (0, 2), (1, 2); a
 * rotation is skipped when A_pq == 0; otherwise theta = (A_qq - A_pp) / (2 A_pq), t = 1 / (|theta| + sqrt(theta *
 * theta + 1)) negated when theta < 0, c = 1 / sqrt(t * t + 1), s = t * c, h = t * A_pq; A_pp -= h, A_qq += h, A_pq = 0;
 * with r the third index (A_rp, A_rq) <- (c A_rp - s A_rq, s A_rp + c A_rq); the columns p, q of V get the same
 * two-term update in each of their three rows.  An infinite theta * theta gives t = 0, the identity rotation; no NaN
 * arises from finite input.  lambda is A's diagonal, a the index of the smallest lambda (the first on ties), w column a
 * of V, L = sqrt((w0 w0 + w1 w1) + w2 w2), n = w / L.  Sign: the component of n of largest magnitude (the lowest axis
 * on ties) is made positive; with RTR_NORMAL_VIEWPOINT, g = (n0 * ((double)vp0 - (double)p0) + n1 * (..1)) + n2 * (..2)
 * is then formed and n negated when g < 0 (g == 0 keeps the default sign).  Only then is n rounded to fp32.
 * Curvature is PCL's surface variation: lambda'_b = lambda_b > 0 ? lambda_b : 0, Sigma = (lambda'_0 + lambda'_1) +
 * lambda'_2; curvature = (float)(lambda'_a / Sigma), or +0 when Sigma == 0.  It lies in [0, 1/3].
 * Points with found[i] < RTR_NORMAL_MIN_FOUND -- every non-finite point included -- get the normal (+0, +0, +0) and the
 * curvature +inf (0x7F800000).  DEGENERATE neighbourhoods (collinear, coincident) get whatever the routine yields, and
 * it is still deterministic: an all-zero C gives the normal (1, 0, 0) and the curvature +0; a line gives some unit
 * vector across it.
 * normals (3 n floats: x, y, z of point 0, of point 1, ..), curvature (n floats), found (n entries), each in upload
 * order, each in host or device memory, told apart as section 6i tells labels, and each may be NULL on its own (all
 * NULL: the statistics alone).  They and stats are written only when the call succeeds.
 * stats (may be NULL): [0] points with a normal, [1] finite points with found < RTR_NORMAL_MIN_FOUND, [2] non-finite
 * points, [3] normals negated by the viewpoint rule.
 * Independence: the result depends on the coordinates and the upload indices alone -- not on the resident order, the
 * library's sort, the packed form, any option or the internal grid: packed, "pack" 0 and sorted contexts of one cloud,
 * and repeated calls, return the same bits.  No floating-point atomic anywhere.
 * The internal grid and its SPAN: section 6h's -- every cloud whose finite coordinates lie within +-2^20 * radius of
 * the world origin is covered; a finite coordinate beyond fails the call before anything is written.
 * Indices are the point pass's; a cloud sorted by the library needs option "point_ids" = 1.  A sharded context works on
 * its own points: there are no neighbourhoods across shards.
 * Ordering: as section 6h.  Queued on the context's stream behind everything issued before it; the call ALWAYS waits
 * for its own work before it returns (and twice on the way: section 6h's two).
 * Memory and cost: section 6h's sweep, sort, gather and work list, then section 6n's pair tests: one wave per work
 * item, one query point per lane, each lane keeping its k smallest (d2, position among the sorted records) in a row of
 * its own in LDS -- no atomics --, a candidate entering a full row only when it beats the row's worst entry (its d2 in
 * a register; the upload index is looked up only where two d2 are equal), followed by one scan of the row.  At the end
 * each lane sorts its row, reads its neighbours' coordinates again, forms the sums and runs the 24 rotations.  A pile
 * of m coincident or near-coincident points costs O(m^2) pair tests, as in section 6i; so does a radius far larger
 * than the point spacing.  Scratch for the duration of the call: section 6h's plus 20 B per point (the three outputs),
 * and in host memory a staging copy of every output that lies in host memory.
 * Option keys, read by rtr_get_option after a call: "normals_us0", "normals_us1", "normals_us2" (the key kernel; the
 * sort with the wait for the key kernel's counters; everything from the gather to the normals), "normals_pair_tests_k"
 * and "normals_row_updates_k" (the entries written into rows), both in thousands.
 * Errors, with nothing written (normals, curvature, found, stats): section 6h's list -- no cloud, a radius that is not
 * finite and > 0, an r2 that is not a finite normal fp32 number, a sorted cloud without point_ids -> RTR_ERR_INVALID;
 * 2^32 points or more, or a finite coordinate beyond the span -> RTR_ERR_UNSUPPORTED; a failed allocation ->
 * RTR_ERR_HIP -- and, all RTR_ERR_INVALID: k == 0 or k > RTR_NORMAL_MAX_K; unknown bits in flags;
 * RTR_NORMAL_VIEWPOINT with viewpoint NULL or with a non-finite component.  rtr_last_error names the argument.  The
 * outputs are written through scratch copies, and only on success. */
#define RTR_NORMAL_MAX_K 64
#define RTR_NORMAL_MIN_FOUND 2        /* a normal needs the point and two neighbours */
#define RTR_NORMAL_VIEWPOINT 1        /* flags: orient every normal towards viewpoint[3] */
int rtr_estimate_normals(rtr_ctx *ctx, uint32_t k, float radius, int flags, const float viewpoint[3],
                         float *normals,     /* 3 n floats, upload order, host or device, or NULL */
                         float *curvature,   /* n floats, or NULL */
                         uint32_t *found,    /* n entries, or NULL */
                         uint64_t stats[4]);

#ifdef __cplusplus
}
#endif

#endif /* RTR_NORMALS_H */
