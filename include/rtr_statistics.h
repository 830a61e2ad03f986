/* rtr_statistics.h -- analysis calls of librtr_hip.so that take their threshold from the resident cloud itself.  The
 * header continues section 6 of rtr.h (6f - 6m: the selection and analysis calls) and includes it; a program that
 * includes this one needs nothing else.  RTR_ABI_VERSION is rtr.h's and unchanged: the call below adds a symbol and
 * changes no struct and no existing signature. */
#ifndef RTR_STATISTICS_H
#define RTR_STATISTICS_H

#include "rtr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 6n. selection by mean neighbour distance: the statistical outlier filter ---------------------------------------
 * rtr_select_statistical names the resident points whose MEAN DISTANCE to their k nearest neighbours lies at most
 * std_mul standard deviations above the cloud's average of that mean (PCL's StatisticalOutlierRemoval, Open3D's
 * remove_statistical_outlier).  Where section 6h's threshold is absolute, this one adapts to the cloud: the clean-up a
 * scan pipeline runs first.  It writes into RTR_BUF_SELECTION exactly as rtr_select_neighbours does -- the same buffer,
 * the same life, the same five op values with RTR_SELECT_OUTSIDE OR-ed in, bits past n clear.
 * Relation: exactly section 6h's, with the same rounding.  r2 = radius * radius, rounded once to fp32 on the host.  The
 * CANDIDATES of point i are the points j != i (upload indices) with ((dx*dx + dy*dy) + dz*dz) <= r2, every difference,
 * product and sum rounded to fp32 on its own (no FMA, denormals kept); the comparison is inclusive; coincident points
 * are candidates of each other at d2 == +0; a point is never its own candidate (by index, not by position).  Non-finite
 * points have no candidates and are nobody's.  `radius` BOUNDS the search, as in sections 6l and 6m, and is the edge of
 * the internal grid: there is no unbounded search, and a point with fewer than k candidates averages over those it has.
 * EVERY resident point counts: the keep mask, the clip planes and the selection are ignored.
 * Per point: found[i] = min(k, candidates of i).  mean_dist[i] is computed from the found[i] SMALLEST d2 of i's
 * candidates, taken in ascending order of their bits: the fp32 sequential sum s = s + sqrtf(d2), the square root
 * correctly rounded and each addition rounded on its own, then s / (float)found[i], correctly rounded.  Only the
 * multiset of the smallest d2 matters, so no tie rule by index is needed; the d2 are those of section 6m's row for the
 * point itself (k + 1 asked for) with its own index dropped.  found[i] == 0 -- every non-finite point too -- gives +inf
 * (0x7F800000); coincident neighbours give +0.  numpy float32 is a bit-for-bit reference for both arrays: np.sqrt of
 * the sorted d2, np.cumsum in float32, `/`.
 * Moments, in fp64, over the c points with found > 0: mu = S1 / c with S1 the sum of (double)mean_dist[i];
 * sigma = sqrt(S2 / (c - 1)) with S2 the sum of ((double)mean_dist[i] - mu)^2 (two passes, PCL's sample form);
 * sigma = 0 for c < 2, mu = sigma = 0 for c = 0.  t = mu + std_mul * sigma, computed on the host without FMA.  Sum
 * order: both sums are taken over the upload index in a FIXED shape -- blocks of 1024 consecutive indices, inside a
 * block 256 strided sequential sums of four and a binary tree over them, the blocks' sums folded the same way -- that
 * depends on n alone, not on the grid, the timing or the form of the cloud, with no floating-point atomics: packed,
 * "pack" 0 and sorted contexts of one cloud, and repeated calls, return the same bits.  Against any other order of
 * summation (numpy float64) a sum of c non-negative doubles differs by at most (c - 1) * 2^-53 relative.
 * moments (3 doubles, host memory): mu, sigma, t as used.  With RTR_STAT_THRESHOLD_GIVEN the caller's moments[2] is t
 * and std_mul is ignored; mu and sigma are still computed and returned, moments[2] comes back as it was given.
 * hit(i) holds iff found[i] > 0 && (double)mean_dist[i] <= t, with the t returned: this step is exact.  With
 * RTR_SELECT_OUTSIDE hit = !hit for the points below n: the outliers, isolated (found == 0) and non-finite points
 * included -- what a clean-up removes.  op combines the hits with the selection so far as in section 6f.
 * mean_dist, found (each may be NULL on its own): n entries in upload order, host or device memory, told apart as
 * section 6i tells labels.  They and moments are written only when the call succeeds.
 * stats (may be NULL): [0] the points selected after op, [1] hits before RTR_SELECT_OUTSIDE, [2] finite points with
 * found == 0, [3] non-finite points.
 * Independence: the result depends on the coordinates and the upload indices alone -- not on the resident order, the
 * library's sort, the packed form, any option or the internal grid.
 * The internal grid and its SPAN: section 6h's -- every cloud whose finite coordinates lie within +-2^20 * radius of
 * the world origin is covered; a finite coordinate beyond fails the call before anything changes.
 * What it reads and leaves alone: section 6f's list.  The call reads the uploaded coordinates only.  It changes no
 * frame, frame buffer, tile store, pool, statistics, point-pass buffer or keep mask, and an open peer-to-peer exchange
 * stays open.  Indices are the point pass's; a cloud sorted by the library needs option "point_ids" = 1.  A sharded
 * context works on its own points: there are no statistics across shards.
 * Ordering: as section 6h.  Queued on the context's stream behind everything issued before it; the call ALWAYS waits
 * for its own work before it returns (and four times on the way: section 6h's two, and for each of the two sums).
 * Memory and cost: section 6h's sweep, sort, gather and work list, then the pair tests WITHOUT an early exit: one wave
 * per work item, one query point per lane, each lane keeping its k smallest d2 in a row of its own in LDS -- no atomics
 * --, a candidate entering a full row only when it beats the row's worst value (held in a register), followed by one
 * scan of the row for the new worst.  A pile of m coincident or near-coincident points costs O(m^2) pair tests, as in
 * section 6i; so does a radius far larger than the point spacing.  Scratch for the duration of the call: section 6h's
 * plus 8 B per point (the means and found) and 8 B per 1024 points (the partial sums), and in host memory a staging
 * copy of every output that lies in host memory.  Everything is allocated before the first selection word changes.
 * Option keys, read by rtr_get_option after a call: "statistical_us0", "statistical_us1", "statistical_us2" (the key
 * kernel; the sort with the wait for the key kernel's counters; everything from the gather to the hits, the waits for
 * the sums included), "statistical_pair_tests_k" and "statistical_row_updates_k" (the values written into rows), both in
 * thousands.
 * Errors, with nothing changed (the selection, mean_dist, found, moments and stats): section 6h's list -- no cloud, a
 * radius that is not finite and > 0, an r2 that is not a finite normal fp32 number, an unknown op, a sorted cloud
 * without point_ids -> RTR_ERR_INVALID; 2^32 points or more, or a finite coordinate beyond the span ->
 * RTR_ERR_UNSUPPORTED; a failed allocation -> RTR_ERR_HIP -- and, all RTR_ERR_INVALID: k == 0 or k > RTR_STAT_MAX_K; a
 * std_mul that is not finite (without the flag); unknown bits in flags; RTR_STAT_THRESHOLD_GIVEN with moments NULL or
 * with a NaN moments[2].  rtr_last_error names the argument.  The outputs are written through scratch copies, and only
 * on success. */
#define RTR_STAT_MAX_K 64
#define RTR_STAT_THRESHOLD_GIVEN 1   /* flags: moments[2] is read as the threshold t, std_mul is ignored */
int rtr_select_statistical(rtr_ctx *ctx, uint32_t k, float radius, double std_mul, int flags, int op,
                           float *mean_dist,    /* n entries, upload order, host or device, or NULL */
                           uint32_t *found,     /* n entries, upload order, host or device, or NULL */
                           double moments[3],   /* mu, sigma, t; may be NULL without the flag */
                           uint64_t stats[4]);

#ifdef __cplusplus
}
#endif

#endif /* RTR_STATISTICS_H */
