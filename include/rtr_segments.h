/* rtr_segments.h -- selecting the resident points by smooth surface segment, computed by librtr_hip.so on the device.
 * The header continues section 6 of rtr.h (6f - 6m), rtr_statistics.h (6n), rtr_normals.h (6o) and rtr_register.h (6p)
 * and includes rtr.h; a program that includes this one needs nothing else.  RTR_ABI_VERSION is rtr.h's and unchanged:
 * the call below adds a symbol and changes no struct and no existing signature. */
#ifndef RTR_SEGMENTS_H
#define RTR_SEGMENTS_H

#include "rtr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 6q. selection by smooth segment: region growing over normals ---------------------------------------------------
 * rtr_select_segments names the resident points by the size of the smooth surface segment they belong to (PCL's
 * RegionGrowing in an exact, order-free form): section 6i's clusters with an edge kept only where the two points'
 * normals agree and both points are smooth enough.  Where walls, floor and ceiling touch, section 6i sees one giant
 * cluster; this call sees the faces.  The normals and the curvature are the caller's -- section 6o writes them in the
 * very layout read here, into host or device memory -- and are never written.  The call writes into
 * RTR_BUF_SELECTION exactly as section 6i does.
 * The edge relation.  Points i != j (upload indices) are JOINED iff all of
 *   1. they are section 6h neighbours, exactly: r2 = radius * radius rounded once to fp32 on the host, then
 *      ((dx*dx + dy*dy) + dz*dz) <= r2 in fp32, every difference, product and sum rounded on its own (no FMA),
 *      inclusive; coincident points are neighbours; non-finite points are nobody's neighbour;
 *   2. both are USABLE: usable(i) holds when curvature == NULL or curvature[i] <= max_curvature -- one fp32 compare.  A
 *      NaN curvature fails it, and section 6o's +inf for a point without a normal fails any finite limit
 *      (max_curvature = +inf admits +inf; -inf admits only -inf);
 *   3. dot = (nx_i * nx_j + ny_i * ny_j) + nz_i * nz_j in fp32, every product and sum rounded on its own, no FMA;
 *      fp32 products commute, so dot is the same from either end and the relation is symmetric.  The pair passes iff
 *      fabsf(dot) >= cos_angle, or with RTR_SEGMENT_ORIENTED iff dot >= cos_angle.  A NaN dot fails.  Because
 *      cos_angle > 0, section 6o's zero normal (found < RTR_NORMAL_MIN_FOUND) joins nothing.  Normals are NOT checked
 *      for unit length: the relation is whatever this arithmetic says.
 * Segments: the connected components of that relation over all n resident points.  A segment's LABEL is the smallest
 * upload index in it; a point with no joined partner -- every non-finite point, every unusable point -- is a segment
 * of one, labelled by its own index.  numpy float32 in this order with any correct component labelling is a
 * bit-for-bit reference (tests/segments_ref.py): nothing here has a tolerance.
 * Everything else is section 6i's, word for word, with "segment" for "cluster": the hit rule (min_points, max_points,
 * RTR_SEGMENT_SEEDED as RTR_CLUSTER_SEEDED with the seeds read before op is applied, RTR_SELECT_OUTSIDE, the five op
 * values); labels (may be NULL; n uint32_t in host or device memory, told apart as there; written only on success);
 * stats (may be NULL): [0] the points selected after op, [1] segments, [2] segments that hit (before OUTSIDE), [3] the
 * points of the largest segment; the independence from the resident order, the library's sort, the packed form, any
 * option and the internal grid; the grid's SPAN; what the call reads and leaves alone (the uploaded coordinates and,
 * when seeded, the selection; no frame, frame buffer, tile store, pool, statistics, point-pass buffer, keep mask or
 * clip plane, and an open peer-to-peer exchange stays open); the ordering and the waits (queued on the context's stream
 * behind everything issued before it; the call ALWAYS waits for its own work before it returns, and twice on the way).
 * normals and curvature are read between the call's start and its return; arrays in host memory are copied to the
 * device first.
 * Memory and cost: section 6i's, plus one gather that builds a 16-byte normal record per sorted position -- the normal
 * of the point there, or (+0, +0, +0) when the point is not usable, which joins nothing because cos_angle > 0, so the
 * curvature test is paid once per point and not per pair -- and, per pair test, three more broadcasts and five fp32
 * operations.  Scratch on top of section 6i's: those records and a staging copy of each input array that lies in host
 * memory, at most 32 B per point (16 + 12 + 4).  The call adds no option key: the stage times and the pair tests of
 * sections 6h and 6i are not touched by it.
 * Errors, with nothing changed: section 6i's list in full (no cloud, radius, r2, min_points, max_points, an unknown op,
 * a sorted cloud without point_ids -> RTR_ERR_INVALID; 2^32 points or more, or a finite coordinate beyond the span ->
 * RTR_ERR_UNSUPPORTED; a failed allocation -> RTR_ERR_HIP) and, all RTR_ERR_INVALID: a cos_angle that is not finite,
 * <= 0 or > 1; normals == NULL; curvature != NULL with a NaN max_curvature; unknown bits in flags.  rtr_last_error
 * names the call and the argument.  Every scratch buffer -- the staging copies among them -- is allocated before the
 * first selection word changes: after any of these the selection and everything else are as they were, the caller's
 * labels and stats included. */
#define RTR_SEGMENT_SEEDED   1   /* as RTR_CLUSTER_SEEDED */
#define RTR_SEGMENT_ORIENTED 2   /* signed normals: dot >= cos_angle, not |dot| >= cos_angle */
int rtr_select_segments(rtr_ctx *ctx, float radius, float cos_angle,
                        const float *normals,    /* 3 n floats, upload order, host or device */
                        const float *curvature,  /* n floats, upload order, host or device, or NULL */
                        float max_curvature,     /* read only when curvature != NULL */
                        uint32_t min_points, uint32_t max_points, int flags, int op,
                        uint32_t *labels, uint64_t stats[4]);

#ifdef __cplusplus
}
#endif

#endif /* RTR_SEGMENTS_H */
