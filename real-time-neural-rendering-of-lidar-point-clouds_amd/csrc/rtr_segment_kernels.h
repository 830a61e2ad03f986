// rtr_segment_kernels.h -- launch wrappers of rtr_segments.hip (internal to librtr_hip.so): the kernels of
// rtr_select_segments (include/rtr_segments.h section 6q).  A header of its own beside rtr_kernels.h, which the frame
// path is compiled from and which stays as it is.  Everything up to the work list is rtr_select_neighbours'; the
// union-find's init, flatten and hits and the combine are rtr_select_clusters' (rtr_kernels.h: launch_cluster_init,
// launch_cluster_flatten, launch_cluster_hits, launch_voxel_combine).
#pragma once
#include "rtr_kernels.h"

namespace rtr {

// segment_gather: out[j] = (the normal of upload index vals[j]; 0) for the m sorted positions with a cell -- or
// (+0, +0, +0; 0) when curvature (device, n floats, upload order; may be null: every point usable) has
// !(curvature[vals[j]] <= max_curvature).  normals: device, 3 floats per upload index.
void launch_segment_gather(hipStream_t s, const uint32_t *vals, uint64_t m, const float *normals, const float *curvature,
                           float max_curvature, float4 *out);
// segment_link: cluster_link with the normal test on top of the distance test: a pair at ((dx dx + dy dy) + dz dz) <= r2
// whose gathered normals are joined (rtr_segment_rule.h) unites the two positions' sets in parent[].  nrec:
// segment_gather's records, in the order of rec.  *tests += the pair tests of live lanes.
void launch_segment_link(hipStream_t s, const float4 *rec, const float4 *nrec, const uint32_t *items, const uint32_t *cursor, uint64_t cap,
                         float r2, float cos_angle, bool oriented, uint32_t *parent, uint64_t *tests);

}  // namespace rtr
