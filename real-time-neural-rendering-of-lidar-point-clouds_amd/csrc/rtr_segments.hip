// rtr_segments.hip -- gfx950 kernels of rtr_select_segments (rtr_segments.h section 6q): the connected components of
// "section 6h neighbours whose normals agree and which are both smooth enough".  The front half is rtr_neighbours.hip's
// and the back half rtr_clusters.hip's, both unchanged (key sweep, sort, gather, work list; k_cl_init, k_cl_flatten,
// k_cl_hits, k_voxel_combine).  Between them:
//   k_sg_gather   one 16-byte normal record per sorted position, the zero normal for a point that is not usable
//   k_sg_link     k_cl_link with the normal test behind the distance test
// The union-find is rtr_union_find.h's.  The arithmetic contract of rtr_kernels.hip holds here too (-ffp-contract=off);
// the rule itself is rtr_segment_rule.h's, which the host check compiles as it stands.
#include "rtr_segment_kernels.h"
#include "rtr_device.h"
#include "rtr_segment_rule.h"
#include "rtr_union_find.h"

namespace rtr {

namespace {

constexpr int kItemWords = kNbItemWords;

// ---------------------------------------------------------------------------------
// Gather.  Sorted position j < m holds upload index u = vals[j]; its record is u's normal, or (+0, +0, +0) when u is not
// usable.  The zero normal joins nothing (rtr_segment_rule.h, "THE ZERO NORMAL": cos_angle > 0 makes |+-0| and NaN
// fail), which is exactly what the contract asks of an unusable end: the curvature test is paid once per point here
// and k_sg_link carries no curvature at all.
__global__ __launch_bounds__(kBlock) void k_sg_gather(const uint32_t *__restrict__ vals, uint64_t m, const float *__restrict__ normals,
                                                      const float *__restrict__ curvature, float max_curvature, float4 *__restrict__ out) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kBlock) {
        const uint64_t u = vals[j];
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!curvature || segment_usable(curvature[u], max_curvature)) r.x = normals[3 * u], r.y = normals[3 * u + 1], r.z = normals[3 * u + 2];
        out[j] = r;
    }
}

// ---------------------------------------------------------------------------------
// Link: k_cl_link's shape, unchanged -- one wave per item, one query point per lane, the nine ranges streamed 64
// candidates at a time and broadcast by v_readlane, a pair accepted only from its upper end in sorted position, the
// tile's parent words loaded with the tile, the "already in my set" shortcut, the c0 < q0 + qn - 1 cut (see there for
// the reasons).  On top of it the lane holds its own normal in three registers, the tile's normals are loaded with its
// coordinates (one more coalesced 16-byte load per lane and tile), and three more broadcasts and five fp32 operations
// per candidate decide segment_joined.  The relation is symmetric (segment_dot), so accepting a pair from its upper end
// alone still unites every edge exactly once.  A lane that is not live holds the zero normal and joins nothing.
template <bool ORIENTED>
__global__ __launch_bounds__(kBlock) void k_sg_link(const float4 *__restrict__ rec, const float4 *__restrict__ nrec,
                                                    const uint32_t *__restrict__ items, const uint32_t *__restrict__ cursor, uint32_t cap,
                                                    float r2, float cos_angle, uint32_t *parent, unsigned long long *__restrict__ tests) {
    __shared__ unsigned long long s_tests;
    if (threadIdx.x == 0) s_tests = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t listed = *cursor, nitems = listed < cap ? listed : cap;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6));
    const uint32_t nwaves = (uint32_t)(((uint64_t)gridDim.x * kBlock) >> 6);
    uint64_t n_tests = 0;  // (wave-uniform)
    for (uint32_t it = wave; it < nitems; it += nwaves) {
        const uint32_t *I = items + (uint64_t)it * kItemWords;
        const uint32_t q0 = I[0], qn = I[1];
        const bool live = (uint32_t)lane < qn;
        const uint32_t qp = q0 + (uint32_t)lane;
        float x = 0.f, y = 0.f, z = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        if (live) {
            const float4 me = rec[qp], mn = nrec[qp];
            x = me.x, y = me.y, z = me.z;
            nx = mn.x, ny = mn.y, nz = mn.z;
        }
        const uint32_t nlive = (uint32_t)__popcll((unsigned long long)__ballot(live));
        uint32_t mine = qp;  // a position of qp's set, <= qp
        for (int t = 0; t < 9; ++t) {
            const uint32_t lo = I[2 + 2 * t], hi = I[3 + 2 * t];
            for (uint32_t c0 = lo; c0 < hi && c0 < q0 + qn - 1u; c0 += 64u) {  // (a tile from q0 + qn - 1 on holds no smaller position)
                const int m = (int)__builtin_amdgcn_readfirstlane((int)(hi - c0 < 64u ? hi - c0 : 64u));
                float4 cd = make_float4(0.f, 0.f, 0.f, 0.f), cn = make_float4(0.f, 0.f, 0.f, 0.f);
                if (lane < m) cd = rec[c0 + (uint32_t)lane], cn = nrec[c0 + (uint32_t)lane];
                const int cxi = __float_as_int(cd.x), cyi = __float_as_int(cd.y), czi = __float_as_int(cd.z);
                const int nxi = __float_as_int(cn.x), nyi = __float_as_int(cn.y), nzi = __float_as_int(cn.z);
                // the candidates' parents as they are now, one coalesced load per tile (a lane past the tile's end reads c0's)
                const int cpi = (int)ld_parent(parent + (lane < m ? c0 + (uint32_t)lane : c0));
                for (int j = 0; j < m; ++j) {
                    const float cx = __int_as_float(__builtin_amdgcn_readlane(cxi, j)), cy = __int_as_float(__builtin_amdgcn_readlane(cyi, j)),
                                cz = __int_as_float(__builtin_amdgcn_readlane(czi, j));
                    const float cnx = __int_as_float(__builtin_amdgcn_readlane(nxi, j)), cny = __int_as_float(__builtin_amdgcn_readlane(nyi, j)),
                                cnz = __int_as_float(__builtin_amdgcn_readlane(nzi, j));
                    const float d2 = pair_dist2(x, y, z, cx, cy, cz);
                    const bool joined = segment_joined(nx, ny, nz, cnx, cny, cnz, cos_angle, ORIENTED);
                    const uint32_t cp = c0 + (uint32_t)j;
                    const uint32_t par = (uint32_t)__builtin_amdgcn_readlane(cpi, j);  // parent[cp] a moment ago: an ancestor of cp
                    if (live && d2 <= r2 && joined && cp < qp && par != mine) mine = cl_unite(parent, mine, par);
                }
                n_tests += (uint64_t)m * nlive;
            }
        }
    }
    if (lane == 0 && n_tests) atomicAdd(&s_tests, (unsigned long long)n_tests);
    __syncthreads();
    if (threadIdx.x == 0 && s_tests) atomicAdd(tests, s_tests);
}

unsigned flat_grid(uint64_t items, uint64_t cap) {
    const uint64_t blocks = (items + kBlock - 1) / kBlock;
    return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

void launch_segment_gather(hipStream_t s, const uint32_t *vals, uint64_t m, const float *normals, const float *curvature,
                           float max_curvature, float4 *out) {
    if (m == 0) return;
    hipLaunchKernelGGL(k_sg_gather, dim3(flat_grid(m, 4096)), dim3(kBlock), 0, s, vals, m, normals, curvature, max_curvature, out);
}

void launch_segment_link(hipStream_t s, const float4 *rec, const float4 *nrec, const uint32_t *items, const uint32_t *cursor, uint64_t cap,
                         float r2, float cos_angle, bool oriented, uint32_t *parent, uint64_t *tests) {
    if (cap == 0) return;
    const dim3 grid(flat_grid(cap * 64, 4096)), block(kBlock);
    if (oriented)
        hipLaunchKernelGGL(k_sg_link<true>, grid, block, 0, s, rec, nrec, items, cursor, (uint32_t)cap, r2, cos_angle, parent,
                           (unsigned long long *)tests);
    else
        hipLaunchKernelGGL(k_sg_link<false>, grid, block, 0, s, rec, nrec, items, cursor, (uint32_t)cap, r2, cos_angle, parent,
                           (unsigned long long *)tests);
}

}  // namespace rtr
