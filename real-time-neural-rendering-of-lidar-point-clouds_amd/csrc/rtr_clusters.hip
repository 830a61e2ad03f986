// rtr_clusters.hip -- gfx950 kernels of rtr_select_clusters (rtr.h section 6i): the connected components of section
// 6h's neighbour relation.  The front half is rtr_neighbours.hip's, unchanged: key sweep, stable sort, gather into cell
// order, work list (one item per occupied cell and 64-point slice of it, nine candidate ranges each).  Behind it:
//   k_cl_init     parent[j] = j over the n sorted positions; the roots' size, smallest upload index and seed flag reset
//   k_cl_link     one wave per item, one query point per lane, k_nb_count's pair test; every accepted pair unites the
//                 two points' sets in parent[] (lock-free union-find over sorted positions)
//   k_cl_flatten  parent[j] = root(j); at the root: size += 1, min upload index, OR of the point's selection bit
//   k_cl_hits     per point the hit from its root's size and flag into the zeroed hit words; labels; stats [1..3]
//   k_voxel_combine  rtr_voxel.hip's: selection := op(selection, hits)
// The positions m .. n - 1 of the sorted pairs are the non-finite points: no item names them, so they stay roots of
// their own and go through k_cl_flatten and k_cl_hits like every other cluster of one.
// The arithmetic contract of rtr_kernels.hip holds here too (-ffp-contract=off).
#include "rtr_kernels.h"
#include "rtr_device.h"
#include "rtr_union_find.h"

namespace rtr {

namespace {

constexpr int kItemWords = kNbItemWords;

// The union-find over sorted positions -- ld_parent, cl_find, cl_unite, with the invariant parent[v] <= v and the
// termination argument -- is rtr_union_find.h's, shared with rtr_segments.hip.

__global__ __launch_bounds__(kBlock) void k_cl_init(uint64_t n, uint32_t *__restrict__ parent, uint32_t *__restrict__ size,
                                                    uint32_t *__restrict__ minu, uint32_t *__restrict__ seed) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock)
        parent[j] = (uint32_t)j, size[j] = 0u, minu[j] = 0xFFFFFFFFu, seed[j] = 0u;
}

// ---------------------------------------------------------------------------------
// Link: the hot kernel, k_nb_count's shape.  One wave per item; lane l < qn owns the query point at sorted position
// q0 + l.  Each of the 9 ranges is streamed 64 candidates at a time (one coalesced load, one candidate per lane) and the
// tile's candidates are broadcast one after the other by v_readlane with a wave-uniform lane; every lane tests its own
// point against the broadcast one.  The relation is symmetric and every pair {a, b} of neighbours, a < b in sorted
// position, is a candidate pair of b's item (a's cell is one of the 27 around b's), so a lane only accepts candidates
// at a SMALLER sorted position than its own: every edge is united exactly once, from its upper end, and a point never
// meets itself.  A range is left as soon as its next tile starts behind the item's last query point (wave-uniform; the
// ranges ascend).  There is no early exit otherwise: every edge matters.
// The lane keeps the root it last saw for its own point and starts the next walk there.  The tile's parent words are
// loaded with the tile, one per lane, and broadcast with the coordinates: a candidate whose parent (as loaded: an
// ancestor of it for good, whatever happens since) is that very position is in the lane's set already and costs no
// memory access at all; any other accepted candidate is united through that ancestor.  Dense cells, where nearly
// every pair is accepted and nearly every union is redundant, then run at the count kernel's pace instead of waiting
// for one L2 round trip per candidate.
// *tests += pair tests of live lanes, folded per wave and per workgroup as in k_nb_count.
__global__ __launch_bounds__(kBlock) void k_cl_link(const float4 *__restrict__ rec, const uint32_t *__restrict__ items,
                                                    const uint32_t *__restrict__ cursor, uint32_t cap, float r2, uint32_t *parent,
                                                    unsigned long long *__restrict__ tests) {
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
        float x = 0.f, y = 0.f, z = 0.f;
        if (live) {
            const float4 me = rec[qp];
            x = me.x, y = me.y, z = me.z;
        }
        const uint32_t nlive = (uint32_t)__popcll((unsigned long long)__ballot(live));
        uint32_t mine = qp;  // a position of qp's set, <= qp
        for (int t = 0; t < 9; ++t) {
            const uint32_t lo = I[2 + 2 * t], hi = I[3 + 2 * t];
            for (uint32_t c0 = lo; c0 < hi && c0 < q0 + qn - 1u; c0 += 64u) {  // (a tile from q0 + qn - 1 on holds no smaller position)
                const int m = (int)__builtin_amdgcn_readfirstlane((int)(hi - c0 < 64u ? hi - c0 : 64u));
                float4 cd = make_float4(0.f, 0.f, 0.f, 0.f);
                if (lane < m) cd = rec[c0 + (uint32_t)lane];
                const int cxi = __float_as_int(cd.x), cyi = __float_as_int(cd.y), czi = __float_as_int(cd.z);
                // the candidates' parents as they are now, one coalesced load per tile (a lane past the tile's end reads c0's)
                const int cpi = (int)ld_parent(parent + (lane < m ? c0 + (uint32_t)lane : c0));
                for (int j = 0; j < m; ++j) {
                    const float cx = __int_as_float(__builtin_amdgcn_readlane(cxi, j)), cy = __int_as_float(__builtin_amdgcn_readlane(cyi, j)),
                                cz = __int_as_float(__builtin_amdgcn_readlane(czi, j));
                    const float d2 = pair_dist2(x, y, z, cx, cy, cz);
                    const uint32_t cp = c0 + (uint32_t)j;
                    const uint32_t par = (uint32_t)__builtin_amdgcn_readlane(cpi, j);  // parent[cp] a moment ago: an ancestor of cp
                    if (live && d2 <= r2 && cp < qp && par != mine) mine = cl_unite(parent, mine, par);
                }
                n_tests += (uint64_t)m * nlive;
            }
        }
    }
    if (lane == 0 && n_tests) atomicAdd(&s_tests, (unsigned long long)n_tests);
    __syncthreads();
    if (threadIdx.x == 0 && s_tests) atomicAdd(tests, s_tests);
}

// ---------------------------------------------------------------------------------
// Flatten.  parent[j] = root(j) for every sorted position j < n; the root gathers its set's size, the smallest upload
// index (vals[j]: the sorted pairs' values) and whether any member's bit is set in the selection words as they are NOW,
// before the combine (sel null: no flag asked for).  The walks run beside the stores of other threads: a store replaces
// a word by the root of the same set, which is <= it, so the invariant and the walks' ends are k_cl_link's.
// Neighbours in sorted order mostly share their root, and a cluster of a million points would otherwise send a million
// atomics to one address, which the memory system serves one after the other: the wave first folds its lanes root by
// root (the distinct roots taken one at a time, wave-uniform; members by ballot, the smallest index by a butterfly
// minimum) and one lane per root issues the three atomics.
__global__ __launch_bounds__(kBlock) void k_cl_flatten(const uint32_t *__restrict__ vals, uint64_t n, const uint32_t *__restrict__ sel,
                                                       uint32_t *parent, uint32_t *__restrict__ size, uint32_t *__restrict__ minu,
                                                       uint32_t *__restrict__ seed) {
    const int lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j0 = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); j0 < n; j0 += stride) {  // (wave-uniform)
        const uint64_t j = j0 + (uint64_t)lane;
        const bool valid = j < n;
        uint32_t r = 0xFFFFFFFFu, u = 0xFFFFFFFFu;
        bool seeded = false;
        if (valid) {
            r = (uint32_t)j;
            uint32_t p = ld_parent(parent + r);
            while (p != r) r = p, p = ld_parent(parent + r);
            if (r != (uint32_t)j) atomicMin(parent + j, r);
            u = vals[j];
            seeded = sel && ((sel[u >> 5] >> (u & 31u)) & 1u);
        }
        uint64_t todo = __ballot(valid);
        while (todo) {  // (wave-uniform: one round per distinct root among the wave's lanes)
            const int first = __ffsll((unsigned long long)todo) - 1;
            const uint32_t root = (uint32_t)__builtin_amdgcn_readlane((int)r, first);
            const bool same = valid && r == root;
            const uint64_t members = __ballot(same);
            uint32_t smallest = same ? u : 0xFFFFFFFFu;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)smallest, off, 64);
                smallest = o < smallest ? o : smallest;
            }
            const bool any_seed = __ballot(same && seeded) != 0;
            if (lane == first) {
                atomicAdd(size + root, (uint32_t)__popcll((unsigned long long)members));
                atomicMin(minu + root, smallest);
                if (any_seed) atomicOr(seed + root, 1u);
            }
            todo &= ~members;
        }
    }
}

// ---------------------------------------------------------------------------------
// Hits.  Position j < n, upload index u = vals[j], root r = parent[j] (flat): hit iff min_points <= size[r] and
// (max_points == 0 or size[r] <= max_points) and (not seeded or seed[r]).  A hit ORs bit u into the zeroed hit words;
// labels (device, may be null) [u] = minu[r].  stats [1] / [2] += roots / roots that hit, [3] = max(size of a root):
// folded per wave (popcounts of ballots, a butterfly maximum), per workgroup in LDS, three atomics per workgroup.
__global__ __launch_bounds__(kBlock) void k_cl_hits(const uint32_t *__restrict__ vals, uint64_t n, const uint32_t *__restrict__ parent,
                                                    const uint32_t *__restrict__ size, const uint32_t *__restrict__ minu,
                                                    const uint32_t *__restrict__ seed, uint32_t min_points, uint32_t max_points, bool seeded,
                                                    uint32_t *__restrict__ hit, uint32_t *__restrict__ labels,
                                                    unsigned long long *__restrict__ stats) {
    __shared__ unsigned long long s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    uint64_t n_roots = 0, n_hits = 0;  // (wave-uniform)
    uint32_t largest = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t j0 = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); j0 < n; j0 += stride) {  // (wave-uniform)
        const uint64_t j = j0 + (uint64_t)lane;
        bool root = false, pass = false;
        if (j < n) {
            const uint32_t r = parent[j], u = vals[j], sz = size[r];
            root = r == (uint32_t)j;
            pass = sz >= min_points && (max_points == 0u || sz <= max_points) && (!seeded || seed[r] != 0u);
            if (pass) atomicOr(hit + (u >> 5), 1u << (u & 31u));
            if (labels) labels[u] = minu[r];
            if (root && sz > largest) largest = sz;
        }
        n_roots += (uint64_t)__popcll((unsigned long long)__ballot(root));
        n_hits += (uint64_t)__popcll((unsigned long long)__ballot(root && pass));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)largest, off, 64);
        largest = o > largest ? o : largest;
    }
    if (lane == 0) {
        if (n_roots) atomicAdd(&s_cnt[0], (unsigned long long)n_roots);
        if (n_hits) atomicAdd(&s_cnt[1], (unsigned long long)n_hits);
        if (largest) atomicMax(&s_cnt[2], (unsigned long long)largest);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(stats + 1 + threadIdx.x, s_cnt[threadIdx.x]);
    if (threadIdx.x == 2 && s_cnt[2]) atomicMax(stats + 3, s_cnt[2]);
}

unsigned flat_grid(uint64_t items, uint64_t cap) {
    const uint64_t blocks = (items + kBlock - 1) / kBlock;
    return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

void launch_cluster_init(hipStream_t s, uint64_t n, uint32_t *parent, uint32_t *size, uint32_t *minu, uint32_t *seed) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_cl_init, dim3(flat_grid(n, 4096)), dim3(kBlock), 0, s, n, parent, size, minu, seed);
}

void launch_cluster_link(hipStream_t s, const float4 *rec, const uint32_t *items, const uint32_t *cursor, uint64_t cap, float r2,
                         uint32_t *parent, uint64_t *tests) {
    if (cap == 0) return;
    hipLaunchKernelGGL(k_cl_link, dim3(flat_grid(cap * 64, 4096)), dim3(kBlock), 0, s, rec, items, cursor, (uint32_t)cap, r2, parent,
                       (unsigned long long *)tests);
}

void launch_cluster_flatten(hipStream_t s, const uint32_t *vals, uint64_t n, const uint32_t *sel, uint32_t *parent, uint32_t *size,
                            uint32_t *minu, uint32_t *seed) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_cl_flatten, dim3(flat_grid(n, 4096)), dim3(kBlock), 0, s, vals, n, sel, parent, size, minu, seed);
}

void launch_cluster_hits(hipStream_t s, const uint32_t *vals, uint64_t n, const uint32_t *parent, const uint32_t *size, const uint32_t *minu,
                         const uint32_t *seed, uint32_t min_points, uint32_t max_points, bool seeded, uint32_t *hit, uint32_t *labels,
                         uint64_t *stats) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_cl_hits, dim3(flat_grid(n, 4096)), dim3(kBlock), 0, s, vals, n, parent, size, minu, seed, min_points, max_points,
                       seeded, hit, labels, (unsigned long long *)stats);
}

}  // namespace rtr
