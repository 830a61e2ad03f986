// rtr_near.hip -- gfx950 kernels of rtr_select_near (rtr.h section 6k): the resident points within a radius of GIVEN
// points, and the given points within that radius of a resident one.
//   k_near_keys      the given points, a plain strided array: (cell key, given index) pairs and one 16-byte record
//                    (x, y, z, given index) per point in given-order slots -- rtr_neighbour_cell.h's key with section 6h's
//                    grid --; counts the non-finite points and the finite ones beyond the span, and folds the fp32
//                    bounding box of the points that have a cell
//   radix sort       rtr_voxel.hip's voxel_sort (rocPRIM, stable), then rtr_neighbours.hip's gather: the m given points
//                    with a cell lie cell by cell, 16 bytes each, their keys beside them
//   k_near_sweep     the hot kernel: k_count_bands' skeleton over the RESIDENT chunks (rtr_near_sweep.h, shared with
//                    rtr_nearest.hip), see there
// The cost is set by the given points: nothing is sorted or gathered on the resident side, and a 256-point chunk whose box
// is nowhere near a given point is decided on its header.
// The arithmetic contract of rtr_kernels.hip holds here too (-ffp-contract=off): a pair test is three fp32 differences,
// three products and two sums, each rounded on its own, in the order ((dx dx + dy dy) + dz dz).
#include "rtr_near_sweep.h"

#include <algorithm>
#include <type_traits>

namespace rtr {

namespace {

// ---------------------------------------------------------------------------------
// Given keys.  One point per thread, grid-stride.  Pair j goes to slot j (a point without a cell: kNbOut | j, a run of
// its own behind every cell), record j likewise.  cn[0] / cn[1] += points that are not finite / finite but beyond the
// span: folded per wave by popcounts of ballots.  box[0 .. 2] / box[3 .. 5]: the smallest / largest x, y, z among the
// points WITH a cell as float_order_key patterns (unsigned order = float order); the caller presets them to 2^32 - 1 / 0.
__global__ __launch_bounds__(kBlock) void k_near_keys(const uint8_t *__restrict__ xyz, uint64_t stride, uint32_t count, double h,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ vals, float4 *__restrict__ rec,
                                                      unsigned long long *__restrict__ cn, uint32_t *__restrict__ box) {
    const int lane = threadIdx.x & 63;
    uint32_t bad = 0, far = 0;  // (wave-uniform)
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    const uint64_t total = ((uint64_t)count + 63u) & ~63ull;  // (whole waves: the ballots below are full)
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < total; j += (uint64_t)gridDim.x * kBlock) {
        int kind = -1;
        if (j < count) {
            const float *p = reinterpret_cast<const float *>(xyz + j * stride);
            const float x = p[0], y = p[1], z = p[2];
            uint64_t k = neighbour_key(x, y, z, h, &kind);
            if (kind != 0) k |= j;
            keys[j] = k;
            vals[j] = (uint32_t)j;
            rec[j] = make_float4(x, y, z, __uint_as_float((uint32_t)j));
            if (kind == 0) {
                const uint32_t b[3] = {float_order_key(__float_as_uint(x)), float_order_key(__float_as_uint(y)), float_order_key(__float_as_uint(z))};
#pragma unroll
                for (int a = 0; a < 3; ++a) lo[a] = b[a] < lo[a] ? b[a] : lo[a], hi[a] = b[a] > hi[a] ? b[a] : hi[a];
            }
        }
        bad += (uint32_t)__popcll(__ballot(kind == 2));
        far += (uint32_t)__popcll(__ballot(kind == 1));
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t l = __shfl_xor(lo[a], off, 64), g = __shfl_xor(hi[a], off, 64);
            lo[a] = l < lo[a] ? l : lo[a], hi[a] = g > hi[a] ? g : hi[a];
        }
    }
    if (lane == 0) {
        if (bad) atomicAdd(cn, (unsigned long long)bad);
        if (far) atomicAdd(cn + 1, (unsigned long long)far);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (lo[a] <= hi[a]) atomicMin(box + a, lo[a]), atomicMax(box + 3 + a, hi[a]);
        }
    }
}

// ---------------------------------------------------------------------------------
// Sweep: rtr_near_sweep.h's, with this OP.  NEARW: the candidates of a tile that some lane accepted are gathered in a
// wave-uniform 64-bit mask by one ballot each, and after the tile the lanes of the mask OR their OWN candidate's bit into
// the near words: one atomic per accepted candidate and tile.  Not NEARW: the wave leaves the chunk as soon as all its
// points have hit.
// A point that hit ORs its bit into the zeroed hit words at its UPLOAD index (perm[i] when PERM), one atomic per lane
// without PERM.  hit null (RTR_NEAR_GIVEN_ONLY): no hits are kept or counted.

// the lane's four pair tests against one candidate: bits of the points that accept it
__device__ __forceinline__ uint32_t near_test4(const float xs[4], const float ys[4], const float zs[4], float cx, float cy, float cz, float r2) {
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float d2 = pair_dist2(xs[k], ys[k], zs[k], cx, cy, cz);
        acc |= (d2 <= r2 ? 1u : 0u) << k;
    }
    return acc;
}

template <bool PERM, bool NEARW>
struct NearBitsOp {
    uint32_t *hit, *near;
    static constexpr bool kEarlyExit = !NEARW;
    struct Chunk {};
    __device__ __forceinline__ void begin(Chunk &, const NearArgs &, uint64_t) const {}
    __device__ __forceinline__ void tile(Chunk &, const NearArgs &a, const float xs[4], const float ys[4], const float zs[4], float4 cd, int mm,
                                         int lane, uint32_t &hb) const {
        unsigned long long took = 0ull;  // (wave-uniform) the tile's candidates that some point accepted
        for (int j = 0; j < mm; ++j) {
            const uint32_t acc = near_test4(xs, ys, zs, bcastf(cd.x, j), bcastf(cd.y, j), bcastf(cd.z, j), a.r2);
            hb |= acc;
            if (NEARW) took |= __ballot(acc != 0u) ? 1ull << j : 0ull;
        }
        if (NEARW && ((took >> lane) & 1ull)) {
            const uint32_t g = __float_as_uint(cd.w);
            atomicOr(near + (g >> 5), 1u << (g & 31u));
        }
    }
    __device__ __forceinline__ void accept(Chunk &, int, float, float4 cd) const {
        const uint32_t g = __float_as_uint(cd.w);
        atomicOr(near + (g >> 5), 1u << (g & 31u));
    }
    __device__ __forceinline__ void finish(Chunk &, const NearArgs &a, uint64_t i0, int, uint32_t hb, NearWave &w) const {
        if (!hit) return;
        if (hb) {
            if (PERM) {  // (perm holds whole quads: its arrays are padded to a multiple of 4 points)
                const uint4 pq = *reinterpret_cast<const uint4 *>(a.perm + i0);
                const uint32_t u[4] = {pq.x, pq.y, pq.z, pq.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if ((hb >> k) & 1u) atomicOr(hit + (u[k] >> 5), 1u << (u[k] & 31u));
            } else {  // (i0 is a multiple of 4: the quad's bits lie in one word)
                atomicOr(hit + (i0 >> 5), hb << (uint32_t)(i0 & 31u));
            }
        }
        near_count_hits(hb, w);
    }
};

template <bool PACKED, bool PERM, bool NEARW>
__global__ __launch_bounds__(kBlock) void k_near_sweep(NearArgs a, NearBitsOp<PERM, NEARW> op) {
    near_sweep<PACKED>(a, op);
}

}  // namespace

void launch_near_keys(hipStream_t s, const uint8_t *xyz, uint64_t stride, uint64_t count, float radius, uint64_t *keys, uint32_t *vals,
                      float4 *rec, uint64_t *counters, uint32_t *box) {
    if (count == 0) return;
    const uint64_t blocks = (count + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_near_keys, dim3((unsigned)std::min<uint64_t>(blocks, 4096)), dim3(kBlock), 0, s, xyz, stride, (uint32_t)count,
                       neighbour_cell_edge(radius), keys, vals, rec, (unsigned long long *)counters, box);
}

void near_box_from_keys(const uint32_t box[6], double lo[3], double hi[3]) {
    for (int a = 0; a < 3; ++a) {
        lo[a] = (double)__builtin_bit_cast(float, float_order_bits(box[a]));
        hi[a] = (double)__builtin_bit_cast(float, float_order_bits(box[3 + a]));
    }
}

void launch_near_sweep(hipStream_t s, const Cloud &c, const float *bounds, const uint32_t *perm, const uint64_t *keys, const float4 *rec,
                       uint64_t m, float radius, float r2, const double glo[3], const double ghi[3], uint32_t *hit, uint32_t *near,
                       uint64_t *counters) {
    const uint64_t nchunks = (c.n + 255) / 256;
    if (nchunks == 0) return;
    NearArgs a{};
    near_sweep_args(a, c, bounds, perm, keys, rec, m, radius, r2, glo, ghi, counters);
    const dim3 grid((unsigned)std::min<uint64_t>((nchunks + 3) / 4, 2048)), block(kBlock);  // (k_select's grid)
    auto go = [&](auto pk, auto pm, auto nw) {  // (PACKED, PERM, NEARW)
        hipLaunchKernelGGL((k_near_sweep<decltype(pk)::value, decltype(pm)::value, decltype(nw)::value>), grid, block, 0, s, a,
                           NearBitsOp<decltype(pm)::value, decltype(nw)::value>{hit, near});
    };
    const std::true_type on;
    const std::false_type off;
    const bool packed = c.pk.hdr != nullptr;
    auto with_near = [&](auto pk, auto pm) { if (near) go(pk, pm, on); else go(pk, pm, off); };
    if (packed && perm) with_near(on, on);
    else if (packed) with_near(on, off);
    else if (perm) with_near(off, on);
    else with_near(off, off);
}

}  // namespace rtr
