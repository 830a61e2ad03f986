// rtr_nearest.hip -- gfx950 kernels of rtr_nearest_points (rtr.h section 6l): for every GIVEN point the nearest resident
// point within a radius, and for every resident point the nearest given one.
//   given points     rtr_near.hip's k_near_keys, rtr_voxel.hip's sort and rtr_neighbours.hip's gather, as section 6k
//   k_nearest_sweep  the hot kernel: rtr_near_sweep.h's sweep over the RESIDENT chunks -- every chunk near a given point is
//                    tested against every candidate, no early exit -- keeping minima where rtr_near.hip ORs bits
//   k_nearest_unpack the given slots into the caller's two arrays, and their count
// A pair's KEY is (bits of d2) << 32 | index: d2 is a sum of squares, never negative and never NaN when accepted, so the
// unsigned order of the keys is the order of (d2, index) -- the contract's order, its tie rule included.
// The arithmetic contract of rtr_kernels.hip holds here too (-ffp-contract=off), and fp32 denormals are kept (hipcc's
// default for gfx950: the code object's float mode has them on): d2 = 2^-140 comes out as it is.
#include "rtr_near_sweep.h"

#include <algorithm>
#include <type_traits>

namespace rtr {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;                       // RTR_NEAREST_NONE
constexpr uint64_t kNoKey = 0x7F800000FFFFFFFFull;            // (+inf, NONE): above every accepted pair's key

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {  // the smallest v of the wave, in every lane
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// GIVEN side: slots[g] (all ones before the sweep) = the smallest key (d2 bits, UPLOAD index) over the resident points
// that accept given point g.  Per tile the wave keeps the candidate-broadcast loop of section 6k: where the ballot says
// some lane accepted candidate j, the 32-bit minimum of the accepted d2 bits across the wave, then the smallest upload
// index among the points that tie at it (without PERM the upload index grows with lane and component: the first lane of
// the tie has it), go to lane j -- the lane that owns candidate j's record --, and after the tile every such lane issues
// ONE atomicMin (global_atomic_umin_x2) for its own candidate.  The per-point path issues its atomics directly.
// RESIDENT side (RES; compiled out otherwise): each lane keeps a running key (d2 bits, GIVEN index) for its four points,
// updated behind the same ballot -- only for a candidate that some lane accepted --, and stores index and d2 at their
// upload indices after the chunk -- a point belongs to one lane: no atomics; ridx / rd2 are preset to NONE / +inf, whole
// quads (padded to a multiple of 4 points), and a chunk that is skipped writes nothing.
template <bool PERM, bool RES>
struct NearestOp {
    unsigned long long *slots;
    uint32_t *ridx, *rd2;
    static constexpr bool kEarlyExit = false;
    struct Chunk {
        uint32_t u[4];   // the upload indices of the lane's points
        uint64_t rk[4];  // RES: their running keys
    };
    __device__ __forceinline__ void begin(Chunk &ch, const NearArgs &a, uint64_t i0) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) ch.u[k] = (uint32_t)(i0 + (uint64_t)k), ch.rk[k] = kNoKey;
        if (PERM && i0 < a.n) {  // (perm holds whole quads: its arrays are padded to a multiple of 4 points)
            const uint4 pq = *reinterpret_cast<const uint4 *>(a.perm + i0);
            ch.u[0] = pq.x, ch.u[1] = pq.y, ch.u[2] = pq.z, ch.u[3] = pq.w;
        }
    }
    __device__ __forceinline__ void tile(Chunk &ch, const NearArgs &a, const float xs[4], const float ys[4], const float zs[4], float4 cd, int mm,
                                         int lane, uint32_t &hb) const {
        uint64_t mine = ~0ull;  // the tile's smallest key for the lane's OWN candidate
        for (int j = 0; j < mm; ++j) {
            const float cx = bcastf(cd.x, j), cy = bcastf(cd.y, j), cz = bcastf(cd.z, j);
            uint32_t b[4], lb = kNone;  // the accepted d2 bits per point (all ones: not accepted), and the smallest
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d2 = pair_dist2(xs[k], ys[k], zs[k], cx, cy, cz);
                b[k] = d2 <= a.r2 ? __float_as_uint(d2) : kNone;
                lb = b[k] < lb ? b[k] : lb;
            }
            // Everything but the pair tests happens only for a candidate that some lane accepted (wave-uniform): most
            // (candidate, chunk) pairs that are tested accept nothing
            if (__ballot(lb != kNone) != 0ull) {
#pragma unroll
                for (int k = 0; k < 4; ++k) hb |= (b[k] != kNone ? 1u : 0u) << k;
                if (RES) {
                    const uint32_t g = (uint32_t)__builtin_amdgcn_readlane(__float_as_int(cd.w), j);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint64_t key = ((uint64_t)b[k] << 32) | g;  // (not accepted: above kNoKey)
                        ch.rk[k] = key < ch.rk[k] ? key : ch.rk[k];
                    }
                }
                const uint32_t wmin = wave_min_u32(lb);
                uint32_t lu = kNone;  // the smallest upload index among the lane's points that tie at wmin
#pragma unroll
                for (int k = 0; k < 4; ++k) lu = (b[k] == wmin && ch.u[k] < lu) ? ch.u[k] : lu;
                uint32_t wu;
                if (PERM) wu = wave_min_u32(lu);
                else wu = (uint32_t)__builtin_amdgcn_readlane((int)lu, __ffsll((long long)__ballot(lu != kNone)) - 1);
                mine = lane == j ? (((uint64_t)wmin << 32) | wu) : mine;
            }
        }
        if (mine != ~0ull) atomicMin(slots + __float_as_uint(cd.w), (unsigned long long)mine);
    }
    __device__ __forceinline__ void accept(Chunk &ch, int k, float d2, float4 cd) const {
        const uint32_t g = __float_as_uint(cd.w), bits = __float_as_uint(d2);
        atomicMin(slots + g, ((unsigned long long)bits << 32) | ch.u[k]);
        if (RES) {
            const uint64_t key = ((uint64_t)bits << 32) | g;
            ch.rk[k] = key < ch.rk[k] ? key : ch.rk[k];
        }
    }
    __device__ __forceinline__ void finish(Chunk &ch, const NearArgs &a, uint64_t i0, int, uint32_t hb, NearWave &w) const {
        if (RES && hb) {
            if (PERM) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if ((hb >> k) & 1u) ridx[ch.u[k]] = (uint32_t)ch.rk[k], rd2[ch.u[k]] = (uint32_t)(ch.rk[k] >> 32);
            } else {  // (one 16-byte store per quad and array; a point that accepted nothing still holds (+inf, NONE))
                *reinterpret_cast<uint4 *>(ridx + i0) = make_uint4((uint32_t)ch.rk[0], (uint32_t)ch.rk[1], (uint32_t)ch.rk[2], (uint32_t)ch.rk[3]);
                *reinterpret_cast<uint4 *>(rd2 + i0) = make_uint4((uint32_t)(ch.rk[0] >> 32), (uint32_t)(ch.rk[1] >> 32), (uint32_t)(ch.rk[2] >> 32),
                                                                 (uint32_t)(ch.rk[3] >> 32));
            }
        }
        near_count_hits(hb, w);
    }
};

template <bool PACKED, bool PERM, bool RES>
__global__ __launch_bounds__(kBlock) void k_nearest_sweep(NearArgs a, NearestOp<PERM, RES> op) {
    near_sweep<PACKED>(a, op);
}

// Given slots -> the caller's arrays: all ones becomes (NONE, +inf); *have += the slots that hold a pair.  idx / d2 may be
// null on their own.  One slot per thread, whole waves.
__global__ __launch_bounds__(kBlock) void k_nearest_unpack(const unsigned long long *__restrict__ slots, uint32_t count, uint32_t *__restrict__ idx,
                                                           uint32_t *__restrict__ d2, unsigned long long *__restrict__ have) {
    const uint64_t total = ((uint64_t)count + 63u) & ~63ull;
    uint32_t found = 0;  // (wave-uniform)
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < total; j += (uint64_t)gridDim.x * kBlock) {
        bool has = false;
        if (j < count) {
            const unsigned long long key = slots[j];
            has = key != ~0ull;
            if (idx) idx[j] = has ? (uint32_t)key : kNone;
            if (d2) d2[j] = has ? (uint32_t)(key >> 32) : 0x7F800000u;
        }
        found += (uint32_t)__popcll(__ballot(has));
    }
    if ((threadIdx.x & 63) == 0 && found) atomicAdd(have, (unsigned long long)found);
}

}  // namespace

void launch_nearest_sweep(hipStream_t s, const Cloud &c, const float *bounds, const uint32_t *perm, const uint64_t *keys, const float4 *rec,
                          uint64_t m, float radius, float r2, const double glo[3], const double ghi[3], uint64_t *slots, uint32_t *ridx,
                          uint32_t *rd2, uint64_t *counters) {
    const uint64_t nchunks = (c.n + 255) / 256;
    if (nchunks == 0) return;
    NearArgs a{};
    near_sweep_args(a, c, bounds, perm, keys, rec, m, radius, r2, glo, ghi, counters);
    const dim3 grid((unsigned)std::min<uint64_t>((nchunks + 3) / 4, 2048)), block(kBlock);  // (k_near_sweep's grid)
    auto go = [&](auto pk, auto pm, auto rs) {  // (PACKED, PERM, RES)
        hipLaunchKernelGGL((k_nearest_sweep<decltype(pk)::value, decltype(pm)::value, decltype(rs)::value>), grid, block, 0, s, a,
                           NearestOp<decltype(pm)::value, decltype(rs)::value>{(unsigned long long *)slots, ridx, rd2});
    };
    const std::true_type on;
    const std::false_type off;
    const bool packed = c.pk.hdr != nullptr;
    auto with_res = [&](auto pk, auto pm) { if (ridx) go(pk, pm, on); else go(pk, pm, off); };
    if (packed && perm) with_res(on, on);
    else if (packed) with_res(on, off);
    else if (perm) with_res(off, on);
    else with_res(off, off);
}

void launch_nearest_unpack(hipStream_t s, const uint64_t *slots, uint64_t count, uint32_t *idx, uint32_t *d2, uint64_t *have) {
    if (count == 0) return;
    const uint64_t blocks = (count + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_nearest_unpack, dim3((unsigned)std::min<uint64_t>(blocks, 4096)), dim3(kBlock), 0, s, (const unsigned long long *)slots,
                       (uint32_t)count, idx, d2, (unsigned long long *)have);
}

}  // namespace rtr
