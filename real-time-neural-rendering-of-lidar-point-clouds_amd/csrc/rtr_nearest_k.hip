// rtr_nearest_k.hip -- gfx950 kernels of rtr_nearest_k_points (rtr.h section 6m): for every GIVEN point its k nearest
// resident points within a radius, in ascending order of (d2 bits, upload index).
//   given points        as rtr_nearest.hip: k_near_keys, the sort and the gather of section 6k
//   k_nearest_k_sweep   the hot kernel: rtr_near_sweep.h's sweep over the RESIDENT chunks, no early exit; an accepted pair's
//                       key -- rtr_nearest.hip's (bits of d2) << 32 | upload index -- goes into the given point's ROW of
//                       k 64-bit slots by rtr_topk_cascade.h's cascade of returning atomic minima
//   k_nearest_k_unpack  the rows into the caller's three arrays, and their three counts
// The keys of one given point are distinct (their indices are), which is all the cascade asks; no wave waits for another.
// The arithmetic contract of rtr_kernels.hip holds here too (-ffp-contract=off), and fp32 denormals are kept.
#include "rtr_near_sweep.h"
#include "rtr_topk_cascade.h"

#include <algorithm>
#include <type_traits>

namespace rtr {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // RTR_NEAREST_NONE

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {  // the smallest v of the wave, in every lane
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// a read of a slot that may be stale but comes from memory, not from a scalar cache that nothing refreshes
__device__ __forceinline__ uint64_t slot_peek(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// rows[g * k + s] (all ones before the sweep): the row of given point g.
// tile: lane t reads the BOUND of its own candidate, row[k - 1], once per tile, before the pair tests (a stale bound is
// safe: rtr_topk_cascade.h).  The candidate-broadcast loop and its ballot are rtr_nearest.hip's.  For a candidate that
// some lane accepted, the keys that do not beat the bound are dropped, and the wave then takes its survivors in ascending
// order -- rtr_nearest.hip's wave minimum of the d2 bits and smallest tying upload index, once per round, the winner
// struck out of its lane -- for at most k rounds or until none is left: a chunk can contribute no more than its k
// smallest.  Round r's key goes to lane r (k <= 64), and the lanes that hold one cascade side by side, each starting
// behind the leading slots that one load of the row (slot s by lane s) showed below its key.
// ONE (k = 1): a single round, and as in rtr_nearest.hip the winner goes to the lane that owns the candidate, which
// issues one atomicMin after the tile: section 6l's atomics, plus the bound.
// accept (per-point path): bound, then the cascade, directly.
// cascades (device): += the cascades started.
template <bool PERM, bool ONE>
struct NearestKOp {
    unsigned long long *rows;
    uint32_t k;
    unsigned long long *cascades;
    static constexpr bool kEarlyExit = false;
    struct Chunk {
        uint32_t u[4];  // the upload indices of the lane's points
        uint32_t started;  // the cascades this lane started
    };
    __device__ __forceinline__ void begin(Chunk &ch, const NearArgs &a, uint64_t i0) const {
#pragma unroll
        for (int q = 0; q < 4; ++q) ch.u[q] = (uint32_t)(i0 + (uint64_t)q);
        ch.started = 0u;
        if (PERM && i0 < a.n) {  // (perm holds whole quads: its arrays are padded to a multiple of 4 points)
            const uint4 pq = *reinterpret_cast<const uint4 *>(a.perm + i0);
            ch.u[0] = pq.x, ch.u[1] = pq.y, ch.u[2] = pq.z, ch.u[3] = pq.w;
        }
    }
    __device__ __forceinline__ unsigned long long *row_of(uint32_t g) const { return rows + (uint64_t)g * k; }
    __device__ __forceinline__ void tile(Chunk &ch, const NearArgs &a, const float xs[4], const float ys[4], const float zs[4], float4 cd, int mm,
                                         int lane, uint32_t &hb) const {
        uint64_t bound = 0ull;  // (a lane without a candidate is never asked)
        if (lane < mm) bound = slot_peek(row_of(__float_as_uint(cd.w)) + (k - 1u));
        uint64_t mine = kTopkEmpty;  // ONE: the tile's smallest key for the lane's OWN candidate
        for (int j = 0; j < mm; ++j) {
            const float cx = bcastf(cd.x, j), cy = bcastf(cd.y, j), cz = bcastf(cd.z, j);
            uint32_t b[4], lb = kNone;  // the accepted d2 bits per point (all ones: not accepted), and the smallest
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float d2 = pair_dist2(xs[q], ys[q], zs[q], cx, cy, cz);
                b[q] = d2 <= a.r2 ? __float_as_uint(d2) : kNone;
                lb = b[q] < lb ? b[q] : lb;
            }
            if (__ballot(lb != kNone) == 0ull) continue;  // (wave-uniform: most tested pairs accept nothing)
#pragma unroll
            for (int q = 0; q < 4; ++q) hb |= (b[q] != kNone ? 1u : 0u) << q;
            const uint64_t bj = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bound, j) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(bound >> 32), j) << 32);
            lb = kNone;
#pragma unroll
            for (int q = 0; q < 4; ++q) {  // the prune
                b[q] = (b[q] != kNone && topk_beats(((uint64_t)b[q] << 32) | ch.u[q], bj)) ? b[q] : kNone;
                lb = b[q] < lb ? b[q] : lb;
            }
            if (__ballot(lb != kNone) == 0ull) continue;
            // the row as it stands, slot `lane` (one load, in flight during the rounds): where each survivor's walk may start
            unsigned long long *row = row_of((uint32_t)__builtin_amdgcn_readlane(__float_as_int(cd.w), j));
            uint64_t snap = 0ull;
            if (!ONE && (uint32_t)lane < k) snap = slot_peek(row + lane);
            uint64_t sel = kTopkEmpty;  // round `lane`'s key
            const uint32_t rounds = ONE ? 1u : k;
            for (uint32_t r = 0; r < rounds; ++r) {  // (wave-uniform)
                const uint32_t wmin = wave_min_u32(lb);
                if (wmin == kNone) break;
                uint32_t lu = kNone;  // the smallest upload index among the lane's points that tie at wmin
#pragma unroll
                for (int q = 0; q < 4; ++q) lu = (b[q] == wmin && ch.u[q] < lu) ? ch.u[q] : lu;
                uint32_t wu;
                if (PERM) wu = wave_min_u32(lu);
                else wu = (uint32_t)__builtin_amdgcn_readlane((int)lu, __ffsll((long long)__ballot(lu != kNone)) - 1);
                const uint64_t key = ((uint64_t)wmin << 32) | wu;
                if (ONE) {
                    mine = lane == j ? key : mine;
                } else {
                    sel = (uint32_t)lane == r ? key : sel;
                    lb = kNone;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {  // struck out where it came from (one point of one lane: the indices are distinct)
                        b[q] = (b[q] == wmin && ch.u[q] == wu) ? kNone : b[q];
                        lb = b[q] < lb ? b[q] : lb;
                    }
                }
            }
            if (!ONE) {
                uint32_t first = 0;  // the leading slots read below the lane's key (rtr_topk_cascade.h, "The SKIP")
                bool run = sel != kTopkEmpty;
                for (uint32_t s = 0; s < k && __ballot(run) != 0ull; ++s) {  // (wave-uniform)
                    const uint64_t v = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)snap, (int)s) |
                                       ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(snap >> 32), (int)s) << 32);
                    run = run && v < sel;
                    first += run ? 1u : 0u;
                }
                if (sel != kTopkEmpty && first < k) {
                    topk_cascade(k, sel, [row](uint32_t s, uint64_t v) { return (uint64_t)atomicMin(row + s, (unsigned long long)v); }, first);
                    ch.started += 1u;
                }
            }
        }
        if (ONE && mine != kTopkEmpty) {
            atomicMin(rows + __float_as_uint(cd.w), (unsigned long long)mine);
            ch.started += 1u;
        }
    }
    __device__ __forceinline__ void accept(Chunk &ch, int q, float d2, float4 cd) const {
        unsigned long long *row = row_of(__float_as_uint(cd.w));
        const uint64_t key = ((uint64_t)__float_as_uint(d2) << 32) | ch.u[q];
        if (!topk_beats(key, slot_peek(row + (k - 1u)))) return;
        topk_cascade(k, key, [row](uint32_t s, uint64_t v) { return (uint64_t)atomicMin(row + s, (unsigned long long)v); });
        ch.started += 1u;
    }
    __device__ __forceinline__ void finish(Chunk &ch, const NearArgs &, uint64_t, int lane, uint32_t hb, NearWave &w) const {
        uint32_t st = ch.started;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) st += __shfl_xor(st, off, 64);
        if (lane == 0 && st) atomicAdd(cascades, (unsigned long long)st);
        near_count_hits(hb, w);
    }
};

template <bool PACKED, bool PERM, bool ONE>
__global__ __launch_bounds__(kBlock) void k_nearest_k_sweep(NearArgs a, NearestKOp<PERM, ONE> op) {
    near_sweep<PACKED>(a, op);
}

// Rows -> the caller's arrays, one slot per thread, whole waves: idx / d2 (count * k words each) get the low / high half of
// the slot, all ones becoming (NONE, +inf); found[j] = the row's real entries (a row is sorted: they come first).  Each
// of the three may be null.  tally[0] += rows with an entry, [1] += entries, [2] += rows that are full.
__global__ __launch_bounds__(kBlock) void k_nearest_k_unpack(const unsigned long long *__restrict__ rows, uint64_t count, uint32_t k,
                                                             uint32_t *__restrict__ idx, uint32_t *__restrict__ d2, uint32_t *__restrict__ found,
                                                             unsigned long long *__restrict__ tally) {
    const uint64_t slots = count * k, total = (slots + 63u) & ~63ull;
    uint32_t t0 = 0, t1 = 0, t2 = 0;  // (wave-uniform)
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kBlock) {
        bool has = false, first = false, last = false;
        if (e < slots) {
            const uint64_t j = e / k;
            const uint32_t s = (uint32_t)(e - j * k);
            const unsigned long long key = rows[e];
            has = key != kTopkEmpty, first = s == 0u, last = s == k - 1u;
            if (idx) idx[e] = has ? (uint32_t)key : kNone;
            if (d2) d2[e] = has ? (uint32_t)(key >> 32) : 0x7F800000u;
            if (found) {
                if (first && !has) found[j] = 0u;
                if (has && (last || rows[e + 1] == kTopkEmpty)) found[j] = s + 1u;
            }
        }
        t0 += (uint32_t)__popcll(__ballot(has && first));
        t1 += (uint32_t)__popcll(__ballot(has));
        t2 += (uint32_t)__popcll(__ballot(has && last));
    }
    if ((threadIdx.x & 63) == 0) {
        if (t0) atomicAdd(tally + 0, (unsigned long long)t0);
        if (t1) atomicAdd(tally + 1, (unsigned long long)t1);
        if (t2) atomicAdd(tally + 2, (unsigned long long)t2);
    }
}

}  // namespace

void launch_nearest_k_sweep(hipStream_t s, const Cloud &c, const float *bounds, const uint32_t *perm, const uint64_t *keys, const float4 *rec,
                            uint64_t m, float radius, float r2, const double glo[3], const double ghi[3], uint64_t *rows, uint32_t k,
                            uint64_t *cascades, uint64_t *counters) {
    const uint64_t nchunks = (c.n + 255) / 256;
    if (nchunks == 0) return;
    NearArgs a{};
    near_sweep_args(a, c, bounds, perm, keys, rec, m, radius, r2, glo, ghi, counters);
    const dim3 grid((unsigned)std::min<uint64_t>((nchunks + 3) / 4, 2048)), block(kBlock);  // (k_near_sweep's grid)
    auto go = [&](auto pk, auto pm, auto one) {  // (PACKED, PERM, ONE)
        hipLaunchKernelGGL((k_nearest_k_sweep<decltype(pk)::value, decltype(pm)::value, decltype(one)::value>), grid, block, 0, s, a,
                           NearestKOp<decltype(pm)::value, decltype(one)::value>{(unsigned long long *)rows, k, (unsigned long long *)cascades});
    };
    const std::true_type on;
    const std::false_type off;
    const bool packed = c.pk.hdr != nullptr;
    auto with_k = [&](auto pk, auto pm) { if (k == 1u) go(pk, pm, on); else go(pk, pm, off); };
    if (packed && perm) with_k(on, on);
    else if (packed) with_k(on, off);
    else if (perm) with_k(off, on);
    else with_k(off, off);
}

void launch_nearest_k_unpack(hipStream_t s, const uint64_t *rows, uint64_t count, uint32_t k, uint32_t *idx, uint32_t *d2, uint32_t *found,
                             uint64_t *tally) {
    if (count == 0) return;
    const uint64_t blocks = (count * k + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_nearest_k_unpack, dim3((unsigned)std::min<uint64_t>(blocks, 4096)), dim3(kBlock), 0, s, (const unsigned long long *)rows,
                       count, k, idx, d2, found, (unsigned long long *)tally);
}

}  // namespace rtr
