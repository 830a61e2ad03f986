// rtr_neighbours.hip -- gfx950 kernels of rtr_select_neighbours (rtr.h section 6h): the points with at least k others
// within a radius.
//   k_key_sweep      rtr_key_sweep.h's sweep with this file's NeighbourKey: (cell key, upload index) pairs and one 16-byte
//                    record (x, y, z, upload index) per point in upload-order slots; counts the non-finite points and
//                    the finite ones beyond the grid's span
//   radix sort       rtr_voxel.hip's voxel_sort (rocPRIM, stable): the points with a cell come first, cell by cell
//   k_nb_gather      the records into sorted order, so that a cell's points are contiguous 16-byte loads
//   k_nb_cells       counts the occupied cells (the work list's size is bounded by cells + points / 64)
//   k_nb_items       one work item per (occupied cell, 64-point slice of it) with the 9 ranges of the sorted array that
//                    hold the cell's 27 neighbours, each bound found by binary search, 19 lanes searching side by side
//   k_nb_count       one wave per item, one query point per lane: candidates 64 at a time, pair tests, early exit
//   k_voxel_combine  rtr_voxel.hip's: selection := op(selection, hits)
// The arithmetic contract of rtr_kernels.hip holds here too (-ffp-contract=off): a pair test is three fp32 differences,
// three products and two sums, each rounded on its own, in the order ((dx dx + dy dy) + dz dz).
#include "rtr_key_sweep.h"
#include "rtr_neighbour_cell.h"

namespace rtr {

namespace {

static_assert(kNbOut == kSweepOut, "the sweep marks a point without a cell by the neighbour key's bit");

// ---------------------------------------------------------------------------------
// Keys.  cnt[0] / cnt[1]: points that are not finite / finite but beyond the span.  The record goes to slot u like the
// pair, whatever the point's kind (the records of points without a cell are never read).
struct NeighbourKey {
    static constexpr int kCounters = 2;
    double h;
    float4 *rec;
    __device__ __forceinline__ uint64_t operator()(float x, float y, float z, uint32_t u, uint32_t *cnt) const {
        int kind;
        const uint64_t k = neighbour_key(x, y, z, h, &kind);
        cnt[0] += kind == 2, cnt[1] += kind == 1;
        rec[u] = make_float4(x, y, z, __uint_as_float(u));
        return k;
    }
};

// ---------------------------------------------------------------------------------
// Gather.  out[j] = rec[vals[j]] for the m sorted pairs that have a cell: a 4-byte coalesced read, a 16-byte random
// read, a 16-byte coalesced store per point.
__global__ __launch_bounds__(kBlock) void k_nb_gather(const uint32_t *__restrict__ vals, const float4 *__restrict__ rec, uint64_t m,
                                                      float4 *__restrict__ out) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kBlock) out[j] = rec[vals[j]];
}

// Cells.  *cells += the runs of equal keys among the first m sorted keys: one atomic per wave.
__global__ __launch_bounds__(kBlock) void k_nb_cells(const uint64_t *__restrict__ keys, uint64_t m, unsigned long long *__restrict__ cells) {
    uint32_t cnt = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kBlock)
        cnt += j == 0 || keys[j - 1] != keys[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(cells, (unsigned long long)cnt);
}

__device__ __forceinline__ uint32_t bcast(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }

// ---------------------------------------------------------------------------------
// Work list.  One wave per 64 sorted pairs; the heads among them (key[j] != key[j - 1]) are taken one after the other
// (wave-uniform), and for each lanes 0 .. 18 search side by side: lane t < 9 the first pair of range t -- the cells
// (qx + t / 3 - 1, qy + t % 3 - 1, qz - 1 .. qz + 1), one contiguous key range since z is the lowest field --, lane 9 + t
// the first pair behind it, lane 18 the end of the cell's own run.  The cell's ceil(len / 64) items take their slots from
// one atomic cursor (their order is arbitrary; nothing downstream depends on it) and are written by as many lanes.
// An item: 20 words {q0, qn, lo_0, hi_0, .. lo_8, hi_8}: query points q0 .. q0 + qn - 1 (qn <= 64) of the sorted
// records, candidates [lo_t, hi_t).  cap: the slots of `items` (never reached: cells + m / 64 bounds the sum).
constexpr int kItemWords = kNbItemWords;

__global__ __launch_bounds__(kBlock) void k_nb_items(const uint64_t *__restrict__ keys, uint32_t m, uint32_t *__restrict__ items,
                                                     uint32_t *__restrict__ cursor, uint32_t cap) {
    const int lane = threadIdx.x & 63;
    const uint32_t nbatches = (m + 63u) / 64u;
    const uint32_t wave = (uint32_t)(((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6), nwaves = (uint32_t)(((uint64_t)gridDim.x * kBlock) >> 6);
    for (uint32_t b = wave; b < nbatches; b += nwaves) {  // (wave-uniform; b * 64 < 2^32)
        const uint32_t j = b * 64u + (uint32_t)lane;
        uint64_t k = 0;
        bool head = false;
        if (j < m) {
            k = keys[j];
            head = j == 0u || keys[j - 1u] != k;
        }
        uint64_t heads = __ballot(head);
        while (heads) {  // (wave-uniform)
            const int hl = __ffsll((unsigned long long)heads) - 1;
            heads &= heads - 1u;
            const uint64_t kh = (uint64_t)bcast((uint32_t)k, hl) | ((uint64_t)bcast((uint32_t)(k >> 32), hl) << 32);
            const uint32_t jh = b * 64u + (uint32_t)hl;
            uint32_t r = 0;
            if (lane < 19) {
                const int t = lane < 9 ? lane : lane - 9;
                const uint64_t target = lane == 18 ? kh + 1u
                                                   : neighbour_key_offset(kh, t / 3 - 1, t % 3 - 1, lane < 9 ? -1 : 1) + (lane < 9 ? 0u : 1u);
                r = key_lower_bound(keys, m, target);
            }
            const uint32_t len = bcast(r, 18) - jh, nsl = (len + 63u) / 64u;
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(cursor, nsl);
            base = bcast(base, 0);
            uint32_t w[kItemWords];
#pragma unroll
            for (int t = 0; t < 9; ++t) w[2 + 2 * t] = bcast(r, t), w[3 + 2 * t] = bcast(r, 9 + t);
            for (uint32_t sl = (uint32_t)lane; sl < nsl; sl += 64u) {
                if (base + sl >= cap) continue;
                w[0] = jh + sl * 64u;
                w[1] = len - sl * 64u < 64u ? len - sl * 64u : 64u;
                uint4 *o = reinterpret_cast<uint4 *>(items + (uint64_t)(base + sl) * kItemWords);
#pragma unroll
                for (int q = 0; q < kItemWords / 4; ++q) o[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// Count: the hot kernel.  One wave per item; lane l < qn owns query point q0 + l (its record in registers).  Each of
// the 9 ranges is streamed 64 candidates at a time: one coalesced load of up to 1 KB, each lane holding one candidate,
// then the tile's candidates are broadcast one after the other out of the lanes' registers (v_readlane with a
// wave-uniform lane: the cross-lane form of a same-address LDS read, with no LDS round trip and no barrier) and every
// lane tests its own point against the broadcast one: 64 pair tests per lane and full tile, none against the lane's
// own upload index.  After each tile the wave leaves as soon as every live lane has min_nb neighbours (wave-uniform).
// A lane with min_nb neighbours ORs its point's bit into the zeroed hit words.  stats [1] / [2] += lanes with at least
// min_nb neighbours / live lanes with none; *tests += pair tests of live lanes: folded per wave by popcounts of ballots
// (the wave-wide sums of one-bit values), per workgroup in LDS, three atomics per workgroup.
__global__ __launch_bounds__(kBlock) void k_nb_count(const float4 *__restrict__ rec, const uint32_t *__restrict__ items,
                                                     const uint32_t *__restrict__ cursor, uint32_t cap, float r2, uint32_t min_nb,
                                                     uint32_t *__restrict__ hit, unsigned long long *__restrict__ stats,
                                                     unsigned long long *__restrict__ tests) {
    __shared__ unsigned long long s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t listed = *cursor, nitems = listed < cap ? listed : cap;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6));
    const uint32_t nwaves = (uint32_t)(((uint64_t)gridDim.x * kBlock) >> 6);
    uint64_t n_hit = 0, n_none = 0, n_tests = 0;  // (wave-uniform)
    for (uint32_t it = wave; it < nitems; it += nwaves) {
        const uint32_t *I = items + (uint64_t)it * kItemWords;
        const uint32_t q0 = I[0], qn = I[1];
        const bool live = (uint32_t)lane < qn;
        float x = 0.f, y = 0.f, z = 0.f;
        uint32_t u = 0xFFFFFFFFu;
        if (live) {
            const float4 me = rec[q0 + (uint32_t)lane];
            x = me.x, y = me.y, z = me.z, u = __float_as_uint(me.w);
        }
        const uint64_t live_mask = __ballot(live);
        const uint32_t nlive = (uint32_t)__popcll((unsigned long long)live_mask);
        uint32_t cnt = 0;
        bool done = false;
        for (int tt = 0; tt < 9 && !done; ++tt) {
            const int t = tt < 5 ? 4 - tt : tt;  // (the cell's own column first: where most neighbours are, so the wave leaves soonest)
            const uint32_t lo = I[2 + 2 * t], hi = I[3 + 2 * t];
            for (uint32_t c0 = lo; c0 < hi; c0 += 64u) {
                const int m = (int)__builtin_amdgcn_readfirstlane((int)(hi - c0 < 64u ? hi - c0 : 64u));
                float4 cd = make_float4(0.f, 0.f, 0.f, 0.f);
                if (lane < m) cd = rec[c0 + (uint32_t)lane];
                const int cxi = __float_as_int(cd.x), cyi = __float_as_int(cd.y), czi = __float_as_int(cd.z), cui = __float_as_int(cd.w);
#pragma unroll 4
                for (int j = 0; j < m; ++j) {
                    const float cx = __int_as_float(__builtin_amdgcn_readlane(cxi, j)), cy = __int_as_float(__builtin_amdgcn_readlane(cyi, j)),
                                cz = __int_as_float(__builtin_amdgcn_readlane(czi, j));
                    const uint32_t cu = (uint32_t)__builtin_amdgcn_readlane(cui, j);
                    const float d2 = pair_dist2(x, y, z, cx, cy, cz);
                    cnt += (d2 <= r2 && cu != u) ? 1u : 0u;
                }
                n_tests += (uint64_t)m * nlive;
                if (__ballot(live && cnt < min_nb) == 0) {
                    done = true;
                    break;
                }
            }
        }
        const bool pass = live && cnt >= min_nb;
        if (pass) atomicOr(hit + (u >> 5), 1u << (u & 31u));
        n_hit += (uint64_t)__popcll((unsigned long long)__ballot(pass));
        n_none += (uint64_t)__popcll((unsigned long long)__ballot(live && cnt == 0u));
    }
    if (lane == 0) {
        if (n_hit) atomicAdd(&s_cnt[0], (unsigned long long)n_hit);
        if (n_none) atomicAdd(&s_cnt[1], (unsigned long long)n_none);
        if (n_tests) atomicAdd(&s_cnt[2], (unsigned long long)n_tests);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(stats + 1 + threadIdx.x, s_cnt[threadIdx.x]);
    if (threadIdx.x == 2 && s_cnt[2]) atomicAdd(tests, s_cnt[2]);
}

unsigned flat_grid(uint64_t items, uint64_t cap) {
    const uint64_t blocks = (items + kBlock - 1) / kBlock;
    return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

void launch_neighbour_keys(hipStream_t s, const Cloud &c, const uint32_t *perm, float radius, uint64_t *keys, uint32_t *vals, float4 *rec,
                           uint64_t *counters) {
    launch_key_sweep(s, c, perm, NeighbourKey{neighbour_cell_edge(radius), rec}, keys, vals, counters);
}

void launch_neighbour_gather(hipStream_t s, const uint32_t *vals, const float4 *rec, uint64_t m, float4 *out) {
    if (m == 0) return;
    hipLaunchKernelGGL(k_nb_gather, dim3(flat_grid(m, 4096)), dim3(kBlock), 0, s, vals, rec, m, out);
}

void launch_neighbour_cells(hipStream_t s, const uint64_t *keys, uint64_t m, uint64_t *cells) {
    if (m == 0) return;
    hipLaunchKernelGGL(k_nb_cells, dim3(flat_grid(m, 4096)), dim3(kBlock), 0, s, keys, m, (unsigned long long *)cells);
}

void launch_neighbour_items(hipStream_t s, const uint64_t *keys, uint64_t m, uint32_t *items, uint32_t *cursor, uint64_t cap) {
    if (m == 0) return;
    const uint64_t waves = (m + 63) / 64;
    hipLaunchKernelGGL(k_nb_items, dim3(flat_grid(waves * 64, 4096)), dim3(kBlock), 0, s, keys, (uint32_t)m, items, cursor, (uint32_t)cap);
}

void launch_neighbour_count(hipStream_t s, const float4 *rec, const uint32_t *items, const uint32_t *cursor, uint64_t cap, float r2,
                            uint32_t min_neighbours, uint32_t *hit, uint64_t *stats, uint64_t *tests) {
    if (cap == 0) return;
    hipLaunchKernelGGL(k_nb_count, dim3(flat_grid(cap * 64, 4096)), dim3(kBlock), 0, s, rec, items, cursor, (uint32_t)cap, r2, min_neighbours, hit,
                       (unsigned long long *)stats, (unsigned long long *)tests);
}

}  // namespace rtr
