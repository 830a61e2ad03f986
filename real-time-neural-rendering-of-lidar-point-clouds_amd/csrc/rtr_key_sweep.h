// rtr_key_sweep.h -- the one sweep over the resident coordinates that gives every point a 64-bit key, shared by
// rtr_voxel.hip (rtr_select_voxel_grid) and rtr_neighbours.hip (rtr_select_neighbours).  Device-only, like rtr_device.h.
// What differs between the two is the functor KEY:
//   uint64_t operator()(float x, float y, float z, uint32_t u, uint32_t *cnt) const
//       the key of the point with upload index u; bit 63 (kSweepOut) set: the point has no cell.  cnt: the lane's
//       KEY::kCounters private counters, which the functor may add to.
//   static constexpr int kCounters    0 .. 4; the kernel folds them per wave by shuffles and adds them to `counters`
#pragma once
#include "rtr_device.h"

#include <type_traits>

namespace rtr {

constexpr uint64_t kSweepOut = 1ull << 63;

// k_select's skeleton: one wave per 256-point chunk (lane l: points 4 l .. 4 l + 3), chunks dealt round robin; PACKED
// decodes the chunk (every lane, as k_remove_compact: lanes past the end read the spare bytes), else the lane streams
// its quad of the fp32 SoA.  Every point needs its own key, so no chunk is decided on its box.
// Pair u -- u the upload index: perm[i] when PERM, else the resident index i -- is written to slot u of keys / vals, so
// the pairs lie in ascending upload index and a stable sort by key leaves each cell's smallest upload index first.
// A point without a cell gets kSweepOut | u: unique, a run of its own behind every cell.
// Without PERM a lane's four pairs are contiguous: two 16-byte key stores and one 16-byte index store per lane, the
// wave's stores 2 KB and 1 KB in a row.  With PERM they scatter, 8 + 4 bytes per point.
// Points at or past n are masked by index: the arrays hold n pairs.
template <bool PACKED, bool PERM, class KEY>
__global__ __launch_bounds__(kBlock) void k_key_sweep(PackedXyz pk, const float4 *__restrict__ x4, const float4 *__restrict__ y4,
                                                      const float4 *__restrict__ z4, const uint32_t *__restrict__ perm, uint64_t n,
                                                      KEY key, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                      unsigned long long *__restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const uint64_t n4 = (n + 3) / 4, nchunks = (n4 + 63) / 64;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    uint32_t cnt[KEY::kCounters > 0 ? KEY::kCounters : 1] = {};
    for (uint64_t c = wave; c < nchunks; c += nwaves) {  // (wave-uniform)
        const uint64_t i = c * 64u + (uint64_t)lane, i0 = 4u * i;
        float4 X, Y, Z;
        if (PACKED) {
            const uint4 h0 = pk.hdr[2 * c], h1 = pk.hdr[2 * c + 1];
            const ChunkRawA raw_a = load_chunk_a(pk.planes, h0, h1, lane);
            const ChunkRaw raw = load_chunk_b(pk.planes_b, h0, h1, lane);
            unpack_chunk(raw_a, raw, h0.w, h0.x, h0.y, h0.z, X, Y, Z, lane);
        } else {
            const uint64_t ic = i < n4 ? i : n4 - 1u;
            X = ld_stream(x4 + ic), Y = ld_stream(y4 + ic), Z = ld_stream(z4 + ic);
        }
        if (i0 >= n) continue;
        uint32_t u[4];
        if (PERM) {  // (perm holds whole quads: its arrays are padded to a multiple of 4 points)
            const uint4 q = *reinterpret_cast<const uint4 *>(perm + i0);
            u[0] = q.x, u[1] = q.y, u[2] = q.z, u[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] = (uint32_t)(i0 + j);
        }
        const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
        uint64_t k[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j >= n) {  // (the padding of the last quad: no key, no count)
                k[j] = 0;
                continue;
            }
            k[j] = key(xs[j], ys[j], zs[j], u[j], cnt);
            if (k[j] & kSweepOut) k[j] |= (uint64_t)u[j];
        }
        if (!PERM && i0 + 4u <= n) {  // (slots i0 .. i0 + 3: 32 and 16 contiguous, aligned bytes)
            uint4 *kq = reinterpret_cast<uint4 *>(keys + i0);
            kq[0] = make_uint4((uint32_t)k[0], (uint32_t)(k[0] >> 32), (uint32_t)k[1], (uint32_t)(k[1] >> 32));
            kq[1] = make_uint4((uint32_t)k[2], (uint32_t)(k[2] >> 32), (uint32_t)k[3], (uint32_t)(k[3] >> 32));
            *reinterpret_cast<uint4 *>(vals + i0) = make_uint4(u[0], u[1], u[2], u[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j >= n) continue;  // (with PERM u < n for every point below n)
                keys[u[j]] = k[j];
                vals[u[j]] = u[j];
            }
        }
    }
    if (KEY::kCounters > 0) {
#pragma unroll
        for (int q = 0; q < KEY::kCounters; ++q) {
            uint32_t v = cnt[q];  // (a lane sees at most 2^32 / 64 points)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0 && v) atomicAdd(counters + q, (unsigned long long)v);
        }
    }
}

// the launch: k_select's grid (up to 8 waves per CU); counters: KEY::kCounters device words the caller zeroed, or null
template <class KEY>
void launch_key_sweep(hipStream_t s, const Cloud &c, const uint32_t *perm, const KEY &key, uint64_t *keys, uint32_t *vals,
                      uint64_t *counters) {
    const uint64_t n4 = (c.n + 3) / 4, nchunks = (n4 + 63) / 64;
    if (nchunks == 0) return;
    const uint64_t blocks = (nchunks + 3) / 4;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048)), block(kBlock);
    auto go = [&](auto pk, auto pm) {  // (PACKED, PERM)
        hipLaunchKernelGGL((k_key_sweep<decltype(pk)::value, decltype(pm)::value, KEY>), grid, block, 0, s, c.pk, (const float4 *)c.x,
                           (const float4 *)c.y, (const float4 *)c.z, perm, c.n, key, keys, vals, (unsigned long long *)counters);
    };
    const std::true_type on;
    const std::false_type off;
    const bool packed = c.pk.hdr != nullptr;
    if (packed && perm) go(on, on);
    else if (packed) go(on, off);
    else if (perm) go(off, on);
    else go(off, off);
}

}  // namespace rtr
