// rtr_voxel.hip -- gfx950 kernels of rtr_select_voxel_grid (rtr.h section 6g): one point per cell of a regular grid.
//   k_voxel_keys     one sweep over the resident coordinates: (cell key, upload index) pairs in upload-order slots
//   radix sort       rocPRIM's, stable, by key alone (called directly, as rtr_reorder.hip does)
//   k_voxel_heads    the first pair of every run of equal keys is its cell's representative: its bit into the hit words
//   k_voxel_combine  selection := op(selection, hits)
// The arithmetic contract of rtr_kernels.hip holds here too (-ffp-contract=off: rtr_voxel_key.h rounds the difference and
// the product on their own).
#include "rtr_device.h"
#include "rtr_voxel_key.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <type_traits>

namespace rtr {

namespace {

// ---------------------------------------------------------------------------------
// Keys.  k_select's skeleton: one wave per 256-point chunk (lane l: points 4 l .. 4 l + 3), chunks dealt round robin;
// PACKED decodes the chunk (every lane, as k_remove_compact: lanes past the end read the spare bytes), else the lane
// streams its quad of the fp32 SoA.  Every point needs its own key, so no chunk is decided on its box.
// Pair u -- u the upload index: perm[i] when PERM, else the resident index i -- is written to slot u of keys / vals, so
// the pairs lie in ascending upload index and a stable sort by key leaves each cell's smallest upload index first.
// An out-of-grid point's key is kVoxelOut | u: unique, a run of its own behind every cell.
// Without PERM a lane's four pairs are contiguous: two 16-byte key stores and one 16-byte index store per lane, the
// wave's stores 2 KB and 1 KB in a row.  With PERM they scatter, 8 + 4 bytes per point.
// Points at or past n are masked by index: the arrays hold n pairs.
template <bool PACKED, bool PERM>
__global__ __launch_bounds__(kBlock) void k_voxel_keys(PackedXyz pk, const float4 *__restrict__ x4, const float4 *__restrict__ y4,
                                                       const float4 *__restrict__ z4, const uint32_t *__restrict__ perm, uint64_t n,
                                                       VoxelGrid g, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int lane = threadIdx.x & 63;
    const uint64_t n4 = (n + 3) / 4, nchunks = (n4 + 63) / 64;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
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
        uint64_t k[4] = {voxel_key(X.x, Y.x, Z.x, g.origin, g.inv), voxel_key(X.y, Y.y, Z.y, g.origin, g.inv),
                         voxel_key(X.z, Y.z, Z.z, g.origin, g.inv), voxel_key(X.w, Y.w, Z.w, g.origin, g.inv)};
        uint32_t u[4];
        if (PERM) {  // (perm holds whole quads: its arrays are padded to a multiple of 4 points)
            const uint4 q = *reinterpret_cast<const uint4 *>(perm + i0);
            u[0] = q.x, u[1] = q.y, u[2] = q.z, u[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] = (uint32_t)(i0 + j);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k[j] & kVoxelOut) k[j] |= (uint64_t)u[j];
        if (!PERM && i0 + 4u <= n) {  // (slots i0 .. i0 + 3: 32 and 16 contiguous, aligned bytes)
            uint4 *kq = reinterpret_cast<uint4 *>(keys + i0);
            kq[0] = make_uint4((uint32_t)k[0], (uint32_t)(k[0] >> 32), (uint32_t)k[1], (uint32_t)(k[1] >> 32));
            kq[1] = make_uint4((uint32_t)k[2], (uint32_t)(k[2] >> 32), (uint32_t)k[3], (uint32_t)(k[3] >> 32));
            *reinterpret_cast<uint4 *>(vals + i0) = make_uint4(u[0], u[1], u[2], u[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j >= n) continue;  // (the padding of the last quad; with PERM u < n for every point below n)
                keys[u[j]] = k[j];
                vals[u[j]] = u[j];
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// Heads.  Pair j of the sorted arrays is the head of its run iff j == 0 or key[j] != key[j - 1]; the run holds at least
// min_count pairs iff min_count == 1 or key[j + min_count - 1] == key[j] (the array is sorted: no run lengths, no scan).
// A passing head sets its point's bit in the zeroed hit words.  stats [1] / [2] / [3] += in-grid heads / those that pass
// / out-of-grid pairs (each a run of its own), folded per wave by shuffles, per workgroup in LDS: three atomics per
// workgroup.
__global__ __launch_bounds__(kBlock) void k_voxel_heads(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t n,
                                                        uint64_t min_count, uint32_t *__restrict__ hit,
                                                        unsigned long long *__restrict__ stats) {
    __shared__ uint32_t s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t cnt[3] = {0u, 0u, 0u};  // (a thread sees at most 2^32 / 256 pairs)
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
        const uint64_t k = keys[j];
        if (j != 0 && keys[j - 1] == k) continue;
        const bool out = (k & kVoxelOut) != 0;
        const uint64_t last = j + (min_count - 1u);  // (min_count <= 2^32, j < 2^32: no overflow)
        const bool pass = min_count == 1u || (last < n && keys[last] == k);
        cnt[0] += !out, cnt[1] += !out && pass, cnt[2] += out;
        if (pass) {
            const uint32_t v = vals[j];
            atomicOr(hit + (v >> 5), 1u << (v & 31u));
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt[q] += __shfl_xor(cnt[q], off, 64);
        if ((threadIdx.x & 63) == 0 && cnt[q]) atomicAdd(&s_cnt[q], cnt[q]);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(stats + 1 + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

// ---------------------------------------------------------------------------------
// Combine.  sel has 8 words per 256-point chunk (`words`), hit only (n + 31) / 32 (`nw`): the words behind count as
// empty, and the mask of the bits below n keeps the selection's invariant under `invert` and TOGGLE.
__global__ __launch_bounds__(kBlock) void k_voxel_combine(const uint32_t *__restrict__ hit, uint64_t nw, uint64_t words, uint64_t n, int op,
                                                          int invert, uint32_t *__restrict__ sel) {
    for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < words; w += (uint64_t)gridDim.x * kBlock) {
        const uint64_t first = 32u * w;
        const uint32_t below = first >= n ? 0u : (n - first >= 32u ? 0xFFFFFFFFu : (1u << (uint32_t)(n - first)) - 1u);
        uint32_t h = w < nw ? hit[w] : 0u;
        h = (invert ? ~h : h) & below;
        const uint32_t old = sel[w];
        sel[w] = op == 0 ? h : (op == 1 ? (old | h) : (op == 2 ? (old & ~h) : (op == 8 ? (old ^ h) : (old & h))));
    }
}

unsigned flat_grid(uint64_t items, uint64_t cap) {
    const uint64_t blocks = (items + kBlock - 1) / kBlock;
    return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

void launch_voxel_keys(hipStream_t s, const Cloud &c, const uint32_t *perm, const VoxelGrid &g, uint64_t *keys, uint32_t *vals) {
    const uint64_t n4 = (c.n + 3) / 4, nchunks = (n4 + 63) / 64;
    if (nchunks == 0) return;
    const uint64_t blocks = (nchunks + 3) / 4;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048)), block(kBlock);  // (k_select's grid: up to 8 waves per CU)
    auto go = [&](auto pk, auto pm) {  // (PACKED, PERM)
        hipLaunchKernelGGL((k_voxel_keys<decltype(pk)::value, decltype(pm)::value>), grid, block, 0, s, c.pk, (const float4 *)c.x,
                           (const float4 *)c.y, (const float4 *)c.z, perm, c.n, g, keys, vals);
    };
    const std::true_type on;
    const std::false_type off;
    const bool packed = c.pk.hdr != nullptr;
    if (packed && perm) go(on, on);
    else if (packed) go(on, off);
    else if (perm) go(off, on);
    else go(off, off);
}

// the radix sort's temporary for n pairs (the size-query call), and the sort itself: by all 64 key bits, stable; the
// sorted pairs end in k1 / v1.  Both return a hipError_t as int.
int voxel_sort_temp_bytes(uint64_t n, size_t *bytes) {
    uint64_t *k = nullptr;
    uint32_t *v = nullptr;
    *bytes = 0;
    return (int)rocprim::radix_sort_pairs(nullptr, *bytes, k, k, v, v, (size_t)n, 0u, 64u, (hipStream_t)0);
}
int voxel_sort(hipStream_t s, void *tmp, size_t tmp_bytes, const uint64_t *k0, uint64_t *k1, const uint32_t *v0, uint32_t *v1,
               uint64_t n) {
    return (int)rocprim::radix_sort_pairs(tmp, tmp_bytes, k0, k1, v0, v1, (size_t)n, 0u, 64u, s);
}

void launch_voxel_heads(hipStream_t s, const uint64_t *keys, const uint32_t *vals, uint64_t n, uint32_t min_count, uint32_t *hit,
                        uint64_t *stats) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_voxel_heads, dim3(flat_grid(n, 4096)), dim3(kBlock), 0, s, keys, vals, n, (uint64_t)min_count, hit,
                       (unsigned long long *)stats);
}

void launch_voxel_combine(hipStream_t s, const uint32_t *hit, uint64_t n, int op, bool invert, uint32_t *sel) {
    const uint64_t words = ((n + 255) / 256) * 8;
    if (words == 0) return;
    hipLaunchKernelGGL(k_voxel_combine, dim3(flat_grid(words, 2048)), dim3(kBlock), 0, s, hit, (n + 31) / 32, words, n, op, invert ? 1 : 0,
                       sel);
}

}  // namespace rtr
