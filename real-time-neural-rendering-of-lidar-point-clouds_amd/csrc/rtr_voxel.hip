// rtr_voxel.hip -- gfx950 kernels of rtr_select_voxel_grid (rtr.h section 6g): one point per cell of a regular grid.
//   k_key_sweep      one sweep over the resident coordinates: (cell key, upload index) pairs in upload-order slots
//                    (rtr_key_sweep.h, with this file's VoxelKey)
//   radix sort       rocPRIM's, stable, by key alone (called directly, as rtr_reorder.hip does)
//   k_voxel_heads    the first pair of every run of equal keys is its cell's representative: its bit into the hit words
//   k_voxel_combine  selection := op(selection, hits)
// The arithmetic contract of rtr_kernels.hip holds here too (-ffp-contract=off: rtr_voxel_key.h rounds the difference and
// the product on their own).
#include "rtr_key_sweep.h"
#include "rtr_voxel_key.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace rtr {

namespace {

// ---------------------------------------------------------------------------------
// Keys.  The sweep is rtr_key_sweep.h's (shared with rtr_neighbours.hip); this is its functor: rtr_voxel_key.h's cell
// of the call's grid, no counters.
struct VoxelKey {
    static constexpr int kCounters = 0;
    VoxelGrid g;
    __device__ __forceinline__ uint64_t operator()(float x, float y, float z, uint32_t, uint32_t *) const {
        return voxel_key(x, y, z, g.origin, g.inv);
    }
};
static_assert(kVoxelOut == kSweepOut, "the sweep marks a point without a cell by the voxel key's bit");

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
    launch_key_sweep(s, c, perm, VoxelKey{g}, keys, vals, nullptr);
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
