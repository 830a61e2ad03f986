// rtr_statistical.hip -- gfx950 kernels of rtr_select_statistical (include/rtr_statistics.h section 6n): the points whose
// mean distance to their k nearest neighbours lies within a threshold taken from the cloud itself.  Everything up to the
// work list is rtr_select_neighbours' (rtr_neighbours.hip: key sweep, sort, gather, cells, items).
//   k_nb_rows        one wave per item, one query point per lane, as k_nb_count -- but every lane keeps the k smallest
//                    squared distances of its point in a row in LDS (rtr_knn_row.h), with no early exit and no atomics,
//                    then sorts the row, sums the square roots in order, divides, and writes the mean and the row's
//                    length to its point's upload-order slot
//   k_stat_partial   one fp64 partial sum per 1024 consecutive upload indices, in a fixed shape
//   k_stat_final     the partial sums into one, in a fixed shape: one workgroup
//   k_stat_hits      the means against the threshold: the hit words and two statistics
//   k_voxel_combine  rtr_voxel.hip's: selection := op(selection, hits)
// The arithmetic contract of rtr_kernels.hip holds here too (-ffp-contract=off): a pair test is rtr_device.h's
// pair_dist2, a mean is rtr_knn_row.h's knn_row_mean -- sqrtf and the division are correctly rounded, denormals kept.
#include "rtr_device.h"
#include "rtr_knn_row.h"

namespace rtr {

namespace {

constexpr int kItemWords = kNbItemWords;

// ---------------------------------------------------------------------------------
// Rows: the hot kernel.  The wave's LDS region holds 64 rows of CAP slots, slot s of lane l at word s * 64 + l: whatever
// slots the lanes of one access ask for, lane l reads bank l, so no access of the kernel has a bank conflict.  CAP is
// the capacity bucket of k (8, 16, 32 or 64) and WAVES the workgroup's size, chosen so that a workgroup takes at most
// 32 KB: 8 / 16 / 32 KB with four waves, 32 KB with two at CAP = 64 (launch_stat_rows).  A small k does not pay for 64.
struct LdsRow {
    float *base;  // slot 0 of this lane
    __device__ __forceinline__ float get(uint32_t s) const { return base[s * 64u]; }
    __device__ __forceinline__ void set(uint32_t s, float v) { base[s * 64u] = v; }
};

// Candidates are streamed and broadcast exactly as k_nb_count does (64 at a time, v_readlane with a wave-uniform lane);
// a pair within r2 that is not the lane's own upload index goes to the lane's row.  Most candidates fail the lane's one
// comparison with its worst value in registers; the lanes that take one diverge into the row's update.  mean[u] /
// found[u] (upload-order slots, preset by the caller for the points no item holds): the mean distance and min(k,
// candidates).  *tests += pair tests of live lanes, *updates += values written into rows: per wave in registers, two
// atomics per wave at its end (the waves are persistent: at most 16 384 of them).  The rows are the kernel's only LDS,
// so that five workgroups of 32 KB fill a CU's 160 KiB exactly.
template <int CAP, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_nb_rows(const float4 *__restrict__ rec, const uint32_t *__restrict__ items,
                                                        const uint32_t *__restrict__ cursor, uint32_t cap, float r2, uint32_t k,
                                                        float *__restrict__ mean, uint32_t *__restrict__ found,
                                                        unsigned long long *__restrict__ tests, unsigned long long *__restrict__ updates) {
    __shared__ float s_row[WAVES * 64 * CAP];
    const int lane = threadIdx.x & 63;
    LdsRow row{s_row + (threadIdx.x >> 6) * (64 * CAP) + lane};
    const uint32_t listed = *cursor, nitems = listed < cap ? listed : cap;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((uint64_t)blockIdx.x * (WAVES * 64) + threadIdx.x) >> 6));
    const uint32_t nwaves = (uint32_t)(((uint64_t)gridDim.x * (WAVES * 64)) >> 6);
    uint64_t n_tests = 0;  // (wave-uniform)
    uint32_t n_upd = 0;    // (per lane)
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
        const uint32_t nlive = (uint32_t)__popcll((unsigned long long)__ballot(live));
        KnnRowState st;
        for (int t = 0; t < 9; ++t) {
            const uint32_t lo = I[2 + 2 * t], hi = I[3 + 2 * t];
            for (uint32_t c0 = lo; c0 < hi; c0 += 64u) {
                const int m = (int)__builtin_amdgcn_readfirstlane((int)(hi - c0 < 64u ? hi - c0 : 64u));
                float4 cd = make_float4(0.f, 0.f, 0.f, 0.f);
                if (lane < m) cd = rec[c0 + (uint32_t)lane];
                const int cxi = __float_as_int(cd.x), cyi = __float_as_int(cd.y), czi = __float_as_int(cd.z), cui = __float_as_int(cd.w);
                for (int j = 0; j < m; ++j) {
                    const float cx = __int_as_float(__builtin_amdgcn_readlane(cxi, j)), cy = __int_as_float(__builtin_amdgcn_readlane(cyi, j)),
                                cz = __int_as_float(__builtin_amdgcn_readlane(czi, j));
                    const uint32_t cu = (uint32_t)__builtin_amdgcn_readlane(cui, j);
                    const float d2 = pair_dist2(x, y, z, cx, cy, cz);
                    if (live && d2 <= r2 && cu != u) n_upd += knn_row_insert(row, k, st, d2) ? 1u : 0u;
                }
                n_tests += (uint64_t)m * nlive;
            }
        }
        if (live) {
            knn_row_sort(row, st.count);
            mean[u] = knn_row_mean(row, st.count);
            found[u] = st.count;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_upd += __shfl_xor(n_upd, off, 64);  // (a wave's items: < 2^32 updates would need > 2^26 full rows)
    if (lane == 0) {
        if (n_tests) atomicAdd(tests, (unsigned long long)n_tests);
        if (n_upd) atomicAdd(updates, (unsigned long long)n_upd);
    }
}

// ---------------------------------------------------------------------------------
// The moments.  A sum over the n means that returns the same bits whatever the grid and the timing: partial[c] covers
// the upload indices 1024 c .. 1024 c + 1023, thread t of the workgroup adding the terms of 1024 c + t, + 256, + 512,
// + 768 in that order, the 64 lanes of a wave folded by a butterfly (lane l ends with the same tree for every l), the
// four waves added in order; k_stat_final folds the partial sums the same way, thread t taking partial[t], [t + 256],
// ... in order.  The shape depends on n alone.  Terms: pass 0 the mean itself, pass 1 (mean - mu)^2, both in fp64 with
// every operation rounded on its own; only the points with a row (a finite mean: found > 0) have a term.  *count (pass 0
// only): those points.  No floating-point atomic anywhere.
constexpr int kStatChunk = 1024;

__device__ __forceinline__ double block_sum_fixed(double v, double *s_w /*[4]*/) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    __syncthreads();  // (s_w may still be read from the previous round)
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ __launch_bounds__(kBlock) void k_stat_partial(const float *__restrict__ mean, uint64_t n, int pass, double mu,
                                                         double *__restrict__ partial, unsigned long long *__restrict__ count) {
    __shared__ double s_w[4];
    const uint64_t nchunks = (n + kStatChunk - 1) / kStatChunk;
    uint32_t have = 0;
    for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {  // (workgroup-uniform)
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < kStatChunk / kBlock; ++j) {
            const uint64_t i = c * kStatChunk + (uint64_t)j * kBlock + threadIdx.x;
            if (i >= n) continue;
            const float m = mean[i];
            if (!(m < __builtin_inff())) continue;
            const double d = pass == 0 ? (double)m : (double)m - mu;
            v = v + (pass == 0 ? d : d * d);
            ++have;
        }
        const double sum = block_sum_fixed(v, s_w);
        if (threadIdx.x == 0) partial[c] = sum;
    }
    if (pass != 0) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) have += __shfl_xor(have, off, 64);
    if ((threadIdx.x & 63) == 0 && have) atomicAdd(count, (unsigned long long)have);
}

__global__ __launch_bounds__(kBlock) void k_stat_final(const double *__restrict__ partial, uint64_t nchunks, double *__restrict__ out) {
    __shared__ double s_w[4];
    double v = 0.0;
    for (uint64_t c = threadIdx.x; c < nchunks; c += kBlock) v = v + partial[c];
    const double sum = block_sum_fixed(v, s_w);
    if (threadIdx.x == 0) *out = sum;
}

// ---------------------------------------------------------------------------------
// Hits.  hit(u) iff found[u] > 0 and (double)mean[u] <= t: exact.  A wave takes 64 consecutive upload indices and
// writes their two hit words whole (hit: (n + 31) / 32 words; no atomics).  stats [1] / [2] += hits / points with
// found == 0 (the non-finite points among them are the caller's to subtract): one atomic each per wave.
__global__ __launch_bounds__(kBlock) void k_stat_hits(const float *__restrict__ mean, const uint32_t *__restrict__ found, uint64_t n,
                                                      double t, uint32_t *__restrict__ hit, unsigned long long *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const uint64_t nw = (n + 31) / 32;
    uint64_t n_hit = 0, n_none = 0;  // (wave-uniform)
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i - (uint64_t)lane < n; i += (uint64_t)gridDim.x * kBlock) {
        bool pass = false, none = false;
        if (i < n) {
            const uint32_t f = found[i];
            none = f == 0u;
            pass = f > 0u && (double)mean[i] <= t;
        }
        const uint64_t b = __ballot(pass);
        n_hit += (uint64_t)__popcll((unsigned long long)b);
        n_none += (uint64_t)__popcll((unsigned long long)__ballot(none));
        if (lane == 0) {
            const uint64_t w = (i >> 6) * 2u;
            hit[w] = (uint32_t)b;
            if (w + 1u < nw) hit[w + 1u] = (uint32_t)(b >> 32);
        }
    }
    if (lane == 0) {
        if (n_hit) atomicAdd(stats + 1, (unsigned long long)n_hit);
        if (n_none) atomicAdd(stats + 2, (unsigned long long)n_none);
    }
}

template <int CAP, int WAVES>
void launch_rows(hipStream_t s, const float4 *rec, const uint32_t *items, const uint32_t *cursor, uint64_t cap, float r2, uint32_t k, float *mean,
                 uint32_t *found, uint64_t *tests, uint64_t *updates) {
    const uint64_t blocks = (cap + WAVES - 1) / WAVES;
    hipLaunchKernelGGL((k_nb_rows<CAP, WAVES>), dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(WAVES * 64), 0, s, rec, items, cursor,
                       (uint32_t)cap, r2, k, mean, found, (unsigned long long *)tests, (unsigned long long *)updates);
}

}  // namespace

uint64_t stat_partials(uint64_t n) { return (n + kStatChunk - 1) / kStatChunk; }

void launch_stat_rows(hipStream_t s, const float4 *rec, const uint32_t *items, const uint32_t *cursor, uint64_t cap, float r2, uint32_t k,
                      float *mean, uint32_t *found, uint64_t *tests, uint64_t *updates) {
    if (cap == 0) return;
    if (k <= 8) launch_rows<8, 4>(s, rec, items, cursor, cap, r2, k, mean, found, tests, updates);
    else if (k <= 16) launch_rows<16, 4>(s, rec, items, cursor, cap, r2, k, mean, found, tests, updates);
    else if (k <= 32) launch_rows<32, 4>(s, rec, items, cursor, cap, r2, k, mean, found, tests, updates);
    else launch_rows<64, 2>(s, rec, items, cursor, cap, r2, k, mean, found, tests, updates);
}

void launch_stat_sum(hipStream_t s, const float *mean, uint64_t n, int pass, double mu, double *partial, double *out, uint64_t *count) {
    const uint64_t nchunks = stat_partials(n);
    if (nchunks) {
        hipLaunchKernelGGL(k_stat_partial, dim3((unsigned)(nchunks < 4096 ? nchunks : 4096)), dim3(kBlock), 0, s, mean, n, pass, mu, partial,
                           (unsigned long long *)count);
    }
    hipLaunchKernelGGL(k_stat_final, dim3(1), dim3(kBlock), 0, s, partial, nchunks, out);
}

void launch_stat_hits(hipStream_t s, const float *mean, const uint32_t *found, uint64_t n, double t, uint32_t *hit, uint64_t *stats) {
    if (n == 0) return;
    const uint64_t blocks = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_stat_hits, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, s, mean, found, n, t, hit,
                       (unsigned long long *)stats);
}

}  // namespace rtr
