// rtr_normals.hip -- the gfx950 kernel of rtr_estimate_normals (include/rtr_normals.h section 6o): the unit normal and the
// surface variation of every resident point, from a PCA over the point and its k nearest neighbours within a radius.
// Everything up to the work list is rtr_select_neighbours' (rtr_neighbours.hip: key sweep, sort, gather, cells, items).
//   k_nb_normal_rows  one wave per item, one query point per lane, rtr_statistical.hip's k_nb_rows loop -- but the row
//                     remembers WHICH candidates it holds: two planes in LDS, the squared distance and the candidate's
//                     position among the sorted records, ordered by (d2, upload index) (rtr_normal_fit.h).  At the end
//                     each lane sorts its row, reads its neighbours' records again, forms the nine fp64 sums in row
//                     order, runs normal_fit and writes the normal, the curvature and the row's length to its point's
//                     upload-order slots.  No atomics but the per-wave counters.
// The arithmetic contract of rtr_kernels.hip holds here too (-ffp-contract=off): a pair test is rtr_device.h's
// pair_dist2, the differences of the sums are formed as it forms them, and everything behind them is rtr_normal_fit.h's
// fp64 with every operation rounded on its own; the only fused operations are sqrt_rn's explicit fma() residuals.
#include "rtr_device.h"
#include "rtr_normal_fit.h"

namespace rtr {

namespace {

constexpr int kItemWords = kNbItemWords;
// A/B builds only (make variant NAME=.. DEFS=-DRTR_NORMALS_LDS_PAD=16384; DESIGN.md, "Normals and curvature"): bytes of
// dynamic LDS that every workgroup takes and never touches, to run one capacity bucket at the occupancy of the next
#ifdef RTR_NORMALS_LDS_PAD
constexpr unsigned kLdsPad = RTR_NORMALS_LDS_PAD;
#else
constexpr unsigned kLdsPad = 0;
#endif

// The wave's LDS region holds 64 rows of CAP slots in two planes, slot s of lane l at word s * 64 + l of each: whatever
// slots the lanes of one access ask for, lane l reads bank l, so no access of the kernel has a bank conflict.  CAP is
// the capacity bucket of k (8, 16, 32 or 64) and WAVES the workgroup's size, chosen so that a workgroup takes at most
// 32 KB: 16 / 32 KB with four waves at CAP = 8 / 16, 32 KB with two at 32 and with one at 64 (launch_normal_rows).
struct LdsPairRow {
    float *d;       // slot 0 of this lane, the d2 plane
    uint32_t *p;    // ... the position plane
    __device__ __forceinline__ float d2(uint32_t s) const { return d[s * 64u]; }
    __device__ __forceinline__ uint32_t pos(uint32_t s) const { return p[s * 64u]; }
    __device__ __forceinline__ void set(uint32_t s, float v, uint32_t at) { d[s * 64u] = v, p[s * 64u] = at; }
};

// the upload index of a sorted position: asked for only where two squared distances are equal
struct RecIndex {
    const float4 *__restrict__ rec;
    __device__ __forceinline__ uint32_t operator()(uint32_t pos) const { return __float_as_uint(rec[pos].w); }
};

// Candidates are streamed and broadcast exactly as k_nb_rows does (64 at a time, v_readlane with a wave-uniform lane);
// the candidate's position c0 + j is wave-uniform and costs nothing to know.  A pair within r2 that is not the lane's
// own upload index goes to the lane's row; a candidate farther than the row's worst entry fails one comparison in
// registers.  normals[3 u ..] / curvature[u] / found[u]: upload-order slots, preset by the caller to 0 / +inf / 0; the
// kernel writes found for every point of the list and the other two for the points with a normal (found >= 2), so the
// preset values stand for the points no item holds and for those without a normal.  counts (device, zeroed): [0] +=
// pair tests of live lanes, [1] += entries written into rows, [2] += points with a normal, [3] += normals negated by
// the viewpoint rule: per wave in registers, at most four atomics per wave at its end (the waves are persistent).
template <int CAP, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_nb_normal_rows(const float4 *__restrict__ rec, const uint32_t *__restrict__ items,
                                                               const uint32_t *__restrict__ cursor, uint32_t cap, float r2, uint32_t k,
                                                               int with_view, float vx, float vy, float vz, float *__restrict__ normals,
                                                               float *__restrict__ curvature, uint32_t *__restrict__ found,
                                                               unsigned long long *__restrict__ counts) {
    __shared__ float s_d2[WAVES * 64 * CAP];
    __shared__ uint32_t s_pos[WAVES * 64 * CAP];
    const int lane = threadIdx.x & 63;
    const uint32_t base = (threadIdx.x >> 6) * (64 * CAP) + lane;
    LdsPairRow row{s_d2 + base, s_pos + base};
    const RecIndex index_of{rec};
    const float view[3] = {vx, vy, vz};
    const uint32_t listed = *cursor, nitems = listed < cap ? listed : cap;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((uint64_t)blockIdx.x * (WAVES * 64) + threadIdx.x) >> 6));
    const uint32_t nwaves = (uint32_t)(((uint64_t)gridDim.x * (WAVES * 64)) >> 6);
    uint64_t n_tests = 0, n_have = 0, n_flip = 0;  // (wave-uniform)
    uint32_t n_upd = 0;                            // (per lane)
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
        NormalRowState st;
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
                    if (live && d2 <= r2 && cu != u) n_upd += normal_row_insert(row, k, st, index_of, d2, c0 + (uint32_t)j, cu) ? 1u : 0u;
                }
                n_tests += (uint64_t)m * nlive;
            }
        }
        bool have = false, flipped = false;
        if (live) {
            found[u] = st.count;
            if (st.count >= 2u) {  // (RTR_NORMAL_MIN_FOUND)
                have = true;
                normal_row_sort(row, st.count, index_of);
                double S[3] = {0.0, 0.0, 0.0}, Q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (uint32_t t = 0; t < st.count; ++t) {
                    const float4 c = rec[row.pos(t)];
                    const double ex = (double)f_sub(x, c.x), ey = (double)f_sub(y, c.y), ez = (double)f_sub(z, c.z);
                    S[0] = S[0] + ex, S[1] = S[1] + ey, S[2] = S[2] + ez;
                    Q[0] = Q[0] + ex * ex, Q[1] = Q[1] + ex * ey, Q[2] = Q[2] + ex * ez;
                    Q[3] = Q[3] + ey * ey, Q[4] = Q[4] + ey * ez, Q[5] = Q[5] + ez * ez;
                }
                const float p[3] = {x, y, z};
                float nrm[3], curv;
                flipped = normal_fit(S, Q, st.count + 1u, p, with_view != 0, view, nrm, &curv);
                normals[3ull * u] = nrm[0], normals[3ull * u + 1u] = nrm[1], normals[3ull * u + 2u] = nrm[2];
                curvature[u] = curv;
            }
        }
        n_have += (uint64_t)__popcll((unsigned long long)__ballot(have));
        n_flip += (uint64_t)__popcll((unsigned long long)__ballot(flipped));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_upd += __shfl_xor(n_upd, off, 64);  // (a wave's items: < 2^32 updates would need > 2^26 full rows)
    if (lane == 0) {
        if (n_tests) atomicAdd(counts, (unsigned long long)n_tests);
        if (n_upd) atomicAdd(counts + 1, (unsigned long long)n_upd);
        if (n_have) atomicAdd(counts + 2, (unsigned long long)n_have);
        if (n_flip) atomicAdd(counts + 3, (unsigned long long)n_flip);
    }
}

template <int CAP, int WAVES>
void launch_rows(hipStream_t s, const float4 *rec, const uint32_t *items, const uint32_t *cursor, uint64_t cap, float r2, uint32_t k,
                 const float *view, float *normals, float *curvature, uint32_t *found, uint64_t *counts) {
    const uint64_t blocks = (cap + WAVES - 1) / WAVES;
    hipLaunchKernelGGL((k_nb_normal_rows<CAP, WAVES>), dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(WAVES * 64), kLdsPad, s, rec, items, cursor,
                       (uint32_t)cap, r2, k, view ? 1 : 0, view ? view[0] : 0.f, view ? view[1] : 0.f, view ? view[2] : 0.f, normals, curvature,
                       found, (unsigned long long *)counts);
}

}  // namespace

void launch_normal_rows(hipStream_t s, const float4 *rec, const uint32_t *items, const uint32_t *cursor, uint64_t cap, float r2, uint32_t k,
                        const float *view, float *normals, float *curvature, uint32_t *found, uint64_t *counts) {
    if (cap == 0) return;
    if (k <= 8) launch_rows<8, 4>(s, rec, items, cursor, cap, r2, k, view, normals, curvature, found, counts);
    else if (k <= 16) launch_rows<16, 4>(s, rec, items, cursor, cap, r2, k, view, normals, curvature, found, counts);
    else if (k <= 32) launch_rows<32, 2>(s, rec, items, cursor, cap, r2, k, view, normals, curvature, found, counts);
    else launch_rows<64, 1>(s, rec, items, cursor, cap, r2, k, view, normals, curvature, found, counts);
}

}  // namespace rtr
