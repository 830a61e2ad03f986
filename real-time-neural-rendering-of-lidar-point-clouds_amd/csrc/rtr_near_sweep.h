// rtr_near_sweep.h -- the sweep over the RESIDENT chunks that rtr_near.hip (rtr_select_near, rtr.h section 6k), rtr_nearest.hip
// (rtr_nearest_points, 6l) and rtr_nearest_k.hip (rtr_nearest_k_points, 6m) share: the box rejection on headers, the column
// lookup, the reach test and the per-point fallback, written once.  What a call does with an accepted pair is its OP (see "OP"
// below): 6k ORs bits, 6l keeps minima, 6m the k smallest.  Device-only, as rtr_device.h: included by those three files only.
#pragma once
#include "rtr_device.h"
#include "rtr_neighbour_cell.h"

namespace rtr {

// the key of an IN-SPAN cell given by its three indices (kNbCellMin .. kNbCellMax each)
__device__ __forceinline__ uint64_t near_cell_key(int32_t cx, int32_t cy, int32_t cz) {
    return ((uint64_t)(uint32_t)(cx + kNbBias) << 42) | ((uint64_t)(uint32_t)(cy + kNbBias) << 21) | (uint64_t)(uint32_t)(cz + kNbBias);
}
__device__ __forceinline__ float bcastf(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// ---------------------------------------------------------------------------------
// Sweep: the hot kernel.  One wave per 256-point chunk of the RESIDENT cloud (lane l: points 4 l .. 4 l + 3), chunks dealt
// round robin.  PACKED: 64 headers are classified per wave step, one per lane, on chunk_box; else the boxes are
// k_chunk_bounds' (a NaN may hide behind a finite box there: a NaN point is near nothing, so the box still decides for
// the chunk's other points, and the pair test turns the NaN away by itself).
//   1. A chunk whose box, inflated by h on each side, does not meet the box of the given points is SKIPPED: compared in
//      fp64 (exact differences); a near pair is less than h apart on every axis (rtr_neighbour_cell.h).
//   2. The box's cells, floor(lo / h) .. floor(hi / h) per axis (the division is monotone: every point of the chunk has
//      its cell in that range, wherever it lies), widened by one cell and CLIPPED TO THE SPAN BY CELL INDEX -- a cell
//      beyond the span has no key, and the 21-bit fields have no room for it -- are the only cells that can hold a given
//      point near a point of the chunk.  An empty range (the chunk lies more than one cell beyond the span): skipped.
//   3. Up to kNearCols (x, y) columns: lane t searches the sorted given keys for column t's contiguous range, cells
//      z_lo .. z_hi (two binary searches, the lanes side by side).  Every range empty: skipped, still on the header.
//      Up to kNearColsMax columns are taken in batches of kNearCols (the chunk is decoded before the second batch).
//   4. Else the chunk is decoded once, and the ranges are streamed 64 records at a time with one coalesced load; each
//      candidate is broadcast out of its lane's registers (v_readlane at a wave-uniform lane, as k_nb_count) and every
//      lane tests its four points against it (OP::tile).  A column, and a tile of 64 records, whose cells lie within one
//      cell of NO lane's points is passed over untested (see "REACH" below): a chunk that straddles a seam of the cloud's
//      order has a box far wider than its points, and would otherwise test everything between its halves.
//   A range of more than kNearCols columns in at most kNearCols x slabs gets one coarser look first: lane t asks whether
//   slab t holds any key between the range's first and last cell in it; no slab does: skipped on the header.
//   A chunk without a box decision -- a packed chunk without a box, a box that is not finite, a range of more than
//   kNearColsMax columns -- is decoded and takes the PER-POINT path: every point finds its own cell (neighbour_axis'
//   arithmetic, without its span check), gives up when that lies more than one cell beyond the span, and walks the up to
//   9 column ranges around it, clipped to the span by cell index as above.  Correct, not fast.
// cnt (device): [0] += resident points that hit, [1] += pair tests, [2] / [3] += chunks skipped / decoded: folded per
// wave, per workgroup in LDS, four atomics per workgroup.
//
// OP: what the call keeps of the accepted pairs; passed by value to the kernel, one OP::Chunk of lane state per chunk.
//   kEarlyExit           the wave leaves a chunk as soon as all its points have hit (nothing is kept per candidate)
//   begin(ch, a, i0)     the lane's state for its four points 4 lane .. 4 lane + 3 of the chunk, i0 the first's resident index
//   tile(ch, a, xs, ys, zs, cd, mm, lane, hb)
//                        the tile's mm candidates, lane t's record in cd: every pair test of the tile; hb |= the lane's
//                        points that accepted one
//   accept(ch, k, d2, cd)   per-point path, not kEarlyExit: the lane's point k accepted the candidate cd at distance d2
//   finish(ch, a, i0, lane, hb, w)   the chunk is through: the lane's results, w.hits
constexpr int kNearCols = 64;               // columns looked up side by side, one per lane
constexpr int kNearColsMax = 64 * kNearCols;  // ... and per chunk, in batches

struct NearArgs {
    PackedXyz pk;                // packed form (PACKED)
    const float4 *x4, *y4, *z4;  // fp32 SoA (not PACKED) ...
    const float *bounds;         // ... and its chunk boxes
    const uint32_t *perm;        // PERM: resident index -> upload index
    uint64_t n;
    const uint64_t *keys;  // the m sorted keys of the given points with a cell ...
    const float4 *rec;     // ... and their records
    uint32_t m;
    float r2;
    double h, glo[3], ghi[3];  // the cell edge; the given points' box
    unsigned long long *cnt;
};

struct NearWave {  // one wave's tallies (wave-uniform but `lane_tests`)
    uint64_t hits, tests, lane_tests;
    uint32_t skipped, decoded;
};

// w.hits += the points of the wave with a bit in hb
__device__ __forceinline__ void near_count_hits(uint32_t hb, NearWave &w) {
    uint32_t cnt = (uint32_t)__popc(hb);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    w.hits += cnt;
}

// one chunk, wave-uniform: boxed / lo / hi as classified (the box already meets the given points' box)
template <bool PACKED, class OP>
__device__ __forceinline__ void near_chunk(const NearArgs &a, const OP &op, uint64_t chunk, bool boxed, const float lo[3], const float hi[3],
                                           int lane, NearWave &w) {
    const int32_t cmin = kNbCellMin, cmax = kNbCellMax;
    int32_t c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
    bool per_point = !boxed;
    uint32_t ncols = 0, ny = 1;
    if (boxed) {
        bool empty = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double ql = __builtin_floor((double)lo[k] / a.h) - 1.0, qh = __builtin_floor((double)hi[k] / a.h) + 1.0;
            ql = ql < (double)cmin ? (double)cmin : ql;
            qh = qh > (double)cmax ? (double)cmax : qh;
            empty = empty || !(ql <= qh);
            c0[k] = empty ? 0 : (int32_t)ql, c1[k] = empty ? 0 : (int32_t)qh;
        }
        if (empty) {
            w.skipped += 1u;
            return;
        }
        const uint64_t nx = (uint64_t)(c1[0] - c0[0]) + 1u, nyy = (uint64_t)(c1[1] - c0[1]) + 1u;
        per_point = nx * nyy > (uint64_t)kNearColsMax;
        ncols = per_point ? 0u : (uint32_t)(nx * nyy), ny = (uint32_t)nyy;
        if (nx * nyy > (uint64_t)kNearCols && nx <= (uint64_t)kNearCols) {  // more than one batch of columns, few x slabs: lane t asks whether
            bool any = false;  // slab t holds a key at all between its first and its last cell of the range (a superset of them)
            if ((uint32_t)lane < (uint32_t)nx) {
                const int32_t cx = c0[0] + lane;
                any = key_lower_bound(a.keys, a.m, near_cell_key(cx, c1[1], c1[2]) + 1u) > key_lower_bound(a.keys, a.m, near_cell_key(cx, c0[1], c0[2]));
            }
            if (__ballot(any) == 0ull) {
                w.skipped += 1u;
                return;
            }
        }
    }
    // column `col` of the range (x-major) and its part of the sorted given points: lane t of a batch takes column cb + t
    uint32_t rlo = 0, rhi = 0;
    int32_t colx = 0, coly = 0;
    auto search = [&](uint32_t cb) {
        const uint32_t col = cb + (uint32_t)lane;
        rlo = rhi = 0u;
        if (col < ncols) {
            colx = c0[0] + (int32_t)(col / ny), coly = c0[1] + (int32_t)(col % ny);
            rlo = key_lower_bound(a.keys, a.m, near_cell_key(colx, coly, c0[2]));
            rhi = key_lower_bound(a.keys, a.m, near_cell_key(colx, coly, c1[2]) + 1u);
        }
    };
    if (!per_point) {
        search(0u);
        if (ncols <= (uint32_t)kNearCols && __ballot(rhi > rlo) == 0ull) {
            w.skipped += 1u;
            return;
        }
    }
    w.decoded += 1u;

    // the chunk's points; those at or past n read as NaN, which no test accepts
    float4 X, Y, Z;
    if (PACKED) {
        const uint4 h0 = a.pk.hdr[2 * chunk], h1 = a.pk.hdr[2 * chunk + 1];
        const ChunkRawA raw_a = load_chunk_a(a.pk.planes, h0, h1, lane);
        const ChunkRaw raw = load_chunk_b(a.pk.planes_b, h0, h1, lane);
        unpack_chunk(raw_a, raw, h0.w, h0.x, h0.y, h0.z, X, Y, Z, lane);
    } else {
        const uint64_t n4 = (a.n + 3) / 4, i = chunk * 64u + (uint64_t)lane, ic = i < n4 ? i : n4 - 1u;
        X = ld_stream(a.x4 + ic), Y = ld_stream(a.y4 + ic), Z = ld_stream(a.z4 + ic);
    }
    const uint64_t i0 = chunk * 256u + 4u * (uint64_t)lane;
    const float nan = __uint_as_float(0x7FC00000u);
    float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
    uint32_t valid = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool v = i0 + (uint64_t)k < a.n;
        valid |= (v ? 1u : 0u) << k;
        xs[k] = v ? xs[k] : nan;
    }
    uint32_t hb = 0;  // the lane's points that have hit
    typename OP::Chunk ch;
    op.begin(ch, a, i0);

    if (!per_point) {
        const uint32_t nvalid = (uint32_t)(a.n - chunk * 256u < 256u ? a.n - chunk * 256u : 256u);
        // The lane's REACH: the cells of its points that are numbers (neighbour_axis' quotient and floor, without the span
        // check), widened by one.  A pair the relation accepts has cells at most one apart on every axis
        // (rtr_neighbour_cell.h), so a column or a tile of candidates whose cells lie in no lane's reach holds nothing
        // that any point of the chunk accepts, and is passed over.  (The lanes out of reach of a tile that is tested test
        // it too: for nothing, and harmlessly.)
        int32_t rl[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, rh[3] = {-0x7FFFFFFF, -0x7FFFFFFF, -0x7FFFFFFF};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float p[3] = {xs[k], ys[k], zs[k]};
            const bool num = (p[0] - p[0] == 0.0f) && (p[1] - p[1] == 0.0f) && (p[2] - p[2] == 0.0f);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                double f = __builtin_floor((double)p[ax] / a.h);
                f = f < -2097152.0 ? -2097152.0 : (f > 2097152.0 ? 2097152.0 : f);  // (far beyond the span either way)
                const int32_t q = num ? (int32_t)f : 0;
                rl[ax] = num && q - 1 < rl[ax] ? q - 1 : rl[ax];
                rh[ax] = num && q + 1 > rh[ax] ? q + 1 : rh[ax];
            }
        }
        bool done = false;
        for (uint32_t cb = 0; cb < ncols && !done; cb += (uint32_t)kNearCols) {  // (wave-uniform)
            if (cb) search(cb);
        unsigned long long cols = __ballot(rhi > rlo);
        while (cols && !done) {  // (wave-uniform)
            const int t = __ffsll((long long)cols) - 1;
            cols &= cols - 1;
            const uint32_t lo_t = (uint32_t)__builtin_amdgcn_readlane((int)rlo, t), hi_t = (uint32_t)__builtin_amdgcn_readlane((int)rhi, t);
            const int32_t cxt = __builtin_amdgcn_readlane(colx, t), cyt = __builtin_amdgcn_readlane(coly, t);
            const bool col_reach = cxt >= rl[0] && cxt <= rh[0] && cyt >= rl[1] && cyt <= rh[1];
            if (__ballot(col_reach) == 0ull) continue;
            for (uint32_t b0 = lo_t; b0 < hi_t; b0 += 64u) {
                const int mm = (int)__builtin_amdgcn_readfirstlane((int)(hi_t - b0 < 64u ? hi_t - b0 : 64u));
                // the tile's cells in z: those of its first and last key (one column, sorted by z)
                const int32_t z0 = (int32_t)((uint32_t)a.keys[b0] & 0x1FFFFFu) - kNbBias;
                const int32_t z1 = (int32_t)((uint32_t)a.keys[b0 + (uint32_t)mm - 1u] & 0x1FFFFFu) - kNbBias;
                if (__ballot(col_reach && z1 >= rl[2] && z0 <= rh[2]) == 0ull) continue;
                float4 cd = make_float4(0.f, 0.f, 0.f, 0.f);
                if (lane < mm) cd = a.rec[b0 + (uint32_t)lane];
                op.tile(ch, a, xs, ys, zs, cd, mm, lane, hb);
                w.tests += (uint64_t)mm * nvalid;
                if (OP::kEarlyExit && __ballot(hb != valid) == 0ull) {
                    done = true;
                    break;
                }
            }
        }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // (unrolled: the quad stays in registers)
            const float p[3] = {xs[k], ys[k], zs[k]};
            int32_t q[3];
            bool ok = true;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const double f = __builtin_floor((double)p[ax] / a.h);
                ok = ok && (p[ax] - p[ax] == 0.0f) && f >= (double)cmin - 1.0 && f <= (double)cmax + 1.0;
                q[ax] = ok ? (int32_t)f : 0;
            }
            if (!ok) continue;  // (not a number, or more than one cell beyond the span: near nothing)
            const int32_t z0 = q[2] - 1 < cmin ? cmin : q[2] - 1, z1 = q[2] + 1 > cmax ? cmax : q[2] + 1;
            for (int d = 0; d < 9; ++d) {
                const int32_t cx = q[0] + d / 3 - 1, cy = q[1] + d % 3 - 1;
                if (cx < cmin || cx > cmax || cy < cmin || cy > cmax) continue;
                if (OP::kEarlyExit && ((hb >> k) & 1u)) break;
                const uint32_t b = key_lower_bound(a.keys, a.m, near_cell_key(cx, cy, z0));
                const uint32_t e = key_lower_bound(a.keys, a.m, near_cell_key(cx, cy, z1) + 1u);
                for (uint32_t j = b; j < e; ++j) {
                    const float4 cd = a.rec[j];
                    const float d2 = pair_dist2(p[0], p[1], p[2], cd.x, cd.y, cd.z);
                    w.lane_tests += 1u;
                    if (d2 <= a.r2) {
                        hb |= 1u << k;
                        if (OP::kEarlyExit) break;
                        op.accept(ch, k, d2, cd);
                    }
                }
            }
        }
    }
    op.finish(ch, a, i0, lane, hb, w);
}

// the body of a sweep kernel: kBlock threads per workgroup, any grid
template <bool PACKED, class OP>
__device__ __forceinline__ void near_sweep(const NearArgs &a, const OP &op) {
    __shared__ unsigned long long s_cnt[4];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const uint64_t nchunks = (a.n + 255) / 256;
    NearWave w{0, 0, 0, 0, 0};
    if (!PACKED) {
        for (uint64_t c = wave; c < nchunks; c += nwaves) {  // (wave-uniform)
            const float *b = a.bounds + 6 * c;
            const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
            bool boxed = true, away = false;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                boxed = boxed && (lo[k] - lo[k] == 0.0f) && (hi[k] - hi[k] == 0.0f) && lo[k] <= hi[k];
                away = away || (double)lo[k] - a.h > a.ghi[k] || (double)hi[k] + a.h < a.glo[k];
            }
            if (boxed && away) {
                w.skipped += 1u;
                continue;
            }
            near_chunk<PACKED, OP>(a, op, c, boxed, lo, hi, lane, w);
        }
    } else {
        for (uint64_t j0 = 0; wave + nwaves * j0 < nchunks; j0 += 64u) {  // (wave-uniform)
            const uint64_t chunk = wave + nwaves * (j0 + (uint64_t)lane);
            bool boxed = false, todo = false;
            float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
            if (chunk < nchunks) {
                const uint4 h0 = a.pk.hdr[2 * chunk];
                const uint32_t wbox = reinterpret_cast<const uint32_t *>(a.pk.hdr + 2 * chunk + 1)[3];  // (the header's own 32 bytes)
                boxed = chunk_box(h0.x, h0.y, h0.z, h0.w, wbox, lo, hi);
                bool away = false;
#pragma unroll
                for (int k = 0; k < 3; ++k) away = away || (double)lo[k] - a.h > a.ghi[k] || (double)hi[k] + a.h < a.glo[k];
                todo = !(boxed && away);
            }
            w.skipped += (uint32_t)__popcll(__ballot(chunk < nchunks && !todo));
            unsigned long long rest = __ballot(todo);
            while (rest) {  // (wave-uniform)
                const int l = __ffsll((long long)rest) - 1;
                rest &= rest - 1;
                const float ulo[3] = {bcastf(lo[0], l), bcastf(lo[1], l), bcastf(lo[2], l)};
                const float uhi[3] = {bcastf(hi[0], l), bcastf(hi[1], l), bcastf(hi[2], l)};
                const bool ub = ((__ballot(boxed) >> l) & 1ull) != 0ull;
                near_chunk<PACKED, OP>(a, op, wave + nwaves * (j0 + (uint64_t)l), ub, ulo, uhi, lane, w);
            }
        }
    }
    uint64_t lt = w.lane_tests;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t l0 = __shfl_xor((uint32_t)lt, off, 64), l1 = __shfl_xor((uint32_t)(lt >> 32), off, 64);
        lt += (uint64_t)l0 | ((uint64_t)l1 << 32);
    }
    if (lane == 0) {
        const unsigned long long v[4] = {w.hits, w.tests + lt, w.skipped, w.decoded};
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (v[q]) atomicAdd(&s_cnt[q], v[q]);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(a.cnt + threadIdx.x, s_cnt[threadIdx.x]);
}

// what a sweep's launcher fills in of NearArgs for every OP; grid: k_select's
inline void near_sweep_args(NearArgs &a, const Cloud &c, const float *bounds, const uint32_t *perm, const uint64_t *keys, const float4 *rec,
                            uint64_t m, float radius, float r2, const double glo[3], const double ghi[3], uint64_t *counters) {
    a.pk = c.pk, a.x4 = (const float4 *)c.x, a.y4 = (const float4 *)c.y, a.z4 = (const float4 *)c.z, a.bounds = bounds, a.perm = perm;
    a.n = c.n, a.keys = keys, a.rec = rec, a.m = (uint32_t)m, a.r2 = r2, a.h = neighbour_cell_edge(radius);
    for (int k = 0; k < 3; ++k) a.glo[k] = glo[k], a.ghi[k] = ghi[k];
    a.cnt = (unsigned long long *)counters;
}

}  // namespace rtr
