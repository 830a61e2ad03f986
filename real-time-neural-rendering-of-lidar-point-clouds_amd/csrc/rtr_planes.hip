// rtr_planes.hip -- the gfx950 kernels of rtr.h section 6j.  k_set_bits marks rtr_fit_plane's sample in device words;
// k_count_bands is rtr_count_in_bands: how many resident points lie in each of up to kBandPass bands
// {a, b, c, d_lo, d_hi}, every chunk decoded at most ONCE for all of them.
//   Point test: u = (a x + b y) + c z, in = u + d_lo >= 0 && (-u) + d_hi >= 0, every product and sum rounded to fp32 on
// its own (-ffp-contract=off) -- clip_keep over the planes {a, b, c, d_lo} and {-a, -b, -c, d_hi} bit for bit (negation
// commutes with rounding; a sum's zero may differ in sign, which no comparison sees).
//   k_select's skeleton: one wave per 256-point chunk (lane l: points 4 l .. 4 l + 3), chunks dealt round robin, PACKED
// 64 headers classified per wave step, one per lane, against EVERY band of the pass on the header's box (chunk_box, then
// clip_box_outside / clip_box_inside on the band's two-plane Clip):
//   outside: no point of the chunk is in the band;
//   inside:  every point of it is -- the band's counter takes the chunk's population (256, the tail's count or, SEL, the
//            popcount of its eight selection words) without its coordinates: the wave's inside chunks of a band are
//            found by a ballot, their populations summed by shuffles, one LDS add per wave and band;
//   mixed:   one bit of the lane's 64-bit band mask.
// A chunk whose mask is not empty is decoded by the whole wave, once, and tested against the bands of its mask only (a
// wave-uniform loop over the set bits; the coefficients are kernel arguments read at a uniform index, i.e. scalar
// loads).  Four ballots per (chunk, band), one LDS add per wave; at the end one global 64-bit atomic per workgroup and
// non-zero band.  SEL: res = the selection in RESIDENT order (8 words per chunk); a chunk without a selected point is
// outside for every band before its header is read.
//   Not PACKED the boxes are k_chunk_bounds', which may hide a NaN: such a chunk is outside or mixed on its box, never
// inside (as k_select).  The chunk is wave-uniform there, so lane k classifies band k and the mask is one ballot.
// stats (device): [1] / [2] / [3] += (chunk, band) pairs outside / inside / mixed, three atomics per workgroup.
#include "rtr_device.h"

#include <algorithm>
#include <string.h>

namespace rtr {

namespace {

struct BandArgs {
    const float4 *x4, *y4, *z4;  // fp32 SoA (not PACKED) ...
    const float *bounds;         // ... and its chunk boxes
    PackedXyz pk;                // packed form (PACKED)
    uint64_t n;
    const uint32_t *res;         // SEL: the selection, resident order, 8 words per chunk
    unsigned long long *counts;  // [count] of this pass
    unsigned long long *stats;
};
struct BandSet {  // passed BY VALUE (like Clip): 1284 bytes of kernel arguments
    float v[kBandPass][5];
    int count;
};

__device__ __forceinline__ Clip band_clip(const float *b) {  // the band's two section 6d planes
    Clip c{};
    c.p[0][0] = b[0], c.p[0][1] = b[1], c.p[0][2] = b[2], c.p[0][3] = b[3];
    c.p[1][0] = -b[0], c.p[1][1] = -b[1], c.p[1][2] = -b[2], c.p[1][3] = b[4];
    c.count = 2;
    return c;
}
__device__ __forceinline__ uint32_t chunk_valid(uint64_t n, uint64_t c) {  // the points of chunk c below n (1..256)
    const uint64_t left = n - c * 256u;
    return left >= 256u ? 256u : (uint32_t)left;
}
// The wave counts the decoded chunk's points (ok[k]: point 4 lane + k is part of the population) in the bands of `mask`.
__device__ __forceinline__ void count_chunk(const BandSet &bs, unsigned long long mask, const float4 &X, const float4 &Y, const float4 &Z,
                                            const bool ok[4], int lane, uint32_t *s_cnt) {
    const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
    while (mask) {  // (wave-uniform)
        const int k = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const float a = bs.v[k][0], b = bs.v[k][1], c = bs.v[k][2], dlo = bs.v[k][3], dhi = bs.v[k][4];
        uint32_t hits = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float ax = a * xs[q], by = b * ys[q], s = ax + by, cz = c * zs[q], u = s + cz;
            const float v0 = u + dlo, v1 = (-u) + dhi;
            hits += (uint32_t)__popcll(__ballot(ok[q] && v0 >= 0.f && v1 >= 0.f));
        }
        if (lane == 0 && hits) atomicAdd(&s_cnt[k], hits);
    }
}

template <bool PACKED, bool SEL>
__global__ __launch_bounds__(kBlock) void k_count_bands(BandArgs a, BandSet bs) {
    __shared__ uint32_t s_cnt[kBandPass];  // (a workgroup sees fewer than 2^32 points)
    __shared__ uint32_t s_st[3];
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const uint64_t n4 = (a.n + 3) / 4, nchunks = (n4 + 63) / 64;
    const int nb = bs.count;
    if (threadIdx.x < kBandPass) s_cnt[threadIdx.x] = 0u;
    if (threadIdx.x < 3) s_st[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t st[3] = {0u, 0u, 0u};  // (per lane: pairs outside / inside / mixed)
    if (!PACKED) {
        for (uint64_t c = wave; c < nchunks; c += nwaves) {  // (wave-uniform)
            uint32_t w = 0xFFFFFFFFu;
            if (SEL) w = a.res[8 * c + (lane >> 3)];
            if (SEL && __ballot(w != 0u) == 0ull) {  // (no selected point: outside for every band)
                if (lane < nb) st[0] += 1u;
                continue;
            }
            bool mixed = false;
            if (lane < nb) {
                const float *b = a.bounds + 6 * c;
                const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
                mixed = !clip_box_outside(band_clip(bs.v[lane]), lo, hi);
                st[mixed ? 2 : 0] += 1u;
            }
            const unsigned long long mask = __ballot(mixed);
            if (!mask) continue;
            const uint64_t i = c * 64u + (uint64_t)lane, ic = i < n4 ? i : n4 - 1u;
            const float4 X = ld_stream(a.x4 + ic), Y = ld_stream(a.y4 + ic), Z = ld_stream(a.z4 + ic);
            const uint64_t i0 = c * 256u + 4u * (uint64_t)lane;
            const uint32_t bits = SEL ? keep_lane_bits(w, (uint32_t)lane) : 15u;
            const bool ok[4] = {i0 < a.n && (bits & 1u), i0 + 1 < a.n && (bits & 2u), i0 + 2 < a.n && (bits & 4u), i0 + 3 < a.n && (bits & 8u)};
            count_chunk(bs, mask, X, Y, Z, ok, lane, s_cnt);
        }
    } else {
        for (uint64_t j0 = 0; wave + nwaves * j0 < nchunks; j0 += 64u) {  // (wave-uniform)
            const uint64_t chunk = wave + nwaves * (j0 + (uint64_t)lane);
            const bool valid = chunk < nchunks;
            unsigned long long mine = 0ull;  // the bands this lane's chunk is mixed for
            uint32_t pop = 0u;
            bool boxed = false;  // the lane classifies its chunk band by band
            float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
            if (valid) {
                pop = chunk_valid(a.n, chunk);
                if (SEL) {  // (the selection holds no bit at or past n)
                    const uint4 *w = reinterpret_cast<const uint4 *>(a.res + 8 * chunk);
                    const uint4 w0 = w[0], w1 = w[1];
                    pop = (uint32_t)(__popc(w0.x) + __popc(w0.y) + __popc(w0.z) + __popc(w0.w) + __popc(w1.x) + __popc(w1.y) + __popc(w1.z) + __popc(w1.w));
                }
                if (pop == 0u) {
                    st[0] += (uint32_t)nb;
                } else {
                    const uint4 h0 = a.pk.hdr[2 * chunk];
                    const uint32_t wbox = reinterpret_cast<const uint32_t *>(a.pk.hdr + 2 * chunk + 1)[3];  // (the header's own 32 bytes)
                    boxed = chunk_box(h0.x, h0.y, h0.z, h0.w, wbox, lo, hi);
                    if (!boxed) {
                        mine = nb == 64 ? ~0ull : (1ull << nb) - 1ull;
                        st[2] += (uint32_t)nb;
                    }
                }
            }
            if (__ballot(boxed)) {  // (wave-uniform)
                for (int k = 0; k < nb; ++k) {  // (every lane runs the loop: uniform trip count and coefficient loads)
                    const Clip cl = band_clip(bs.v[k]);
                    const bool out = boxed && clip_box_outside(cl, lo, hi), in = boxed && !out && clip_box_inside(cl, lo, hi);
                    st[0] += out, st[1] += in, st[2] += boxed && !out && !in;
                    if (boxed && !out && !in) mine |= 1ull << k;
                    if (__ballot(in)) {  // (rare for thin bands) the populations of the wave's inside chunks: one LDS add
                        uint32_t sum = in ? pop : 0u;
#pragma unroll
                        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
                        if (lane == 0) atomicAdd(&s_cnt[k], sum);
                    }
                }
            }
            unsigned long long todo = __ballot(mine != 0ull);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const uint64_t cc = wave + nwaves * (j0 + (uint64_t)l);
                const unsigned long long mask = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), l) << 32) |
                                                (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, l);
                const uint4 h0 = a.pk.hdr[2 * cc], h1 = a.pk.hdr[2 * cc + 1];
                const ChunkRawA raw_a = load_chunk_a(a.pk.planes, h0, h1, lane);
                const ChunkRaw raw = load_chunk_b(a.pk.planes_b, h0, h1, lane);
                float4 X, Y, Z;
                unpack_chunk(raw_a, raw, h0.w, h0.x, h0.y, h0.z, X, Y, Z, lane);
                const uint64_t i0 = cc * 256u + 4u * (uint64_t)lane;
                const uint32_t bits = SEL ? keep_lane_bits(a.res[8 * cc + (lane >> 3)], (uint32_t)lane) : 15u;
                const bool ok[4] = {i0 < a.n && (bits & 1u), i0 + 1 < a.n && (bits & 2u), i0 + 2 < a.n && (bits & 4u), i0 + 3 < a.n && (bits & 8u)};
                count_chunk(bs, mask, X, Y, Z, ok, lane, s_cnt);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) st[q] += __shfl_xor(st[q], off, 64);
        if (lane == 0 && st[q]) atomicAdd(&s_st[q], st[q]);
    }
    __syncthreads();
    if ((int)threadIdx.x < nb && s_cnt[threadIdx.x]) atomicAdd(a.counts + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
    if (threadIdx.x < 3 && s_st[threadIdx.x]) atomicAdd(a.stats + 1 + threadIdx.x, (unsigned long long)s_st[threadIdx.x]);
}

}  // namespace

// RTR_BANDS_SELECTED on a sorted cloud: the selection in resident order, res[8 c + j] = word j of chunk c (k_keep_build's
// gather through perm, read-only on `up` and without its summary): once per call, not per pass
__global__ __launch_bounds__(kBlock) void k_sel_gather(const uint32_t *__restrict__ up, const uint32_t *__restrict__ perm, uint64_t n,
                                                       uint32_t *__restrict__ res) {
    const int lane = threadIdx.x & 63;
    const uint64_t nchunks = (n + 255) / 256;
    for (uint64_t c = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; c < nchunks; c += ((uint64_t)gridDim.x * kBlock) >> 6) {
        uint32_t u[4];
        bool kept[4], valid[4];
        remove_gather(up, perm, n, c, lane, u, kept, valid);
        unsigned long long b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = __ballot(kept[k]);
        if (lane < 8) {  // (ballot k: bit l = point 4 l + k; word j = lanes 8 j .. 8 j + 7)
            const int sh = 8 * lane;
            res[8 * c + lane] = spread_nibbles((uint32_t)(b[0] >> sh)) | (spread_nibbles((uint32_t)(b[1] >> sh)) << 1) |
                                (spread_nibbles((uint32_t)(b[2] >> sh)) << 2) | (spread_nibbles((uint32_t)(b[3] >> sh)) << 3);
        }
    }
}
void launch_sel_gather(hipStream_t s, const uint32_t *up, const uint32_t *perm, uint64_t n, uint32_t *res) {
    const uint64_t nchunks = (n + 255) / 256;
    if (nchunks == 0) return;
    hipLaunchKernelGGL(k_sel_gather, dim3((unsigned)std::min<uint64_t>((nchunks + 3) / 4, 4096)), dim3(kBlock), 0, s, up, perm, n, res);
}

// rtr_fit_plane's sample: the bit of every index (below n, the caller's promise) into zeroed upload-order words
__global__ __launch_bounds__(kBlock) void k_set_bits(const uint32_t *__restrict__ idx, uint64_t count, uint32_t *__restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < count) atomicOr(words + (idx[i] >> 5), 1u << (idx[i] & 31u));
}
void launch_set_bits(hipStream_t s, const uint32_t *idx, uint64_t count, uint32_t *words) {
    if (count == 0) return;
    hipLaunchKernelGGL(k_set_bits, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, idx, count, words);
}

void launch_count_bands(hipStream_t s, const Cloud &c, const float *bounds, const float *bands, uint32_t count, const uint32_t *res,
                        uint64_t *counts, uint64_t *stats) {
    const uint64_t n4 = (c.n + 3) / 4, nchunks = (n4 + 63) / 64;
    if (nchunks == 0 || c.n == 0) return;
    const bool packed = c.pk.hdr != nullptr;
    BandArgs a{(const float4 *)c.x, (const float4 *)c.y, (const float4 *)c.z, bounds, c.pk, c.n, res, nullptr, (unsigned long long *)stats};
    const dim3 grid((unsigned)std::min<uint64_t>((nchunks + 3) / 4, 2048)), block(kBlock);  // (k_select's grid)
    for (uint32_t k0 = 0; k0 < count; k0 += kBandPass) {
        BandSet bs{};
        bs.count = (int)std::min<uint32_t>(kBandPass, count - k0);
        memcpy(bs.v, bands + 5 * (size_t)k0, (size_t)bs.count * 5 * sizeof(float));
        a.counts = (unsigned long long *)counts + k0;
        if (packed && res) hipLaunchKernelGGL((k_count_bands<true, true>), grid, block, 0, s, a, bs);
        else if (packed) hipLaunchKernelGGL((k_count_bands<true, false>), grid, block, 0, s, a, bs);
        else if (res) hipLaunchKernelGGL((k_count_bands<false, true>), grid, block, 0, s, a, bs);
        else hipLaunchKernelGGL((k_count_bands<false, false>), grid, block, 0, s, a, bs);
    }
}

}  // namespace rtr
