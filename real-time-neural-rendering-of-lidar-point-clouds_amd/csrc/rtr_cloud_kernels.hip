// rtr_cloud_kernels.hip -- gfx950 kernels that edit or query the resident cloud outside a frame: iota, keep mask, remove,
// scan, the write bits, the packed headers' unit shift and wide-chunk count, select.  The arithmetic contract of
// rtr_kernels.hip holds here too (-ffp-contract=off: the selection runs the frame's own project_point).
#include "rtr_device.h"
#include "rtr_remove_index.h"
#include "rtr_write_index.h"

#include <type_traits>

namespace rtr {

// ---- what the kernels of this file share ----------------------------------------------------------------------------
// One wave per 256-point chunk (lane l: points 4 l .. 4 l + 3): a wave's first chunk (the kernels that start at chunk c0
// add it) and its stride, and the grid of such a launch -- four waves per workgroup, at most `cap` workgroups.
__device__ __forceinline__ uint64_t wave_first() { return ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; }
__device__ __forceinline__ uint64_t wave_stride() { return ((uint64_t)gridDim.x * kBlock) >> 6; }
static dim3 chunk_grid(uint64_t nchunks, uint64_t cap) {  // (nchunks > 0)
    const uint64_t blocks = (nchunks + 3) / 4;
    return dim3((unsigned)(blocks < cap ? blocks : cap));
}
// A chunk's 256 bits from four ballots (ballot k: bit l = point 4 l + k), as upload-order words: word j of the chunk =
// points 32 j .. 32 j + 31 = lanes 8 j .. 8 j + 7.  Returns word `lane` of the eight; only lanes 0..7 may call it.
__device__ __forceinline__ uint32_t chunk_words(unsigned long long b0, unsigned long long b1, unsigned long long b2,
                                                unsigned long long b3, int lane) {
    const int sh = 8 * lane;
    return spread_nibbles((uint32_t)(b0 >> sh)) | (spread_nibbles((uint32_t)(b1 >> sh)) << 1) |
           (spread_nibbles((uint32_t)(b2 >> sh)) << 2) | (spread_nibbles((uint32_t)(b3 >> sh)) << 3);
}

__global__ __launch_bounds__(kBlock) void k_iota(uint32_t *__restrict__ out, uint64_t n, uint64_t first) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) out[i] = (uint32_t)(first + i);
}
void launch_iota(hipStream_t s, uint32_t *out, uint64_t n, uint64_t first) {
    if (n == 0) return;
    const uint64_t blocks = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_iota, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(kBlock), 0, s, out, n, first);
}

// The keep mask in resident order (rtr_set_point_keep, after a sort): one wave per 256-point chunk, lane l gathers the
// bits of its points 4 l .. 4 l + 3 from the upload-order mask (through perm when the cloud is sorted), the four ballots
// are interleaved into the chunk's eight words (chunk_words), and lane 0 writes the chunk's summary
// (keep_chunk_state: the same rule on the ballots).  Points at or past n are hidden and do not count.
__global__ __launch_bounds__(kBlock) void k_keep_build(const uint32_t *__restrict__ up, const uint32_t *__restrict__ perm,
                                                       uint64_t n, uint32_t *__restrict__ res, uint8_t *__restrict__ sum,
                                                       uint64_t c0) {
    const int lane = threadIdx.x & 63;
    const uint64_t nchunks = (n + 255) / 256;
    for (uint64_t c = c0 + wave_first(); c < nchunks; c += wave_stride()) {
        bool kept[4], valid[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t r = c * 256u + 4u * (uint64_t)lane + (uint64_t)k;
            valid[k] = r < n;
            const uint64_t u = valid[k] ? (perm ? (uint64_t)perm[r] : r) : 0u;
            kept[k] = valid[k] && ((up[u >> 5] >> (u & 31u)) & 1u);
        }
        unsigned long long b[4], v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = __ballot(kept[k]), v[k] = __ballot(valid[k]);
        if (lane < 8) res[8 * c + lane] = chunk_words(b[0], b[1], b[2], b[3], lane);
        if (lane == 0) {
            const bool none = (b[0] | b[1] | b[2] | b[3]) == 0ull;
            const bool all = b[0] == v[0] && b[1] == v[1] && b[2] == v[2] && b[3] == v[3];
            sum[c] = none ? kKeepNone : (all ? kKeepAll : kKeepSome);
        }
    }
}
// the bits of the upload-order mask at or past n read back as 0 (after every wave of k_keep_build has read it)
__global__ void k_keep_tail(uint32_t *up, uint64_t n) {
    if (n % 32u) up[n / 32u] &= (1u << (n % 32u)) - 1u;
}
void launch_keep_build(hipStream_t s, uint32_t *up, const uint32_t *perm, uint64_t n, uint32_t *res, uint8_t *sum,
                       uint64_t c0) {
    const uint64_t nchunks = (n + 255) / 256;
    if (c0 >= nchunks) return;
    hipLaunchKernelGGL(k_keep_build, chunk_grid(nchunks - c0, 4096), dim3(kBlock), 0, s, up, perm, n, res, sum, c0);
    hipLaunchKernelGGL(k_keep_tail, dim3(1), dim3(1), 0, s, up, n);
}

// rtr_append_points: the upload-order mask of a cloud of n0 points, grown to n1, keeps the new points -- the bits
// [n0, n1) are set.  Word n0 / 32 keeps its bits below n0 (the ones at or past n0 are clear, k_keep_tail); the words
// behind it are written whole.
__global__ __launch_bounds__(kBlock) void k_keep_append(uint32_t *__restrict__ up, uint64_t n0, uint64_t n1) {
    const uint64_t w0 = n0 / 32u, w1 = (n1 + 31u) / 32u;
    for (uint64_t w = w0 + (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < w1; w += (uint64_t)gridDim.x * kBlock) {
        const uint64_t lo = w * 32u > n0 ? w * 32u : n0, hi = w * 32u + 32u < n1 ? w * 32u + 32u : n1;  // bits [lo, hi)
        const uint32_t bits = (uint32_t)((((1ull << (hi - lo)) - 1ull) << (lo - w * 32u)));
        up[w] = (w == w0 && (n0 % 32u) ? up[w] : 0u) | bits;
    }
}
void launch_keep_append(hipStream_t s, uint32_t *up, uint64_t n0, uint64_t n1) {
    if (n1 <= n0) return;
    const uint64_t words = (n1 + 31) / 32 - n0 / 32, blocks = (words + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_keep_append, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, s, up, n0, n1);
}


// ---- rtr_remove_points (rtr.h section 2c) ------------------------------------------------------------------------
// A stable compaction of the resident order.  keep: the caller's upload-order words (bits at or past n ignored), perm:
// resident index -> upload index (null while the cloud is in upload order).  Lane l of the wave that holds chunk c
// gathers the keep bits of its points 4 l .. 4 l + 3, as k_keep_build does; the four ballots give the chunk's survivor
// count and every survivor's slot in it (rtr_remove_index.h).
// cnt[c] = the survivors of chunk c; *first_loss = the first chunk that loses a point (the caller sets ~0).  A wave's
// chunks ascend, so its first loss is its least; the workgroup folds its waves' in LDS and issues one atomic (one per
// chunk, all on one address, cost 4.4 ms at 1e8 points)
__global__ __launch_bounds__(kBlock) void k_remove_count(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ perm,
                                                         uint64_t n, uint32_t *__restrict__ cnt,
                                                         unsigned long long *__restrict__ first_loss) {
    __shared__ unsigned long long s_first;
    const int lane = threadIdx.x & 63;
    const uint64_t nchunks = (n + 255) / 256;
    if (threadIdx.x == 0) s_first = ~0ull;
    __syncthreads();
    unsigned long long mine = ~0ull;
    for (uint64_t c = wave_first(); c < nchunks; c += wave_stride()) {
        uint32_t u[4];
        bool kept[4], valid[4];
        remove_gather(keep, perm, n, c, lane, u, kept, valid);
        uint32_t s = 0, v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) s += __popcll(__ballot(kept[k])), v += __popcll(__ballot(valid[k]));
        if (lane == 0) cnt[c] = s;
        if (s != v && mine == ~0ull) mine = c;
    }
    if (lane == 0 && mine != ~0ull) atomicMin(&s_first, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_first != ~0ull) atomicMin(first_loss, s_first);
}
void launch_remove_count(hipStream_t s, const uint32_t *keep, const uint32_t *perm, uint64_t n, uint32_t *cnt, uint64_t *first_loss) {
    const uint64_t nchunks = (n + 255) / 256;
    if (nchunks == 0) return;
    hipLaunchKernelGGL(k_remove_count, chunk_grid(nchunks, 8192), dim3(kBlock), 0, s, keep, perm, n, cnt,
                       (unsigned long long *)first_loss);
}

// Exclusive scan of `count` u32 values (popc_bits > 0: of the popcounts of words holding popc_bits bits, the bits past
// them ignored) in three launches: tile sums (kScanTile values per workgroup), one workgroup scans the sums, every
// tile scans itself from its sum's prefix.
constexpr uint64_t kScanPer = 8, kScanTile = kBlock * kScanPer;
__device__ __forceinline__ uint32_t scan_value(const uint32_t *__restrict__ in, uint64_t i, uint64_t count, uint64_t popc_bits) {
    if (i >= count) return 0u;
    const uint32_t v = in[i];
    if (!popc_bits) return v;
    const uint32_t m = (i == popc_bits / 32u && (popc_bits % 32u)) ? (1u << (popc_bits % 32u)) - 1u : 0xFFFFFFFFu;
    return (uint32_t)__popc(v & m);
}
__global__ __launch_bounds__(kBlock) void k_scan_tiles(const uint32_t *__restrict__ in, uint64_t count, uint64_t popc_bits,
                                                       uint32_t *__restrict__ tile_sum) {
    __shared__ uint32_t s_w[8];
    const uint64_t ntiles = (count + kScanTile - 1) / kScanTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i0 = t * kScanTile + threadIdx.x * kScanPer;
        uint32_t v = 0, tot = 0;
#pragma unroll
        for (uint64_t k = 0; k < kScanPer; ++k) v += scan_value(in, i0 + k, count, popc_bits);
        (void)block_scan(v, s_w, tot);
        if (threadIdx.x == 0) tile_sum[t] = tot;
    }
}
__global__ __launch_bounds__(512) void k_scan_top(uint32_t *__restrict__ tile_sum, uint64_t ntiles, uint64_t *__restrict__ total) {
    __shared__ uint32_t s_w[8];
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += 512) {
        const uint64_t t = t0 + threadIdx.x;
        const uint32_t v = t < ntiles ? tile_sum[t] : 0u;
        uint32_t tot = 0;
        const uint32_t incl = block_scan(v, s_w, tot);
        if (t < ntiles) tile_sum[t] = (uint32_t)(carry + (incl - v));  // (sums of fewer than 2^32 points)
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(kBlock) void k_scan_apply(const uint32_t *__restrict__ in, uint64_t count, uint64_t popc_bits,
                                                       const uint32_t *__restrict__ tile_sum, uint32_t *__restrict__ out) {
    __shared__ uint32_t s_w[8];
    const uint64_t ntiles = (count + kScanTile - 1) / kScanTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i0 = t * kScanTile + threadIdx.x * kScanPer;
        uint32_t v[kScanPer], sum = 0, tot = 0;
#pragma unroll
        for (uint64_t k = 0; k < kScanPer; ++k) v[k] = scan_value(in, i0 + k, count, popc_bits), sum += v[k];
        uint32_t run = tile_sum[t] + block_scan(sum, s_w, tot) - sum;
#pragma unroll
        for (uint64_t k = 0; k < kScanPer; ++k) {
            if (i0 + k < count) out[i0 + k] = run;
            run += v[k];
        }
    }
}
uint64_t scan_scratch_words(uint64_t count) { return (count + kScanTile - 1) / kScanTile + 1; }
void launch_scan_u32(hipStream_t s, const uint32_t *in, uint64_t count, uint64_t popc_bits, uint32_t *out, uint32_t *scratch,
                     uint64_t *total) {
    const uint64_t ntiles = (count + kScanTile - 1) / kScanTile;
    const unsigned grid = (unsigned)(ntiles < 8192 ? (ntiles ? ntiles : 1) : 8192);
    if (ntiles) hipLaunchKernelGGL(k_scan_tiles, dim3(grid), dim3(kBlock), 0, s, in, count, popc_bits, scratch);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(512), 0, s, scratch, ntiles, total);
    if (ntiles) hipLaunchKernelGGL(k_scan_apply, dim3(grid), dim3(kBlock), 0, s, in, count, popc_bits, scratch, out);
}

// The survivors of chunks c0.. into the window (fp32 SoA, colours, renumbered upload indices when perm is kept): chunk
// c's go to dst[c] - 256 c0 on, in their order.  Coordinates from the fp32 SoA when resident, else decoded from the
// packed form (bit for bit); wscan: the exclusive popcount scan of `keep` (renumbering; read only with perm).
__global__ __launch_bounds__(kBlock) void k_remove_compact(const uint4 *__restrict__ hdr, const uint32_t *__restrict__ planes,
                                                           const uint32_t *__restrict__ planes_b, const float4 *__restrict__ x4,
                                                           const float4 *__restrict__ y4, const float4 *__restrict__ z4,
                                                           const uint4 *__restrict__ rgba4, const uint32_t *__restrict__ perm,
                                                           const uint32_t *__restrict__ keep, const uint32_t *__restrict__ wscan,
                                                           const uint32_t *__restrict__ dst, uint64_t n, uint64_t c0,
                                                           float *__restrict__ wx, float *__restrict__ wy, float *__restrict__ wz,
                                                           uint32_t *__restrict__ wrgba, uint32_t *__restrict__ wperm) {
    const int lane = threadIdx.x & 63;
    const uint64_t nchunks = (n + 255) / 256, n4 = (n + 3) / 4;
    for (uint64_t c = c0 + wave_first(); c < nchunks; c += wave_stride()) {
        uint32_t u[4];
        bool kept[4], valid[4];
        remove_gather(keep, perm, n, c, lane, u, kept, valid);
        unsigned long long b[4];
        uint32_t below = 0, own = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = __ballot(kept[k]);
            below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b[k] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b[k], below));
            own |= kept[k] ? 1u << k : 0u;
        }
        if ((b[0] | b[1] | b[2] | b[3]) == 0ull) continue;  // (wave-uniform)
        const uint64_t i = c * 64 + lane;
        float4 X, Y, Z;
        if (x4) {
            if (i < n4) X = x4[i], Y = y4[i], Z = z4[i];
        } else {  // (every lane decodes, as k_unpack_soa does: lanes past the end read the spare bytes)
            const uint4 h0 = hdr[2 * c], h1 = hdr[2 * c + 1];
            const ChunkRawA raw_a = load_chunk_a(planes, h0, h1, lane);
            const ChunkRaw raw = load_chunk_b(planes_b, h0, h1, lane);
            unpack_chunk(raw_a, raw, h0.w, h0.x, h0.y, h0.z, X, Y, Z, lane);
        }
        if (!own) continue;  // (i < n4 from here on)
        const uint4 col = rgba4[i];
        const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
        const uint32_t cs[4] = {col.x, col.y, col.z, col.w};
        const uint64_t base = (uint64_t)dst[c] - 256u * c0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!kept[k]) continue;
            const uint64_t o = base + remove_slot(below, own, (uint32_t)k);
            wx[o] = xs[k], wy[o] = ys[k], wz[o] = zs[k], wrgba[o] = cs[k];
            if (wperm) wperm[o] = remove_rank(wscan[u[k] >> 5], keep[u[k] >> 5], u[k]);
        }
    }
}
void launch_remove_compact(hipStream_t s, const Cloud &c, const uint32_t *perm, const uint32_t *keep, const uint32_t *wscan,
                           const uint32_t *dst, uint64_t c0, float *wx, float *wy, float *wz, uint32_t *wrgba, uint32_t *wperm) {
    const uint64_t nchunks = (c.n + 255) / 256;
    if (c0 >= nchunks) return;
    hipLaunchKernelGGL(k_remove_compact, chunk_grid(nchunks - c0, 8192), dim3(kBlock), 0, s, c.pk.hdr, c.pk.planes,
                       c.pk.planes_b, (const float4 *)c.x, (const float4 *)c.y, (const float4 *)c.z, (const uint4 *)c.rgba, perm,
                       keep, wscan, dst, c.n, c0, wx, wy, wz, wrgba, wperm);
}

// The upload-order keep mask in force compacted onto the survivors: the mask bits of word w's kept points go to bits
// wscan[w] .. of up1 (cleared by the caller), in order.
__global__ __launch_bounds__(kBlock) void k_remove_mask(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ wscan,
                                                        const uint32_t *__restrict__ up, uint64_t n, uint32_t *__restrict__ up1) {
    const uint64_t nwords = (n + 31) / 32;
    for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * kBlock) {
        const uint32_t kw = keep[w] & ((w == n / 32u && (n % 32u)) ? (1u << (n % 32u)) - 1u : 0xFFFFFFFFu);
        const uint32_t bits = remove_extract(up[w], kw);
        if (!bits) continue;
        const uint32_t base = wscan[w], sh = base & 31u;
        atomicOr(&up1[base >> 5], bits << sh);
        if (sh && (bits >> (32u - sh))) atomicOr(&up1[(base >> 5) + 1], bits >> (32u - sh));
    }
}
void launch_remove_mask(hipStream_t s, const uint32_t *keep, const uint32_t *wscan, const uint32_t *up, uint64_t n, uint32_t *up1) {
    const uint64_t nwords = (n + 31) / 32, blocks = (nwords + kBlock - 1) / kBlock;
    if (nwords == 0) return;
    hipLaunchKernelGGL(k_remove_mask, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, s, keep, wscan, up, n, up1);
}

// The chunks in front of the first one that loses a point keep their points, but on a sorted cloud not their upload
// indices: a removed point with a smaller index lies in a LATER chunk, and every index above it drops by one.  A quad of
// perm per lane, each index replaced by its rank among the kept points, into the permutation's replacement.
__global__ __launch_bounds__(kBlock) void k_remove_renumber(const uint4 *__restrict__ perm4, uint64_t quads,
                                                            const uint32_t *__restrict__ keep, const uint32_t *__restrict__ wscan,
                                                            uint4 *__restrict__ out4) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < quads; i += (uint64_t)gridDim.x * kBlock) {
        const uint4 u = perm4[i];
        uint4 r;
        r.x = remove_rank(wscan[u.x >> 5], keep[u.x >> 5], u.x);
        r.y = remove_rank(wscan[u.y >> 5], keep[u.y >> 5], u.y);
        r.z = remove_rank(wscan[u.z >> 5], keep[u.z >> 5], u.z);
        r.w = remove_rank(wscan[u.w >> 5], keep[u.w >> 5], u.w);
        out4[i] = r;
    }
}
void launch_remove_renumber(hipStream_t s, const uint32_t *perm, uint64_t count, const uint32_t *keep, const uint32_t *wscan,
                            uint32_t *out) {
    const uint64_t quads = count / 4, blocks = (quads + kBlock - 1) / kBlock;
    if (quads == 0) return;
    hipLaunchKernelGGL(k_remove_renumber, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kBlock), 0, s, (const uint4 *)perm,
                       quads, keep, wscan, (uint4 *)out);
}

// ---- rtr_write_points (rtr.h section 2f) -------------------------------------------------------------------------
// selw[w] = the bits of selection word w whose rank falls in the call's window [first, first + count) (write_word_bits),
// a thread per word.  every: the selection is every point -- the words are synthesised here (all ones below n, their
// scan 32 w) into sel / wscan, so that everything downstream reads sel, wscan and selw alike.
__global__ __launch_bounds__(kBlock) void k_write_bits(uint32_t *__restrict__ sel, uint32_t *__restrict__ wscan, uint64_t n,
                                                       int every, uint64_t first, uint64_t count, uint32_t *__restrict__ selw) {
    const uint64_t nwords = (n + 31) / 32;
    for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * kBlock) {
        if (every) sel[w] = extract_word_mask(w, n), wscan[w] = (uint32_t)(32u * w);
        selw[w] = write_word_bits(sel[w], wscan[w], w, first, count, n);
    }
}
void launch_write_bits(hipStream_t s, uint32_t *sel, uint32_t *wscan, uint64_t n, bool every, uint64_t first, uint64_t count,
                       uint32_t *selw) {
    const uint64_t nwords = (n + 31) / 32, blocks = (nwords + kBlock - 1) / kBlock;
    if (nwords == 0) return;
    hipLaunchKernelGGL(k_write_bits, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(kBlock), 0, s, sel, wscan, n,
                       every ? 1 : 0, first, count, selw);
}

__global__ __launch_bounds__(kBlock) void k_shift_units(uint4 *__restrict__ hdr, uint64_t c_from, uint64_t c_to, long long delta) {
    for (uint64_t c = c_from + (uint64_t)blockIdx.x * kBlock + threadIdx.x; c < c_to; c += (uint64_t)gridDim.x * kBlock) {
        uint4 h = hdr[2 * c + 1];
        const uint64_t off = ((((uint64_t)h.y) << 32) | (uint64_t)h.x) + (uint64_t)delta;
        h.x = (uint32_t)off, h.y = (uint32_t)(off >> 32);
        hdr[2 * c + 1] = h;
    }
}
// out[0] += the wide chunks among hdr's first nchunks headers, out[1] += those of them that carry a box word
__global__ __launch_bounds__(kBlock) void k_wide_counts(const uint4 *__restrict__ hdr, uint64_t nchunks, unsigned long long *out) {
    uint32_t wide = 0, boxed = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c < nchunks; c += (uint64_t)gridDim.x * kBlock) {
        const bool w = (hdr[2 * c].w & kPackWideFlag) != 0u;
        wide += w ? 1u : 0u;
        boxed += w && hdr[2 * c + 1].w != 0u ? 1u : 0u;
    }
    const uint32_t nw = (uint32_t)__popcll(__ballot(wide != 0u));  // (most waves hold none)
    if (nw == 0u) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wide += (uint32_t)__shfl_xor((int)wide, off, 64), boxed += (uint32_t)__shfl_xor((int)boxed, off, 64);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], (unsigned long long)wide);
        atomicAdd(&out[1], (unsigned long long)boxed);
    }
}
void launch_wide_counts(hipStream_t s, const uint4 *hdr, uint64_t nchunks, uint64_t *out) {
    if (nchunks == 0) return;
    const uint64_t blocks = (nchunks + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_wide_counts, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(kBlock), 0, s, hdr, nchunks,
                       (unsigned long long *)out);
}
void launch_shift_units(hipStream_t s, uint4 *hdr, uint64_t c_from, uint64_t c_to, int64_t delta) {
    if (c_from >= c_to || delta == 0) return;
    const uint64_t blocks = (c_to - c_from + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_shift_units, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, s, hdr, c_from, c_to,
                       (long long)delta);
}

// ---------------------------------------------------------------------------------
// Selection (rtr_select_points, rtr.h section 6f): which points lie inside a region -- clip_keep over the call's planes
// and, RECT, the frame's own project_point landing on a pixel of the rectangle -- as upload-order bit words combined
// with the selection so far by `op`.  The point pass's skeleton: one wave per 256-point chunk (lane l: points 4 l ..
// 4 l + 3), chunks dealt round robin, PACKED 64 headers tested per wave step and only the survivors decoded.  The
// chunk decision has three outcomes:
//   outside: the box lies beyond one plane (clip_box_outside) or beyond one half-space of the rectangle (rect_planes +
//            box_outside): no point of it is inside;
//   inside:  planes only -- the box lies within every plane (clip_box_inside): every point of it is inside (a packed
//            chunk that has a box holds no NaN).  No plane and no rectangle: every chunk, boxed or not;
//   mixed:   decoded and tested point by point.
// Not PACKED the boxes are k_chunk_bounds', whose fminf / fmaxf skip NaN coordinates: a NaN may hide behind a finite
// box, so such a chunk is classed outside (a NaN point is not inside either) but never inside on its box.
// hit = inside, or, `invert`, !inside for the points below n; the points at or past n are never hit.
// Writing, PERM = false: a decoded chunk's 256 hits are four ballots interleaved into eight words (lanes 0..7, as the
// point pass) and combined with the old words by plain loads and stores -- each chunk's words belong to one wave.  An
// undecoded chunk's hits are all alike: the header lane itself stores its eight words, and only where `op` changes
// them (ADD / SUBTRACT / TOGGLE of nothing and INTERSECT with everything leave the old words; TOGGLE of everything
// flips them; the rest are constants: the old words hold no bit past n, so nothing is loaded).
// PERM: bits go through perm[resident index] with atomicOr (REPLACE -- the caller cleared the words -- and ADD),
// atomicAnd (SUBTRACT: the hits; INTERSECT: the misses) or atomicXor (TOGGLE); an undecoded chunk reads its 256 perm entries when `op` has
// something to change, never its coordinates.
// stats (null: not requested): [1] / [2] / [3] += chunks outside / inside / decoded, folded per workgroup in LDS: three
// atomics per workgroup ([0] is k_select_count's).
constexpr int kSelReplace = 0, kSelAdd = 1, kSelSubtract = 2, kSelIntersect = 3, kSelToggle = 8;  // (RTR_SELECT_*)
struct SelectArgs {
    const float4 *x4, *y4, *z4;  // fp32 SoA (not PACKED) ...
    const float *bounds;         // ... and its chunk boxes (k_chunk_bounds)
    PackedXyz pk;                // packed form (PACKED)
    uint64_t n;
    uint32_t *sel;               // 8 words per chunk
    const uint32_t *perm;        // resident index -> upload index (PERM)
    unsigned long long *stats;
    int op, invert;
    int x0, y0, x1, y1;          // RECT
};
__device__ __forceinline__ uint32_t select_word_mask(uint64_t n, uint64_t c, uint32_t j) {  // the bits of word j of chunk c below n
    const uint64_t first = c * 256u + 32u * j;
    if (first >= n) return 0u;
    const uint64_t left = n - first;
    return left >= 32u ? 0xFFFFFFFFu : (1u << (uint32_t)left) - 1u;
}
// the eight words of a chunk whose points below n are all hit / all missed (one lane; PERM = false)
__device__ __forceinline__ void select_store_uniform(const SelectArgs &a, uint64_t c, bool hit) {
    if (hit ? a.op == kSelIntersect : (a.op == kSelAdd || a.op == kSelSubtract || a.op == kSelToggle)) return;  // (the old words stay)
    uint4 *w = reinterpret_cast<uint4 *>(a.sel + 8 * c);
    if (a.op == kSelToggle) {  // (of everything below n: the only case that reads the old words)
        const uint4 o0 = w[0], o1 = w[1];
        w[0] = make_uint4(o0.x ^ select_word_mask(a.n, c, 0), o0.y ^ select_word_mask(a.n, c, 1), o0.z ^ select_word_mask(a.n, c, 2), o0.w ^ select_word_mask(a.n, c, 3));
        w[1] = make_uint4(o1.x ^ select_word_mask(a.n, c, 4), o1.y ^ select_word_mask(a.n, c, 5), o1.z ^ select_word_mask(a.n, c, 6), o1.w ^ select_word_mask(a.n, c, 7));
    } else if (!hit || a.op == kSelSubtract) {  // (REPLACE / INTERSECT with nothing, SUBTRACT of everything)
        w[0] = make_uint4(0u, 0u, 0u, 0u);
        w[1] = make_uint4(0u, 0u, 0u, 0u);
    } else {  // (REPLACE by / ADD of everything below n)
        w[0] = make_uint4(select_word_mask(a.n, c, 0), select_word_mask(a.n, c, 1), select_word_mask(a.n, c, 2), select_word_mask(a.n, c, 3));
        w[1] = make_uint4(select_word_mask(a.n, c, 4), select_word_mask(a.n, c, 5), select_word_mask(a.n, c, 6), select_word_mask(a.n, c, 7));
    }
}
// the wave writes the hits of chunk c (hit[k]: point 4 lane + k, already false at or past n)
template <bool PERM>
__device__ __forceinline__ void select_write(const SelectArgs &a, uint64_t c, int lane, const bool hit[4]) {
    if (PERM) {
        const uint64_t i0 = c * 256u + 4u * (uint64_t)lane;
        if (i0 < a.n) {  // (perm holds whole quads: its arrays are padded to a multiple of 4 points)
            const uint4 q = *reinterpret_cast<const uint4 *>(a.perm + i0);
            const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i0 + k >= a.n) continue;
                const uint32_t bit = 1u << (u[k] & 31u);
                if (a.op == kSelIntersect) {
                    if (!hit[k]) atomicAnd(a.sel + (u[k] >> 5), ~bit);
                } else if (hit[k]) {
                    if (a.op == kSelSubtract) atomicAnd(a.sel + (u[k] >> 5), ~bit);
                    else if (a.op == kSelToggle) atomicXor(a.sel + (u[k] >> 5), bit);
                    else atomicOr(a.sel + (u[k] >> 5), bit);
                }
            }
        }
    } else {
        const unsigned long long b0 = __ballot(hit[0]), b1 = __ballot(hit[1]), b2 = __ballot(hit[2]), b3 = __ballot(hit[3]);
        if (lane < 8) {
            const uint32_t h = chunk_words(b0, b1, b2, b3, lane);
            uint32_t *w = a.sel + 8 * c + lane;
            if (a.op == kSelReplace) *w = h;
            else {
                const uint32_t old = *w;
                *w = a.op == kSelAdd ? (old | h) : (a.op == kSelSubtract ? (old & ~h) : (a.op == kSelToggle ? (old ^ h) : (old & h)));
            }
        }
    }
}
// a decoded chunk: the predicate per point
template <bool PERM, bool RECT>
__device__ __forceinline__ void select_chunk(const SelectArgs &a, const Clip &clip, const Proj &P, int W, int H, float fW, float fH,
                                             uint64_t c, const float4 &X, const float4 &Y, const float4 &Z, int lane) {
    const uint64_t i0 = c * 256u + 4u * (uint64_t)lane;
    const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
    bool hit[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bool in = clip_keep(clip, xs[k], ys[k], zs[k]);
        if (RECT) {
            float d;
            const int pix = project_point(P, xs[k], ys[k], zs[k], W, H, fW, fH, d);
            const int py = pix >= 0 ? (int)((uint32_t)pix / (uint32_t)W) : -1, px = pix - py * W;
            in = in && pix >= 0 && px >= a.x0 && px < a.x1 && py >= a.y0 && py < a.y1;
        }
        hit[k] = i0 + k < a.n && in != (a.invert != 0);
    }
    select_write<PERM>(a, c, lane, hit);
}
constexpr int kSelOutside = 0, kSelInside = 1, kSelMixed = 2;
template <bool PACKED, bool PERM, bool RECT>
__global__ __launch_bounds__(kBlock) void k_select(SelectArgs a, Clip clip, Proj P, int W, int H) {
    __shared__ uint32_t s_cnt[3];
    const float fW = (float)W, fH = (float)H;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = wave_first(), nwaves = wave_stride();
    const uint64_t n4 = (a.n + 3) / 4, nchunks = (n4 + 63) / 64;
    const bool every = !RECT && clip.count == 0;  // (no condition at all: every point, NaN included, is inside)
    const bool invert = a.invert != 0;
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    FrustumPlanes rpl{};
    if (RECT) rpl = rect_planes(P.m, (float)a.x0, (float)a.y0, (float)a.x1, (float)a.y1);
    uint32_t cnt[3] = {0u, 0u, 0u};  // (wave-uniform)
    if (!PACKED) {
        for (uint64_t c = wave; c < nchunks; c += nwaves) {  // (wave-uniform)
            int state = every ? kSelInside : kSelMixed;
            if (!every) {
                const float *b = a.bounds + 6 * c;
                const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
                if (clip_box_outside(clip, lo, hi) || (RECT && box_outside(rpl, lo, hi))) state = kSelOutside;
            }
            cnt[kSelOutside] += state == kSelOutside, cnt[kSelInside] += state == kSelInside, cnt[kSelMixed] += state == kSelMixed;
            const bool hit_u = (state == kSelInside) != invert;
            if (state != kSelMixed && !PERM) {
                if (lane == 0) select_store_uniform(a, c, hit_u);
                continue;
            }
            if (state != kSelMixed) {
                if (a.op == kSelIntersect ? !hit_u : hit_u) {
                    const uint64_t i0 = c * 256u + 4u * (uint64_t)lane;
                    const bool hit[4] = {hit_u && i0 < a.n, hit_u && i0 + 1 < a.n, hit_u && i0 + 2 < a.n, hit_u && i0 + 3 < a.n};
                    select_write<PERM>(a, c, lane, hit);
                }
                continue;
            }
            const uint64_t i = c * 64u + (uint64_t)lane, ic = i < n4 ? i : n4 - 1u;
            const float4 X = ld_stream(a.x4 + ic), Y = ld_stream(a.y4 + ic), Z = ld_stream(a.z4 + ic);
            select_chunk<PERM, RECT>(a, clip, P, W, H, fW, fH, c, X, Y, Z, lane);
        }
    } else {
        for (uint64_t j0 = 0; wave + nwaves * j0 < nchunks; j0 += 64u) {  // (wave-uniform)
            const uint64_t chunk = wave + nwaves * (j0 + (uint64_t)lane);
            const bool valid = chunk < nchunks;
            int state = kSelMixed;
            if (valid) {
                if (every) state = kSelInside;
                else {
                    const uint4 h0 = a.pk.hdr[2 * chunk];
                    float lo[3], hi[3];
                    const uint32_t wbox = reinterpret_cast<const uint32_t *>(a.pk.hdr + 2 * chunk + 1)[3];  // (the header's own 32 bytes)
                    if (chunk_box(h0.x, h0.y, h0.z, h0.w, wbox, lo, hi)) {
                        if (clip_box_outside(clip, lo, hi) || (RECT && box_outside(rpl, lo, hi))) state = kSelOutside;
                        else if (!RECT && clip_box_inside(clip, lo, hi)) state = kSelInside;
                    }
                }
            }
            const bool hit_u = (state == kSelInside) != invert;
            bool work = valid && state == kSelMixed;  // (the chunks that need the whole wave)
            if (valid && state != kSelMixed) {
                if (!PERM) select_store_uniform(a, chunk, hit_u);
                else work = a.op == kSelIntersect ? !hit_u : hit_u;
            }
            cnt[kSelOutside] += (uint32_t)__popcll(__ballot(valid && state == kSelOutside));
            cnt[kSelInside] += (uint32_t)__popcll(__ballot(valid && state == kSelInside));
            cnt[kSelMixed] += (uint32_t)__popcll(__ballot(valid && state == kSelMixed));
            const unsigned long long mixed = __ballot(valid && state == kSelMixed);
            unsigned long long mask = __ballot(work);
            while (mask) {
                const int l = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const uint64_t cc = wave + nwaves * (j0 + (uint64_t)l);
                if (PERM && !((mixed >> l) & 1ull)) {  // (an undecoded chunk through the permutation: `work` says all hit / all missed)
                    const bool hu = a.op != kSelIntersect;
                    const uint64_t i0 = cc * 256u + 4u * (uint64_t)lane;
                    const bool hit[4] = {hu && i0 < a.n, hu && i0 + 1 < a.n, hu && i0 + 2 < a.n, hu && i0 + 3 < a.n};
                    select_write<PERM>(a, cc, lane, hit);
                    continue;
                }
                const uint4 h0 = a.pk.hdr[2 * cc], h1 = a.pk.hdr[2 * cc + 1];
                const ChunkRawA raw_a = load_chunk_a(a.pk.planes, h0, h1, lane);
                const ChunkRaw raw = load_chunk_b(a.pk.planes_b, h0, h1, lane);
                float4 X, Y, Z;
                unpack_chunk(raw_a, raw, h0.w, h0.x, h0.y, h0.z, X, Y, Z, lane);
                select_chunk<PERM, RECT>(a, clip, P, W, H, fW, fH, cc, X, Y, Z, lane);
            }
        }
    }
    if (a.stats) {  // (wave-uniform)
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (cnt[k]) atomicAdd(&s_cnt[k], cnt[k]);
        }
        __syncthreads();
        if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(a.stats + 1 + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
    }
}
// *out += the set bits of `words` (16-byte units; the bits past n are clear): one atomic per workgroup
__global__ __launch_bounds__(kBlock) void k_select_count(const uint4 *__restrict__ words, uint64_t n16, unsigned long long *__restrict__ out) {
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0u;
    __syncthreads();
    uint32_t mine = 0u;  // (a thread sees at most 2^32 / 128 units' bits)
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * kBlock) {
        const uint4 q = words[i];
        mine += (uint32_t)(__popc(q.x) + __popc(q.y) + __popc(q.z) + __popc(q.w));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(out, (unsigned long long)s_sum);
}
void launch_select(hipStream_t s, const Cloud &c, const float *bounds, const Clip &clip, const Proj *P, int W, int H,
                   const int rect[4], int op, bool invert, uint32_t *sel, const uint32_t *perm, uint64_t *stats) {
    const uint64_t n4 = (c.n + 3) / 4, nchunks = (n4 + 63) / 64;
    if (nchunks == 0) return;
    const bool packed = c.pk.hdr != nullptr;
    SelectArgs a{(const float4 *)c.x, (const float4 *)c.y, (const float4 *)c.z, bounds, c.pk, c.n, sel, perm,
                 (unsigned long long *)stats, op, invert ? 1 : 0, 0, 0, 0, 0};
    Proj proj{};
    if (P) proj = *P, a.x0 = rect[0], a.y0 = rect[1], a.x1 = rect[2], a.y1 = rect[3];
    const dim3 grid = chunk_grid(nchunks, 2048), block(kBlock);  // (up to 8 waves per CU, every chunk dealt round robin: the point pass's grid)
    auto go = [&](auto pk, auto pm, auto rc) {  // (PACKED, PERM, RECT)
        hipLaunchKernelGGL((k_select<decltype(pk)::value, decltype(pm)::value, decltype(rc)::value>), grid, block, 0, s, a, clip,
                           proj, W, H);
    };
    auto with_rect = [&](auto pk, auto pm) {
        if (P) go(pk, pm, std::true_type{}); else go(pk, pm, std::false_type{});
    };
    const std::true_type on;
    const std::false_type off;
    if (packed && perm) with_rect(on, on);
    else if (packed) with_rect(on, off);
    else if (perm) with_rect(off, on);
    else with_rect(off, off);
}
void launch_select_count(hipStream_t s, const uint32_t *sel, uint64_t n, uint64_t *out) {
    const uint64_t n16 = ((n + 255) / 256) * 2;
    if (n16 == 0) return;
    const uint64_t blocks = (n16 + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_select_count, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(kBlock), 0, s, (const uint4 *)sel, n16,
                       (unsigned long long *)out);
}

}  // namespace rtr
