// rtr_kernels.h -- launch wrappers of the gfx950 kernels (internal to librtr_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtr_barrier_rule.h"
#include "rtr_chunk_box.h"
#include "rtr_stamp_rule.h"

namespace rtr {

// Rows 0..2 of the row-major camera matrix (row 3 is never used: render.cu:33-40
// computes result.w but nothing reads it).  Passed BY VALUE so the twelve floats
// live in SGPRs -- the reference pays a synchronous 64-byte H2D copy per frame
// (project_cloud.cu:320).
struct Proj {
    float m[12];
};

// Lossless resident form of the coordinates for the tile-binned point kernel (option "pack").  A chunk =
// 256 consecutive points = what one wave handles per iteration (lane l: points 4 l .. 4 l + 3).  Per
// chunk and axis the fp32 BIT PATTERNS are stored as base | low bits: base = the leading bits all 256
// patterns share (low b bits clear), b = 0..25 or 32 the number of bits below that common prefix (0: the axis
// is constant in the chunk; 32: nothing is shared -- NaNs, mixed signs -- or more than 25 bits differ).  An
// axis block is the 256 values' low b bits as TWO little-endian bit streams: the A stream holds the FIRST value of
// every lane (lane l's b bits at bit b l: 8 b bytes), the B stream its other three (3 b bits at bit 3 b l: 24 b bytes) --
// the point kernel's lane test needs one point per lane, so nine chunks in ten are read through their A streams
// alone, a quarter of the bytes (round 4; before: one stream, lane l's four values at bit 4 b l).  A lane reads ONE
// dword-aligned 8-byte (16-byte) load per axis and stream and shifts its data down by the 0..31 bits its first value
// starts into that dword.  All A streams lie in one array, chunk after chunk (x, y, z), all B streams in another.
// hdr[2 c] = {base x, base y, base z, bx | by << 6 | bz << 12 | kPackWideFlag if some b is 32},
// hdr[2 c + 1] = {first 32-byte unit (lo, hi) -- the chunk's A streams start 8 bytes x that into the A array, its B
// streams 24 bytes x that into the B array --, lane spread of the chunk (fp32 bits, see Cloud::spread), the box word of
// a wide chunk (rtr_chunk_box.h, wide_box_word; 0: none)}.
// Both arrays end with spare bytes (the last lanes' loads run past their values).
// Spatially ordered clouds need 16-21 bits per coordinate (neighbours share sign, exponent and leading
// mantissa bits): 5-8 B/pt instead of 12 (round 2 stored whole bytes: 6.5-9.2 B/pt).
constexpr uint32_t kPackMaxBits = 25;  // shift (<= 31) + b <= 64, + 3 b <= 128 bits of a lane's two loads
struct PackedXyz {
    const uint4 *hdr;        // null: not packed
    const uint32_t *planes;  // the A streams (every lane's first value); one allocation with ...
    const uint32_t *planes_b;  // ... the B streams (the other three values), pack_b_dwords(units) dwords behind
};
// where the B streams start inside the allocation, in dwords (units: 32-byte units of both streams together, the sum of
// the chunks' axis widths; the A streams end with ~1 KB of spare bytes), and the allocation's size
constexpr uint64_t pack_b_dwords(uint64_t units) { return (units * 2 + 256 + 16 + 15) & ~15ull; }  // (the point kernel requests 1 KB per chunk)
constexpr uint64_t pack_total_dwords(uint64_t units) { return pack_b_dwords(units) + units * 6 + 16; }

struct Cloud {
    const float *x, *y, *z;  // SoA, padded to a multiple of 4 points with NaN
    const uint32_t *rgba;    // packed c0 | c1<<8 | c2<<16 | 255<<24
    uint64_t n;              // real point count
    int grid;                // workgroups of the grid-stride point kernels
    int incoherent;          // consecutive points are unrelated (measured at upload): no wave-level claim groups
    PackedXyz pk;            // the same coordinates, packed (only read by launch_project_bin)
    // Lane spread (k_chunk_bounds): per 256-point chunk the largest |coordinate difference| between a lane's FIRST
    // point (4 l) and its other three (4 l + 1 .. 4 l + 3), over lanes and axes -- +inf when the chunk holds a
    // non-finite or huge (> 1e30) coordinate.  T1 tests one point per lane and bounds the other three by it (see
    // k_project_bin, "lane test").  null: no lane test.  absmax: largest finite |x|, |y|, |z| of the cloud.
    const float *spread;
    float absmax[3];
    Clip clip;  // the user's clip planes (rtr_set_clip_planes; count 0: none): the point kernels take them as Filter pack (Clip)
    Keep keep;  // the user's keep mask in resident order (rtr_set_point_keep; words null: none): Filter pack (Clip, Keep)
};

struct FilterLevels {
    float *lv[9];  // lv[0] = depth buffer (as float), lv[i] = level i
    int w[9], h[9];
    int levels;
};

// peer-to-peer exchange (see the comment on k_p2p_sync): p[r] = rank r's buffer as mapped into this process
constexpr int kMaxPeers = 16;
struct PeerSet {
    void *p[kMaxPeers];
};
// A frame-sized buffer that still lies in per-rank slices of `chunk` elements (the reduced depth /
// the resolved image right after the slice kernels): element i is read from src.p[i / chunk].
// chunk == 0: not sliced, use the local buffer.
// peers > 0 (accumulate pass of a sharded whole frame): src.p[r] is rank r's LOCAL depth buffer and the
// element is the MIN over the ranks whose bit for the tile is set in occ_all[r * 128 + (tile >> 5)] (every
// rank's occupancy bitmap, gathered into local memory by the barrier launch); the completed depth goes to `out`,
// a buffer no peer reads in that launch (NOT into the local depth buffer the peers are reading at that moment).
struct OwnedTab;
struct Sliced {
    PeerSet src;
    size_t chunk;
    const uint32_t *occ_all;
    int peers;
    uint32_t *out;
    int rank;             // tile mode 4 (owner-computes sharded frames): this rank, ...
    const OwnedTab *tab;  // ... and where every rank's tile store / frame buffers are mapped (device memory)
};
// Owner-computes form of the sharded frame (rtr_p2p_render_owned): every screen tile is produced by ONE of the ranks
// that have points in it (tile_owner below), which reads the other occupying ranks' entries straight out of their tile
// stores over xGMI -- no MIN / SUM exchange, no second pass.  The table lives in device memory (one pointer in the
// kernel arguments instead of half a kilobyte).
struct OwnedTab {
    const uint32_t *meta[kMaxPeers];   // rank r's TileStore::meta (stream lengths per tile: ts_cnt4, extent directory)
    const uint64_t *ext0[kMaxPeers];   // ... static extents
    const uint64_t *dyn[kMaxPeers];    // ... dynamic extent pool
    const uint32_t *depth[kMaxPeers];  // ... depth buffer (tiles it owns are final after the tile launch)
    const uint8_t *ximg[kMaxPeers];    // ... image exchange copy (ditto)
};
struct TilePyr {  // F1 folded into T4 (whole-frame calls with the default 4 levels)
    FilterLevels L;
    uint32_t n_eff_rows;
    uint32_t *part_min, *part_max;
    int enable;
};
// Tile store of the binned form.  Every 32x16 screen "storage tile" owns a stream of 8-byte
// entries (depth bits << 33 | in-tile pixel << 24 | colour), appended by T1 straight in tile order:
// the stream's first kS0 entries live in a static extent, later ones in extents of doubling size
// handed out on demand from `dyn` (extent k >= 1 holds stream positions [kS0 << (k-1), kS0 << k)).
constexpr int kS0Shift = 12;             // static extent: 4096 entries = 32 KB per storage tile
constexpr uint32_t kS0 = 1u << kS0Shift;
// (kDirK, the directory words per storage tile, and the frame stamp's rule: rtr_stamp_rule.h)
constexpr int kHeavyExtra = 512;         // extra tile-kernel workgroups available for split tiles
struct TileStore {   // what travels as kernel argument (the point kernel is short of scalar registers)
    uint64_t *ext0;  // [nst * kS0]
    uint32_t *meta;  // every small array of the store in ONE allocation (see the ts_* accessors)
    uint32_t seq;    // 24-bit frame stamp, never 0
    int nst, ntiles; // 32x16 storage tiles, processing tiles
    int fill_shift;  // stream counter of storage tile st = fill[st << fill_shift] (one counter per 2^shift words)
};
constexpr int kFillShiftMax = 6;
struct StoreConsts {  // rarely needed, rarely changing: lives in the store's header (hdr[kHdrConsts ..])
    uint32_t *depth, *acc, *occ;  // frame buffers / occupancy bitmap T1's last workgroup writes to
    uint64_t *dyn;                // [dyn_cap] pool of the dynamic extents
    uint64_t dyn_cap;
    uint32_t heavy, slice;        // split tiles with more entries than `heavy` into slices of >= `slice`
    uint32_t *err_host;           // mapped host word: T1's epilogue ORs a frame's tile-store error code into it
    uint32_t *split_host;         // mapped host word: tiles above the split threshold in the frame T1 has just binned
    uint32_t *entries_host;       // mapped host word: in-frustum entries of the last frame whose statistics are complete
};
// meta, in 32-bit words:
//   fill[nst << kFillShiftMax]  stream length while T1 runs; zero between frames
//   (nst words, unused)
//   tile_cnt[nt]   entries per processing tile (32x32 or 64x32 pixels)
//   hctr[nt]       arrival counters of split tiles
//   items[(2 nt + kHeavyExtra + 1) * 8]  work list of the tile kernel, 32-byte records: word 0 = tile |
//                  slice << 12 | (slices - 1) << 22, words 1..4 = the lengths of the tile's two (four)
//                  streams.  Records [0, nt): one per tile, at position perm[tile] (kItemSkip when the
//                  tile is split); records [nt, nt + hdr[kHdrSplitItems]): the slices of split tiles
//   perm[nt]       tile -> record position: tiles that held more than twice the mean entry count in
//                  the PREVIOUS frame first (written by an extra workgroup of the tile launch)
//   hdr[32]        kHdr* below; hdr[kHdrConsts ..] = StoreConsts
//   ticket[2]      (u64) low word: groups of T1 workgroups that have finished (see sub[] below); high word: 256-point
//                  chunks whose colours were loaded
//   pool_next[2]   (u64) entries of `dyn` handed out in this frame
//   dir[nst * kDirK * 2]  (u64) extent base << 24 | frame stamp (valid iff stamp == seq)
// (every sub-array starts on a 16-byte boundary: the work list is read and written as uint4 records, the
// ticket, the pool cursor and the directory as 8-byte words)
__host__ __device__ constexpr size_t ts_align4(size_t x) { return (x + 3) & ~(size_t)3; }
__host__ __device__ constexpr size_t ts_off_count(int nst, int nt) { return ts_align4((size_t)nst << kFillShiftMax); }
__host__ __device__ constexpr size_t ts_off_tile_cnt(int nst, int nt) { return ts_off_count(nst, nt) + ts_align4((size_t)nst); }
__host__ __device__ constexpr size_t ts_off_hctr(int nst, int nt) { return ts_off_tile_cnt(nst, nt) + ts_align4((size_t)nt); }
__host__ __device__ constexpr size_t ts_off_items(int nst, int nt) { return ts_off_hctr(nst, nt) + ts_align4((size_t)nt); }
__host__ __device__ constexpr size_t ts_off_hdr(int nst, int nt) { return ts_off_items(nst, nt) + ((size_t)2 * nt + kHeavyExtra + 1) * 8; }
__host__ __device__ constexpr size_t ts_off_ticket(int nst, int nt) { return ts_off_hdr(nst, nt) + 32; }
__host__ __device__ constexpr size_t ts_off_pool(int nst, int nt) { return ts_off_ticket(nst, nt) + 2; }
__host__ __device__ constexpr size_t ts_off_dir(int nst, int nt) { return ts_off_pool(nst, nt) + 2; }
__host__ __device__ constexpr size_t ts_off_perm(int nst, int nt) { return ts_off_dir(nst, nt) + (size_t)nst * kDirK * 2; }
__host__ __device__ constexpr size_t ts_off_dbg(int nst, int nt) { return ts_off_perm(nst, nt) + ts_align4((size_t)nt); }
// cnt4[nt * 4]   the lengths of a tile's two (four) streams, indexed by TILE (the work list is in launch order): what a
//                peer reads of this rank's store in the owner-computes sharded form
__host__ __device__ constexpr size_t ts_off_cnt4(int nst, int nt) { return ts_align4(ts_off_dbg(nst, nt) + 128); }  // (dbg: 64 u64 time stamps, RTR_EXPERIMENT builds)
// sub[kSubTickets * 32]  (u64 at the start of each 128-byte line) first level of T1's ticket: the workgroups of the
//                point kernel finish within a few microseconds of each other, and 1024 returning adds on ONE word
//                serialise at ~11 ns each (the last workgroup learnt that it was last ~10 us after it had finished);
//                32 words on lines of their own take 32 adds each, and the last arrival of each adds to ticket[]
constexpr int kSubTickets = 32;
__host__ __device__ constexpr size_t ts_off_sub(int nst, int nt) { return ts_off_cnt4(nst, nt) + (size_t)nt * 4; }
// LEAN frames (whole single-GPU frames without split tiles: the usual case): T1 ends without ticket and epilogue; the
// tile kernel's workgroup at launch position b takes tile order[b], reads that tile's stream counters ITSELF and resets
// them; the frame's book-keeping (statistics, error word, pool cursor, next launch order) is done by the tile launch's
// one extra workgroup, off every critical path.
// order[2][nt]   launch position -> tile (the inverse of perm[]), per frame parity: the tile workgroups of a lean frame of
//                parity p read order[p] while that launch's extra workgroup writes order[p ^ 1] for the next frame
// lcnt[2][nt]    per frame parity: entries per tile of a lean frame, stored by its tile workgroups (plain stores: 2040
//                adds on a handful of statistics words would queue up on one memory channel and hold every tile
//                workgroup's first wave back -- measured: +13 us on the tile kernel); summed up into hdr[] by the NEXT lean
//                frame's extra workgroup (or by rtr_frame_stats), which sees them complete and stable
// lflag[4]       lflag[p] = 1 while lcnt[p] holds a frame that has not been folded into hdr[] yet
__host__ __device__ constexpr size_t ts_off_order(int nst, int nt) { return ts_off_sub(nst, nt) + (size_t)kSubTickets * 32; }
__host__ __device__ constexpr size_t ts_off_lcnt(int nst, int nt) { return ts_off_order(nst, nt) + 2 * ts_align4((size_t)nt); }
__host__ __device__ constexpr size_t ts_off_lflag(int nst, int nt) { return ts_off_lcnt(nst, nt) + 2 * ts_align4((size_t)nt); }
__host__ __device__ constexpr size_t ts_meta_words(int nst, int nt) { return ts_off_lflag(nst, nt) + 4; }
static_assert(ts_off_items(150, 75) % 4 == 0 && ts_off_hdr(150, 75) % 4 == 0 && ts_off_ticket(150, 75) % 2 == 0 &&
              ts_off_pool(150, 75) % 2 == 0 && ts_off_dir(150, 75) % 2 == 0 && ts_off_dbg(150, 75) % 2 == 0 &&
              ts_off_cnt4(150, 75) % 4 == 0,
              "tile store sub-arrays: 16-byte records / 8-byte words must be aligned (320x240: nst = 150)");
__host__ __device__ inline uint32_t *ts_fill(const TileStore &S) { return S.meta; }
__host__ __device__ inline uint32_t *ts_count(const TileStore &S) { return S.meta + ts_off_count(S.nst, S.ntiles); }
__host__ __device__ inline uint32_t *ts_tile_cnt(const TileStore &S) { return S.meta + ts_off_tile_cnt(S.nst, S.ntiles); }
__host__ __device__ inline uint32_t *ts_hctr(const TileStore &S) { return S.meta + ts_off_hctr(S.nst, S.ntiles); }
__host__ __device__ inline uint32_t *ts_items(const TileStore &S) { return S.meta + ts_off_items(S.nst, S.ntiles); }
__host__ __device__ inline uint32_t *ts_hdr(const TileStore &S) { return S.meta + ts_off_hdr(S.nst, S.ntiles); }
__host__ __device__ inline uint32_t *ts_ticket(const TileStore &S) { return S.meta + ts_off_ticket(S.nst, S.ntiles); }
__host__ __device__ inline unsigned long long *ts_pool(const TileStore &S) {
    return reinterpret_cast<unsigned long long *>(S.meta + ts_off_pool(S.nst, S.ntiles));
}
__host__ __device__ inline uint32_t *ts_perm(const TileStore &S) { return S.meta + ts_off_perm(S.nst, S.ntiles); }
constexpr uint32_t kItemSkip = 0xFFFFFFFEu;
__host__ __device__ inline unsigned long long *ts_dbg(const TileStore &S) {
    return reinterpret_cast<unsigned long long *>(S.meta + ts_off_dbg(S.nst, S.ntiles));
}
__host__ __device__ inline unsigned long long *ts_sub(const TileStore &S, uint32_t g) {
    return reinterpret_cast<unsigned long long *>(S.meta + ts_off_sub(S.nst, S.ntiles) + (size_t)g * 32);
}
__host__ __device__ inline uint32_t *ts_order(const TileStore &S, int parity) {
    return S.meta + ts_off_order(S.nst, S.ntiles) + (size_t)parity * ts_align4((size_t)S.ntiles);
}
__host__ __device__ inline uint32_t *ts_lcnt(const TileStore &S, int parity) {
    return S.meta + ts_off_lcnt(S.nst, S.ntiles) + (size_t)parity * ts_align4((size_t)S.ntiles);
}
__host__ __device__ inline uint32_t *ts_lflag(const TileStore &S) { return S.meta + ts_off_lflag(S.nst, S.ntiles); }
// (lean frames: T1's workgroups add their colour-chunk counts to the second 8-byte word of the sub-ticket lines)
__host__ __device__ inline unsigned long long *ts_sub_colour(const TileStore &S, uint32_t g) { return ts_sub(S, g) + 1; }
__host__ __device__ inline uint4 *ts_cnt4(const TileStore &S) { return reinterpret_cast<uint4 *>(S.meta + ts_off_cnt4(S.nst, S.ntiles)); }
__host__ __device__ inline unsigned long long *ts_dir(const TileStore &S) {
    return reinterpret_cast<unsigned long long *>(S.meta + ts_off_dir(S.nst, S.ntiles));
}
// kHdrError: the tile-store error code of the LAST frame (0: none; 1: an extent never appeared, 2: the extent pool
// overflowed -- entries were dropped), published by T1's epilogue from kHdrErrLive, which store_error() ORs into
// while T1 runs; kHdrColourChunks: 256-point chunks with at least one in-frustum point (each loads 1 KiB of colours)
enum { kHdrItems = 0, kHdrSplitItems = 1, kHdrEntries = 2, kHdrHeaviest = 3, kHdrSlice = 4, kHdrError = 5,
       kHdrSplitTiles = 6, kHdrColourChunks = 7, kHdrConsts = 8, kHdrErrLive = 28,
       // k_tile_split: slice records taken in its min phase, slices whose minima are in the depth buffer, records taken
       // in its second phase
       kHdrSplitQ1 = 29, kHdrSplitDone = 30, kHdrSplitQ2 = 31 };
static_assert(kHdrConsts + sizeof(StoreConsts) / 4 <= kHdrErrLive, "StoreConsts overlaps the header words behind it");
__host__ __device__ inline const StoreConsts *ts_consts(const TileStore &S) {
    return reinterpret_cast<const StoreConsts *>(ts_hdr(S) + kHdrConsts);
}

#ifdef RTR_EXPERIMENT
void read_filter_stamps(hipStream_t s, unsigned long long *out16);
#endif
void launch_clear(hipStream_t s, uint32_t *depth, uint32_t *acc, size_t npix);
// mode 0: the reference's structure (two full streams, global atomics)
void launch_min_depth(hipStream_t s, const Cloud &c, const Proj &P, int W, int H, uint32_t *depth);
void launch_accumulate(hipStream_t s, const Cloud &c, const Proj &P, int W, int H, const uint32_t *depth,
                       uint32_t *acc, float window);
// mode 1 (default): tile-binned pipeline -- T1 stream + lists + histogram, T2 scan + T3 scatter,
// T4 per-tile LDS z-buffer (tile mode 0 whole frame, 1 min only, 2 accumulate only)
constexpr int kDefaultPointGrid = 1024;
int tile_count(int W, int H);          // processing tiles (32x32, or 64x32 above 4096 of them)
int storage_tile_count(int W, int H);  // 32x16 storage tiles
// T1: stream the cloud once, append every in-frustum point to its storage tile's stream; the last
// workgroup to finish turns the stream lengths into the tile kernel's work list (and, with
// `clear_split`, resets depth / accumulators of the tiles that will be split; the frame buffers and
// the occupancy bitmap of the peer-to-peer exchange are named by StoreConsts in the store's header).
// bounds != NULL enables per-chunk frustum culling (see k_project_bin)
void launch_project_bin(hipStream_t s, const Cloud &c, const Proj &P, int W, int H, const TileStore &S,
                        const float *bounds, int clear_split, int phases, int xp = 0, hipEvent_t ev_start = nullptr,
                        hipEvent_t ev_stop = nullptr);  // ev_*: signalled by the dispatch itself (time stamps with timing
                                                        // on; ev_stop alone: an overlapped frame's `binned`)
// rtr_render_views: ONE point-kernel launch serves `count` (<= kMaxViews) poses -- view v's in-frustum points go to the tile
// store S[v], each of them a LEAN frame (see ts_off_order) for launch_tile.  tab_host: view_tab_bytes() of host memory
// (pinned: it is copied to tab_dev, the same size of device memory, on the stream, and must not change before the copy
// is done); flags bit 2: no lane test (option "lane_test" = 0)
constexpr int kMaxViews = 8;
size_t view_tab_bytes();
hipError_t launch_project_bin_views(hipStream_t s, const Cloud &c, const Proj *P, const TileStore *S, int count, int W, int H,
                              void *tab_host, void *tab_dev, int flags, int phases, hipEvent_t ev_start = nullptr,
                              hipEvent_t ev_stop = nullptr);
// 6 floats (+ 1) per 256 points; from chunk c0 on (rtr_append_points): c's arrays start at point 256 c0, c.n counts from
// there, bounds + 6 c0, spread + c0
void launch_chunk_bounds(hipStream_t s, const Cloud &c, float *bounds, float *spread);
// packing (see PackedXyz): pack_measure fills hdr[2 nchunks] (bases, widths, block offsets by an exclusive
// scan) and *total_planes (device; in 32-byte units); pack_write fills the blocks; pack_verify counts the points whose decoded
// coordinates differ from the raw ones (must be 0) into *mismatches (device).  nchunks = ceil(ceil(n / 4) / 64).
// Range form (rtr_append_points): `c` is the cloud from chunk c0 on (its arrays start at point 256 c0, c.spread at
// spread + c0, c.n counts from there) and hdr = the headers from chunk c0 on; the scan starts at first_unit, chunk c0's
// block offset, and *total_planes ends as the units of chunks [0, c1).  Every kernel then gives exactly what the
// whole-cloud launch gives for those chunks: a chunk only reads its own 256 points.
void pack_measure(hipStream_t s, const Cloud &c, uint4 *hdr, uint32_t *chunk_planes, uint64_t *total_planes,
                  uint64_t first_unit = 0);  // (c.spread -> hdr[2 c + 1].z)
void pack_write(hipStream_t s, const Cloud &c, const uint4 *hdr, uint32_t *planes, uint32_t *planes_b);
void pack_verify(hipStream_t s, const Cloud &c, const uint4 *hdr, const uint32_t *planes, const uint32_t *planes_b, uint64_t *mismatches);
// x, y, z (padded to a multiple of 4 points) back from the packed form, bit for bit
// (pk.hdr + 2 c0 and n - 256 c0 points: chunks c0.. alone -- the headers' block offsets are absolute)
void unpack_to_soa(hipStream_t s, const PackedXyz &pk, uint64_t n, float *x, float *y, float *z);
// rtr_reorder.hip; perm (may be null) is permuted with the points (option "point_ids": upload index per resident point)
int reorder_morton(hipStream_t s, float *x, float *y, float *z, uint32_t *rgba, uint64_t n, uint32_t *perm = nullptr);
// mean diagonal of the 256-point chunk boxes / diagonal of the cloud's box, from launch_chunk_bounds' output
// absmax[3]: the largest finite |x|, |y|, |z| over the chunk boxes (+inf when no chunk has a finite box)
// scratch: order_quality_scratch_bytes() of device memory the caller owns, or null: the call allocates and frees its own
size_t order_quality_scratch_bytes();
int order_quality(hipStream_t s, const float *bounds, uint64_t n, float *ratio, float absmax[3], void *scratch = nullptr);
// T4: per-tile LDS z-buffer over the tile store.  mode 0 = whole frame (min + accumulate + resolve
// of every unsplit tile, min phase of split tiles), 3 = second phase of the split tiles of a whole
// frame, 1 = min only, 2 = accumulate only, 4 = owner-computes sharded frame: like 0, but only the tiles
// tile_owner() gives to this rank, over the entries of EVERY occupying rank (depth_slices: occ_all, peers, rank, tab).
// write_acc: bit 0 (mode 0) also write the accumulators; bit 1 (modes 1, 2) this launch is the only writer of
// the frame buffer: store instead of folding into what memory holds; bit 2 (modes 1, 2; sharded frames)
// tiles without entries are not written at all (the peers only read tiles of the occupancy bitmap).
// depth_slices (mode 2 only): read the global depth from the ranks' reduced slices and store it to `depth`
// resets depth / accumulators under the tiles T1's epilogue decided to split (what the epilogue itself does when
// launch_project_bin's clear_split is set); for frames whose T1 overlapped the previous frame's tail
void launch_reset_split(hipStream_t s, int W, int H, const TileStore &S, uint32_t *depth, uint32_t *acc);
// write_acc bit 3 (mode 0): a LEAN frame (see ts_off_order) -- T1 ran without epilogue (launch_project_bin's flag 8);
// bit 4 (modes 0, 1): the frame's parity (which lcnt[] half its workgroups write, which order[] they read; the
// launch's extra workgroup writes the OTHER order[])
// ev_stop (modes 0, 3): an event the dispatch itself signals when the launch has ended, as launch_project_bin's
void launch_tile(hipStream_t s, int mode, int W, int H, const TileStore &S, float window, uint32_t *depth,
                 uint32_t *acc, uint8_t *img, int write_acc, const TilePyr *pyr, const Sliced *depth_slices = nullptr,
                 hipEvent_t ev_stop = nullptr);
// folds the statistics of the lean frame of parity `parity` into the store's header now (rtr_frame_stats)
void launch_lean_fold(hipStream_t s, int W, int H, const TileStore &S, int parity);
void launch_stream_probe(hipStream_t s, const Cloud &c, const Proj &P, int W, int H, uint32_t *sink, int variant);
void launch_resolve(hipStream_t s, const uint32_t *acc, uint8_t *img, size_t npix);
// img_slices (4 levels only): read the input image from the ranks' resolved slices (chunk in pixels);
// depth_src (4 levels only): read the unfiltered depth from this buffer instead of depth_bits (which is written)
void launch_filter(hipStream_t s, const FilterLevels &L, uint32_t *depth_bits, uint8_t *img, uint8_t *mask,
                   uint16_t *tensor, uint32_t *minmax, uint32_t *part_min, uint32_t *part_max, int W, int H,
                   float strength, float thr, int pyramid_parts, const Sliced *img_slices = nullptr,
                   const uint32_t *depth_src = nullptr);
void launch_p2p_sync(hipStream_t s, uint32_t *my_flags, const PeerSet &peer_flags, int rank, int world, uint32_t seq,
                     uint32_t *status, unsigned long long timeout_ticks);
// the same barrier + every rank's occupancy bitmap gathered into occ_all[world * 128] (local memory)
void launch_p2p_sync_gather(hipStream_t s, uint32_t *my_flags, const PeerSet &peer_flags, int rank, int world, uint32_t seq,
                            uint32_t *status, unsigned long long timeout_ticks, const PeerSet &occ, uint32_t *occ_all);
constexpr int kP2POccBytes = 512;  // occupancy bitmap: one bit per screen tile (<= 4096)
// the frame owner's last step: every tile another rank produced is copied over xGMI into the local depth buffer /
// image (tiles nobody has points in are cleared) and the prefilter's pyramid levels / min-max partials emitted
void launch_p2p_collect(hipStream_t s, int W, int H, const OwnedTab *tab, const uint32_t *occ_all, int world, int rank,
                        uint32_t *depth, uint8_t *img, const TilePyr *pyr);
void launch_p2p_occupancy(hipStream_t s, const uint32_t *tile_cnt, int W, int H, uint32_t *occ);
void launch_p2p_depth_reduce(hipStream_t s, const PeerSet &depth, const PeerSet &occ, uint32_t *red, size_t first,
                             size_t count, int world, int W, int H);
void launch_p2p_gather(hipStream_t s, const PeerSet &src, void *dst, size_t chunk_bytes, size_t nbytes,
                       int skip_owner);  // skip_owner < 0: copy every slice
void launch_p2p_acc_resolve(hipStream_t s, const PeerSet &acc, const PeerSet &occ, uint8_t *img, size_t first,
                            size_t count, int world, int W, int H);
void launch_generate(hipStream_t s, int scene, uint64_t seed, uint64_t first, uint64_t count, uint64_t total,
                     float *x, float *y, float *z, uint32_t *rgba);
void launch_aos_to_soa(hipStream_t s, const uint8_t *xyz, size_t xyz_stride, const uint8_t *rgb, size_t rgb_stride,
                       uint64_t count, float *x, float *y, float *z, uint32_t *rgba);
void launch_soa_to_aos(hipStream_t s, const float *x, const float *y, const float *z, const uint32_t *rgba,
                       uint64_t count, float *xyzw, uint8_t *rgba_out);
// (a, b: device buffers padded to 16 bytes; ha, hb: device pointers of mapped pinned host buffers, padded likewise)
void launch_copy_to_host(hipStream_t s, const void *a, void *ha, size_t bytes_a, const void *b, void *hb, size_t bytes_b);
void launch_pad_nan(hipStream_t s, float *x, float *y, float *z, uint32_t *rgba, uint64_t n, uint64_t n_pad);  // (rgba may be null)
// rtr_point_pass: streams the RESIDENT coordinates once (packed: chunks rejected on their header boxes, survivors
// decoded; else the fp32 SoA) and, for the frame `depth` holds, atomicMin's the upload index of every point whose
// depth bits are its pixel's into ids[H*W] (cleared to 0xFFFFFFFF by the caller) and sets the bit of every point the
// accumulate pass would count in vis (8 u32 per 256-point chunk; with perm == null every word is stored, with perm
// the caller clears it and the bits go through perm[resident index] = upload index).  ids / vis may be null.
void launch_point_pass(hipStream_t s, const Cloud &c, const Proj &P, int W, int H, const uint32_t *depth, float window,
                       uint32_t *ids, uint32_t *vis, const uint32_t *perm);
void launch_iota(hipStream_t s, uint32_t *out, uint64_t n, uint64_t first = 0);  // out[i] = first + i
// rtr_set_point_keep / a sort: the resident-order keep mask and its chunk summary (Keep) from the upload-order mask
// `up` ((n + 31) / 32 words; perm: resident index -> upload index, null while the cloud is in upload order).  Also
// clears the bits of `up` at or past n.  res: 8 words per chunk, sum: a byte per chunk.  c0 > 0: only chunks [c0, ..)
// are built (rtr_append_points: the earlier ones hold no new point)
void launch_keep_build(hipStream_t s, uint32_t *up, const uint32_t *perm, uint64_t n, uint32_t *res, uint8_t *sum,
                       uint64_t c0 = 0);
// rtr_append_points: the upload-order mask of n0 points grown to n1, the new points kept (bits [n0, n1) set)
void launch_keep_append(hipStream_t s, uint32_t *up, uint64_t n0, uint64_t n1);

// rtr_remove_points (section 2c): keep = the upload-order keep words of the n resident points (bits at or past n are
// ignored), perm = resident index -> upload index (null while the cloud is in upload order).
// remove_count: cnt[c] = the survivors of chunk c, *first_loss (device, set to ~0 by the caller) = the first chunk that
// loses a point.
void launch_remove_count(hipStream_t s, const uint32_t *keep, const uint32_t *perm, uint64_t n, uint32_t *cnt, uint64_t *first_loss);
// out[i] = the exclusive sum of in[0 .. i) -- popc_bits > 0: of the popcounts of words holding popc_bits bits -- and
// *total (device) = the sum of all; scratch: scan_scratch_words(count) words
uint64_t scan_scratch_words(uint64_t count);
void launch_scan_u32(hipStream_t s, const uint32_t *in, uint64_t count, uint64_t popc_bits, uint32_t *out, uint32_t *scratch,
                     uint64_t *total);
// the survivors of chunks c0.. (c: the resident cloud; its fp32 SoA when c.x is set, else its packed form) into the
// window: x / y / z / rgba (and the renumbered upload indices, wperm non-null: perm non-null, wscan = the exclusive
// popcount scan of keep) from dst[c] - 256 c0 on, dst = the exclusive scan of cnt
void launch_remove_compact(hipStream_t s, const Cloud &c, const uint32_t *perm, const uint32_t *keep, const uint32_t *wscan,
                           const uint32_t *dst, uint64_t c0, float *wx, float *wy, float *wz, uint32_t *wrgba, uint32_t *wperm);
// rtr_extract_points (section 2e): one window of the extraction.  The selected points (sel: upload-order words, bits at
// or past n ignored, null = every point; perm as for remove; wscan = the exclusive popcount scan of sel, total = its
// sum) of ranks [first, first + count) go to slot rank - first of the device buffers xyz / rgb / idx (each may be null):
// xyz_form 0 = three floats per record, 1 = x, y, z, 1.0f as four floats, 2 = the same as one 16-byte store (base and
// stride multiples of 16); rgb_form 0 = three bytes, 1 = c0, c1, c2, 255 as four bytes, 2 = the same as one dword (base
// and stride multiples of 4).  Only chunks [c0, c1) are visited; without sel and perm the rank is the resident index
// and the caller passes the window's chunks (extract_all_chunks).  Coordinates from the fp32 SoA (x4, y4, z4) when x4
// is set, else from the packed form pk; rgba4: the resident colours.
struct ExtractArgs {
    PackedXyz pk;
    const float4 *x4, *y4, *z4;
    const uint4 *rgba4;
    const uint32_t *perm, *sel, *wscan;
    uint64_t n, total, c0, c1, first, count;
    uint8_t *xyz, *rgb;
    uint32_t *idx;
    uint64_t xyz_stride, rgb_stride;
    int xyz_form, rgb_form;
};
void launch_extract(hipStream_t s, const ExtractArgs &a);
// the upload-order mask `up` of n points compacted onto the survivors: up1 (zeroed by the caller) gets old[keep]
void launch_remove_mask(hipStream_t s, const uint32_t *keep, const uint32_t *wscan, const uint32_t *up, uint64_t n, uint32_t *up1);
// the upload indices perm[0 .. count) of resident points that all stay (the chunks in front of the window; count a
// multiple of 4) renumbered into out, another array: out[r] = the kept points below perm[r]
void launch_remove_renumber(hipStream_t s, const uint32_t *perm, uint64_t count, const uint32_t *keep, const uint32_t *wscan,
                            uint32_t *out);

// rtr_transform_points (section 2d): sel = the caller's upload-order selection words (bits at or past n ignored; null:
// every point), perm as for remove.
// transform_span: span[0] / span[1] (device, set to ~0 / 0 by the caller) = the first / last chunk holding a selected point
void launch_transform_span(hipStream_t s, const uint32_t *sel, const uint32_t *perm, uint64_t n, uint64_t *span);
// chunks c0 .. c1 of c (its fp32 SoA when c.x is set, else its packed form) with the selected points moved by M
// (affine_apply) into wx / wy / wz from point 256 c0 on (the window's arrays index from there), every quad below n;
// in_place (wx = c.x + 256 c0 ...): only the quads holding a selected point are written
void launch_transform_window(hipStream_t s, const Cloud &c, const uint32_t *perm, const uint32_t *sel, uint64_t c0, uint64_t c1,
                             const Affine &M, float *wx, float *wy, float *wz, bool in_place);
// rtr_write_points (section 2f): sel / wscan = the call's upload-order selection words and their exclusive popcount
// scan, (n + 31) / 32 words each; the ranks [first, first + count) of the selection are written.
// write_bits: selw[w] = the bits of sel[w] whose rank lies in that window (rtr_write_index.h); every: the selection is
// every point, and sel / wscan are filled here first (all ones below n, scan 32 w)
void launch_write_bits(hipStream_t s, uint32_t *sel, uint32_t *wscan, uint64_t n, bool every, uint64_t first, uint64_t count,
                       uint32_t *selw);
// launch_transform_window with another source: a point of selw takes the three floats at xyz + (rank - first) * stride
// (device memory, stride a multiple of 4), bit for bit
void launch_write_window(hipStream_t s, const Cloud &c, const uint32_t *perm, const uint32_t *selw, const uint32_t *sel,
                         const uint32_t *wscan, uint64_t c0, uint64_t c1, const uint8_t *xyz, uint64_t stride, uint64_t first,
                         float *wx, float *wy, float *wz, bool in_place);
// the colours of the points of selw in chunks c0 .. c1: rgba[resident index] = c0 | c1 << 8 | c2 << 16 | 0xFF000000 of the
// three bytes at rgb + (rank - first) * stride (device memory; stride 0: one record for all)
void launch_write_colors(hipStream_t s, const uint32_t *perm, const uint32_t *selw, const uint32_t *sel, const uint32_t *wscan,
                         uint64_t n, uint64_t c0, uint64_t c1, const uint8_t *rgb, uint64_t stride, uint64_t first, uint32_t *rgba);
// the block offsets hdr[2 c + 1].xy of chunks [c_from, c_to) move by delta units (the blocks behind a rebuilt window moved)
void launch_shift_units(hipStream_t s, uint4 *hdr, uint64_t c_from, uint64_t c_to, int64_t delta);
// out[0] / out[1] (device, zeroed by the caller) += the wide chunks of the packed form / those that carry a box word
void launch_wide_counts(hipStream_t s, const uint4 *hdr, uint64_t nchunks, uint64_t *out);
// rtr_select_points: sel (8 u32 per 256-point chunk, upload order, no bit set at or past n) := op(sel, hit) with
// hit = inside or, invert, !inside for the points below n; inside = clip_keep over `clip` (the CALL's planes, not the
// cloud's) and, P given, project_point landing on a pixel of rect {x0, y0, x1, y1}.  c: the resident cloud -- its packed
// form when it has one, else its fp32 SoA with the chunk boxes `bounds`; the cloud's own clip planes and keep mask are
// not read.  perm as for the point pass (with it and op REPLACE the caller clears sel first).  stats (device, may be
// null): [1] / [2] / [3] += chunks decided outside / inside on their boxes / decoded.  op: 0 replace, 1 add, 2 subtract,
// 3 intersect, 8 toggle.
void launch_select(hipStream_t s, const Cloud &c, const float *bounds, const Clip &clip, const Proj *P, int W, int H,
                   const int rect[4], int op, bool invert, uint32_t *sel, const uint32_t *perm, uint64_t *stats);
// *out (device) += the set bits of sel, all 8 words of every chunk of n points
void launch_select_count(hipStream_t s, const uint32_t *sel, uint64_t n, uint64_t *out);

// rtr_select_voxel_grid (rtr_voxel.hip; the cell arithmetic is rtr_voxel_key.h's): inv[k] = 1.0f / cell[k], host-rounded
struct VoxelGrid {
    float origin[3], inv[3];
};
// voxel_keys: keys[u] / vals[u] = voxel_key (kVoxelOut | u when out of the grid) / u for every resident point below n, u
// its upload index (perm as for the point pass; null: the resident index); n pairs each, in ascending upload index
void launch_voxel_keys(hipStream_t s, const Cloud &c, const uint32_t *perm, const VoxelGrid &g, uint64_t *keys, uint32_t *vals);
// rocPRIM's stable radix sort of the n pairs by key, k0 / v0 -> k1 / v1; voxel_sort_temp_bytes: the temporary it asks
// for.  Both return a hipError_t as int
int voxel_sort_temp_bytes(uint64_t n, size_t *bytes);
int voxel_sort(hipStream_t s, void *tmp, size_t tmp_bytes, const uint64_t *k0, uint64_t *k1, const uint32_t *v0, uint32_t *v1,
               uint64_t n);
// voxel_heads: over the sorted pairs, hit ((n + 31) / 32 words, zeroed by the caller) gets the bit vals[j] of the first
// pair j of every run of equal keys that holds at least min_count (>= 1) pairs; stats (device, zeroed by the caller):
// [1] / [2] / [3] += runs of in-grid keys / those of them with at least min_count pairs / out-of-grid pairs
void launch_voxel_heads(hipStream_t s, const uint64_t *keys, const uint32_t *vals, uint64_t n, uint32_t min_count, uint32_t *hit,
                        uint64_t *stats);
// voxel_combine: sel (8 u32 per 256-point chunk) := op(sel, invert ? ~hit : hit), bits at or past n never set by it; op
// as launch_select's
void launch_voxel_combine(hipStream_t s, const uint32_t *hit, uint64_t n, int op, bool invert, uint32_t *sel);

// rtr_select_neighbours (rtr_neighbours.hip; the cell arithmetic is rtr_neighbour_cell.h's, the sweep rtr_key_sweep.h's,
// the sort and the combine rtr_voxel.hip's).
// neighbour_keys: voxel_keys with the internal grid of `radius`; also rec[u] = (x, y, z, bits of u) for every point, and
// counters (device, zeroed by the caller) [0] / [1] += points that are not finite / finite but beyond the grid's span
void launch_neighbour_keys(hipStream_t s, const Cloud &c, const uint32_t *perm, float radius, uint64_t *keys, uint32_t *vals, float4 *rec,
                           uint64_t *counters);
// out[j] = rec[vals[j]] for the first m sorted pairs (those with a cell)
void launch_neighbour_gather(hipStream_t s, const uint32_t *vals, const float4 *rec, uint64_t m, float4 *out);
// *cells (device) += the runs of equal keys among the first m sorted keys
void launch_neighbour_cells(hipStream_t s, const uint64_t *keys, uint64_t m, uint64_t *cells);
// the work list: 20 words per item, one item per (run, 64-pair slice of it), *cursor (device, zeroed by the caller) items,
// at most cap (min(cells + m / 64, m) always suffices)
constexpr int kNbItemWords = 20;  // {q0, qn, lo_0, hi_0, .. lo_8, hi_8}
void launch_neighbour_items(hipStream_t s, const uint64_t *keys, uint64_t m, uint32_t *items, uint32_t *cursor, uint64_t cap);
// the pair tests over the sorted records: hit ((n + 31) / 32 words, zeroed by the caller) gets the bit of every point
// with at least min_neighbours (>= 1) others at ((dx dx + dy dy) + dz dz) <= r2; stats (device, zeroed) [1] / [2] +=
// those points / the points of the list with no neighbour at all; *tests (device, zeroed) += the pair tests made
void launch_neighbour_count(hipStream_t s, const float4 *rec, const uint32_t *items, const uint32_t *cursor, uint64_t cap, float r2,
                            uint32_t min_neighbours, uint32_t *hit, uint64_t *stats, uint64_t *tests);

// rtr_select_statistical (rtr_statistical.hip; include/rtr_statistics.h section 6n; everything up to the work list is
// rtr_select_neighbours').
// stat_rows: the pair tests of neighbour_count without its early exit; mean[u] / found[u] (device, n entries in upload
// order, preset by the caller to +inf / 0) = the mean distance of point u to its found[u] = min(k, candidates) nearest
// candidates, for every point of the list; k is 1 .. 64; *tests / *updates (device, zeroed) += the pair tests made / the
// values written into rows
void launch_stat_rows(hipStream_t s, const float4 *rec, const uint32_t *items, const uint32_t *cursor, uint64_t cap, float r2, uint32_t k,
                      float *mean, uint32_t *found, uint64_t *tests, uint64_t *updates);
// stat_sum: *out (device) = the sum over the finite means of the mean (pass 0) or of (mean - mu)^2 (pass 1), in fp64 and
// in a shape that depends on n alone; partial: stat_partials(n) doubles of scratch; *count (device, zeroed; pass 0 only)
// += the finite means
uint64_t stat_partials(uint64_t n);
void launch_stat_sum(hipStream_t s, const float *mean, uint64_t n, int pass, double mu, double *partial, double *out, uint64_t *count);
// stat_hits: hit ((n + 31) / 32 words, every one written) gets the bit of every point with found > 0 and
// (double)mean <= t; stats (device, zeroed) [1] / [2] += those points / the points with found == 0
void launch_stat_hits(hipStream_t s, const float *mean, const uint32_t *found, uint64_t n, double t, uint32_t *hit, uint64_t *stats);

// rtr_estimate_normals (rtr_normals.hip; include/rtr_normals.h section 6o; everything up to the work list is
// rtr_select_neighbours').
// normal_rows: stat_rows' pair tests with rows of (d2, position) ordered by (d2, upload index); for every point u of the
// list found[u] = min(k, candidates) and, where that is >= 2, normals[3 u ..] / curvature[u] = the contract's normal and
// surface variation (device, upload order, preset by the caller to 0 / +inf / 0); view: the viewpoint (host, 3 floats) or
// nullptr; k is 1 .. 64; counts (device, 4 words, zeroed) += the pair tests made, the entries written into rows, the
// points with a normal, the normals the viewpoint rule negated
void launch_normal_rows(hipStream_t s, const float4 *rec, const uint32_t *items, const uint32_t *cursor, uint64_t cap, float r2, uint32_t k,
                        const float *view, float *normals, float *curvature, uint32_t *found, uint64_t *counts);

// rtr_select_clusters (rtr_clusters.hip; everything up to the work list is rtr_select_neighbours').  The union-find runs
// over the n sorted positions: parent, size, minu, seed are n words each.
// cluster_init: parent[j] = j, size[j] = 0, minu[j] = 2^32 - 1, seed[j] = 0
void launch_cluster_init(hipStream_t s, uint64_t n, uint32_t *parent, uint32_t *size, uint32_t *minu, uint32_t *seed);
// cluster_link: the pair tests of neighbour_count without its early exit; every pair at ((dx dx + dy dy) + dz dz) <= r2
// unites its two sorted positions' sets in parent (parent[v] <= v throughout); *tests (device, zeroed) += the pair tests
void launch_cluster_link(hipStream_t s, const float4 *rec, const uint32_t *items, const uint32_t *cursor, uint64_t cap, float r2,
                         uint32_t *parent, uint64_t *tests);
// cluster_flatten: parent[j] = the root of j; at the root size += 1, minu = min(minu, vals[j]), and, with sel (the
// selection words; null: not asked for), seed |= the bit vals[j] of sel
void launch_cluster_flatten(hipStream_t s, const uint32_t *vals, uint64_t n, const uint32_t *sel, uint32_t *parent, uint32_t *size,
                            uint32_t *minu, uint32_t *seed);
// cluster_hits: hit ((n + 31) / 32 words, zeroed by the caller) gets the bit vals[j] of every position whose root's size
// lies in min_points .. max_points (0: unbounded) and, if seeded, whose root's seed is set; labels (device, n words, may
// be null) [vals[j]] = the root's minu; stats (device, zeroed) [1] / [2] += roots / roots that hit, [3] = the largest size
void launch_cluster_hits(hipStream_t s, const uint32_t *vals, uint64_t n, const uint32_t *parent, const uint32_t *size, const uint32_t *minu,
                         const uint32_t *seed, uint32_t min_points, uint32_t max_points, bool seeded, uint32_t *hit, uint32_t *labels,
                         uint64_t *stats);

// rtr_select_near (rtr_near.hip; rtr.h section 6k; the cell arithmetic is rtr_neighbour_cell.h's, the sort rtr_voxel.hip's,
// the gather rtr_neighbours.hip's).
// near_keys: the `count` (< 2^32) given points at xyz + j * stride (DEVICE memory, stride a multiple of 4): keys[j] / vals[j] =
// the cell key in the internal grid of `radius` (kNbOut | j without a cell) / j, rec[j] = (x, y, z, bits of j); counters
// (device, zeroed by the caller) [0] / [1] += points that are not finite / finite but beyond the span; box (device, preset
// to three words of 2^32 - 1 and three of 0) = the float_order_key of the smallest / largest x, y, z among the points
// with a cell
void launch_near_keys(hipStream_t s, const uint8_t *xyz, uint64_t stride, uint64_t count, float radius, uint64_t *keys, uint32_t *vals,
                      float4 *rec, uint64_t *counters, uint32_t *box);
// that box on the host (only when some point has a cell)
void near_box_from_keys(const uint32_t box[6], double lo[3], double hi[3]);
// near_sweep: keys / rec = the m sorted given points with a cell, glo / ghi their box.  hit (upload order, (n + 31) / 32
// words, zeroed by the caller; null: not asked for) gets the bit of every resident point at ((dx dx + dy dy) + dz dz) <=
// r2 from a given point, near (zeroed; null: not asked for) the bit rec.w of every given point at that distance from a
// resident one.  c / bounds as for launch_select, perm as for the point pass.  counters (device, zeroed) [0] += resident
// points that hit, [1] += pair tests, [2] / [3] += chunks decided without their coordinates / decoded
void launch_near_sweep(hipStream_t s, const Cloud &c, const float *bounds, const uint32_t *perm, const uint64_t *keys, const float4 *rec,
                       uint64_t m, float radius, float r2, const double glo[3], const double ghi[3], uint32_t *hit, uint32_t *near,
                       uint64_t *counters);

// rtr_nearest_points (rtr_nearest.hip; rtr.h section 6l; the given points go through near_keys, the sort and the gather
// above, the sweep is rtr_near_sweep.h's, shared with near_sweep).
// nearest_sweep: keys / rec / glo / ghi / c / bounds / perm / counters as for near_sweep.  slots (m's `count` words of 64
// bits, all ones before the launch) [rec.w] = the smallest (bits of d2) << 32 | upload index over the resident points at
// ((dx dx + dy dy) + dz dz) <= r2 from that given point.  ridx / rd2 (both or neither; upload order, padded to a multiple
// of 4 points, preset to 2^32 - 1 / the bits of +inf) [u] = the given index with the smallest (d2, given index) for
// resident point u / the bits of that d2; a point with no given point at that distance is not written
void launch_nearest_sweep(hipStream_t s, const Cloud &c, const float *bounds, const uint32_t *perm, const uint64_t *keys, const float4 *rec,
                          uint64_t m, float radius, float r2, const double glo[3], const double ghi[3], uint64_t *slots, uint32_t *ridx,
                          uint32_t *rd2, uint64_t *counters);
// nearest_unpack: idx[j] / d2[j] (device, count words each, either may be null) = the low / high half of slots[j], or
// 2^32 - 1 / the bits of +inf for a slot of all ones; *have (device, zeroed by the caller) += the slots that are not
void launch_nearest_unpack(hipStream_t s, const uint64_t *slots, uint64_t count, uint32_t *idx, uint32_t *d2, uint64_t *have);

// rtr_nearest_k_points (rtr_nearest_k.hip; rtr.h section 6m; given points and sweep as for rtr_nearest_points).
// nearest_k_sweep: as nearest_sweep with a ROW of k slots per given point: rows (count * k words of 64 bits, all ones before
// the launch) [rec.w * k + s] = the (s + 1)-th smallest (bits of d2) << 32 | upload index over the resident points within
// r2 of that given point, all ones past their number (rtr_topk_cascade.h).  1 <= k <= 64.  *cascades (device, zeroed by
// the caller) += the cascades started: it depends on timing
void launch_nearest_k_sweep(hipStream_t s, const Cloud &c, const float *bounds, const uint32_t *perm, const uint64_t *keys, const float4 *rec,
                            uint64_t m, float radius, float r2, const double glo[3], const double ghi[3], uint64_t *rows, uint32_t k,
                            uint64_t *cascades, uint64_t *counters);
// nearest_k_unpack: idx / d2 (device, count * k words each) = the low / high halves of the rows, 2^32 - 1 / the bits of
// +inf for a slot of all ones; found[j] (count words) = row j's real entries; any of the three may be null.  tally (device,
// zeroed by the caller) [0] += rows with an entry, [1] += entries, [2] += full rows
void launch_nearest_k_unpack(hipStream_t s, const uint64_t *rows, uint64_t count, uint32_t k, uint32_t *idx, uint32_t *d2, uint32_t *found,
                             uint64_t *tally);

// rtr_count_in_bands (rtr_planes.hip; rtr.h section 6j).  counts[k] (device, zeroed by the caller) += the points of the
// population in band k of `bands` (HOST memory, count x {a, b, c, d_lo, d_hi}), kBandPass bands per launch: every chunk is
// classified on its box against all bands of a pass and decoded at most once per pass.  c / bounds as for launch_select.
// res: null = every resident point, else the selection in RESIDENT order (8 words per chunk, no bit at or past n).
// stats (device, zeroed by the caller): [1] / [2] / [3] += (chunk, band) pairs decided outside / inside on the box / tested
// point by point.
// res (8 words per 256-point chunk, every word written) = the upload-order words `up` (read only; bits at or past n
// ignored) in RESIDENT order through perm (resident index -> upload index)
void launch_sel_gather(hipStream_t s, const uint32_t *up, const uint32_t *perm, uint64_t n, uint32_t *res);
// words (device, (n + 31) / 32, zeroed by the caller) |= the bit of every idx[0 .. count) (device; each below n)
void launch_set_bits(hipStream_t s, const uint32_t *idx, uint64_t count, uint32_t *words);
constexpr int kBandPass = 64;  // (a lane's band mask is one 64-bit word, the not-packed path's one ballot)
void launch_count_bands(hipStream_t s, const Cloud &c, const float *bounds, const float *bands, uint32_t count, const uint32_t *res,
                        uint64_t *counts, uint64_t *stats);

}  // namespace rtr
