// rtr_host.h -- what the host translation units share (rtr_api.hip: contexts, the cloud and its edits, frames, buffers;
// rtr_select_api.hip: the selection and analysis calls of rtr.h sections 6f - 6l): the context, the error path, a call's
// device guard and device buffers, and the handful of helpers of rtr_api.hip that the selection calls use too.  Every
// function declared here is defined once, in rtr_api.hip unless noted, and stays out of the library's exported symbols.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/rtr.h"
#include "rtr_alloc.h"
#include "rtr_kernels.h"
#include "rtr_overlap_policy.h"

struct rtr_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    rtr_params prm{};
    std::string err;

    // resident cloud (SoA)
    float *x = nullptr, *y = nullptr, *z = nullptr;
    uint32_t *rgba = nullptr;
    float *bounds = nullptr;    // bounding box per 256-point chunk (frustum culling option)
    float *spread = nullptr;    // lane spread per 256-point chunk (rtr::Cloud::spread: T1's lane test)
    float absmax[3] = {0.f, 0.f, 0.f};  // largest finite |x|, |y|, |z| of the resident cloud
    int opt_lane_test = 1;      // T1 tests one point per lane first (option "lane_test")
    int opt_chunk_test = 1;     // T1 tests packed chunks on their header boxes first (option "chunk_test")
    int opt_keep_soa = 0;       // 1: the fp32 SoA arrays stay resident beside the packed form (option "keep_soa")
    int opt_pool_worst = 0;     // 1: the extent pool is always sized for the worst case, 2 n entries (option "pool_worst_case")
    int opt_lean = 1;           // whole single-GPU frames without split tiles end T1 without its epilogue (option "lean")
    int opt_lean_identity = 1;  // lean frames: tile workgroup b takes tile b when the whole launch is resident (option "lean_identity")
    int opt_lean_early = -1;    // lean frames: first batch of entries requested before the stream counters are known: 0 never,
                                // 1 always, -1 when the previous frame's tiles were full (option "lean_early")
    bool last_lean = false;     // the last binned frame was a lean one (its statistics are folded on demand; FrontSet::parity)
    uint64_t n = 0, cap = 0;
    uint4 *pk_hdr = nullptr;        // rtr::PackedXyz of the resident cloud (option "pack"); null: not in use
    uint32_t *pk_planes = nullptr, *pk_planes_b = nullptr;  // (one allocation: A streams, then B streams)
    uint64_t pk_bytes = 0;          // headers + planes
    uint64_t pk_units = 0, pk_units_cap = 0;  // 32-byte units of the planes in use / allocated (rtr_append_points grows them)
    uint64_t pk_hdr_chunks = 0;     // chunks the header array holds (+ the zero pair behind them)
    int opt_pack = 1;               // 0 never, 1 when it saves >= 1/8 of the coordinate stream, 2 always + verified after packing

    int W = 0, H = 0;  // resolution
    rtr::Clip clip{};  // the user's clip planes (rtr_set_clip_planes; count 0: none): every point kernel of a frame honours them

    // tile-binned pipeline: the tile store T1 appends to and T4 reads (rtr_kernels.h)
    struct FrontSet {
        rtr::TileStore store{};
        uint64_t pool_n = 0;        // point count the dynamic extent pool was sized for
        int nst = 0, ntiles = 0;    // tile counts the per-tile arrays were sized for
        rtr::StoreConsts consts{};  // host copy of the store's header constants
        uint64_t *dyn = nullptr;    // dynamic extent pool
        uint64_t dyn_cap = 0;
        hipEvent_t binned = nullptr, consumed = nullptr;  // T1 done (front stream) / T4 done (tail stream)
        bool consumed_valid = false;
        int parity = 0;             // lean-frame parity of this store: order[], lcnt[] and the lflag words live in it
        bool lean_pending = false;  // its last frame was a lean one whose statistics no later frame has folded yet
    };

    // What a set of frames renders into: the single frame (rtr_render, the phase calls; with option "overlap" T1 of
    // frame k+1 fills its second set on the front stream while the tail of frame k still reads the other) or a batch
    // of views (rtr_render_views, one set per view).  depth / img / tensor hold `cap` frames (alloc_target); the
    // accumulators, prefilter mask, min / max partials and pyramid levels are scratch that the frames take in turn.
    // Stores are allocated per resolution and pools per cloud by the frames that use them; the minmax words and the
    // mapped words live as long as the context.
    struct Target {
        int cap = 0;
        uint32_t *depth = nullptr, *acc = nullptr, *part_min = nullptr, *part_max = nullptr;
        uint8_t *img = nullptr, *mask = nullptr;
        uint16_t *tensor = nullptr;
        uint32_t *minmax = nullptr;  // 2 words per frame, RTR_MAX_VIEWS frames
        float *lv[9] = {nullptr};    // pyramid levels 1..lv_levels (level 0 is a frame's depth)
        int lv_levels = 0;
        FrontSet fs[RTR_MAX_VIEWS];
        int cur = 0;                 // the set of the last frame (the single frame alternates with option "overlap")
        uint32_t *err_host = nullptr, *err_dev = nullptr;  // mapped word: tile-store error bits of frames since it was last read
        uint32_t *entries_host = nullptr, *entries_dev = nullptr;  // mapped word: entries of the last frame whose statistics are complete
        uint64_t entries_max = 0;    // the most entries a completed frame of this cloud has had
        bool pool_worst = false;     // the pools are worst-case sized for this cloud: a frame overflowed them, or the peers map them
    } frame, views;
    FrontSet &F() { return frame.fs[frame.cur]; }
    rtr::OverlapPolicy ov;      // option "overlap" and the streak of whole frames: which of them run T1 on `front`
    bool frame_overlapped = false;  // the whole frame being queued runs overlapped (mark_consumed)
    int opt_front_priority = 0; // stream priority `front` is created with: 0 default, 1 lowest, 2 highest (option "front_priority")
    int opt_tail_cus = 0;       // CUs per XCD reserved for the tail stream when overlapping (0 = no CU masks)
    hipStream_t front = nullptr;
    hipStream_t masked_tail = nullptr;
    hipEvent_t joined = nullptr;  // recorded on `stream` when a streak of overlapped frames begins: `front` waits for it
    bool list_valid = false;    // bins match list_P / current cloud / resolution / window
    float list_P[12] = {0};
    int opt_mode = 1;           // 0 = two-pass global atomics (the reference's structure),
                                // 1 = tile-binned LDS z-buffer (default)
    int opt_keep_accum = 0;     // whole-frame calls also materialise RTR_BUF_ACCUM
    bool force_atomic = false;       // set around a whole frame that takes the atomic form (> 4096 tiles)
    int opt_heavy = 32768;           // tiles with more entries are split over several workgroups in T4 ...
    int opt_slice = 16384;           // ... into slices of at least this many entries
    int opt_p2p_timeout_ms = 2000;   // peer-to-peer flag barriers give up after this long (option "p2p_timeout_ms")
    int opt_fill_shift = -1;         // spacing of the stream counters, 4 << value bytes; -1: by the frames seen (see "fill_shift")
    int opt_debug_dyn_cap = -1;      // test aid: cap the dynamic extent pool at this many entries (-1: off)
    int opt_debug_extract_window = -1;  // test aid: cap rtr_extract_points' internal window at this many points (-1: off)
    uint32_t debug_store_stamp = 0;  // test aid (option "debug_store_stamp"): the frame stamp tile stores created from now on start at
    int opt_debug_p2p_barrier = -1;  // test aid: the barrier number the next peer-to-peer exchange starts at (-1: off, i.e. 0)
    // whole frames launch k_tile_split (an empty launch costs ~5 us) only while tiles above the split threshold have
    // been seen: T1's epilogue stores their number here (mapped host word, read without a sync -- it describes the
    // last frame whose T1 has COMPLETED, the host may be frames ahead), and the launch stays on for kSplitCooldown
    // frames after the last such report, after an upload, a new resolution or new split options.  A frame that
    // turns out to need it while it is off is still exact (bin_epilogue, `no_split`).
    uint32_t *split_host = nullptr, *split_dev = nullptr;
    int split_cooldown = 0;
    int opt_xp = 0;                  // RTR_EXPERIMENT builds only (tools/kbench.py)
    int opt_phases = 0;         // T1: phase groups of the grid stride (option "phases", see k_project_bin); 0 = automatic
    int opt_probe = 0;          // rtr_stream_probe variant (experiments)
    int opt_cull = 0;           // per-chunk frustum culling in T1
    int opt_auto_reorder = 2;   // Morton-sort a cloud right after upload / generation: 0 never, 1 always, 2 when its
                                // 256-point chunks are not spatially compact (default)
    bool reordered = false;     // the resident cloud was sorted by the library
    int opt_point_ids = 0;      // 1: a sorted cloud keeps its upload order as a resident permutation (option "point_ids")
    uint32_t *perm = nullptr;   // [cap] upload index of every resident point (only while `reordered`)
    // the keep mask (rtr_set_point_keep; keep_up null: none): the caller's upload-order words, and the resident-order
    // copy with its chunk summary the point kernels read (rtr::Keep).  Cleared with every new cloud
    uint32_t *keep_up = nullptr, *keep_res = nullptr;
    uint8_t *keep_sum = nullptr;

    // point pass (rtr_point_pass): per-pixel point IDs [H*W] (per resolution) and the visibility mask (8 words per
    // 256-point chunk; (n + 31) / 32 of them are the buffer)
    uint32_t *pp_ids = nullptr, *pp_vis = nullptr;
    uint64_t pp_vis_words = 0;
    bool pp_vis_current = false;  // the mask was computed for the resident cloud
    hipEvent_t pp_done = nullptr;  // recorded behind the last point pass
    // the selection (rtr_select_points; sel null: none): upload-order words, 8 per 256-point chunk of the cloud it was made
    // for ((n + 31) / 32 of them are the buffer), and the four device words a call with `stats` counts into.  Dropped by
    // everything that renumbers upload indices
    uint32_t *sel = nullptr;
    uint64_t *sel_stats = nullptr;
    int plane_us[2] = {0, 0};     // the last rtr_fit_plane: sampling + extract, counting (host clock, the waits included)
    int voxel_us[3] = {0, 0, 0};  // the last rtr_select_voxel_grid: its key kernel, sort and head kernel, from their own events
    int neighbours_us[3] = {0, 0, 0};  // the last rtr_select_neighbours: key kernel, sort, gather + work list + count kernel
    int neighbours_tests_k = 0;        // ... and its pair tests in thousands (saturating)
    int near_us[2] = {0, 0};           // the last rtr_select_near: the given points' keys, sort and gather; the sweep, combine and counts
    int near_tests_k = 0;              // ... its pair tests in thousands (saturating)
    int near_chunks[2] = {0, 0};       // ... and its resident chunks decided without their coordinates / decoded (saturating)
    int nearest_us[2] = {0, 0};        // the last rtr_nearest_points: the given points' keys, sort and gather; the sweep and the unpack
    int nearest_tests_k = 0;           // ... its pair tests in thousands (saturating)
    int nearest_chunks[2] = {0, 0};    // ... and its resident chunks decided without their coordinates / decoded (saturating)
    int nearest_k_us[2] = {0, 0};      // the last rtr_nearest_k_points: the same five ...
    int nearest_k_tests_k = 0;
    int nearest_k_chunks[2] = {0, 0};
    int nearest_k_cascades_k = 0;      // ... and the cascades its sweep started, in thousands (saturating; depends on timing)
    int clusters_us[3] = {0, 0, 0};    // the last rtr_select_clusters: key kernel, sort, gather + work list + union-find + hits
    int clusters_tests_k = 0;          // ... and its pair tests in thousands (saturating)
    int statistical_us[3] = {0, 0, 0}; // the last rtr_select_statistical: key kernel, sort, gather + work list + rows + sums + hits
    int statistical_tests_k = 0;       // ... its pair tests in thousands (saturating)
    int statistical_updates_k = 0;     // ... and the values written into rows, in thousands (saturating)
    int normals_us[3] = {0, 0, 0};     // the last rtr_estimate_normals: key kernel, sort, gather + work list + rows and fits
    int normals_tests_k = 0;           // ... its pair tests in thousands (saturating)
    int normals_updates_k = 0;         // ... and the entries written into rows, in thousands (saturating)
    float order_ratio = 0.f;    // mean chunk diagonal / cloud diagonal as uploaded
    int opt_grid = rtr::kDefaultPointGrid;  // workgroups of the point kernels

    // peer-to-peer exchange (rtr_p2p_*): own exchange buffers, the peers' mappings, barrier state
    struct P2P {
        uint32_t *red = nullptr;          // [npix] reduced depth; this rank writes its slice, peers read it
        uint8_t *ximg = nullptr;          // [3 * npix] resolved image; same (the prefilter rewrites RTR_BUF_IMAGE in place)
        uint32_t *flags = nullptr;        // [RTR_P2P_MAX_RANKS] uncached: barrier counters written by the peers
        uint32_t *occ = nullptr;          // [128] one bit per screen tile: this rank's frame has entries there
        uint32_t *occ_all = nullptr;      // [kMaxPeers * 128] every rank's bitmap, gathered by the first barrier of a frame
        bool depth_peers = false;         // rtr_p2p_render: the accumulate launch takes the MIN over the peers' depth itself
        bool depth_in_red = false;        // ... and has left the completed depth in `red` (the peers were reading `depth`)
        bool occ_current = false;         // occ was computed from the bins that are valid now
        bool occ_from_scan = false;       // ... by the epilogue of this frame's T1 (no separate launch)
        bool whole_frame = false;         // inside rtr_p2p_render: the tile launches are the only writers of depth /
                                          // accumulators (no clear, no read-modify-write) and T4<2> emits the pyramid
        bool pyramid_done = false;
        bool depth_sliced = false;        // ... RTR_BUF_DEPTH is completed by the accumulate launch (no depth gather)
        bool image_sliced = false;        // ... the prefilter reads the image from the ranks' slices (no image gather)
        bool acc_from_bins = false;       // the last accumulate pass used exactly those bins
        uint32_t *status_host = nullptr;  // mapped host word: barrier timeouts
        uint32_t *status_dev = nullptr;
        rtr::PeerSet depth{}, accum{}, image{}, reduced{}, flags_of{}, occ_of{}, meta_of{}, ext0_of{}, dyn_of{};
        rtr::OwnedTab *tab = nullptr;     // device copy of the peers' tile-store / frame-buffer mappings (owner-computes form)
        void *opened[9][RTR_P2P_MAX_RANKS] = {};
        int rank = 0, world = 0;
        uint32_t seq = 0;
        uint32_t start = 0;               // the barrier number the flag words were filled with (p2p_alloc): where seq starts at open
        bool open = false;
    } p2p;

    // asynchronous host outputs (rtr_project_async): per slot a device snapshot of depth + image (so the next
    // frame's kernels may overwrite the frame buffers), pinned host buffers, and the events that order the two
    // streams -- the device-to-host copies run on `copy_stream` beside the next frame's kernels
    struct HostOut {
        uint8_t *img = nullptr, *dimg = nullptr;
        float *depth = nullptr;
        uint32_t *ddepth = nullptr;
        void *img_map = nullptr, *depth_map = nullptr;  // the pinned buffers as the device addresses them
        hipEvent_t snap = nullptr, done = nullptr;  // snapshot taken (frame stream) / copies finished (copy stream)
        bool busy = false;
    } ho[RTR_ASYNC_SLOTS];
    hipStream_t copy_stream = nullptr;

    // timing
    int timing = 0;  // 0 off, 1 every phase, 2 only the streaming kernel (RTR_K_MIN_DEPTH / ACCUMULATE), 3 = 2 on every 4th launch
    uint32_t timing_tick = 0;
    struct Span { hipEvent_t a, b; int k; };
    std::vector<Span> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double total_ms[RTR_K_COUNT] = {0};
    uint64_t launches[RTR_K_COUNT] = {0};

    uint64_t cloud_seq = 0;  // +1 per upload / generation (alloc_cloud)

    // rtr::launch_project_bin_views' table (pinned / device); `copied`: the last copy of `host` has been read
    struct ViewTab {
        void *host = nullptr, *dev = nullptr;
        hipEvent_t copied = nullptr;
        bool pending = false;
    } vtab;

    // What a synchronising call renders again when it learns that the adaptive extent pool was too small (repair)
    struct Journal {
        struct Frames {
            float P[RTR_MAX_VIEWS * 16] = {0};
            int count = 0, filter = 0;
            rtr::Clip clip{};  // the clip planes the frames were issued with
        };
        Frames frame;  // the last whole frame (rtr_render): count 0 or 1
        Frames views;  // the last batch of views (rtr_render_views); count 0: none, or it is incomplete
        struct Pass {  // the last point pass
            float P[16] = {0};
            int what = 0;
            bool behind = false;     // queued right behind the last whole frame, nothing rendered since: repeated with it
            bool unchecked = false;  // queued, and not yet known to have read a complete frame
            bool invalid = false;    // its outputs came from a frame the tile store reported incomplete
            rtr::Clip clip{};
        } pass;
        struct Slot {  // the frame queued into each async slot; `stale`: queued before the pool grew (rtr_wait repeats it)
            float P[16] = {0};
            int filter = 0;
            bool stale = false;
            bool sealed = false;  // finished and checked by rtr_set_point_keep: no later overflow makes it stale
            uint64_t cloud = 0;  // cloud_seq when it was queued
            rtr::Clip clip{};
        } slot[RTR_ASYNC_SLOTS];
    } jr;
};

#pragma GCC visibility push(hidden)

int fail(rtr_ctx *c, int code, const char *fmt, ...);  // sets rtr_last_error (c NULL: rtr_create's) and returns code

#define HIP_TRY(c, expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((c), RTR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                     \
    } while (0)

#define NEED(c, cond, msg) \
    do { if (!(cond)) return fail((c), RTR_ERR_INVALID, "%s", msg); } while (0)

struct DevGuard {  // contexts pin their device for the duration of a call and hand the caller's back
    int prev = -1;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev); else prev = -1;
    }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DevGuard(const DevGuard &) = delete;
    DevGuard &operator=(const DevGuard &) = delete;
};

struct DevBufs {  // a call's device buffers: freed on every exit path unless a resident array has taken them (swap_in)
    std::vector<void *> p;
    ~DevBufs() { for (void *q : p) (void)rtr::dev_free(q); }
    template <class T> hipError_t get(T **out, size_t bytes) {
        void *q = nullptr;
        const hipError_t e = rtr::dev_malloc(&q, bytes ? bytes : 4);
        if (e == hipSuccess) p.push_back(q);
        *out = static_cast<T *>(q);
        return e;
    }
    template <class T> void swap_in(T *&field, T *next) {  // a resident array replaced: the old one goes with the scratch
        if (field == next) return;
        p.push_back((void *)field);
        for (auto &x : p) if (x == (void *)next) x = nullptr;
        field = next;
    }
};

int launch_check(rtr_ctx *c, const char *what);  // hipGetLastError behind a launch: "<what> launch failed: ..."
hipError_t d2d(hipStream_t s, void *dst, const void *src, size_t bytes);  // (nothing queued for 0 bytes)
bool on_device(const void *p);  // a caller's array is device (or managed) memory, as opposed to anything the host owns
// Calls that take or return upload-order indices: a cloud sorted by the library must have kept its permutation.
// `verb`: what the call would do with the indices; `or_else`: the call's own way round it, if it has one
int need_upload_order(rtr_ctx *c, const char *verb = "mapped", const char *or_else = "");
int check_indexable(rtr_ctx *c);  // point indices are 32-bit: RTR_ERR_UNSUPPORTED for a larger cloud (rtr_select_api.hip)
rtr::Cloud cloud_of(const rtr_ctx *c);
rtr::Proj make_proj(const float P[16]);
void free_select(rtr_ctx *c);  // waits for the context's streams, then drops the selection
// The read-only option keys that include/rtr_statistics.h documents (rtr.h's list is rtr_get_option's own): *value = the
// key's value and true, or false for any other key (rtr_select_api.hip)
bool statistics_option(const rtr_ctx *c, const char *key, int *value);
// ... and those that include/rtr_normals.h documents
bool normals_option(const rtr_ctx *c, const char *key, int *value);

#pragma GCC visibility pop
