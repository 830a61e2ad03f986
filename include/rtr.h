/*
 * rtr.h -- C ABI of the MI355X point-cloud -> framebuffer projector (librtr_hip.so).
 *
 * Drop-in boundary for the hot path of the reference's `ProjectCloud` class
 * (reference: src/RTRenderer/include/project_cloud.h:11-19).  The reference has no
 * C ABI / FFI of its own -- its boundary is a C++ class dragging in OpenCV, glm
 * and libtorch -- so these entry points are what a binding of that class would
 * need: plain pointers and sizes, no torch / OpenCV / glm types.  The header-
 * compatible C++ facade (include/rtr_project_cloud.hpp) and the Python mirror are
 * thin wrappers over exactly these calls; INTEGRATION.md shows the reference-side
 * binding.
 *
 * Conventions
 *   - every call returns RTR_OK (0) or a negative rtr_status; rtr_last_error()
 *     gives the text.  The library never calls exit() (the reference does:
 *     project_cloud.cu:13-17).
 *   - one context = one GPU = one host thread at a time (project_cloud.cu is not
 *     re-entrant either).  Multi-GPU = one process (context) per GPU; the caller
 *     reduces the exposed device buffers between the phase calls (section 5).
 *   - all work is enqueued on the context's HIP stream; calls that fill host
 *     buffers synchronise that stream before returning, others do not.
 *   - the HIP extension is the only implementation: there is no CPU fallback.
 */
#ifndef RTR_H
#define RTR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct a caller allocates changes size or an entry point changes meaning (2: rtr_p2p_handles grew
 * from 6 to 9 handle blocks, RTR_ERR_INTERNAL, the asynchronous outputs).  A binding compares rtr_abi_version() -- what
 * the loaded library was built with -- against the RTR_ABI_VERSION it was compiled with and refuses to go on when they
 * differ (the Python mirror and rtr::ProjectCloud do). */
#define RTR_ABI_VERSION 2
#define RTR_EMPTY_DEPTH 0x7F7FFFFFu /* render.cu:166, project_cloud.cu:316: bits of FLT_MAX */

typedef struct rtr_ctx rtr_ctx;

typedef enum {
    RTR_OK = 0,
    RTR_ERR_INVALID = -1,   /* bad argument / call order                         */
    RTR_ERR_HIP = -2,       /* a HIP runtime call failed (text in last_error)    */
    RTR_ERR_NO_OUTPUT = -3, /* both host outputs NULL (project_cloud.cu:270-273) */
    RTR_ERR_UNSUPPORTED = -4,/* e.g. filter with W % 2^levels != 0 (quirk Q3)    */
    RTR_ERR_INTERNAL = -5   /* the tile store dropped entries: frames rendered since the last synchronising call
                               are incomplete (returned by rtr_synchronize and by every call that copies results
                               to the host; cannot happen unless the extent pool is mis-sized) */
} rtr_status;

/* Compile-time constants of the reference, made run-time parameters. */
typedef struct {
    float depth_window;       /* render.cu:106            default 0.02f  */
    float filter_strength;    /* project_cloud.cu:24      default 1.025f */
    float gradient_threshold; /* project_cloud.cu:25      default 0.03f  */
    int32_t levels;           /* project_cloud.cu:23      default 4      */
} rtr_params;

typedef enum { RTR_SCENE_UNIFORM_BOX = 0, RTR_SCENE_ROOM_SHELL = 1 } rtr_scene;

/* ---- 1. life cycle (ProjectCloud ctor/dtor, project_cloud.cu:189-266) ---------- */
int rtr_abi_version(void);
/* device: HIP ordinal of the GPU this context owns. */
int rtr_device_count(void); /* HIP devices visible to this process (0 when there is none or HIP fails) */
int rtr_create(rtr_ctx **out, int device);
int rtr_destroy(rtr_ctx *ctx);
const char *rtr_last_error(const rtr_ctx *ctx); /* ctx may be NULL: error of a failed rtr_create */
void rtr_default_params(rtr_params *p);
int rtr_set_params(rtr_ctx *ctx, const rtr_params *p);
int rtr_get_params(const rtr_ctx *ctx, rtr_params *p);
/* Tuning knobs that never change the frame.
 *  "mode": 1 (default) tile-binned -- the cloud is streamed ONCE, every in-frustum point is
 *          appended as one 8-byte entry to the stream of its screen tile and a per-tile LDS
 *          z-buffer does min + accumulate + resolve (no global atomics on the frame buffers);
 *          0 = the reference's structure: two full passes with atomicMin / atomicAdd
 *          (render.cu:53-130).
 *  "split_threshold" (default 32768; 0 = never), "split_slice" (default 16384): a screen tile
 *          holding more entries than the threshold is processed by several workgroups, each
 *          taking a slice of at least split_slice entries (a distant overview that packs the
 *          whole cloud into a few tiles would otherwise serialise on them).  Whole-frame calls launch the
 *          kernel that does this only while such tiles have been seen (the library learns it from the frames
 *          that have completed, without a sync; eight frames of grace after an upload, a new resolution or a
 *          change of these options): the first frame(s) of a view that suddenly packs the cloud into a few
 *          tiles are therefore rendered unsplit -- exact, slower -- until the report arrives.
 *  "auto_reorder": what follows every later rtr_upload_points / rtr_generate_synthetic.  2 (default): the
 *          cloud is Morton-sorted once (rtr_reorder_points) when its 256-point chunks are not spatially
 *          compact -- mean chunk-box diagonal above twice what an ideally ordered volume cloud of that
 *          size has, (256 / n)^(1/3) of the cloud's diagonal.  Scanner sweeps and Morton-like surfaces
 *          pass; a hash-ordered cloud and the reference loader's 0.25 m blocks (unordered inside) are
 *          sorted, which is worth 13 % ... 2.4 x per frame.  1: always, 0: never.  Best effort
 *          (skipped when the sort's scratch does not fit); clouds under 65536 points are left alone.
 *          Frames never depend on the point order; rtr_download_points returns the RESIDENT order, a
 *          permutation of the uploaded one when rtr_get_option("reordered") reads 1
 *          ("order_ratio_ppm": the measured chunk / cloud diagonal ratio in millionths).
 *  "point_ids": 1 = a cloud the library sorts (option "auto_reorder", rtr_reorder_points) keeps its u32 upload-order
 *          permutation resident (+4 B per point, counted in "resident_millibytes_per_point"), so that rtr_point_pass can
 *          still name points by their upload index.  Read when a cloud is uploaded or sorted; a cloud that is never
 *          sorted needs nothing.  Default 0: nothing about residency or frames changes, and the point pass of a sorted
 *          cloud fails with RTR_ERR_INVALID.
 *  "cull": 1 = skip 256-point chunks whose bounding box is provably outside the frustum
 *          (exact: same frame; an algorithmic byte reduction, off by default and reported
 *          separately from the roofline figure; needs a spatially coherent point order).
 *  "lean": 1 (default) = a whole single-GPU frame (rtr_render and the calls built on it) whose point kernel needs no
 *          epilogue -- no tile above "split_threshold" seen lately, no peer-to-peer exchange open; overlapped or not
 *          -- ends that kernel without last-workgroup detection and bookkeeping pass: the tile kernel's workgroups read
 *          and reset their stream counters themselves, one extra workgroup does the frame's bookkeeping off the
 *          critical path (5-6 us per frame).  0 = always the epilogue.  After a lean frame rtr_accumulate_pass
 *          re-projects the cloud (the bins were consumed).
 *  "lean_identity": 1 (default) = in a lean frame tile workgroup b takes tile b -- no look-up in the launch order
 *          (heaviest tiles first) -- whenever every workgroup of the tile launch is resident at once (1080p: 2041
 *          of 2048 slots), where the order buys nothing and costs a dependent memory round trip.  0 = always the order.
 *  "lean_early": lean frames: the tile workgroups request their first batch of entries BEFORE they know the
 *          streams' lengths (one round trip less; right when most tiles are full) -- 1 always, 0 never (after the
 *          lengths, from indices clamped to them: a near-empty tile then moves no stale memory), -1 (default) = when
 *          the previous frame had at least 1024 entries per tile on average.  Same frame either way.
 *  "lane_test": 1 (default) = the tile-binned point kernel first decodes and projects ONE point per lane (of
 *          the four consecutive points a lane holds) and bounds the other three by the chunk's "lane spread"
 *          (the largest coordinate difference inside a lane, measured once per upload): a 256-point chunk with
 *          no lane near the frustum is neither decoded nor projected in full.  Every point still goes through
 *          the exact arithmetic before it can reach a pixel; 0 = every point of every chunk, as before.
 *  "chunk_test": 1 (default) = with the packed coordinates, the tile-binned point kernel first tests 64
 *          chunks at once on the boxes their headers give (the five frustum half-spaces, with the slack of
 *          option "cull") and streams only the chunks that may reach the frustum; the lane test and the exact
 *          arithmetic then run on those as before.  0 = every chunk through the stream (the loop structure
 *          of round 4, in a kernel instance of its own).  Same
 *          frame either way; no effect on unpacked clouds or with "cull" = 1.  A chunk with an axis the packed
 *          form cannot bound by a common prefix (mixed signs: every chunk on a coordinate plane) is tested on
 *          a box word its header carries for that axis, written when the cloud is packed.  rtr_get_option:
 *          "wide_chunks" (such chunks in the resident packed form) and "wide_chunks_boxed" (those of them that
 *          carry the word: all but chunks holding a NaN or an infinity); both read-only, 0 for an unpacked cloud.
 *  "pack": the tile-binned point kernel reads the coordinates from a LOSSLESS packed form, built once after
 *          every upload / generation / sort (and at once for the resident cloud when the option is set): per
 *          256-point chunk and axis the fp32 bit patterns are a common prefix + the 0..25 (or 32) bits below it
 *          of every value, i.e. 5-9 B/pt instead of 12 for spatially ordered clouds (neighbours share sign,
 *          exponent and leading mantissa bits), in two bit streams per axis -- every lane's first value, and its
 *          other three -- so that the chunks the point kernel rejects on one point per lane are read through a
 *          quarter of their bytes; any bit pattern round-trips (NaNs, -0, mixed signs take 32 bits).  1 (default):
 *          used when it saves at least 1/8 of the stream; 0: never; 2: always, and the packed form is
 *          decoded and compared with the SoA arrays once (an error if a single point differs).  rtr_get_option:
 *          "packed" (1: in use), "packed_millibytes_per_point" (coordinate stream incl. headers, 12000 = raw).
 *          Applied to the resident cloud, a failed allocation of the fp32 arrays a packed-only cloud is decoded into
 *          -> RTR_ERR_HIP, and the cloud keeps its form and the option its previous value; where the packed form
 *          itself does not fit the cloud stays (or becomes) unpacked and the call returns RTR_OK ("packed" 0).
 *  "keep_soa": 0 (default) = a packed cloud is resident in packed form ONLY: the fp32 SoA arrays (12 B per point) are
 *          freed once the cloud has been packed and decoded again -- bit for bit -- by the calls that read fp32
 *          coordinates (mode 0 and the phase calls with another matrix, rtr_reorder_points, rtr_download_points,
 *          option "pack" = 0); 1 = they stay resident beside the packed form.
 *  "pool_worst_case": 0 (default) = the pool of dynamic stream extents is sized by the frames the cloud has had (8 x the
 *          most in-frustum entries a completed frame reported, at least n / 2: 4 B per point instead of 16).  A frame
 *          whose entries jump past that overflows it; the next synchronising call (every call that copies results to the
 *          host, rtr_synchronize, rtr_download_buffer, rtr_wait) then sizes the pool for the worst case and renders that
 *          frame again before it returns -- rtr_wait every slot whose frame was queued before the pool grew, into its
 *          own buffers.  Transparent, except for whoever consumes frames on the stream without ever synchronising.
 *          The phase calls are consumed that way (a sharded frame is reduced first): a binned rtr_min_depth_pass
 *          sizes the pool for the worst case for the rest of the cloud's life.  computeFull synchronises before its
 *          model runs.  1 = sized for the worst case (2 n entries) from the start.
 *          rtr_get_option("resident_millibytes_per_point"): device memory held for the cloud and its frames, per point.
 *  "keep_accum": 1 = the whole-frame calls also write RTR_BUF_ACCUM (default 0; the phase
 *          calls always do).
 *  "overlap": rtr_render queues the point kernel (T1) of a frame on a second, internal stream and into a second tile
 *          store and extent pool, so it runs beside the tile kernel and prefilter of the previous frame; results are
 *          still ordered on the context's stream, and every frame is bit-identical to the serial one.  1 = every
 *          whole frame; 0 = never; -1 (default) = automatic: from the third consecutive rtr_render of the context on
 *          -- with the prefilter, same resolution and cloud, tile-binned form, one GPU, no peer-to-peer exchange
 *          exported or open -- and until any other entry point is called (all but rtr_get_option and the other read-only queries end the
 *          streak; the next one counts from one again).  Footprint while in use: the second tile store, 134 MB at
 *          1920x1080, and the second extent pool, 4 B per point with the adaptive pool (0.4 GB for 1e8 points).  Both
 *          are first allocated by the frame that engages; if that fails in the automatic mode the context stays
 *          serial, without an error.  They are kept until the resolution changes (the store), the cloud is replaced
 *          (the pool), the context closes -- or the option is set to 0, which gives both back.
 *          Frames without the prefilter stay serial in the automatic mode: their tail is the tile kernel alone, and
 *          overlapped they are 1-9 % slower ("Overlap"); 1 overlaps them all the same.
 *          rtr_get_option("overlap_active") reads 1 when the last whole frame ran overlapped.
 *          "front_priority": the stream priority the internal stream is created with -- 0 (default) the default
 *          priority, 1 the lowest the device offers (the context's stream, i.e. the tail and what the caller queues
 *          behind a frame, then wins dispatch), 2 the highest.  Read when the stream is created: set it before
 *          "overlap".  Measured on MI355X ("Overlap"): 0 is fastest.
 *          "tail_cus" = t (0..31, set before "overlap" = 1, which alone uses it) gives the two streams disjoint CU
 *          masks instead, t CUs of every XCD for the tail.
 *  "point_grid": workgroups of the grid-stride point kernels (default 1024 = 4 per CU; at the default the
 *          tile-binned point kernel takes what is resident at once: 5 per CU when it reads packed coordinates
 *          and its registers admit it, else 4).
 *  "phases": the point kernel's workgroups are cut into this many groups that start at different
 *          places of the cloud (default 0 = automatic: 1, which keeps one dense streaming front, unless the
 *          previous frame had more than a quarter of the cloud inside the frustum, then 16 -- the claims of
 *          a distant overview spread over more stream counters); "fill_shift": the per-tile stream counters
 *          lie 4 << value bytes apart (0..6; packed counters share memory channels and queue up: a distant
 *          overview with every point in a dozen tiles takes 3.0 ms in the point kernel at 2, 1.5 ms at 4, for +1 %
 *          on an ordinary view).  Default -1 = automatic: 1 (8 bytes) on ordinary frames, 4 (64 bytes) while frames
 *          with tiles above "split_threshold" have been seen lately (and in the phase / sharded calls).
 *  "p2p_timeout_ms": how long a flag barrier of the peer-to-peer exchange (section 5b) waits for a rank
 *          that does not arrive before it flags the frame in rtr_p2p_status (default 2000).  rtr_get_option("p2p_open")
 *          reads 1 while the peers' buffers are mapped: a new cloud (rtr_upload_points, rtr_generate_synthetic with
 *          another point count) or resolution closes the exchange on this rank -- every rank must then export /
 *          open again, together.  The exchange and option "overlap" = 1 exclude each other (-1 is inactive meanwhile).
 *  "debug_dyn_cap": test aid -- caps the pool of dynamic stream extents at this many entries (-1 = off), so that a
 *          heavy tile overflows it and the error path (RTR_ERR_INTERNAL) can be exercised.
 *  "debug_extract_window": test aid -- caps the points per internal window of rtr_extract_points (section 2e; -1 = off).
 *  "debug_store_stamp": test aid, frames never depend on it -- sets the 24-bit frame stamp (0 .. 0xFFFFFF) of every tile
 *          store the context holds (both sets of the single frame, every view's store) and of the stores it creates
 *          later, so that the stamp's wrap -- reached after 2^24 frames into one store -- can be had within a few frames.
 *          Forward only: a value below the stamp of a store is RTR_ERR_INVALID and changes nothing.  Host state only:
 *          nothing is launched or written to the device.  rtr_get_option reads the stamp of the single frame's current
 *          store: that of its last frame, never 0 once it has rendered one.
 *  "debug_p2p_barrier": test aid, frames never depend on it -- the barrier number the peer-to-peer exchange starts at,
 *          as the 32 bits of the value (-1 = off: it starts at 0), so that the wrap of the barrier counter -- reached after
 *          2^32 barriers -- can be had within a few frames.  Read once per exchange, by the rtr_p2p_export that allocates
 *          this rank's flag words (the first for a resolution and cloud, or after rtr_p2p_close): the words start
 *          there, and rtr_p2p_open starts the counter at the same number; a value set later waits for the next such
 *          export.  Set it before rtr_p2p_export, to the same value on every rank.
 *          rtr_get_option reads, while the exchange is open, the 32 bits of the number of the last barrier queued
 *          (otherwise the value set), so that a test can see the counter pass 0.
 *  "debug_alloc_fail": test aid -- N >= 1: the N-th device or pinned-host allocation the library attempts from now on
 *          fails, once, as if the device had run out of memory, and the switch disarms itself; 0 disarms it.  The
 *          library does not ask HIP for that allocation at all: nothing absurd is requested, nothing is launched, HIP's
 *          last error stays clean.  Every allocation of the library goes through the switch.  rtr_get_option reads the
 *          attempts still to go, 0 once it has fired or is off (so a test can tell that it fired from a call
 *          that made fewer than N allocations).  Process-wide, not per context, like the two counters below; setting it
 *          does not end a streak of option "overlap".  What each call leaves behind after a failed allocation is stated
 *          with the call.
 *  "debug_alloc_count" (rtr_get_option only): the allocation attempts of the process so far, failed ones included.
 *  "debug_alloc_live" (rtr_get_option only): the allocations of the process made through the library and not yet freed,
 *          over all its contexts (both saturate at 2^31 - 1).
 *  "xp": only in RTR_EXPERIMENT builds (make experiment): switches parts of the point kernel off for
 *          timing attribution -- frames are WRONG while it is non-zero; the shipped library rejects it.
 *  "probe_variant": measurement aid of tools/probe_variants.py (selects the rtr_stream_probe kernel).
 *  rtr_get_option("views") reads the view count of the last rtr_render_views batch (section 6c; 0: none current).
 *  rtr_get_option("point_keep") reads 1 while a keep mask is set (section 6e).
 *  rtr_get_option("selection") reads 1 while a selection exists (section 6f).
 *  rtr_get_option("voxel_keys_us" / "voxel_sort_us" / "voxel_heads_us") read the device time, in microseconds, that the last
 *          rtr_select_voxel_grid (section 6g) spent in its key kernel, its sort and its head kernel (0 before the first).
 *  rtr_get_option("neighbours_keys_us" / "neighbours_sort_us" / "neighbours_count_us") read the same for the last
 *          rtr_select_neighbours (section 6h): its key kernel, its sort (with the wait for the key kernel's counters), and
 *          its gather, work-list and count kernels together; "neighbours_pair_tests_k" reads the pair tests that call
 *          made, in thousands (saturating at 2^31 - 1).
 *  rtr_get_option("clusters_keys_us" / "clusters_sort_us" / "clusters_label_us") read the same for the last
 *          rtr_select_clusters (section 6i): its key kernel, its sort (with the wait for the key kernel's counters), and
 *          its gather, work-list, union-find, flatten and hit kernels together; "clusters_pair_tests_k" reads that call's
 *          pair tests, in thousands (saturating at 2^31 - 1).
 *  rtr_get_option("near_given_us" / "near_sweep_us") read the device time, in microseconds, that the last rtr_select_near
 *          (section 6k) spent on the given points (their copy, key kernel, sort and gather) and on the resident sweep with
 *          the combine and the counts; "near_pair_tests_k" reads that call's pair tests, in thousands, and
 *          "near_chunks_skipped" / "near_chunks_decoded" its resident chunks decided without reading their coordinates /
 *          decoded (all three saturating at 2^31 - 1).
 *  rtr_get_option("nearest_given_us" / "nearest_sweep_us" / "nearest_pair_tests_k" / "nearest_chunks_skipped" /
 *          "nearest_chunks_decoded") read the same five for the last rtr_nearest_points (section 6l): the sweep's time
 *          includes the unpacking of the given side.
 *  rtr_get_option("nearest_k_given_us" / "nearest_k_sweep_us" / "nearest_k_pair_tests_k" / "nearest_k_chunks_skipped" /
 *          "nearest_k_chunks_decoded") read the same five for the last rtr_nearest_k_points (section 6m), and
 *          "nearest_k_cascades_k" the row insertions its sweep started, in thousands (saturating at 2^31 - 1): that one
 *          depends on the timing of the waves and differs from run to run.
 *  rtr_get_option("plane_sample_us" / "plane_count_us") read the host time, in microseconds and with its waits, that the
 *          last rtr_fit_plane (section 6j) spent drawing and extracting its sample and counting its candidates. */
int rtr_set_option(rtr_ctx *ctx, const char *key, int value);
/* Reads an option back; also "p2p_open" (see "p2p_timeout_ms"), "reordered" (1: the resident cloud was sorted by the library),
 * "order_ratio_ppm" (mean chunk-box diagonal / cloud diagonal as uploaded, in millionths), "packed" and
 * "packed_millibytes_per_point" (see "pack"). */
int rtr_get_option(rtr_ctx *ctx, const char *key, int *value);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream) instead of the context's
 * own non-blocking stream; NULL means HIP's default stream.  rtr_reset_stream returns to the
 * private stream. */
int rtr_set_stream(rtr_ctx *ctx, void *hip_stream);
int rtr_reset_stream(rtr_ctx *ctx);
int rtr_synchronize(rtr_ctx *ctx);

/* ---- 2. the resident cloud (project_cloud.cu:191-206) --------------------------- */
/* Copies n points from HOST memory and stores them as SoA x[] y[] z[] + packed
 * colour.  xyz_stride_bytes = 16 for the reference's float4 (x,y,z,1) layout
 * (Octreegrid.h:162-170), 12 for tight xyz.  rgb_stride_bytes = 4 for uchar4
 * (c0,c1,c2,255) (Octreegrid.h:172-180), 3 for tight triples; channel order is
 * preserved end to end (B,G,R in the reference).  Replaces any previous cloud.
 * A failed allocation -> RTR_ERR_HIP, and the context holds either the previous cloud, untouched, with its keep mask
 * and selection (only when the call fails before anything of that cloud has gone), or no points at all, as after an
 * upload of 0 points: rtr_num_points reads 0, no keep mask, no selection, "packed" and "reordered" read 0; clip planes,
 * options and resolution stay.  Never part of one cloud and part of the other: the previous cloud's arrays are given
 * back or overwritten first (two clouds may not fit), so the new one cannot be had all-or-nothing beside it.
 * The sort of option "auto_reorder" and the packing of option "pack" behind the upload are best effort: where their
 * scratch does not fit the call returns RTR_OK with the cloud unsorted ("reordered" 0) / unpacked ("packed" 0). */
int rtr_upload_points(rtr_ctx *ctx, const float *xyz, size_t xyz_stride_bytes, const uint8_t *rgb,
                      size_t rgb_stride_bytes, size_t n);
/* Synthesises points [first, first+count) of a `total`-point scene directly in
 * HBM (counter-based generator; bit-identical to the oracle's).  A failed allocation: as for
 * rtr_upload_points -- RTR_ERR_HIP, and the previous cloud untouched or no points at all. */
int rtr_generate_synthetic(rtr_ctx *ctx, int scene, uint64_t seed, uint64_t first, uint64_t count,
                           uint64_t total);
/* One-off Morton (Z-order) sort of the resident cloud: consecutive points become spatial
 * neighbours, like the reference loader's 0.25 m block order (cloudreader.cpp:8-82).  Never
 * changes a frame (min and integer sums commute); it changes rtr_download_points' order and
 * makes the per-tile appends long runs and option "cull" effective.
 * A failed allocation up to and including the sort -> RTR_ERR_HIP and the cloud is as it was (order, "reordered", the
 * permutation of "point_ids", the packed form): the sort writes nothing back before it holds all its scratch.  Behind
 * the sort the packing is best effort, as after an upload: RTR_OK with "packed" 0. */
int rtr_reorder_points(rtr_ctx *ctx);
int rtr_num_points(const rtr_ctx *ctx, uint64_t *n);
/* Copies the resident cloud back as float4 / uchar4 AoS (tests, debugging), in the RESIDENT order (see
 * option "auto_reorder").  A cloud resident in packed form only is decoded for the copy; a failed allocation ->
 * RTR_ERR_HIP, the cloud stays as it was (in packed form only) and the outputs hold nothing defined. */
int rtr_download_points(rtr_ctx *ctx, float *xyzw, uint8_t *rgba, uint64_t first, uint64_t count);

/* ---- 2b. appending points to the resident cloud ------------------------------------------------------------------
 * Adds m points from HOST memory behind the resident cloud without uploading it again (one scan of a survey, one
 * piece of a growing capture per call).  Arguments, strides and channel order are those of rtr_upload_points.
 *
 * Indices: the m points get upload indices n .. n + m - 1, n the count before the call -- the indices of the point
 * pass (RTR_BUF_POINT_ID, RTR_BUF_VISIBLE) and of the keep mask.  Points of rtr_generate_synthetic keep their
 * i - first indices.  m = 0 returns RTR_OK and changes nothing; on a context without points the call is
 * rtr_upload_points.
 *
 * Equivalence: a cloud built by rtr_upload_points(A), then rtr_append_points(B1) .. rtr_append_points(Bk) renders bit
 * for bit what one rtr_upload_points(A ++ B1 ++ .. ++ Bk) renders with the same options, params, clip planes and
 * resolution: the host outputs of rtr_project(_filtered) / rtr_project_async, RTR_BUF_DEPTH, _ACCUM, _IMAGE, _TENSOR,
 * _MASK, _MINMAX, RTR_BUF_POINT_ID and _VISIBLE (whenever the point pass is allowed on both clouds), RTR_BUF_VIEW_*, the
 * phase calls and rtr_frame_stats words [2] and [3].  What depends on the resident order may differ:
 * rtr_download_points' order, the option read-backs "reordered", "order_ratio_ppm", "packed_millibytes_per_point",
 * "resident_millibytes_per_point", and the chunk-counting words of rtr_frame_stats.
 *
 * Resident order: points already resident never move; the block goes behind them (its first points may complete the
 * cloud's last partial 256-point chunk).  Option "auto_reorder" applies to the BLOCK by itself: 0 appends it as given,
 * 1 Morton-sorts it on its own, 2 (default) sorts it when m >= 65536 and its own chunk measure (mean chunk diagonal
 * over block diagonal) is above 2 (256 / m)^(1/3).  A block sort makes "reordered" read 1, so the point pass then
 * needs option "point_ids" = 1, which extends the resident permutation.  The block is NOT sorted when that would lose
 * the upload order a keep mask in force needs (cloud in upload order, "point_ids" = 0, mask set: the rule of
 * rtr_reorder_points); this costs speed only.
 *
 * Form: a packed cloud stays packed (the new chunks are packed losslessly, and verified with "pack" = 2), an unpacked
 * one stays unpacked; "keep_soa" is honoured.  A keep mask in force is extended and the new points are KEPT:
 * RTR_BUF_POINT_KEEP and the nwords of rtr_set_point_keep grow to (n + m + 31) / 32.
 *
 * Ordering: like rtr_set_point_keep, the call first completes every frame, pass, view batch and async slot issued
 * before it (rtr_synchronize); frames that overflowed the adaptive extent pool are rendered again with the cloud they
 * were issued with -- if that fails, the call returns the error and the cloud is unchanged.
 *
 * Side effects, as after an upload: an open peer-to-peer exchange is closed ("p2p_open" reads 0; every rank exports
 * and opens again), the adaptive extent pools are sized for the new n by the next frame, RTR_BUF_VISIBLE by the next
 * point pass.
 *
 * Errors (RTR_ERR_INVALID, nothing changes): the argument checks of rtr_upload_points, n + m >= 2^32.  A failed
 * allocation leaves the cloud as it was too: every new buffer is allocated before anything is committed.
 *
 * Cost: kernel work proportional to m, plus O(n / 256) passes over per-chunk arrays and, when the resident arrays'
 * capacity (1/8 head-room) is exceeded, one device-to-device copy of them. */
int rtr_append_points(rtr_ctx *ctx, const float *xyz, size_t xyz_stride_bytes, const uint8_t *rgb,
                      size_t rgb_stride_bytes, size_t m);

/* ---- 2c. removing points from the resident cloud ------------------------------------------------------------------
 * Takes points out of the resident cloud and gives their memory back (a bad scan, outliers, passers-by; the last append
 * again).  keep_words: (n + 31) / 32 words in UPLOAD order, bit i % 32 of word i / 32 set = point i stays -- the layout
 * of rtr_set_point_keep and RTR_BUF_VISIBLE, so RTR_BUF_POINT_KEEP or a point pass's visibility can be passed as they
 * are.  Host memory or device memory of the context's device; the words are copied, the caller may reuse them when the
 * call returns.  Bits past n are ignored.
 *
 * Indices: the survivors keep their relative upload order and are renumbered 0 .. n' - 1: survivor i gets the number
 * of kept points with an upload index below i.  This applies to the point pass (RTR_BUF_POINT_ID, _VISIBLE), to the
 * keep mask and to later appends, which continue at n'.
 *
 * Equivalence: rtr_upload_points(A), then rtr_remove_points(keep), renders bit for bit what one
 * rtr_upload_points(A[keep]) renders with the same options, params, clip planes and resolution -- the outputs section 2b
 * lists, with what depends on the resident order excepted as there; and so across any sequence of uploads, appends and
 * removals.
 *
 * Resident order: a stable compaction; points never change their relative order (a sorted cloud stays sorted and is
 * not sorted again).  The 256-point chunks before the first one that loses a point are untouched; the ones from there
 * on are rebuilt.  A packed cloud stays packed ("pack" = 2 verifies the rebuilt chunks), an unpacked one unpacked;
 * "keep_soa" is honoured.  The permutation of "point_ids" is compacted and renumbered.  A keep mask in force is
 * compacted onto the survivors: RTR_BUF_POINT_KEEP then reads old[keep] and the nwords of rtr_set_point_keep shrink.
 * Device arrays holding more than 1/8 head-room over the survivors are reallocated to that size.
 *
 * Ordering and side effects as for rtr_append_points: the call first completes everything issued before it (async slots
 * come out with the old cloud); then an open peer-to-peer exchange is closed, the adaptive extent pools are sized again
 * by the next frame and RTR_BUF_VISIBLE by the next point pass.  A mask that keeps every point changes nothing (the
 * exchange stays open) except that the selection of section 6f is dropped, as by every removal; one that keeps none
 * leaves the context of an upload of 0 points, without a keep mask.
 *
 * Errors (RTR_ERR_INVALID, nothing changes): no cloud, nwords != (n + 31) / 32, keep_words NULL, a cloud the library
 * sorted without option "point_ids" = 1 (upload indices cannot be mapped).  A failed allocation leaves the cloud as it
 * was too: every new buffer is allocated before anything is committed.
 *
 * Cost: a pass over the keep bits of every resident point (through the permutation when sorted), kernel work
 * proportional to the points from the first chunk that loses one, and O(n / 256) passes over per-chunk arrays; removing
 * a tail costs about what appending it did. */
int rtr_remove_points(rtr_ctx *ctx, const uint32_t *keep_words, uint64_t nwords);

/* ---- 2d. moving points of the resident cloud ----------------------------------------------------------------------
 * Moves resident points by an affine transform where they lie, without uploading the cloud again (a loop closure that
 * corrects the poses of scans already resident, one re-registered scan, a georeferenced cloud).  M: row-major 3 x 4,
 * fp32; a selected point (x, y, z) becomes
 *     x' = ((M[0] x + M[1] y) + M[2] z) + M[3],  y' = ((M[4] x + M[5] y) + M[6] z) + M[7],
 *     z' = ((M[8] x + M[9] y) + M[10] z) + M[11],
 * every product and every sum rounded to fp32 on its own (no FMA; the clip planes' contract, section 6d).  There is no
 * shortcut for special matrices: [I|0] maps -0 to +0, and a point with an infinite coordinate gets NaN in its other
 * coordinates (0 x inf) -- what the formula gives.  Which NaN such an operation gives (sign, payload) is the device's, not part of
 * the contract: section 2e returns the bits that are resident, so a NaN made here need not equal a host's bit for bit.
 *
 * select_words: (n + 31) / 32 words in UPLOAD order, bit i % 32 of word i / 32 set = point i moves -- the layout of
 * rtr_remove_points, rtr_set_point_keep and RTR_BUF_VISIBLE.  Host memory or device memory of the context's device; the
 * words are copied.  Bits past n are ignored.  select_words = NULL with nwords = 0 moves every point, on any cloud; a
 * selection on a cloud the library sorted needs option "point_ids" = 1.  A selection without a set bit returns RTR_OK
 * and changes nothing.
 *
 * Equivalence: rtr_upload_points(A), then rtr_transform_points(M, sel), renders bit for bit what one
 * rtr_upload_points(A') renders, A'[i] = M applied to A[i] for the selected i and A[i] for the others, with the same
 * options, params, clip planes and resolution -- the outputs section 2b lists, with what depends on the resident order
 * excepted as there; and so across any sequence of uploads, appends, removals and moves.  rtr_download_points returns A'
 * in the resident order.  Clip planes are world-space: they act on the new coordinates.
 *
 * What stays: upload indices, the resident order (no sort: option "auto_reorder" is not applied; rtr_reorder_points
 * sorts on request), colours, the permutation of "point_ids", the keep mask in force (RTR_BUF_POINT_KEEP reads the same
 * words).  A packed cloud stays packed (even when packing no longer saves 1/8; "pack" = 2 verifies the rebuilt chunks),
 * an unpacked one unpacked; "keep_soa" is honoured.  An open peer-to-peer exchange stays open: nothing the peers map is
 * reallocated; each rank moves its own points by its own upload indices.  Only the 256-point chunks from the first to
 * the last one holding a selected point are rebuilt; the packed blocks behind them move without being decoded.
 *
 * Ordering: like rtr_append_points, the call first completes everything issued before it (async slots come out with the
 * old cloud); frames that overflowed the adaptive extent pool are rendered again with the old cloud -- if that fails,
 * the call returns the error and the cloud is unchanged.  Bins of an earlier rtr_min_depth_pass are not reused.
 *
 * Errors (RTR_ERR_INVALID, nothing changes): no cloud, M NULL or a non-finite coefficient, nwords != (n + 31) / 32 with a
 * selection, select_words NULL with nwords > 0, a selection on a sorted cloud without "point_ids" = 1.  A failed
 * allocation leaves the cloud as it was too: every new buffer is allocated before anything is committed.
 *
 * Cost: with a selection, a pass over its bits (through the permutation when sorted); kernel work proportional to the
 * points of the chunks rebuilt; a device-to-device move of the packed blocks behind them when their size changes; and
 * O(n / 256) passes over per-chunk arrays. */
int rtr_transform_points(rtr_ctx *ctx, const float M[12], const uint32_t *select_words, uint64_t nwords);

/* ---- 2e. reading points back out of the resident cloud ------------------------------------------------------------
 * Gives resident points back in UPLOAD order, all of them or a selection, without decoding the rest of the cloud (save
 * an edited session, hand a selected region to another tool, context or rank).  The read side of sections 2b-2d and 6f.
 *
 * Selection: select_words is (n + 31) / 32 words in UPLOAD order, bit i % 32 of word i / 32 set = point i is extracted
 * -- the layout of rtr_remove_points, rtr_set_point_keep, RTR_BUF_VISIBLE and RTR_BUF_SELECTION.  Host memory or device
 * memory of the context's device (the pointer of rtr_device_buffer(RTR_BUF_SELECTION) or RTR_BUF_POINT_KEEP can be passed
 * as it is); the words are copied.  Bits past n are ignored.  select_words = NULL with nwords = 0 means every point, on
 * any cloud; a selection on a cloud the library sorted needs option "point_ids" = 1, as everywhere else.
 *
 * Order: let the selected upload indices in ascending order be s_0 < s_1 < ... < s_{k-1}.  *total (when non-NULL)
 * receives k.  The call writes the points of ranks r in [first, min(first + count, k)) to output slot r - first.  With
 * first >= k or count = 0 it writes nothing and returns RTR_OK: a caller sizes its buffers with one call with count = 0
 * and may then extract in pieces.
 *
 * Sorted clouds without a selection: every point of a cloud the library sorted with "point_ids" = 0 cannot be put into
 * upload order.  In that one case the order is the RESIDENT one (rtr_download_points') and indices must be NULL
 * (RTR_ERR_INVALID otherwise; the message names point_ids).  With "point_ids" = 1 the order is the upload order.
 *
 * Outputs: each of xyz, rgb and indices may be NULL (that stream is skipped), and each may be host memory or device
 * memory of the context's device, independently of the others.  Slot j of xyz is the three floats at byte offset
 * j * xyz_stride_bytes (the rules of rtr_upload_points: at least 12, a multiple of 4), slot j of rgb three bytes at
 * j * rgb_stride_bytes (at least 3), in the channel order as uploaded.  At strides of exactly 16 and 4 the fourth float
 * is written as 1.0f and the fourth byte as 255 -- the reference's float4 / uchar4 layouts, what rtr_download_points
 * gives; at any other stride the bytes beyond the first 12 or 3 of a record are left untouched.  indices[j] is
 * s_{first + j}.  Coordinates are bit for bit the resident ones: any bit pattern round-trips (NaN payloads, -0,
 * denormals); after rtr_transform_points they are the moved coordinates.  The output can be fed unchanged to
 * rtr_upload_points or rtr_append_points, of this context or another.
 *
 * What it ignores and leaves alone: like rtr_download_points and rtr_select_points the call reads the cloud only.  The
 * context's clip planes and keep mask are ignored (hidden points are extracted too); no frame, frame buffer, tile store,
 * pool, statistic, point-pass buffer, selection or keep mask changes, and an open peer-to-peer exchange stays open.  A
 * cloud resident in packed form only is NOT decoded into fp32 arrays: the chunks holding a requested point are decoded
 * on the fly.  Scratch: one internal window of outputs (at most 2^24 points, for host destinations) plus O(n / 32)
 * words.  Option "debug_extract_window" (test aid, -1 = off) caps the points per internal window so that small clouds
 * reach the multi-window path.
 *
 * Ordering: the work is queued on the context's stream behind everything issued before it, and the call waits for it
 * before it returns, as rtr_download_points does.  It does not repeat overflowed frames; a pending frame error stays
 * pending for the next synchronising call.
 *
 * Cost: one pass over the selection words (none without a selection); then kernel work proportional to the 256-point
 * chunks that hold a selected point of the requested window -- a chunk with none is skipped before its header or
 * streams are read.  On a sorted cloud the selection bits are gathered through the permutation, for every chunk and
 * internal window.
 *
 * Sharded use: each rank extracts its own points by its own indices.
 *
 * Errors (RTR_ERR_INVALID, nothing is written): no cloud; nwords != (n + 31) / 32 with a selection; select_words NULL
 * with nwords > 0; a bad stride for a non-NULL stream; a selection on a sorted cloud without "point_ids" = 1; indices on
 * a sorted cloud without "point_ids" = 1; xyz, rgb, indices and total all NULL.  2^32 points or more:
 * RTR_ERR_UNSUPPORTED.  A failed allocation -> RTR_ERR_HIP: the call only reads, so the cloud and the context are as
 * they were; what the outputs and *total hold is not defined. */
int rtr_extract_points(rtr_ctx *ctx, const uint32_t *select_words, uint64_t nwords,
                       uint64_t first, uint64_t count,
                       float *xyz, size_t xyz_stride_bytes,
                       uint8_t *rgb, size_t rgb_stride_bytes,
                       uint32_t *indices, uint64_t *total);

/* ---- 2f. writing points back into the resident cloud ---------------------------------------------------------------
 * Gives resident points new coordinates and / or colours, point by point, where they lie: the mirror image of section
 * 2e (a selection extracted, recoloured by class or intensity and put back; a highlight; a non-rigid loop-closure or
 * bundle-adjustment correction; de-noised ranges).  Upload indices do not change, so the selection, the keep mask and
 * a block sort survive, which uploading the cloud again or removing and appending the points would lose.
 *
 * Selection and ranks: exactly section 2e's.  select_words is (n + 31) / 32 words in UPLOAD order, host memory or
 * device memory of the context's device (the pointer of rtr_device_buffer(RTR_BUF_SELECTION) can be passed as it is);
 * the words are copied, bits past n are ignored, NULL with nwords = 0 means every point.  Let the selected upload
 * indices be s_0 < s_1 < ... < s_{k-1}; *total (when non-NULL) receives k.  Record j of the caller's arrays is written
 * into point s_{first + j}, for j in [0, min(count, k - first)); no record beyond that is read.  first >= k or count = 0
 * changes nothing and returns RTR_OK, so a sizing call is possible, and a caller may write in pieces.  A selection on a
 * cloud the library sorted needs option "point_ids" = 1, as everywhere else; on a cloud sorted without it "every point"
 * addresses the RESIDENT order, as section 2e reads it, so extract-all, edit, write-all round-trips on any cloud.
 *
 * Streams: each of xyz and rgb may be NULL -- that stream stays as it is resident; both NULL is an error -- and each may
 * be host memory or device memory of the context's device, independently of the other.  Strides follow
 * rtr_upload_points (xyz at least 12 and a multiple of 4, rgb at least 3); only the first 12 bytes of an xyz record and
 * the first 3 bytes of an rgb record are read.  The resident colour becomes c0 | c1 << 8 | c2 << 16 | 0xFF000000, as an
 * upload builds it.  rgb_stride_bytes = 0 is the one extension: every written point takes record 0 (one colour for the
 * whole selection).  xyz_stride_bytes = 0 is an error.
 *
 * Values: coordinates are stored bit for bit -- NaN payloads, -0, infinities and denormals round-trip through
 * rtr_extract_points.  Unlike section 2d there is no device arithmetic, hence no "which NaN" caveat.
 *
 * Equivalence: rtr_upload_points(A), then rtr_write_points(sel, first, count, X, C), renders bit for bit what one
 * rtr_upload_points(A') renders with the same options, params, clip planes and resolution, A' = A except that the points
 * s_{first + j} take X[j] and / or C[j] -- the outputs section 2b lists, with what depends on the resident order excepted
 * as there; and so across any sequence of uploads, appends, removals, moves and writes.
 *
 * What stays: section 2d's list -- the point count, upload indices and the resident order (no sort), the permutation,
 * the keep mask in force, the SELECTION (indices do not change), an open peer-to-peer exchange (nothing the peers map is
 * reallocated).  A packed cloud stays packed ("pack" = 2 verifies the rebuilt chunks), an unpacked one unpacked;
 * "keep_soa" is honoured.  A colour-only write touches no chunk box, header or packed block.
 *
 * Ordering: section 2d's.  The call first completes everything issued before it: frames, passes, view batches and
 * async slots come out with the old cloud; a frame that overflowed the adaptive extent pool is rendered again with the
 * old cloud -- if that fails, the call returns the error and changes nothing.  It ends an overlap streak.
 *
 * Errors (RTR_ERR_INVALID, nothing changes): no cloud; xyz and rgb both NULL; a bad stride for a non-NULL stream;
 * nwords != (n + 31) / 32 with a selection; select_words NULL with nwords > 0; a selection on a sorted cloud without
 * "point_ids" = 1.  2^32 points or more: RTR_ERR_UNSUPPORTED.  A failed allocation leaves the cloud as it was: every
 * buffer, the device copy of host records included, is allocated before the first resident byte changes -- colours too,
 * which are written with the commit and never before the rebuilt chunks have been measured.
 *
 * Scratch and cost: three arrays of (n + 31) / 32 words (the selection, its scan, the window's bits; also for "every
 * point", 12.5 MB at 1e8 points); host records are copied to the device once, at the caller's stride --
 * min(count, k - first) x stride bytes; device records are read where they lie.  A caller who wants bounded scratch
 * writes in pieces through first / count; each piece is a commit of its own.  Kernel work is proportional to the chunks
 * from the first to the last one that holds a written point (fp32 scratch for those chunks when the cloud is packed);
 * for a packed cloud whose rebuilt chunks change size, add the device-to-device move of the blocks behind them, as in
 * section 2d; and O(n / 256) passes over per-chunk arrays. */
int rtr_write_points(rtr_ctx *ctx, const uint32_t *select_words, uint64_t nwords,
                     uint64_t first, uint64_t count,
                     const float *xyz, size_t xyz_stride_bytes,
                     const uint8_t *rgb, size_t rgb_stride_bytes,
                     uint64_t *total);

/* ---- 3. camera (project_cloud.cu:318, project_cloud.h:50-59) -------------------- */
/* P = K4 * E in fp32, row-major, exactly as the reference composes it with glm:
 * K row-major 3x3 intrinsics, E row-major 4x4 world->camera, both double. */
int rtr_compose_projection(const double K[9], const double E[16], float P[16]);
/* (Re)allocates the frame buffers; cheap no-op when unchanged (project_cloud.cu:275-298).  The buffers of the previous
 * resolution are given back first (and an exported peer-to-peer exchange with them), so a failed allocation ->
 * RTR_ERR_HIP leaves the context with NO resolution, as rtr_create left it: the calls that need one return
 * RTR_ERR_INVALID until rtr_set_resolution succeeds.  The cloud, its mask, selection and clip planes are untouched. */
int rtr_set_resolution(rtr_ctx *ctx, int width, int height);

/* ---- 4. whole-frame calls (the reference's public methods) ---------------------- */
/* computeRGBD (project_cloud.cu:268-312): clear, min-depth pass, accumulate pass,
 * resolve.  host_img: W*H*3 u8 or NULL; host_depth: W*H float or NULL (empty
 * pixel = FLT_MAX).  Both NULL -> RTR_ERR_NO_OUTPUT like the reference's -1;
 * use rtr_render() for device-resident output.  A failed allocation: see rtr_render. */
int rtr_project(rtr_ctx *ctx, const float P[16], uint8_t *host_img, float *host_depth);
/* computeFilteredRGBD (project_cloud.cu:394-434): rtr_project + depth-heuristic
 * prefilter; masked pixels read depth -1 and colour 0; also fills the fp16
 * {1,5,H,W} device tensor consumed by the U-Net (project_cloud.cu:471).  A failed allocation: see rtr_render. */
int rtr_project_filtered(rtr_ctx *ctx, const float P[16], uint8_t *host_img, float *host_depth);
/* Same frame sequences without any host copy or host sync (outputs stay in HBM).
 * P may be any finite 3x4 (row 3 is never read) -- off-axis, rolled, skewed, mirrored, left-handed, rescaled,
 * composed for a cloud far from the origin: the frame is the oracle's for it, bit for bit; what the library
 * rejects early (chunk boxes, lanes, quads) is speed only and never changes a pixel.  Tested for row magnitudes
 * from 2^-104 to 2^40 times a pixel camera's and coordinates up to 2.4e6; not for r.z above 2^126 (the exact
 * test's reciprocal is subnormal there) nor for rows x coordinates below ~4e-40 (tests/README_cameras.md).
 * The three calls of this section make what they need on first use and keep it: a tile store per resolution, an extent
 * pool per cloud (both again for the second set of option "overlap"), the prefilter's pyramid levels.  A failed
 * allocation of one of them -> RTR_ERR_HIP: the frame buffers hold nothing defined, the cloud, mask, selection, clip
 * planes and resolution are untouched, a resource is either complete or absent, and the same call made again starts
 * from there and renders the exact frame.  A frame that a synchronising call (rtr_synchronize, rtr_wait,
 * rtr_download_buffer, the host copies of rtr_project) renders again after an overflow of the adaptive pool allocates
 * the larger pool: if that fails the synchronising call returns RTR_ERR_HIP and the frame must be rendered again. */
int rtr_render(rtr_ctx *ctx, const float P[16], int with_filter);

/* ---- 4b. the same frames with the host copies off the critical path ---------------
 * The reference's call shape runs the kernels and then the two device-to-host copies (W*H*4 + W*H*3 bytes:
 * 14.5 MB at 1080p, ~0.29 ms over PCIe) one after the other, every frame (project_cloud.cu:302-309,424-431).
 * rtr_project_async renders a frame like rtr_project / rtr_project_filtered, snapshots depth and image on the
 * device and queues their copies into the library's PINNED host buffers of `slot` on a second stream; it does
 * not wait.  With the slots used in rotation, frame k's copies run beside frame k + 1's kernels.
 * rtr_wait(slot) blocks until that slot's outputs are complete (slot = -1: all of them) and reports errors of
 * the frames since the last synchronising call.  When the adaptive extent pool overflowed in one of them
 * (option "pool_worst_case"), every slot still queued is rendered again with the grown pool, synchronously,
 * before RTR_OK is returned; a slot whose cloud has been replaced since fails instead.  The buffers (rtr_host_output_buffers: W*H*3 u8, W*H float,
 * valid until the next rtr_set_resolution) may be read until the slot is used again.  A caller that needs the
 * frame in its own arrays copies from there (or keeps using the synchronous calls).
 * The slots' pinned buffers and device snapshots are made by the first rtr_project_async / rtr_host_output_buffers at a
 * resolution, slot by slot; a failed allocation -> RTR_ERR_HIP, nothing is queued, a slot is either complete or absent
 * (no slot is marked busy), and the cloud and the frame resources of section 4 are as they were. */
#define RTR_ASYNC_SLOTS 2
int rtr_host_output_buffers(rtr_ctx *ctx, int slot, uint8_t **img, float **depth);
int rtr_project_async(rtr_ctx *ctx, const float P[16], int slot, int with_filter);
int rtr_wait(rtr_ctx *ctx, int slot);

/* ---- 5. phase calls (multi-GPU sharding: reduce between phases) ----------------- */
/*   rtr_clear -> rtr_min_depth_pass -> [all-reduce MIN of depth]
 *   -> rtr_accumulate_pass -> [all-reduce / reduce-scatter SUM of accum]
 *   -> rtr_resolve -> rtr_filter (optional)                                          */
int rtr_clear(rtr_ctx *ctx);                           /* render.cu:16-31 + project_cloud.cu:317 */
int rtr_min_depth_pass(rtr_ctx *ctx, const float P[16]);  /* render.cu:53-83   */
int rtr_accumulate_pass(rtr_ctx *ctx, const float P[16]); /* render.cu:85-130  */
int rtr_resolve(rtr_ctx *ctx);                         /* render.cu:132-163 */
/* Resolve only pixels [first_pixel, first_pixel + count) (first_pixel % 4 == 0) into
 * RTR_BUF_IMAGE, reading the accumulators either from RTR_BUF_ACCUM (acc_dev NULL) or from
 * a caller-owned device array of count*4 u32 -- the slice a reduce-scatter hands to a rank. */
int rtr_resolve_range(rtr_ctx *ctx, const void *acc_dev, uint64_t first_pixel, uint64_t count);
int rtr_filter(rtr_ctx *ctx);                          /* project_cloud.cu:331-392 */

/* ---- 5b. peer-to-peer exchange for the phase calls (one process per GPU on one node) ----
 * The hand-written counterpart of the two collectives above: every rank maps
 * the other ranks' frame buffers through hipIpc and pulls over xGMI.  Set up once per
 * resolution: each rank calls rtr_p2p_export, the handle blocks are exchanged by the host (any
 * transport: they are plain bytes), then every rank calls rtr_p2p_open with all of them.
 *   rtr_clear -> rtr_min_depth_pass -> rtr_p2p_min_depth     (RTR_BUF_DEPTH := MIN over ranks)
 *   -> rtr_accumulate_pass -> rtr_p2p_sum_resolve             (RTR_BUF_IMAGE := resolve(SUM of
 *   RTR_BUF_ACCUM over ranks); RTR_BUF_ACCUM itself stays local) -> rtr_filter (optional)
 * All ranks must issue the same sequence of rtr_p2p_* calls.  A rank that does not arrive
 * within the barrier timeout (option "p2p_timeout_ms", default 2 s) is flagged in rtr_p2p_status on the
 * ranks that waited for it; their frames since then are undefined.  The caller polls rtr_p2p_status
 * (a host word, no synchronisation), agrees with the other ranks and falls back to the collectives --
 * sharded.ShardedProjector does that every `check_every` frames.  rtr_set_resolution closes the mapping.
 * rtr_p2p_export allocates this rank's tile store, worst-case extent pool and exchange buffers; a failed allocation ->
 * RTR_ERR_HIP, the handle block holds nothing defined, the exchange buffers are all given back (nothing is exported:
 * rtr_p2p_open refuses until an export succeeds), and the cloud and the frame buffers are untouched.  rtr_p2p_open
 * after a failed allocation of its own has closed every mapping it made and dropped the export. */
#define RTR_P2P_MAX_RANKS 16
typedef struct rtr_p2p_handles {
    unsigned char depth[64], accum[64], image[64], reduced[64], flags[64], tiles[64];
    /* one hipIpcMemHandle_t each: the depth buffer and accumulators, exchange copies of the resolved
     * image and the reduced depth, the barrier flags, the per-tile occupancy bitmap */
    unsigned char store_meta[64], store_ext0[64], store_dyn[64];
    /* ... and this rank's tile store (stream lengths and extent directory, static extents, dynamic extent pool): the
     * owner-computes form reads the peers' entries out of it.  The store is sized by the resident cloud: export (and
     * open) again after rtr_upload_points / rtr_generate_synthetic. */
} rtr_p2p_handles;
int rtr_p2p_export(rtr_ctx *ctx, rtr_p2p_handles *mine);
int rtr_p2p_open(rtr_ctx *ctx, int rank, int world, const rtr_p2p_handles *all /* [world] */);
int rtr_p2p_close(rtr_ctx *ctx);
int rtr_p2p_min_depth(rtr_ctx *ctx);
int rtr_p2p_sum_resolve(rtr_ctx *ctx);
/* The whole sharded frame in one call: rtr_clear, rtr_min_depth_pass, rtr_p2p_min_depth,
 * rtr_accumulate_pass, rtr_p2p_sum_resolve and, if with_filter, rtr_filter -- trimmed in the tile-binned form
 * to eight launches (no clear, no slice reduction of the depth: one barrier, then the accumulate launch takes
 * the MIN over the occupying ranks' depth tiles itself; no gathers).  Afterwards RTR_BUF_DEPTH,
 * RTR_BUF_IMAGE (and the prefilter's outputs) hold the GLOBAL frame on every rank; RTR_BUF_ACCUM holds
 * this rank's partial sums, and in the tile-binned form only under the screen tiles that contain
 * points of this rank (the peers read nothing else: tiles without local points are not written). */
int rtr_p2p_render(rtr_ctx *ctx, const float P[16], int with_filter);
/* The owner-computes form of the sharded frame (tile-binned mode): every screen tile is produced by ONE of the ranks
 * that have points in it, which reads the other occupying ranks' entries out of their tile stores over xGMI and runs the
 * fused per-tile z-buffer once -- no MIN / SUM exchange, no second tile pass, two barriers and at most six launches per
 * frame.  Afterwards only rank `frame_owner` holds the GLOBAL frame (RTR_BUF_DEPTH / IMAGE and the prefilter's outputs:
 * it collects the other ranks' tiles); the buffers of the other ranks hold their own tiles only.  All ranks must pass
 * the same frame_owner; rotating it (frame k -> rank k mod world) spreads the collect + prefilter over the ranks, e.g.
 * one U-Net consumer per GPU.  Tiles are not split over workgroups in this form (split_threshold is ignored).
 * PRECONDITION on the ranks that are NOT the frame's owner: the call returns (its work queued) right after the second
 * barrier, while the owner is still reading this rank's RTR_BUF_DEPTH and image exchange copy over the mappings.  Only
 * the next rtr_p2p_render_owned's first barrier orders those reads against new writes: between two owned frames a
 * non-owner must not queue anything else that writes the frame buffers (rtr_render, rtr_clear, the phase calls,
 * rtr_p2p_render) without a barrier of the caller's own across the ranks (the Python ShardedProjector and bench.py
 * put a torch.distributed barrier / all-reduce there). */
int rtr_p2p_render_owned(rtr_ctx *ctx, const float P[16], int with_filter, int frame_owner);
int rtr_p2p_status(rtr_ctx *ctx, uint32_t *barrier_timeouts);

/* ---- 6. device-resident buffers (owned by the context, valid until the next
 *         rtr_set_resolution / rtr_destroy) ---------------------------------------- */
typedef enum {
    RTR_BUF_DEPTH = 0,  /* u32 [H*W]    float bits, RTR_EMPTY_DEPTH when empty (project_cloud.h:34) */
    RTR_BUF_ACCUM = 1,  /* u32 [H*W*4]  (sum c0, sum c1, sum c2, count)          (project_cloud.h:33) */
    RTR_BUF_IMAGE = 2,  /* u8  [H*W*3]  interleaved, input channel order         (project_cloud.h:26) */
    RTR_BUF_TENSOR = 3, /* f16 [5*H*W]  planar {1,5,H,W}                         (project_cloud.h:32) */
    RTR_BUF_MASK = 4,   /* u8  [H*W]    final keep-mask of the prefilter                              */
    RTR_BUF_MINMAX = 5, /* u32 [2]      depth min / max bits (project_cloud.h:30-31)                  */
    RTR_BUF_POINT_ID = 6, /* u32 [H*W]  upload index of the point each pixel shows (rtr_point_pass)       */
    RTR_BUF_VISIBLE = 7,  /* u32 [(n + 31) / 32]  bit i % 32 of word i / 32: point i contributed (ditto)  */
    /* the last rtr_render_views batch of `count` views (section 6c), view-major: */
    RTR_BUF_VIEW_DEPTH = 8,   /* u32 [count, H, W]                                                       */
    RTR_BUF_VIEW_IMAGE = 9,   /* u8  [count, H, W, 3]                                                    */
    RTR_BUF_VIEW_TENSOR = 10, /* f16 [count, 5, H, W]  one contiguous batch tensor                       */
    RTR_BUF_VIEW_MINMAX = 11, /* u32 [count, 2]                                                          */
    RTR_BUF_POINT_KEEP = 12,  /* u32 [(n + 31) / 32]  the keep mask in force (section 6e), upload order, bits past n clear */
    RTR_BUF_SELECTION = 13    /* u32 [(n + 31) / 32]  the selection (section 6f), upload order, bits past n clear */
} rtr_buffer;
int rtr_device_buffer(rtr_ctx *ctx, int which, void **dev_ptr, size_t *bytes);
/* Synchronous device->host copy of one buffer (bytes must equal its size). */
int rtr_download_buffer(rtr_ctx *ctx, int which, void *host, size_t bytes);

/* ---- 6b. point pass: which points a frame shows ------------------------------------
 * Take the frame the depth buffer holds (RTR_BUF_DEPTH as the frame left it: after a filtered frame, pixels the
 * prefilter removed hold the bits of -1.0f; pixels no point reached hold RTR_EMPTY_DEPTH), made with matrix P.  For
 * point i (UPLOAD order: the index in the rtr_upload_points array, or i - first of rtr_generate_synthetic) the
 * projection of the frame gives (pix, d) or nothing.
 *   RTR_BUF_POINT_ID: pixel p holds the smallest i with pix == p and bits(d) == depth[p]; 0xFFFFFFFF where there is
 *     none (empty pixels and pixels the prefilter removed).  Ties on equal depth bits go to the smallest upload index,
 *     so the buffer does not depend on the resident order or on any option.
 *   RTR_BUF_VISIBLE: bit i % 32 of word i / 32 is set iff point i projects and !(d > depth[pix] + depth_window) -- the
 *     accumulate pass's own test (render.cu:106).  On an unfiltered frame the visible points of pixel p number
 *     RTR_BUF_ACCUM[4 p + 3] and their colours sum to RTR_BUF_ACCUM[4 p .. 4 p + 2]; removed pixels contribute none.
 *     Bits past n are clear.
 * rtr_point_pass computes the buffers `what` asks for (RTR_POINTS_IDS | RTR_POINTS_VISIBLE), queued on the context's
 * stream behind the frame; P is passed explicitly like in the phase calls.  rtr_device_buffer / rtr_download_buffer
 * then serve them.  A frame that a synchronising call renders again (option "pool_worst_case") is rendered together
 * with the point pass queued right behind it; a point pass that read a frame reported incomplete otherwise makes
 * rtr_download_buffer of its outputs fail with RTR_ERR_INTERNAL.
 * Errors: RTR_ERR_INVALID without a cloud or a resolution, for `what` outside 1..3, and when the cloud was sorted
 * without option "point_ids" (rtr_last_error says so); RTR_ERR_UNSUPPORTED for 2^32 points or more.  The two buffers
 * are made on first use; a failed allocation -> RTR_ERR_HIP, nothing is launched, the frame and the cloud are
 * untouched, and a buffer the call could not make reads as before any pass (RTR_ERR_INVALID from rtr_device_buffer).
 * Sharded frames: on a rank the indices are rank-local (its own upload), and only its own points are tested against
 * the depth buffer it holds; a global ID needs the rank's offset and a MIN across ranks, which the library does not do. */
#define RTR_POINTS_IDS 1
#define RTR_POINTS_VISIBLE 2
int rtr_point_pass(rtr_ctx *ctx, const float P[16], int what);

/* ---- 6c. several views: one pass over the cloud for up to RTR_MAX_VIEWS poses ----------------
 * rtr_render_views renders `count` poses (P: count x 16 floats, each row-major like rtr_render's) at the context's
 * resolution and rtr_params into the RTR_BUF_VIEW_* buffers: view v is bit for bit what rtr_render(ctx, P + 16 v,
 * with_filter) would leave in RTR_BUF_DEPTH / IMAGE (and, filtered, TENSOR / MINMAX; unfiltered batches leave those
 * two undefined, as rtr_render leaves them stale).  rtr_get_option(ctx, "views", &k) gives the last batch's count.
 * The single frame is left alone: RTR_BUF_DEPTH .. RTR_BUF_VISIBLE, the frame rtr_synchronize would repeat, the
 * asynchronous slots and the point pass keep what they held.
 * Binned form (option "mode" 1, <= 4096 tiles, no open p2p group, option "overlap" 0): ONE point-kernel launch
 * streams the cloud for every view (timed as RTR_K_MIN_DEPTH), then one tile launch per view (RTR_K_TILE) and the
 * prefilter.  Every other case -- mode 0, more than 4096 tiles, an open p2p group, option "overlap" 1 -- loops over
 * the two-pass atomic form into the view buffers: exact, no sharing.
 * Asynchronous like rtr_render.  Each view has its own tile store (a 32 KB static extent per 32x16 storage tile:
 * ~134 MB per view at 1920x1080) and adaptive extent pool, allocated on first use for the largest count seen (stores
 * per resolution, pools per cloud).  A batch that overflows an adaptive pool is rendered again by the next
 * rtr_synchronize or rtr_download_buffer(RTR_BUF_VIEW_*), with every view's pool worst-case sized (16 B per point and
 * view) from then on for this cloud; a caller who consumes batches on the stream without such a call sets option
 * "pool_worst_case" 1.
 * Errors: count outside 1..RTR_MAX_VIEWS, P NULL, no cloud or no resolution -> RTR_ERR_INVALID, nothing changed.
 * A failed allocation (batch buffers, pyramid levels, a view's store or pool, the views' table) -> RTR_ERR_HIP: no batch
 * is current ("views" reads 0, RTR_BUF_VIEW_* hold nothing defined), every resource is complete or absent, the single
 * frame and the cloud are untouched, and the same call made again renders the exact batch. */
#define RTR_MAX_VIEWS 8
int rtr_render_views(rtr_ctx *ctx, int count, const float *P, int with_filter);

/* ---- 6d. clip planes: leave part of the cloud out of every frame ------------------------------------
 * Up to RTR_MAX_CLIP_PLANES world-space half-spaces, each {a, b, c, d} (planes: count x 4 floats).  A point (x, y, z)
 * of the uploaded cloud -- the coordinates as uploaded: packing and the Morton sort do not change them -- is kept iff
 * for every plane
 *     ((a*x + b*y) + c*z) + d >= 0
 * with every product and sum rounded to fp32 on its own (no FMA; NaN is not >= 0): numpy float32 arithmetic in that
 * order is an exact reference.  For the unit-normal planes of an axis-aligned box -- {1,0,0,-lo.x}, {-1,0,0,hi.x}, and
 * the same in y and z -- the test is exactly lo <= p <= hi per axis, points on the faces included.
 * A point that is not kept acts as if it were absent from the cloud in every output: depth, accumulators, image,
 * prefilter mask / tensor / min-max, RTR_BUF_POINT_ID never names it, its RTR_BUF_VISIBLE bit is 0, and the frame
 * statistics and the adaptive extent pool's sizing never count it.  Every call that renders honours them: rtr_project
 * (_filtered), rtr_render, rtr_project_async, the phase calls, rtr_point_pass, rtr_render_views (the planes are shared
 * by every view) and rtr_p2p_render(_owned) -- a sharded frame uses each rank's own planes, so the caller sets the same
 * ones on every rank.  rtr_stream_probe ignores them.  Chunks that lie outside a plane are rejected on their boxes
 * before their coordinates are read, so a crop costs less than the whole frame.
 * The planes are context state like rtr_params: a call uses the planes in force when it is issued, and a frame that a
 * synchronising call renders again (an overflow of the adaptive pool, an async slot that rtr_wait repeats) comes out
 * with the planes it was issued with.  count = 0 (the default) clears them; frames are then exactly as without this
 * section.
 * Errors: count outside 0..RTR_MAX_CLIP_PLANES, planes NULL with count > 0, a non-finite coefficient or a = b = c = 0
 * -> RTR_ERR_INVALID, nothing changed.  rtr_get_clip_planes writes the count and count x 4 floats (room for
 * RTR_MAX_CLIP_PLANES x 4; planes may be NULL while none are set). */
#define RTR_MAX_CLIP_PLANES 8
int rtr_set_clip_planes(rtr_ctx *ctx, int count, const float *planes);
int rtr_get_clip_planes(rtr_ctx *ctx, int *count, float *planes);

/* ---- 6e. keep mask: hide any set of points from every frame ---------------------------------------------------------
 * words: (n + 31) / 32 u32 in upload order -- bit i % 32 of word i / 32 set = point i is kept: the layout of
 * RTR_BUF_VISIBLE, so a point pass's output can be fed straight back.  Host memory or device memory of the context's
 * device (copied; the caller may reuse it at once).  words == NULL with nwords == 0 clears the mask.  Bits past n are
 * ignored and read back as 0 (RTR_BUF_POINT_KEEP; rtr_get_option("point_keep") reads 1 while a mask is set).
 * Indices are the point pass's: the index in the rtr_upload_points array, or i - first for rtr_generate_synthetic.  A
 * cloud sorted by the library needs option "point_ids" = 1 (the mask goes through its permutation; rtr_reorder_points
 * keeps the mask in force and refuses to sort a masked cloud without point_ids).
 * A hidden point acts as if it were absent from the cloud in every output, exactly as a clipped point (section 6d):
 * depth, accumulators, image, prefilter mask / tensor / min-max, RTR_BUF_POINT_ID never names it, its RTR_BUF_VISIBLE
 * bit is 0, and the frame statistics and the adaptive extent pool's sizing never count it.  Every call that renders
 * honours it: rtr_project(_filtered), rtr_render, rtr_project_async, the phase calls, rtr_point_pass,
 * rtr_render_views (shared by every view) and rtr_p2p_render(_owned) -- each rank its own mask, in its own rank-local
 * indices.  rtr_stream_probe and rtr_download_points ignore it.  With clip planes a point is drawn iff the mask AND
 * every plane keep it.  Chunks of 256 resident points that the mask hides entirely are rejected before their
 * coordinates are read.
 * Ordering: the call first completes every frame, pass, view batch and async slot issued before it, as rtr_synchronize
 * does (frames that overflowed the adaptive pool are rendered again with the mask they were issued with); if that
 * fails it returns the error and the old mask stays.  A new cloud (rtr_upload_points, rtr_generate_synthetic) clears it.
 * Memory: while a mask is set, 2 bits per point (upload-order and resident-order copies) + 1 byte per 256 points; none
 * without one.
 * Errors: no cloud, nwords != (n + 31) / 32, words NULL with nwords > 0, a sorted cloud without point_ids
 * -> RTR_ERR_INVALID, nothing changed.  A failed allocation -> RTR_ERR_HIP and the old mask (or none) stays in force:
 * the new words are built in buffers of their own and swapped in at the end. */
int rtr_set_point_keep(rtr_ctx *ctx, const uint32_t *words, uint64_t nwords);

/* ---- 6f. selection: name the points of a region on the device -----------------------------------------------------
 * rtr_set_point_keep, rtr_remove_points and rtr_transform_points name their points by (n + 31) / 32 words in upload
 * order.  rtr_select_points makes such words on the device from a region, without the coordinates leaving it, into
 * RTR_BUF_SELECTION: bit i % 32 of word i / 32 set = point i is selected, bits past n clear.  rtr_device_buffer gives
 * its device pointer, which the three editing calls accept as it is (they copy their words before they change anything).
 * inside(i) holds iff both
 *   1. every one of the plane_count planes GIVEN TO THIS CALL keeps point i: the contract of section 6d exactly
 *      (0..RTR_MAX_CLIP_PLANES planes {a, b, c, d}, ((a*x + b*y) + c*z) + d >= 0 with every product and sum rounded on
 *      its own, NaN is not kept).  plane_count = 0: true;
 *   2. P is NULL, or the projection of a frame with matrix P at the context's resolution accepts the point at a pixel
 *      (px, py) with rect[0] <= px < rect[2] and rect[1] <= py < rect[3] (rect = {x0, y0, x1, y1}): the frame's own
 *      arithmetic, so a point is in the rectangle exactly when that frame would splat it there, before any depth test.
 * plane_count = 0 with P NULL selects every point.  hit = inside, or, with RTR_SELECT_OUTSIDE OR-ed into op, !inside
 * for the points below n -- the keep words rtr_remove_points wants in order to delete the inside of a box.  op combines
 * the hits with the selection so far; one that does not exist yet counts as empty.  RTR_SELECT_TOGGLE with no plane and
 * no P inverts the selection: no sequence of the other four ops can, and "remove / hide what is selected" needs the
 * complement as keep words.
 * The call reads the uploaded coordinates and nothing else: the context's own clip planes and keep mask are ignored, as
 * in rtr_download_points.  It changes no frame, frame buffer, tile store, pool, statistics or point-pass buffer, and an
 * open peer-to-peer exchange stays open.  Chunks of 256 resident points whose box lies wholly outside the region, or
 * (planes only) wholly inside it, are decided without reading their coordinates.
 * Ordering: queued on the context's stream like rtr_point_pass.  stats NULL: the call does not wait.  With stats it
 * waits for the stream, like rtr_download_buffer, and writes [0] the points selected after op, [1] chunks decided on
 * their boxes as wholly outside the region, [2] chunks decided wholly inside, [3] chunks decoded and tested point by
 * point; [1] + [2] + [3] is the chunk count, (n + 255) / 256.
 * Life: the buffer is allocated by the first call (8 words per 256-point chunk; counted in option
 * "resident_millibytes_per_point" while it exists) and survives rtr_transform_points, rtr_reorder_points,
 * rtr_set_point_keep, rtr_set_clip_planes and rtr_set_resolution.  Whatever renumbers upload indices drops it --
 * rtr_upload_points, rtr_generate_synthetic, rtr_append_points, rtr_remove_points -- as does rtr_clear_selection:
 * rtr_device_buffer(RTR_BUF_SELECTION) then fails with RTR_ERR_INVALID and rtr_get_option("selection") reads 0.
 * Indices are the point pass's; a cloud sorted by the library needs option "point_ids" = 1.
 * Sharded frames: each rank selects among its own points by its own indices, as with the keep mask.
 * Errors: no cloud, plane_count outside 0..RTR_MAX_CLIP_PLANES, planes NULL with plane_count > 0, a non-finite
 * coefficient or a = b = c = 0, P given without a resolution or with rect NULL, a rectangle not within 0 <= x0 < x1 <= W
 * and 0 <= y0 < y1 <= H, an unknown op, a sorted cloud without point_ids -> RTR_ERR_INVALID, nothing changed;
 * RTR_ERR_UNSUPPORTED for 2^32 points or more.  The call allocates only when no selection exists yet: a failed
 * allocation -> RTR_ERR_HIP, there is still no selection ("selection" reads 0) and stats is untouched. */
#define RTR_SELECT_REPLACE   0   /* sel  = hit          */
#define RTR_SELECT_ADD       1   /* sel |= hit          */
#define RTR_SELECT_SUBTRACT  2   /* sel &= ~hit         */
#define RTR_SELECT_INTERSECT 3   /* sel &= hit          */
#define RTR_SELECT_OUTSIDE   4   /* flag, OR-ed into op: hit = !inside (for the points below n) */
#define RTR_SELECT_TOGGLE    8   /* sel ^= hit          */
/* RTR_BUF_SELECTION = 13: u32 [(n + 31) / 32], upload order, bits past n clear */
int rtr_select_points(rtr_ctx *ctx, int plane_count, const float *planes, const float *P, const int rect[4],
                      int op, uint64_t stats[4]);
int rtr_clear_selection(rtr_ctx *ctx);

/* ---- 6g. selection by density: one point per cell of a voxel grid -------------------------------------------------
 * rtr_select_voxel_grid thins the resident cloud on the device: of the points that fall into one cell of a regular grid
 * it names one (PCL's VoxelGrid, spatial subsampling).  It writes into RTR_BUF_SELECTION exactly as rtr_select_points
 * does -- the same buffer, the same life, the same op values with RTR_SELECT_OUTSIDE OR-ed in -- so the words feed
 * rtr_remove_points, rtr_set_point_keep, rtr_transform_points, rtr_extract_points and rtr_write_points as they are.
 * Cell of a point: inv[k] = 1.0f / cell[k], one IEEE fp32 division on the host; per axis t[k] = (p[k] - origin[k]) * inv[k]
 * with the difference and the product each rounded to fp32 on its own (no FMA): numpy float32 in that order is an exact
 * reference.  Point i is IN THE GRID iff on all three axes t[k] is finite and -2^20 <= t[k] < 2^20; its cell is then
 * q[k] = floor(t[k]), three integers in [-2^20, 2^20).  Every other point -- a NaN or infinite coordinate, a difference
 * or a product that overflows, a cell beyond +-2^20 -- is OUT OF THE GRID and counts as a cell of its own holding that
 * one point.
 * The representative of a cell is its point with the SMALLEST UPLOAD INDEX: it does not depend on the resident order,
 * the library's sort, the packed form or any option.  hit(i) holds iff point i is the representative of its cell and the
 * cell holds at least min_count (>= 1) points.  min_count = 1 is plain thinning; min_count = k also drops the cells with
 * fewer than k returns (isolated stragglers).  Out-of-grid points are hits exactly when min_count == 1: thinning never
 * silently loses a far-away point.  With RTR_SELECT_OUTSIDE hit = !hit for the points below n: thinning is this call with
 * OUTSIDE followed by "remove / hide what is selected", or plain REPLACE with the words as rtr_remove_points' keep words.
 * What it reads and leaves alone: section 6f's list.  The call reads the uploaded coordinates only; the context's clip
 * planes and keep mask are ignored.  It changes no frame, frame buffer, tile store, pool, statistics, point-pass buffer
 * or keep mask, and an open peer-to-peer exchange stays open.  Indices are the point pass's; a cloud sorted by the
 * library needs option "point_ids" = 1.
 * Ordering: queued on the context's stream behind everything issued before it.  Unlike rtr_select_points the call ALWAYS
 * waits for its own work before it returns, stats or not: it frees its scratch.  It does not repeat frames whose extent
 * pool overflowed: a frame's error stays pending for the next synchronising call, as in section 2e.
 * stats (may be NULL): [0] the points selected after op, [1] occupied in-grid cells, [2] those of them holding at least
 * min_count points, [3] out-of-grid points.  Without OUTSIDE and with op REPLACE, [0] == [2] + (min_count == 1 ? [3] : 0).
 * Memory and cost: one sweep over the coordinates, a stable radix sort of n (64-bit key, 32-bit index) pairs and two
 * passes over the sorted pairs and the words.  Scratch for the duration of the call: 24 B per point (the pairs, twice:
 * the sort is out of place), the sort's temporary and (n + 31) / 32 words -- about 2.4 GB at 1e8 points.
 * Errors: no cloud, origin or cell NULL, a non-finite origin, a cell size that is not finite and > 0 or whose fp32
 * reciprocal is not, min_count == 0, an unknown op, a sorted cloud without point_ids -> RTR_ERR_INVALID;
 * RTR_ERR_UNSUPPORTED for 2^32 points or more; a failed allocation -> RTR_ERR_HIP.  Every scratch buffer is allocated
 * before the first selection word changes: after any of these the selection and everything else are as they were, the
 * caller's stats included (they are written by a call that succeeds, and by no other). */
int rtr_select_voxel_grid(rtr_ctx *ctx, const float origin[3], const float cell[3], uint32_t min_count, int op,
                          uint64_t stats[4]);

/* ---- 6h. selection by neighbour count: the radius outlier filter ---------------------------------------------------
 * rtr_select_neighbours names the resident points that have at least min_neighbours OTHER points within `radius` (PCL's
 * RadiusOutlierRemoval, Open3D's remove_radius_outlier).  It writes into RTR_BUF_SELECTION exactly as rtr_select_points
 * does -- the same buffer, the same life, the same five op values with RTR_SELECT_OUTSIDE OR-ed in, bits past n clear --
 * so the words feed rtr_remove_points, rtr_set_point_keep, rtr_transform_points, rtr_extract_points and
 * rtr_write_points as they are.
 * Neighbour relation: exact and symmetric.  r2 = radius * radius, rounded once to fp32 on the host.  Points i != j
 * (upload indices) are NEIGHBOURS iff ((dx*dx + dy*dy) + dz*dz) <= r2 with dx = x[i] - x[j], dy = y[i] - y[j],
 * dz = z[i] - z[j], every difference, product and sum rounded to fp32 on its own (no FMA): numpy float32 in that order
 * is a bit-for-bit reference.  The comparison is inclusive; coincident points are neighbours of each other (d2 == 0); a
 * point is never its own neighbour (by index, not by position).
 * Non-finite points: a point with a NaN or infinite coordinate has no neighbours and is nobody's neighbour.  (A
 * difference that overflows to infinity fails the comparison by itself.)
 * hit(i) holds iff point i has at least min_neighbours (>= 1) neighbours.  With RTR_SELECT_OUTSIDE hit = !hit for the
 * points below n: the outliers, non-finite points included -- what a clean-up removes (select with OUTSIDE, then
 * rtr_remove_points with the complement as keep words, or rtr_set_point_keep, or rtr_extract_points).
 * Independence: the result depends on the coordinates and the upload indices alone -- not on the resident order, the
 * library's sort, the packed form, any option or the internal grid.
 * The internal grid: cubic cells of edge h = radius * (1 + 2^-10), anchored at the world origin, a coordinate's cell
 * floor(p / h) in fp64; two neighbours never lie more than one cell apart on an axis (the proof: csrc/rtr_neighbour_cell.h).
 * Its SPAN is the cells -(2^20 - 1) .. 2^20 - 2 per axis, i.e. -(2^20 - 1) h <= p < (2^20 - 1) h: every cloud whose finite
 * coordinates lie within +-2^20 * radius of the world origin is covered.  (Since r2 must be finite, +-FLT_MAX is always
 * beyond the span.)
 * What it reads and leaves alone: section 6f's list.  The call reads the uploaded coordinates only; the context's clip
 * planes and keep mask are ignored.  It changes no frame, frame buffer, tile store, pool, statistics, point-pass buffer
 * or keep mask, and an open peer-to-peer exchange stays open.  Indices are the point pass's; a cloud sorted by the
 * library needs option "point_ids" = 1.  A sharded context selects among its own points.
 * Ordering: as section 6g.  Queued on the context's stream behind everything issued before it; the call ALWAYS waits
 * for its own work before it returns, stats or not: it frees its scratch (and it waits twice on the way, for the key
 * sweep's counters and for the number of occupied cells).  It does not repeat frames whose extent pool overflowed.
 * stats (may be NULL): [0] the points selected after op, [1] points with at least min_neighbours neighbours, [2] finite
 * points with no neighbour at all, [3] non-finite points.
 * Memory and cost: one sweep over the coordinates, a stable radix sort of n (64-bit key, 32-bit index) pairs, a gather
 * of 16-byte records into cell order, and the pair tests.  Scratch for the duration of the call: 56 B per point (the
 * pairs and the records, twice each), the sort's temporary, (n + 31) / 32 words and 80 B per work item -- one item per
 * occupied cell and 64-point slice of it, at most min(cells + n / 64, n) -- about 6 to 14 GB at 1e8 points.  The work is
 * proportional to the candidate pairs actually tested: a query point is tested against the points of the 27 cells
 * around it, 64 at a time, and its wave stops as soon as all of its up to 64 query points have min_neighbours
 * neighbours.  A pile of m coincident or near-coincident points with min_neighbours > m therefore costs O(m^2) pair
 * tests; so does a radius far larger than the point spacing.
 * Errors, with nothing changed: no cloud, a radius that is not finite and > 0, an r2 that is not a finite normal fp32
 * number, min_neighbours == 0, an unknown op, a sorted cloud without point_ids -> RTR_ERR_INVALID; 2^32 points or more ->
 * RTR_ERR_UNSUPPORTED; a finite coordinate beyond the span -> RTR_ERR_UNSUPPORTED (found by a counter of the key sweep,
 * before any selection word changes); a failed allocation -> RTR_ERR_HIP.  Every scratch buffer is allocated before the
 * first selection word changes: after any of these the selection and everything else are as they were, the caller's
 * stats included. */
int rtr_select_neighbours(rtr_ctx *ctx, float radius, uint32_t min_neighbours, int op, uint64_t stats[4]);

/* ---- 6i. selection by connected cluster: Euclidean clustering -------------------------------------------------------
 * rtr_select_clusters names the resident points by the size of the cluster they belong to (PCL's
 * EuclideanClusterExtraction, Open3D's cluster_dbscan with min_points = 1, "label connected components"): drop every
 * floating blob of fewer than 50 returns, keep the largest structure, grow the selection to everything connected to it,
 * label the segments.  It writes into RTR_BUF_SELECTION exactly as rtr_select_points does -- the same buffer, the same
 * life, the same five op values with RTR_SELECT_OUTSIDE OR-ed in, bits past n clear -- so the words feed
 * rtr_remove_points, rtr_set_point_keep, rtr_transform_points, rtr_extract_points and rtr_write_points as they are.
 * Neighbour relation: exactly section 6h's, with the same rounding.  r2 = radius * radius, rounded once to fp32 on the
 * host; points i != j are neighbours iff ((dx*dx + dy*dy) + dz*dz) <= r2 in fp32, every difference, product and sum
 * rounded on its own (no FMA), inclusive; coincident points are neighbours of each other; a point is never its own
 * neighbour (by index, not by position); a non-finite point has no neighbours and is nobody's neighbour.
 * Clusters: the connected components of that relation over the n resident points.  A point without neighbours is a
 * cluster of one -- every non-finite point among them.  The LABEL of a cluster is the smallest upload index among its
 * members; its size is its member count.  numpy float32 in section 6h's order with any correct component labelling is
 * a bit-for-bit reference: nothing here has a tolerance.
 * Independence: clusters, labels and sizes depend on the coordinates and the upload indices alone -- not on the
 * resident order, the library's sort, the packed form, any option or the internal grid.
 * hit(i) holds iff all of
 *   1. size(cluster(i)) >= min_points (>= 1);
 *   2. max_points == 0 (unbounded) or size(cluster(i)) <= max_points;
 *   3. flags has no RTR_CLUSTER_SEEDED, or the cluster of i contains at least one point that was selected BEFORE this
 *      call (the seeds are read before op is applied; a selection that does not exist yet is empty, so nothing hits --
 *      and the call creates an empty selection).  Seeded with op REPLACE grows the selection to everything connected to
 *      it; with SUBTRACT or INTERSECT the seeds are likewise the selection as it was before the call.
 * With RTR_SELECT_OUTSIDE hit = !hit for the points below n: "remove the small blobs" is min_points = k with OUTSIDE,
 * then "remove what is selected".  op combines the hits with the selection so far as in section 6f.
 * labels (may be NULL): room for n uint32_t, in host memory or in device memory of the context's device -- told apart
 * as rtr_extract_points tells its outputs apart.  labels[i] = the label of point i's cluster, in upload order, for
 * every point (hit or not, finite or not: a non-finite point's label is its own index).  It is written only when the
 * call succeeds; after any error every element is as it was.  There is no resident label buffer.
 * stats (may be NULL): [0] the points selected after op, [1] clusters, [2] clusters that hit (before OUTSIDE),
 * [3] the points of the largest cluster.
 * The internal grid and its SPAN: section 6h's -- every cloud whose finite coordinates lie within +-2^20 * radius of the
 * world origin is covered.
 * What it reads and leaves alone: section 6f's list.  The call reads the uploaded coordinates and, when seeded, the
 * selection; the context's clip planes and keep mask are ignored.  It changes no frame, frame buffer, tile store, pool,
 * statistics, point-pass buffer or keep mask, and an open peer-to-peer exchange stays open.  Indices are the point
 * pass's; a cloud sorted by the library needs option "point_ids" = 1.  A sharded context clusters its own points.
 * Ordering: as section 6h.  Queued on the context's stream behind everything issued before it; the call ALWAYS waits
 * for its own work before it returns, stats or not (and it waits twice on the way, for the key sweep's counters and for
 * the number of occupied cells).  It does not repeat frames whose extent pool overflowed.
 * Memory and cost: section 6h's sweep, sort, gather and work list, then a lock-free union-find over the sorted
 * positions (every accepted pair unites two sets; the larger root is hooked under the smaller, so a parent never
 * exceeds its child and no wave ever waits for another), a pass that flattens it and gathers size, label and seed flag
 * at the roots, and a pass that writes hits and labels.  Scratch for the duration of the call: section 6h's and nothing
 * on top -- 56 B per point, the sort's temporary, (n + 31) / 32 words and 80 B per work item; the union-find's 16 B per
 * point and the labels' 4 B per point reuse buffers that the sort and the gather have finished with -- about 6 to 14 GB
 * at 1e8 points.  Every candidate pair of the 27 cells around a point is tested once per direction at most (the
 * library tests a pair only from its end later in cell order, and skips the 64-candidate tiles that lie wholly behind
 * the querying slice).  There is NO early exit: unlike section 6h every edge matters, so a pile of m coincident or
 * near-coincident points costs O(m^2) pair tests whatever the arguments are; so does a radius far larger than the point
 * spacing.
 * Errors, with nothing changed: no cloud, a radius that is not finite and > 0, an r2 that is not a finite normal fp32
 * number, min_points == 0, max_points != 0 && max_points < min_points, unknown bits in flags, an unknown op, a sorted
 * cloud without point_ids -> RTR_ERR_INVALID; 2^32 points or more -> RTR_ERR_UNSUPPORTED; a finite coordinate beyond the
 * span -> RTR_ERR_UNSUPPORTED (found by a counter of the key sweep, before any selection word or any element of labels
 * changes, and before a selection is created); a failed allocation -> RTR_ERR_HIP.  Every scratch buffer is allocated
 * before the first selection word changes: after any of these the selection and everything else are as they were, the
 * caller's labels and stats included. */
#define RTR_CLUSTER_SEEDED 1   /* flags: only clusters holding a currently selected point */
int rtr_select_clusters(rtr_ctx *ctx, float radius, uint32_t min_points, uint32_t max_points,
                        int flags, int op, uint32_t *labels, uint64_t stats[4]);

/* ---- 6j. fitting the dominant plane: counting points in bands, RANSAC on top -----------------------------------------
 * The ground-plane stage of a LiDAR pipeline (PCL's SACSegmentation with SACMODEL_PLANE, Open3D's segment_plane):
 * rtr_fit_plane finds the plane that has the most resident points within `dist` of it, rtr_count_in_bands is the
 * primitive it is built on.  Neither writes the selection: the facades' selectPlane turns a fitted plane into one with
 * rtr_select_points (section 6f), and from there section 6i can cluster what is left.
 *
 * rtr_count_in_bands.  A BAND is five floats {a, b, c, d_lo, d_hi}.  Point i is IN band k iff
 *     u + d_lo >= 0  and  (-u) + d_hi >= 0,   u = (a*x + b*y) + c*z,
 * every product and every sum rounded to fp32 on its own (no FMA); NaN is in no band.  This is bit for bit the section
 * 6d test of the two planes {a, b, c, d_lo} and {-a, -b, -c, d_hi}: negation commutes with round-to-nearest, so the
 * second plane's sum is exactly -u and sharing u is no approximation.  Hence numpy float32 in that order is a
 * bit-for-bit reference, and counts[k] equals stats[0] of rtr_select_points(ctx, 2, those two planes, NULL, NULL,
 * RTR_SELECT_REPLACE, stats).  counts[k] = the number of points of the POPULATION in band k, k < count <= RTR_MAX_BANDS.
 * Population: every resident point, or, with RTR_BANDS_SELECTED in flags, the points selected now (RTR_BUF_SELECTION as
 * it is; a selection that does not exist counts as empty, and the call does not create one).
 * What it reads and leaves alone: the uploaded coordinates and, with the flag, the selection; the context's clip planes
 * and keep mask are ignored.  It changes NOTHING in the context -- section 6f's list, and the selection too: no frame,
 * frame buffer, tile store, pool, statistics, point-pass buffer, keep mask or selection word, and an open peer-to-peer
 * exchange stays open.  Indices are the point pass's: with the flag a cloud sorted by the library needs option
 * "point_ids" = 1; without it no index is involved and every cloud works.  A sharded context counts its own points;
 * counts are plain sums, so the ranks may all-reduce them (which is why the primitive is public).
 * Ordering: queued on the context's stream behind everything issued before it; the call ALWAYS waits for its own work,
 * since the counts go to the host.  It does not repeat frames whose extent pool overflowed.
 * stats (may be NULL): [0] the population size, [1] (chunk, band) pairs decided on the chunk's box as wholly outside the
 * band, [2] pairs decided on the box as wholly inside, [3] pairs tested point by point; [1] + [2] + [3] =
 * ((n + 255) / 256) * count.  With the flag a chunk without a selected point is outside for every band.
 * Memory and cost: the bands are taken 64 at a time (one launch each).  In a pass every 256-point chunk is classified
 * on its box against all bands of the pass; a chunk that is neither outside nor inside for some band is decoded ONCE
 * and tested against those bands only; an inside decision adds the chunk's population without its coordinates.
 * Scratch: 8 * count bytes, and with the flag on a sorted cloud 32 bytes per 256 points (the selection in resident
 * order, gathered once per call).
 * Errors, with counts and stats untouched: no cloud, count outside 1..RTR_MAX_BANDS, bands or counts NULL, a non-finite
 * value in a band or a = b = c = 0, unknown bits in flags, the flag on a sorted cloud without point_ids ->
 * RTR_ERR_INVALID; 2^32 points or more -> RTR_ERR_UNSUPPORTED; a failed allocation -> RTR_ERR_HIP.
 *
 * rtr_fit_plane.  RANSAC with `iterations` candidates, each the plane through three points of the population, scored by
 * rtr_count_in_bands.  Every host step is csrc/rtr_plane_fit.h, in fp64 / uint64 with one rounding per operation: a
 * numpy float64 / uint64 program is an exact reference.
 *   Sampler: m = the population size (n, or the selected count with RTR_BANDS_SELECTED).  Draw t = 3 c + j (candidate c,
 *     j = 0..2) is z = seed + (t + 1) * 0x9E3779B97F4A7C15 followed by z ^= z >> 30; z *= 0xBF58476D1CE4E5B9;
 *     z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 (splitmix64, modulo 2^64).  Its rank is z % m, its point the
 *     rank-th point of the population in upload order (with the flag: the rank-th selected index).  The sample's
 *     coordinates come through rtr_extract_points' path.
 *   Candidate, from the fp32 points p0, p1, p2 widened to double: e1 = p1 - p0, e2 = p2 - p0, nv = e1 x e2 with each
 *     component (f*g) - (h*k), both products rounded on their own; len = sqrt((nx*nx + ny*ny) + nz*nz).  The candidate is
 *     DEGENERATE if two of its ranks coincide, a sample coordinate is not finite, len is not finite and > 0, or the
 *     offset below does not fit fp32.  Otherwise A = nv / len per component, negated if needed so that (c, b, a) is
 *     lexicographically positive (the normal points up in a z-up cloud); D = -((A.x*x0 + A.y*y0) + A.z*z0);
 *     plane = {(float)A.x, (float)A.y, (float)A.z, (float)D}; its band = {a, b, c, d + dist, dist - d} in fp32 (a band
 *     with a non-finite bound makes the candidate DEGENERATE too).
 *   Result: the winner is the non-degenerate candidate with the largest count, ties to the smallest c; plane[4] is its
 *     plane.  stats (may be NULL): [0] its count, [1] non-degenerate candidates, [2] the winner's c, [3] m.  If every
 *     candidate is degenerate (m < 3 among other cases) the call returns RTR_OK with plane = {0, 0, 0, 0} and stats[0]
 *     = [1] = [2] = 0: the facades raise / throw.  There is no least-squares refit.
 * It changes nothing in the context and neither changes nor creates the selection; ordering as rtr_count_in_bands (it
 * waits for the sample, then for the counts).  The sample is drawn by upload index, so a cloud sorted by the library
 * needs option "point_ids" = 1 with or without the flag.
 * Memory and cost: (n + 31) / 32 words of scratch for the sample's bits (set on the device), one extract of at most
 * 3 * iterations points, then rtr_count_in_bands over the non-degenerate candidates.  With the flag the selection words
 * are copied to the host once (the rank-th selected index is found there).
 * Errors, with plane and stats untouched: those of rtr_count_in_bands (plane NULL in place of bands / counts), dist not
 * finite or < 0 (dist = 0 is allowed), iterations outside 1..RTR_MAX_BANDS, a sorted cloud without point_ids. */
#define RTR_MAX_BANDS 4096
#define RTR_BANDS_SELECTED 1   /* flags: count only the currently selected points */
int rtr_count_in_bands(rtr_ctx *ctx, uint32_t count, const float *bands /* count x 5, host */, int flags,
                       uint64_t *counts /* count, host */, uint64_t stats[4]);
int rtr_fit_plane(rtr_ctx *ctx, float dist, uint32_t iterations, uint64_t seed, int flags, float plane[4],
                  uint64_t stats[4]);

/* ---- 6k. selection by distance to given points: what a new scan touches ------------------------------------------------
 * rtr_select_near relates the resident cloud to ANOTHER set of points: it names the resident points that have a given
 * point within `radius` and, in near_words, the given points that have a resident point within it -- merging a scan
 * without piling up duplicates ("append only the returns with no resident point within 2 cm"), change detection in
 * both directions, brush and trajectory selection.  It writes into RTR_BUF_SELECTION exactly as rtr_select_points does
 * -- the same buffer, the same life, the same five op values with RTR_SELECT_OUTSIDE OR-ed in, bits past n clear, a
 * selection that does not exist yet counts as empty and is created -- so the words feed rtr_remove_points,
 * rtr_set_point_keep, rtr_transform_points, rtr_extract_points and rtr_write_points as they are.
 * Given points: `count` points at xyz + j * xyz_stride_bytes, three floats each; strides as rtr_upload_points takes them
 * (12 for tight points, 16 for float4).  The memory is host memory or device memory of the context's device, told
 * apart as rtr_extract_points tells its outputs apart.  The call copies or reads the given points before it returns.
 * count == 0 is legal: xyz may then be NULL and nothing is near anything.
 * Relation: exactly section 6h's, between a resident point i and a given point j.  r2 = radius * radius, rounded once
 * to fp32 on the host.  The pair is NEAR iff ((dx*dx + dy*dy) + dz*dz) <= r2 with dx = x[i] - gx[j], dy = y[i] - gy[j],
 * dz = z[i] - gz[j], every difference, product and sum rounded to fp32 on its own (no FMA): numpy float32 in that order
 * is a bit-for-bit reference, nothing has a tolerance.  The comparison is inclusive.  The direction of the subtraction
 * does not matter: negation is exact and the squares are equal.  There is no self-exclusion: the two sets are distinct,
 * and a given point coincident with a resident one is near it.  A non-finite point on either side is near nothing.
 * Resident side: hit(i) holds iff resident point i is near at least one given point.  With RTR_SELECT_OUTSIDE hit = !hit
 * for the points below n.  op combines the hits with the selection so far as in section 6f.
 * Given side: near_words may be NULL.  Otherwise (count + 31) / 32 words, in host or device memory: bit j % 32 of word
 * j / 32 set iff given point j is near at least one resident point -- EVERY resident point counts: the keep mask, the
 * clip planes and the selection are ignored.  Bits past count are clear.  The words are written only when the call
 * succeeds.
 * RTR_NEAR_GIVEN_ONLY: only near_words and stats[2..3]; the selection is neither read, changed nor created.  op must be
 * 0 and near_words must not be NULL.  ("Append only what is new": a scan that adds nothing leaves the selection alone.)
 * Independence: the results depend on the coordinates and on the upload and given indices alone -- not on the resident
 * order, the library's sort, the packed form, any option, the internal grid or the order of the given points.
 * The internal grid and its SPAN: section 6h's grid (csrc/rtr_neighbour_cell.h).  Only the GIVEN points must lie inside
 * the span, every given point within +-2^20 * radius of the world origin does; a finite given coordinate beyond it ->
 * RTR_ERR_UNSUPPORTED before anything changes.  RESIDENT points may lie anywhere -- unlike section 6h, because chunks
 * rejected on their boxes are never looked at --: a resident point is tested exactly wherever it is; one whose cell on
 * some axis lies more than one cell beyond the span is near no given point, and one a single cell beyond the span can
 * be near a given point in the last cell, and then hits.
 * stats (may be NULL): [0] the points selected after op, [1] the resident points with hit (before OUTSIDE and op),
 * [2] the given points whose near bit is set (0 when near_words is NULL), [3] the non-finite given points.  With
 * RTR_NEAR_GIVEN_ONLY [0] = [1] = 0.  All four are exact and independent of the form of the cloud.
 * What it reads and leaves alone: section 6f's list.  The call reads the uploaded coordinates only; the context's clip
 * planes and keep mask are ignored.  It changes no frame, frame buffer, tile store, pool, statistics, point-pass buffer
 * or keep mask, and an open peer-to-peer exchange stays open.  Indices are the point pass's; a cloud sorted by the
 * library needs option "point_ids" = 1 -- but not with RTR_NEAR_GIVEN_ONLY, which needs no upload index: near bits go by
 * given index.  A sharded context works on its own points.
 * Ordering: as section 6h.  Queued on the context's stream behind everything issued before it; the call ALWAYS waits
 * for its own work before it returns, stats or not: it frees its scratch (and it waits once on the way, for the given
 * points' counters and bounding box).  It does not repeat frames whose extent pool overflowed.
 * Memory and cost: set by the GIVEN points.  They are keyed, sorted (a stable radix sort of count (64-bit key, 32-bit
 * index) pairs) and gathered into 16-byte records in cell order; the resident cloud is neither sorted nor gathered.
 * Scratch for the duration of the call: 56 B per GIVEN point (the pairs and the records, twice each), the sort's
 * temporary, a copy of a host array at its stride, plus (n + 31) / 32 hit words, plus (count + 31) / 32 near words
 * (rounded up to 8 per 256): nothing is proportional to n beyond the hit words.  One sweep over the resident chunks: a
 * chunk of 256 points whose box, grown by a cell, does not meet the given points' bounding box, or whose cells have no
 * given point in or next to them (up to 64 cell columns looked up in the sorted keys), is decided on its header and
 * never decoded; the work is proportional to the chunks near a given point and to the candidate pairs tested.  A
 * decoded chunk is tested against the given points of the cells around its box, 64 at a time, leaving out the cells
 * that lie more than one cell from all four points of every lane (up to 4096 cell columns).  Without near_words a
 * wave stops testing a chunk once all its points hit; with near_words every candidate pair is tested, because the given
 * side needs them.  A pile of m coincident given points next to a chunk costs O(256 m) pair tests, a pile on both sides
 * O(pile x candidates), as in section 6h; so does a radius far larger than the point spacing.  Chunks without a box (a
 * non-finite coordinate among their points, or -- packed -- mixed signs on more than one axis without a box word) and
 * chunks whose box covers more than 4096 cell columns take a slower per-point path.
 * Option keys, read by rtr_get_option after a call: "near_given_us" (key, sort and gather of the given points),
 * "near_sweep_us" (the resident sweep, combine and count), "near_pair_tests_k" (pair tests in thousands),
 * "near_chunks_skipped" (chunks decided without reading their coordinates) and "near_chunks_decoded";
 * near_chunks_skipped + near_chunks_decoded = (n + 255) / 256.
 * Errors, with nothing changed (the selection, the option "selection", near_words and stats): no cloud, a radius that
 * is not finite and > 0, an r2 that is not a finite normal fp32 number, xyz NULL with count > 0, a stride below 12 or
 * not a multiple of 4, unknown bits in flags, an unknown op, RTR_NEAR_GIVEN_ONLY with op != 0 or near_words NULL, a
 * sorted cloud without point_ids (unless RTR_NEAR_GIVEN_ONLY) -> RTR_ERR_INVALID; n or count >= 2^32, or a finite given
 * point beyond the span -> RTR_ERR_UNSUPPORTED; a failed allocation -> RTR_ERR_HIP.  Every scratch buffer is allocated,
 * and every check that can fail is made, before the first selection word changes. */
#define RTR_NEAR_GIVEN_ONLY 1   /* flags: only near_words and stats[2..3]; the selection is neither read, changed nor created */
int rtr_select_near(rtr_ctx *ctx, const float *xyz, size_t xyz_stride_bytes, uint64_t count, float radius,
                    int flags, int op, uint32_t *near_words, uint64_t stats[4]);

/* ---- 6l. the nearest resident point to each given point: which one, and how far ----------------------------------------
 * rtr_nearest_points answers what section 6k's bits cannot: for every GIVEN point the resident point closest to it within
 * `radius` and its squared distance, and, the other way round, for every resident point the closest given one -- the
 * correspondences of a scan registered against the map (with rtr_transform_points: one ICP step), cloud-to-cloud distance
 * and change detection with a magnitude, colouring or labelling a scan from the map, snapping picked coordinates to real
 * returns.  Everything it shares with rtr_select_near is section 6k's; only the differences are spelled out here.
 * Given points: exactly as in section 6k -- strides, host or device memory, the span rule, non-finite points.  count == 0
 * is legal: xyz may then be NULL.
 * Relation: section 6k's.  d2 = ((dx*dx + dy*dy) + dz*dz), every operation rounded to fp32 on its own (no FMA); a pair
 * is a CANDIDATE iff d2 <= r2, inclusive, r2 = radius * radius rounded once to fp32 on the host.  numpy float32 in that
 * order is a bit-for-bit reference, nothing has a tolerance.  `radius` is the search bound (ICP's maximum correspondence
 * distance), and the reason section 6k's sweep applies: a chunk nowhere near a given point is never decoded.
 * Given side: given_index[j] = the upload index of the resident point with the smallest d2 among the candidates of given
 * point j; of several candidates with the same d2 bits, the smallest upload index wins.  given_dist2[j] = that d2, bit
 * for bit: subnormal values are kept as they are (the kernels do not flush denormals), a coincident point gives +0.  A
 * given point with no candidate -- every non-finite one among them -- gets RTR_NEAREST_NONE and +inf (0x7F800000).  EVERY
 * resident point counts, as in section 6k: the keep mask, the clip planes and the selection are ignored.
 * Resident side: resident_index[i] = the given index with the smallest d2 among the candidates of resident point i, ties
 * to the smallest given index; resident_dist2[i] = that d2.  A resident point with no candidate gets RTR_NEAREST_NONE
 * and +inf; so does one more than a cell beyond the span, by section 6k's rule.  Both arrays hold n entries and are
 * indexed by UPLOAD index.
 * Outputs: each of the four pointers may be NULL on its own; all four NULL is legal (stats only; both sides are computed
 * all the same).  Each is host or device memory, told apart as section 6k tells near_words.  They are written only when
 * the call succeeds.  n and count are below 2^32, so RTR_NEAREST_NONE is never a real index.
 * Coordinates are not returned: the library keeps no map from upload to resident index, and the 64 bits of the atomic
 * that decides a given point's winner hold a distance and an index and nothing more.  Gather them with
 * rtr_extract_points from the winning indices (rtr_project_cloud.hpp: matchPoints does).
 * flags must be 0.
 * stats (may be NULL): [0] the given points that have a nearest, [1] the resident points that have one, [2] the
 * non-finite given points, [3] 0.  All are exact and independent of the form of the cloud; [0] equals rtr_select_near's
 * stats[2] for the same arguments (with near_words), [1] its stats[1].
 * Independence: the results depend on the coordinates and on the upload and given indices alone -- not on the resident
 * order, the library's sort, the packed form, any option, the internal grid or the order of the given points: when the
 * given points are permuted, the given outputs permute with them (and the resident indices map through the permutation).
 * What it reads and leaves alone: section 6k's list, and the selection besides, which is neither read, changed nor
 * created.  The call reads the uploaded coordinates only; it changes no frame, frame buffer, tile store, pool,
 * statistics, point-pass buffer or keep mask, and an open peer-to-peer exchange stays open.  Indices are the point pass's:
 * a cloud sorted by the library needs option "point_ids" = 1.  A sharded context works on its own points.
 * Ordering: as section 6k.  Queued on the context's stream behind everything issued before it; the call ALWAYS waits for
 * its own work before it returns (and once on the way, for the given points' counters and bounding box).
 * Memory and cost: section 6k's sweep without its early exit -- every chunk near a given point is tested against every
 * candidate around it --, keeping a minimum where section 6k ORs a bit: per tile of 64 candidates one 64-bit atomic
 * minimum per candidate that some point of the chunk accepted.  Scratch for the duration of the call: section 6k's 56 B
 * per given point, the sort's temporary and the copy of a host array, plus 8 B per GIVEN point for the given slots (and
 * 4 B per given point and given output asked for), plus 8 B per RESIDENT point only when a resident output is asked for
 * (the caller's arrays change only on success, so the kernel writes a scratch copy).  Everything is allocated before
 * anything is written.
 * Option keys, read by rtr_get_option after a call: "nearest_given_us", "nearest_sweep_us" (with the unpacking of the
 * given side), "nearest_pair_tests_k", "nearest_chunks_skipped" and "nearest_chunks_decoded";
 * nearest_chunks_skipped + nearest_chunks_decoded = (n + 255) / 256.
 * Errors, with nothing changed (the four outputs and stats): no cloud, a radius that is not finite and > 0, an r2 that
 * is not a finite normal fp32 number, xyz NULL with count > 0, a stride below 12 or not a multiple of 4, flags != 0, a
 * sorted cloud without point_ids -> RTR_ERR_INVALID; n or count >= 2^32, or a finite given point beyond the span ->
 * RTR_ERR_UNSUPPORTED; a failed allocation -> RTR_ERR_HIP. */
#define RTR_NEAREST_NONE 0xFFFFFFFFu   /* the index of "no point within radius" */
int rtr_nearest_points(rtr_ctx *ctx, const float *xyz, size_t xyz_stride_bytes, uint64_t count, float radius, int flags,
                       uint32_t *given_index, float *given_dist2,        /* count entries each, or NULL */
                       uint32_t *resident_index, float *resident_dist2,  /* n entries each, upload order, or NULL */
                       uint64_t stats[4]);

/* ---- 6m. the k nearest resident points to each given point ---------------------------------------------------------------
 * rtr_nearest_k_points is section 6l's given side with k answers per given point in place of one: the input of normal
 * and curvature estimation (PCA over k neighbours), of the statistical outlier filter (mean distance to k neighbours),
 * of local density, of colouring a scan from several map points.  It runs section 6k's sweep: a chunk nowhere near a
 * given point is never decoded.
 * Section 6l's rules apply unchanged to: the given points (strides, host or device memory, the span rule, non-finite
 * points; count == 0 is legal); the relation (fp32 ((dx*dx + dy*dy) + dz*dz) <= r2, inclusive, no FMA, denormals kept);
 * EVERY resident point counts; the independence from the resident order, the library's sort, the packed form, any
 * option, the internal grid and the order of the given points (the rows permute with them); what the call reads and
 * leaves alone; the ordering (the call ALWAYS waits for its own work); "point_ids" = 1 for a cloud sorted by the library.
 * Row j of `index` and `dist2` (k entries each, at [j * k]): the CANDIDATES of given point j in ascending order of (d2
 * bits, upload index), the first min(k, candidates) of them; the remaining entries of the row are RTR_NEAREST_NONE and
 * +inf (0x7F800000).  found[j] = the number of real entries of row j.  numpy float32 plus a stable sort on (bits, index)
 * is a bit-for-bit reference; nothing has a tolerance.  With k = 1 the row equals rtr_nearest_points' given_index[j] and
 * given_dist2[j] bit for bit.
 * Self queries: a given point coincident with a resident one is its own neighbour at +0.  For the k neighbours of the
 * resident points themselves: extract them (rtr_extract_points), ask for k + 1, and drop from each row the entry whose
 * index is the point's own -- not the row's first entry: a coincident duplicate with a smaller upload index sorts before
 * the point itself.
 * There is no resident side: it would be n * k entries, and section 6l serves k = 1 there.
 * k is 1 .. RTR_NEAREST_MAX_K.  flags must be 0.  Each of the three outputs may be NULL on its own; all three NULL is
 * legal (stats only).  Each is host or device memory, told apart as in section 6l.  Outputs and stats are written only
 * when the call succeeds.
 * stats (may be NULL): [0] the given points with found > 0 (= rtr_select_near's stats[2] for the same arguments), [1] the
 * sum of found, [2] the non-finite given points, [3] the given points with found == k.  All four are exact and
 * independent of the form of the cloud.
 * Memory and cost: section 6l's sweep; every given point has a ROW of k 64-bit slots, and an accepted pair's key walks
 * the row by returning 64-bit atomic minima, each slot keeping the smaller and passing the larger on, so that the row
 * ends sorted for any interleaving: no lock, no retry, no wave waiting for another.  A key that does not beat the row's
 * last slot is dropped unread.  Scratch for the duration of the call: section 6k's 56 B per given point, the sort's
 * temporary and the copy of a host array, plus 8 * k B per given point for the rows, plus a staging copy of every output
 * that lies in host memory (4 * k B per given point for index and for dist2, 4 B for found).  Everything is allocated
 * before anything is written.
 * Option keys, read by rtr_get_option after a call: "nearest_k_given_us", "nearest_k_sweep_us" (with the unpacking),
 * "nearest_k_pair_tests_k", "nearest_k_chunks_skipped" and "nearest_k_chunks_decoded" (their sum is (n + 255) / 256), and
 * "nearest_k_cascades_k", the row insertions started, in thousands: it depends on timing, not on the inputs alone.
 * Errors, with nothing changed (the three outputs and stats): section 6l's list as it is -- no cloud, a radius that is
 * not finite and > 0, an r2 that is not a finite normal fp32 number, xyz NULL with count > 0, a stride below 12 or not a
 * multiple of 4, flags != 0, a sorted cloud without point_ids -> RTR_ERR_INVALID; n or count >= 2^32, or a finite given
 * point beyond the span -> RTR_ERR_UNSUPPORTED; a failed allocation -> RTR_ERR_HIP --, and k == 0 or
 * k > RTR_NEAREST_MAX_K -> RTR_ERR_INVALID.  rtr_last_error names the argument. */
#define RTR_NEAREST_MAX_K 64
int rtr_nearest_k_points(rtr_ctx *ctx, const float *xyz, size_t xyz_stride_bytes, uint64_t count, float radius,
                         uint32_t k, int flags,
                         uint32_t *index, float *dist2,   /* count * k entries each, row j at [j * k], or NULL */
                         uint32_t *found,                 /* count entries, or NULL */
                         uint64_t stats[4]);

/* ---- 7. measurement -------------------------------------------------------------- */
typedef enum {
    RTR_K_CLEAR = 0, RTR_K_MIN_DEPTH = 1, RTR_K_ACCUMULATE = 2, RTR_K_RESOLVE = 3, RTR_K_FILTER = 4,
    RTR_K_PROBE = 5, RTR_K_TILE = 6, RTR_K_BIN = 7, RTR_K_COUNT = 8
} rtr_kernel_id;
/* mode 1: RTR_K_MIN_DEPTH = streaming projection + append to the tile streams (T1), RTR_K_TILE =
 * per-tile z-buffer (T4); RTR_K_BIN is unused since the tile sort was removed (kept for ABI
 * stability); RTR_K_CLEAR / ACCUMULATE / RESOLVE are then only used by the phase calls. */
/* Read-only probe: same loads and projection arithmetic as the point passes, no frame-
 * buffer traffic -- measures the streaming ceiling of the access pattern. */
int rtr_stream_probe(rtr_ctx *ctx, const float P[16]);
/* on = 1: every phase is bracketed by hipEvents on the context's stream; on = 2: only the
 * streaming point kernels (RTR_K_MIN_DEPTH, RTR_K_ACCUMULATE), i.e. two event records per
 * frame; on = 3: like 2 but only every 4th launch is bracketed (a bracket costs ~8 us of stream
 * time, 3 % of a frame), on = 4: every 2nd; 0: off.  The tile-binned form's RTR_K_MIN_DEPTH launch carries its two
 * events in the dispatch itself (start / stop stamps of that kernel: no extra packets, but a timed
 * dispatch still costs ~10 us of stream time).  rtr_timing_get synchronises and returns the
 * accumulated device time and the number of bracketed launches. */
int rtr_timing_enable(rtr_ctx *ctx, int on);
/* Statistics of the last binned frame (mode 1; synchronises the stream): out[0] work items of the
 * tile kernel, [1] of them slices of split tiles, [2] in-frustum entries, [3] entries of the
 * heaviest tile, [4] slice size used, [5] tile-store error bits of THAT frame's point kernel (0 = none; 1 = an extent
 * never appeared, 2 = the extent pool overflowed: entries were dropped; the tile kernels' own bits -- 4 = a contested
 * tile of an owner-computes sharded frame had more stream pieces than its table holds, 8 = the split tiles' second
 * phase gave up waiting for the first -- go straight to the word every synchronising call checks and surface there
 * as RTR_ERR_INTERNAL), [6] split tiles, [7] 256-point chunks with
 * at least one in-frustum point (each loads 1 KiB of colours). */
int rtr_frame_stats(rtr_ctx *ctx, uint32_t out[8]);
int rtr_timing_reset(rtr_ctx *ctx);
int rtr_timing_get(rtr_ctx *ctx, int kernel, double *total_ms, uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* RTR_H */
