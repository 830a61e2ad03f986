// rtr_api.hip -- the C ABI of include/rtr.h on top of the gfx950 kernels.
//
// Host orchestration that replaces project_cloud.cu:189-434: the cloud stays
// resident in HBM as SoA, frame buffers and all pyramid levels are allocated once
// per resolution (the reference mallocs/frees 12 buffers per filtered frame,
// project_cloud.cu:346-390), every launch goes to one stream with no device-wide
// synchronisation in between (the reference calls cudaDeviceSynchronize ten times
// per frame), and the camera matrix travels as a kernel argument.
// The selection and analysis calls (rtr.h sections 6f - 6k) are in rtr_select_api.hip;
// rtr_host.h holds what both files share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "rtr_host.h"
#include "rtr_extract_index.h"

constexpr int kSplitCooldown = 8;  // whole frames keep launching k_tile_split this long after the last report of a tile above the threshold

static thread_local std::string g_create_err;

int fail(rtr_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_err = buf;
    return code;
}

namespace {

template <class T>
void dfree(T *&p) {
    (void)rtr::dev_free(p);
    p = nullptr;
}

void p2p_release(rtr_ctx *c) {  // the peers' mappings and this rank's exchange buffers
    auto &q = c->p2p;
    for (auto &kind : q.opened)
        for (auto &ptr : kind) {
            if (ptr) (void)hipIpcCloseMemHandle(ptr);
            ptr = nullptr;
        }
    dfree(q.red);
    dfree(q.ximg);
    dfree(q.flags);
    dfree(q.occ);
    dfree(q.occ_all);
    dfree(q.tab);
    q.open = false;
    q.world = 0;
    q.seq = q.start = 0;
}

struct Slice { size_t chunk, first, count; };
Slice p2p_slice(const rtr_ctx *c) {  // pixels owned by this rank: slices are multiples of 16 pixels
    const size_t npix = (size_t)c->W * c->H, w = (size_t)c->p2p.world;
    Slice s;
    s.chunk = (((npix + w - 1) / w) + 15) & ~(size_t)15;  // 16 pixels: 64 B of depth, 48 B of image
    s.first = s.chunk * (size_t)c->p2p.rank;
    if (s.first > npix) s.first = npix;
    s.count = (npix - s.first) < s.chunk ? npix - s.first : s.chunk;
    return s;
}
void free_host_out(rtr_ctx *c) {
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (auto &h : c->ho) {
        (void)rtr::host_free(h.img);
        (void)rtr::host_free(h.depth);
        dfree(h.dimg); dfree(h.ddepth);
        if (h.snap) (void)hipEventDestroy(h.snap);
        if (h.done) (void)hipEventDestroy(h.done);
        h = rtr_ctx::HostOut{};
    }
}

hipError_t sync_streams(rtr_ctx *c);

// One zeroed word of pinned host memory that the device writes through its mapping (error bits, statistics)
hipError_t mapped_word(uint32_t **host, uint32_t **dev) {
    hipError_t e = rtr::host_malloc(host, sizeof(uint32_t), hipHostMallocMapped);
    if (e != hipSuccess) {
        *host = nullptr;
        return e;
    }
    **host = 0u;
    void *d = nullptr;
    e = hipHostGetDevicePointer(&d, *host, 0);
    *dev = static_cast<uint32_t *>(d);
    if (e != hipSuccess) {
        (void)rtr::host_free(*host);
        *host = nullptr;
    }
    return e;
}

void free_target(rtr_ctx::Target &t) {  // the frame buffers and pyramid levels (the stores, pools and words stay)
    dfree(t.depth); dfree(t.acc); dfree(t.img); dfree(t.mask); dfree(t.part_min); dfree(t.part_max); dfree(t.tensor);
    for (auto &l : t.lv) dfree(l);
    t.lv_levels = 0;
    t.cap = 0;
}

// Frame buffers for `count` frames at the current resolution, all or nothing: after a failure the target holds none
int alloc_target(rtr_ctx *c, rtr_ctx::Target &t, int count) {
    free_target(t);
    const size_t npix = (size_t)c->W * c->H, n = (size_t)count * npix;
    const size_t nparts = (size_t)((c->W + 31) / 32) * ((c->H + 31) / 32);
    hipError_t e = rtr::dev_malloc(&t.depth, n * 4);
    if (e == hipSuccess) e = rtr::dev_malloc(&t.img, (n * 3 + 15) & ~(size_t)15);
    if (e == hipSuccess) e = rtr::dev_malloc(&t.tensor, n * 5 * sizeof(uint16_t));
    if (e == hipSuccess) e = rtr::dev_malloc(&t.acc, npix * 16);
    if (e == hipSuccess) e = rtr::dev_malloc(&t.mask, npix);
    if (e == hipSuccess) e = rtr::dev_malloc(&t.part_min, nparts * 4);
    if (e == hipSuccess) e = rtr::dev_malloc(&t.part_max, nparts * 4);
    if (e != hipSuccess) {
        free_target(t);
        return fail(c, RTR_ERR_HIP, "hipMalloc of the frame buffers (%d x %dx%d) failed: %s", count, c->W, c->H,
                    hipGetErrorString(e));
    }
    t.cap = count;
    return RTR_OK;
}

void free_frame(rtr_ctx *c) {
    c->list_valid = false;
    c->split_cooldown = kSplitCooldown;  // (a new resolution: nothing is known about its frames)
    free_host_out(c);
    p2p_release(c);
    dfree(c->pp_ids);
    for (auto *t : {&c->frame, &c->views}) {
        free_target(*t);
        for (auto &f : t->fs) {
            dfree(f.store.ext0); dfree(f.store.meta);
            f.nst = f.ntiles = 0;
            f.consts = rtr::StoreConsts{};
        }
    }
    c->W = c->H = 0;
    c->jr.views.count = 0;
}

void reset_pool_sizing(rtr_ctx::Target &t) {  // a new cloud: the adaptive extent pools start over
    t.pool_worst = false;
    t.entries_max = 0;
    if (t.entries_host) *t.entries_host = 0u;
}

void free_lists(rtr_ctx *c) {  // the dynamic extent pools (sized by the point count)
    if (c->p2p.open || c->p2p.red) p2p_release(c);  // (the peers map this rank's pool: they must re-open after a new cloud)
    for (auto *t : {&c->frame, &c->views})
        for (auto &f : t->fs) {
            dfree(f.dyn);
            f.dyn_cap = 0;
            f.pool_n = 0;
        }
    c->list_valid = false;
    c->split_cooldown = kSplitCooldown;  // (a new cloud)
    reset_pool_sizing(c->frame);
    reset_pool_sizing(c->views);
    c->jr.frame.count = 0;
    c->jr.views.count = 0;
}

void free_pack(rtr_ctx *c) {
    dfree(c->pk_hdr); dfree(c->pk_planes);
    c->pk_planes_b = nullptr;
    c->pk_bytes = 0;
    c->pk_units = c->pk_units_cap = c->pk_hdr_chunks = 0;
}

void free_keep(rtr_ctx *c) {
    dfree(c->keep_up); dfree(c->keep_res); dfree(c->keep_sum);
}

void free_cloud(rtr_ctx *c) {
    free_keep(c);
    free_select(c);
    dfree(c->x); dfree(c->y); dfree(c->z); dfree(c->rgba); dfree(c->bounds); dfree(c->spread); dfree(c->perm);
    dfree(c->pp_vis);
    c->pp_vis_words = 0;
    free_pack(c);
    free_lists(c);
    c->n = c->cap = 0;
}

// Tile store of frame k of a target, s: the stream T1 will run on.  Per resolution: a static 32 KB extent, a stream
// length, an extent directory per 32x16 storage tile, and the tile kernel's work list.  Then the header constants:
// the buffers T1's last workgroup resets for split tiles / writes the occupancy bitmap to, the dynamic extent pool,
// the mapped words, the split parameters (uploaded only when one of them changes).
int ensure_store(rtr_ctx *c, rtr_ctx::Target &t, rtr_ctx::FrontSet &f, int k, hipStream_t s) {
    const bool single = &t == &c->frame;
    const int nt = rtr::tile_count(c->W, c->H), nst = rtr::storage_tile_count(c->W, c->H);
    auto &st = f.store;
    if (!(st.ext0 && f.nst == nst && f.ntiles == nt)) {
        if (single) c->list_valid = false;
        dfree(st.ext0); dfree(st.meta);
        f.nst = f.ntiles = 0;
        f.consts = rtr::StoreConsts{};
        f.lean_pending = false;
        const size_t meta_bytes = rtr::ts_meta_words(nst, nt) * sizeof(uint32_t);
        // (+ 16 entries of slack: the tile kernel's sweeps read a few entries past the piece they are masking)
        // (ext0 and meta stand or fall together: after a failure the set holds neither, and f.nst == 0 sends the next
        // frame through here again)
        hipError_t e = rtr::dev_malloc(&st.ext0, ((size_t)nst * rtr::kS0 + 16) * sizeof(uint64_t));
        if (e == hipSuccess) e = rtr::dev_malloc(&st.meta, meta_bytes);
        if (e != hipSuccess) {
            dfree(st.ext0); dfree(st.meta);
            return fail(c, RTR_ERR_HIP, "allocating the tile store (%d storage tiles) failed: %s", nst, hipGetErrorString(e));
        }
        HIP_TRY(c, hipMemsetAsync(st.meta, 0, meta_bytes, s));  // stream lengths 0, directory stamps 0 (never current)
        st.seq = c->debug_store_stamp;  // (0 unless option "debug_store_stamp" was set)
        st.nst = f.nst = nst;
        st.ntiles = f.ntiles = nt;
        {   // launch order of the tile kernel: identity until a frame has been rendered
            std::vector<uint32_t> ident((size_t)nt);
            for (int i = 0; i < nt; ++i) ident[(size_t)i] = (uint32_t)i;
            HIP_TRY(c, hipMemcpyAsync(rtr::ts_perm(st), ident.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(rtr::ts_order(st, 0), ident.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(rtr::ts_order(st, 1), ident.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipStreamSynchronize(s));  // `ident` goes out of scope
        }
    }
    rtr::StoreConsts want{};
    want.depth = t.depth + (size_t)k * c->W * c->H; want.acc = t.acc; want.occ = c->p2p.open ? c->p2p.occ : nullptr;
    want.dyn = f.dyn; want.dyn_cap = f.dyn_cap;
    if (c->opt_debug_dyn_cap >= 0 && (uint64_t)c->opt_debug_dyn_cap < want.dyn_cap) want.dyn_cap = (uint64_t)c->opt_debug_dyn_cap;
    want.err_host = t.err_dev;
    want.split_host = single ? c->split_dev : nullptr;
    want.entries_host = t.entries_dev;
    want.heavy = single && c->opt_heavy > 0 ? (uint32_t)c->opt_heavy : 0xFFFFFFFFu;  // (views are lean frames: nothing is split)
    want.slice = (uint32_t)c->opt_slice;
    if (memcmp(&want, &f.consts, sizeof want) != 0) {
        f.consts = want;
        HIP_TRY(c, hipMemcpyAsync(rtr::ts_hdr(st) + rtr::kHdrConsts, &f.consts, sizeof f.consts, hipMemcpyHostToDevice, s));
    }
    return RTR_OK;
}

// the store's next 24-bit frame stamp (rtr_stamp_rule.h); when it wraps every directory entry is forgotten once, on
// the stream the frame's point kernel will run on: behind everything that still reads the directory, ahead of that kernel
int next_seq(rtr_ctx *c, rtr_ctx::FrontSet &f, hipStream_t s) {
    auto &t = f.store;
    const rtr::StampStep step = rtr::next_stamp(t.seq);
    if (step.clear) HIP_TRY(c, hipMemsetAsync(rtr::ts_dir(t), 0, rtr::dir_bytes(f.nst), s));
    t.seq = step.stamp;
    return RTR_OK;
}

int t1_flags(const rtr_ctx *c, bool clear_split, bool no_split, bool lean) {  // rtr::launch_project_bin's flag word
    return (clear_split ? 1 : 0) | (no_split ? 2 : 0) | (c->opt_lane_test ? 0 : 4) | (lean ? 8 : 0) | (c->opt_chunk_test ? 0 : 16);
}

// Tile-launch bits of a lean frame (tile_body): bit 5 = no launch order when the launch is resident at once; bit 6 =
// the first batch of entries before the counters, when the tiles are expected full: the entry count of the target's
// last frame whose statistics are complete -- a mapped word, no sync -- is at least half a batch, 1024 entries, per tile
int lean_bits(const rtr_ctx *c, const rtr_ctx::Target &t) {
    int bits = 8 | (c->opt_lean_identity ? 32 : 0);
    const uint64_t e_last = __atomic_load_n(t.entries_host, __ATOMIC_RELAXED);
    if (c->opt_lean_early > 0 || (c->opt_lean_early < 0 && e_last >= 1024ull * (uint64_t)rtr::tile_count(c->W, c->H)))
        bits |= 64;
    return bits;
}

// The dynamic extents of one frame sum to less than twice its entries (every extent doubles its stream,
// rtr_kernels.h), and a frame has at most n entries: 2 n + 64 entries = 16 B per point is the worst case (round 1's
// wave lists + sorted copy: 24).  An ordinary view has a few per cent of the cloud inside the frustum, so the pool is
// sized by the frames this cloud has had: 8 x the most entries a completed frame reported (a mapped host word, read
// without a sync), at least n / 2 and 2^20 -- 4 B per point (n / 4 re-allocated in the middle of BASELINE C2's frames:
// a sync, a free and a malloc cost more than the memory is worth).  A frame whose entries jump past that (the camera suddenly
// sees four times more of the cloud than ever before) overflows the pool, reports it (tile-store error 2), and the next
// synchronising call grows the pool to the worst case and renders the frame again (repair) -- the caller never
// sees it, unless it consumes frames on the stream without ever synchronising: option "pool_worst_case" is for that.
// other_max: entries of the densest frame seen elsewhere that count too (the views': the single frame's).
uint64_t pool_worst_cap(const rtr_ctx *c) { return 2 * c->n + 64; }
uint64_t pool_want_cap(rtr_ctx *c, rtr_ctx::Target &t, uint64_t have, uint64_t other_max) {
    const uint64_t worst = pool_worst_cap(c);
    if (c->opt_pool_worst || t.pool_worst || c->p2p.open) return worst;
    const uint64_t e = __atomic_load_n(t.entries_host, __ATOMIC_RELAXED);
    if (e > t.entries_max) t.entries_max = e;
    const uint64_t emax = t.entries_max > other_max ? t.entries_max : other_max;
    uint64_t floor_ = c->n / 2 > (1ull << 20) ? c->n / 2 : (1ull << 20);
    // (hysteresis: grown to 8 x when the head-room over the densest frame seen falls under 4 x)
    uint64_t want = have >= 4 * emax && have >= floor_ ? have : (8 * emax > floor_ ? 8 * emax : floor_);
    return want < worst ? want : worst;
}
int ensure_pool(rtr_ctx *c, rtr_ctx::Target &t, rtr_ctx::FrontSet &f, uint64_t other_max) {
    const uint64_t want = pool_want_cap(c, t, f.pool_n == c->n ? f.dyn_cap : 0, other_max);
    if (f.dyn && f.pool_n == c->n && f.dyn_cap >= want) return RTR_OK;
    // (the peers map the pool that was EXPORTED -- the single frame's set 0: export / open again after a new cloud.
    // The second set's pool, first allocated by a frame with option "overlap", is nobody else's business)
    if (&f == &c->frame.fs[0] && (c->p2p.open || c->p2p.red)) p2p_release(c);
    HIP_TRY(c, sync_streams(c));  // (frames in flight may still read the old pool)
    dfree(f.dyn);
    if (&t == &c->frame) c->list_valid = false;
    // (the old pool is given back first: the two together may not fit.  The sizes are set behind the allocation they
    // describe: after a failure the set has no pool and says so -- ensure_store copies dyn / dyn_cap into the store's
    // header, and set_overlap and rtr_p2p_export read them -- and the next frame allocates again)
    f.dyn_cap = 0;
    f.pool_n = 0;
    HIP_TRY(c, rtr::dev_malloc(&f.dyn, want * sizeof(uint64_t)));
    f.dyn_cap = want;
    f.pool_n = c->n;
    return RTR_OK;
}

// The fp32 SoA arrays of a cloud that is resident in packed form only (option "keep_soa" = 0, the default): decoded
// from the packed form -- bit for bit, it is lossless -- for the calls that read fp32 coordinates (the atomic form, the
// sort, rtr_download_points, option "pack" = 0, the stream probe).  They stay until the cloud is packed again.
// x, y and z stand or fall together: every reader takes a set c->x to mean three decoded arrays, so after a failed
// allocation the context holds none of them and the cloud stays resident in packed form only, as it was.
hipError_t alloc_xyz(rtr_ctx *c, uint64_t points) {
    hipError_t e = rtr::dev_malloc(&c->x, points * 4);
    if (e == hipSuccess) e = rtr::dev_malloc(&c->y, points * 4);
    if (e == hipSuccess) e = rtr::dev_malloc(&c->z, points * 4);
    if (e != hipSuccess) { dfree(c->x); dfree(c->y); dfree(c->z); }
    return e;
}
int ensure_soa(rtr_ctx *c) {
    if (c->x) return RTR_OK;
    if (!c->pk_hdr || c->cap == 0) return fail(c, RTR_ERR_INTERNAL, "no resident coordinates");
    const hipError_t ea = alloc_xyz(c, c->cap);
    if (ea != hipSuccess) return fail(c, RTR_ERR_HIP, "allocating the fp32 coordinate arrays failed: %s", hipGetErrorString(ea));
    rtr::unpack_to_soa(c->stream, rtr::PackedXyz{c->pk_hdr, c->pk_planes, c->pk_planes_b}, c->n, c->x, c->y, c->z);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {  // (never decoded: they must not pass for coordinates)
        dfree(c->x); dfree(c->y); dfree(c->z);
        return fail(c, RTR_ERR_HIP, "unpack launch failed: %s", hipGetErrorString(e));
    }
    return RTR_OK;
}
void drop_soa(rtr_ctx *c) {  // after the cloud has been packed: 12 B per point back
    if (!c->pk_hdr || c->opt_keep_soa || !(c->x || c->y || c->z)) return;
    (void)sync_streams(c);
    dfree(c->x); dfree(c->y); dfree(c->z);
}

int alloc_cloud(rtr_ctx *c, uint64_t n) {
    uint64_t n_pad = (n + 3) & ~3ull;
    if (n_pad == 0) n_pad = 4;
    if (n_pad > c->cap) {
        // (the old cloud goes first: the two together may not fit.  The six arrays stand or fall together: after a
        // failure the context holds no cloud at all, n = cap = 0 as free_cloud left it -- the callers see to the rest,
        // discard_cloud)
        free_cloud(c);
        hipError_t e = alloc_xyz(c, n_pad);
        if (e == hipSuccess) e = rtr::dev_malloc(&c->rgba, n_pad * 4);
        if (e == hipSuccess) e = rtr::dev_malloc(&c->bounds, ((n_pad / 4 + 63) / 64) * 6 * sizeof(float));
        if (e == hipSuccess) e = rtr::dev_malloc(&c->spread, ((n_pad / 4 + 63) / 64) * sizeof(float));
        if (e != hipSuccess) {
            free_cloud(c);
            return fail(c, RTR_ERR_HIP, "allocating a cloud of %llu points failed: %s", (unsigned long long)n, hipGetErrorString(e));
        }
        c->cap = n_pad;
    }
    if (!c->x) {  // (the previous cloud was resident in packed form only: nothing of it has changed yet, it stays as it was)
        const hipError_t e = alloc_xyz(c, c->cap);
        if (e != hipSuccess) return fail(c, RTR_ERR_HIP, "allocating the fp32 coordinate arrays failed: %s", hipGetErrorString(e));
    }
    if (n != c->n) {  // (the adaptive extent pool starts over; the peers of a sharded frame must map the new one)
        if (c->p2p.open || c->p2p.red) p2p_release(c);
        reset_pool_sizing(c->frame);
    }
    free_keep(c);  // (a new cloud: no mask)
    free_select(c);  // (... and no selection)
    c->n = n;
    ++c->cloud_seq;
    c->list_valid = false;
    c->jr.frame.count = 0;
    c->pp_vis_current = false;
    c->split_cooldown = kSplitCooldown;  // (a new cloud: nothing is known about its frames)
    return RTR_OK;
}

struct Timed {  // brackets one phase with hipEvents on the stream it is launched on
    rtr_ctx *c; int k; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    bool in_dispatch;  // the launch itself carries the two events (hipExtLaunchKernelGGL): nothing to record here
    Timed(rtr_ctx *c_, int k_, hipStream_t s_ = nullptr, bool in_dispatch_ = false)
        : c(c_), k(k_), s(s_ ? s_ : c_->stream), in_dispatch(in_dispatch_) {
        if (!c->timing) return;
        if (c->timing >= 2 && k != RTR_K_MIN_DEPTH && k != RTR_K_ACCUMULATE) return;
        if (c->timing == 3 && (c->timing_tick++ & 3u) != 0u) return;  // a bracket costs ~8-10 us of stream time
        if (c->timing == 4 && (c->timing_tick++ & 1u) != 0u) return;
        if (c->pool.empty()) {
            (void)hipEventCreate(&a); (void)hipEventCreate(&b);
        } else {
            a = c->pool.back().first; b = c->pool.back().second; c->pool.pop_back();
        }
        if (!in_dispatch) (void)hipEventRecord(a, s);
    }
    ~Timed() {
        if (!a) return;
        if (!in_dispatch) (void)hipEventRecord(b, s);
        c->pending.push_back({a, b, k});
    }
};

// everything queued by this context is finished (the tail stream waits for the front stream's
// T1 of every frame it completes, so the order below drains both)
hipError_t sync_streams(rtr_ctx *c) {
    if (c->front) {
        hipError_t e = hipStreamSynchronize(c->front);
        if (e != hipSuccess) return e;
    }
    return hipStreamSynchronize(c->stream);
}

// Which of an overlapped frame's two events ride on a dispatch packet instead of a packet of their own behind the launch
// (bit 0: `consumed` on the tile launch, bit 1: `binned` on T1); an A/B switch of the build, DESIGN.md section 4
#ifndef RTR_DISPATCH_EVENTS
#define RTR_DISPATCH_EVENTS 3
#endif

// the event the LAST reader of the active store -- one about to be launched on the tail stream -- signals from its
// dispatch packet, or null where mark_consumed has to record it: only whole overlapped frames (rtr_render) ask
hipEvent_t consumed_in_dispatch(rtr_ctx *c) {
    if (!(RTR_DISPATCH_EVENTS & 1) || !c->front || !c->frame_overlapped) return nullptr;
    return c->F().consumed;
}

// after the last reader of the active list / bin set has been queued on the tail stream
// (with option "overlap" = 1 behind every reader, as ever; otherwise only behind overlapped frames -- a streak starts
// by joining the two streams, bin_points).  in_dispatch: that reader's launch carried the event (consumed_in_dispatch)
void mark_consumed(rtr_ctx *c, bool in_dispatch = false) {
    if (!c->front || !(c->ov.mode == 1 || c->frame_overlapped)) return;
    auto &f = c->F();
    if (in_dispatch || hipEventRecord(f.consumed, c->stream) == hipSuccess) f.consumed_valid = true;
}

int collect_timing(rtr_ctx *c) {
    if (c->pending.empty()) return RTR_OK;
    HIP_TRY(c, sync_streams(c));
    for (auto &s : c->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
            c->total_ms[s.k] += ms;
            c->launches[s.k] += 1;
        }
        c->pool.emplace_back(s.a, s.b);
    }
    c->pending.clear();
    return RTR_OK;
}

int check_frame(rtr_ctx *c) {
    NEED(c, c->W > 0 && c->H > 0, "rtr_set_resolution has not been called");
    return RTR_OK;
}

// The prefilter's conditions, checked before anything changes
int check_prefilter(rtr_ctx *c) {
    const int L = c->prm.levels;
    if (L < 1 || L > 8) return fail(c, RTR_ERR_UNSUPPORTED, "levels must be in 1..8");
    if ((c->W % (1 << L)) != 0 || (c->H >> L) < 1)
        return fail(c, RTR_ERR_UNSUPPORTED,
                    "prefilter needs W %% 2^levels == 0 and H >= 2^levels (got %dx%d, levels %d): the reference's "
                    "pyramid strides are only defined then (project_cloud.cu:39,336-362)", c->W, c->H, L);
    return RTR_OK;
}

int ensure_levels(rtr_ctx *c, rtr_ctx::Target &t) {  // the pyramid levels 1..levels a target's frames take in turn
    const int L = c->prm.levels;
    if (t.lv_levels == L) return RTR_OK;
    for (auto &l : t.lv) dfree(l);
    t.lv_levels = 0;
    // (all or nothing: lv_levels, which is what says the levels exist, is set behind the last of them, and after a
    // failure none is kept -- the next filtered frame starts over)
    for (int i = 1, w = c->W / 2, h = c->H / 2; i <= L; ++i, w /= 2, h /= 2) {
        const hipError_t e = rtr::dev_malloc(&t.lv[i], sizeof(float) * (size_t)w * h);
        if (e != hipSuccess) {
            for (auto &l : t.lv) dfree(l);
            return fail(c, RTR_ERR_HIP, "allocating pyramid level %d (%dx%d) failed: %s", i, w, h, hipGetErrorString(e));
        }
    }
    t.lv_levels = L;
    return RTR_OK;
}

int ensure_pyramid(rtr_ctx *c) {
    if (int rc = check_prefilter(c)) return rc;
    return ensure_levels(c, c->frame);
}

rtr::FilterLevels levels_of(const rtr_ctx *c, const rtr_ctx::Target &t, int k) {  // frame k's pyramid
    rtr::FilterLevels L{};
    L.levels = t.lv_levels;
    L.lv[0] = reinterpret_cast<float *>(t.depth + (size_t)k * c->W * c->H);
    L.w[0] = c->W; L.h[0] = c->H;
    for (int i = 1; i <= L.levels; ++i) L.lv[i] = t.lv[i], L.w[i] = L.w[i - 1] / 2, L.h[i] = L.h[i - 1] / 2;
    return L;
}

// what a tile launch needs to emit frame k's prefilter pyramid and min / max partials (when `enable`)
rtr::TilePyr tile_pyr(const rtr_ctx *c, const rtr_ctx::Target &t, int k, bool enable) {
    rtr::TilePyr pyr{};
    pyr.enable = enable ? 1 : 0;
    if (enable) {
        pyr.L = levels_of(c, t, k);
        pyr.n_eff_rows = (uint32_t)((c->H >> 4) << 4);
        pyr.part_min = t.part_min;
        pyr.part_max = t.part_max;
    }
    return pyr;
}

}  // namespace

// ---- shared with rtr_select_api.hip (declared in rtr_host.h) -------------------------------------------------------
void free_select(rtr_ctx *c) {
    if (!c->sel) return;
    (void)sync_streams(c);  // (a selection in flight may still write it)
    dfree(c->sel); dfree(c->sel_stats);
}

rtr::Proj make_proj(const float P[16]) {
    rtr::Proj p;
    for (int i = 0; i < 12; ++i) p.m[i] = P[i];
    return p;
}

rtr::Cloud cloud_of(const rtr_ctx *c) {
    // (a chunk of 256 points spanning more than half of the cloud: consecutive points are unrelated.  A hash-ordered
    // cloud measures ~1.0; the reference loader's 0.25 m blocks in hash-map order, unordered inside, measure 0.28 for a
    // 10 m room and must keep the wave-level claim groups: 0.33 ms instead of 0.66 ms per frame without them)
    return rtr::Cloud{c->x, c->y, c->z, c->rgba, c->n, c->opt_grid, (!c->reordered && c->order_ratio > 0.5f) ? 1 : 0,
                      rtr::PackedXyz{c->pk_hdr, c->pk_planes, c->pk_planes_b}, c->spread, {c->absmax[0], c->absmax[1], c->absmax[2]},
                      c->clip, rtr::Keep{c->keep_up ? c->keep_res : nullptr, c->keep_sum}};
}

int launch_check(rtr_ctx *c, const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, RTR_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return RTR_OK;
}

hipError_t d2d(hipStream_t s, void *dst, const void *src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
}

// Where a caller's array lies (rtr_extract_points, rtr_write_points: each stream may be host or device memory)
bool on_device(const void *p) {  // device (or managed) memory, as opposed to anything the host owns
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // (plain host memory is unknown to the runtime)
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

int need_upload_order(rtr_ctx *c, const char *verb, const char *or_else) {
    if (!c->reordered || c->perm) return RTR_OK;
    return fail(c, RTR_ERR_INVALID, "the resident cloud was reordered without option point_ids = 1, so upload-order indices "
                "cannot be %s: set point_ids = 1 before the upload (or upload with auto_reorder = 0)%s", verb, or_else);
}

static int set_overlap(rtr_ctx *c, int value);
static void overlap_teardown(rtr_ctx *c);

extern "C" {

int rtr_abi_version(void) { return RTR_ABI_VERSION; }

void rtr_default_params(rtr_params *p) {
    if (!p) return;
    p->depth_window = 0.02f;        // render.cu:106
    p->filter_strength = 1.025f;    // project_cloud.cu:24
    p->gradient_threshold = 0.03f;  // project_cloud.cu:25
    p->levels = 4;                  // project_cloud.cu:23
}

int rtr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int rtr_create(rtr_ctx **out, int device) {
    if (!out) return fail(nullptr, RTR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, RTR_ERR_HIP, "no HIP device available (%s): this library has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= ndev) return fail(nullptr, RTR_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    rtr_ctx *c = new rtr_ctx();
    c->device = device;
    rtr_default_params(&c->prm);
    DevGuard g(device);
    e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        int rc = fail(nullptr, RTR_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
        delete c;
        return rc;
    }
    c->stream = c->own_stream;
    c->split_cooldown = kSplitCooldown;
    c->ov.set_mode(-1);
    // (the minmax words serve RTR_BUF_MINMAX before any resolution is set)
    e = mapped_word(&c->split_host, &c->split_dev);
    for (auto *t : {&c->frame, &c->views}) {
        if (e == hipSuccess) e = rtr::dev_malloc(&t->minmax, RTR_MAX_VIEWS * 2 * sizeof(uint32_t));
        if (e == hipSuccess) e = mapped_word(&t->err_host, &t->err_dev);
        if (e == hipSuccess) e = mapped_word(&t->entries_host, &t->entries_dev);
    }
    if (e != hipSuccess) {
        int rc = fail(nullptr, RTR_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(e));
        (void)rtr_destroy(c);
        return rc;
    }
    *out = c;
    return RTR_OK;
}

int rtr_destroy(rtr_ctx *c) {
    if (!c) return RTR_OK;
    DevGuard g(c->device);
    (void)sync_streams(c);
    (void)collect_timing(c);
    overlap_teardown(c);
    for (auto &p : c->pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    free_frame(c);
    free_cloud(c);
    for (auto *t : {&c->frame, &c->views}) {
        dfree(t->minmax);
        (void)rtr::host_free(t->err_host);
        (void)rtr::host_free(t->entries_host);
    }
    (void)rtr::host_free(c->p2p.status_host);
    (void)rtr::host_free(c->split_host);
    (void)rtr::host_free(c->vtab.host);
    dfree(c->vtab.dev);
    if (c->vtab.copied) (void)hipEventDestroy(c->vtab.copied);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->pp_done) (void)hipEventDestroy(c->pp_done);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return RTR_OK;
}

const char *rtr_last_error(const rtr_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int rtr_set_params(rtr_ctx *c, const rtr_params *p) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, p != nullptr, "params is NULL");
    NEED(c, p->levels >= 1 && p->levels <= 8, "levels must be in 1..8");
    c->prm = *p;
    c->list_valid = false;
    return RTR_OK;
}

// Option "overlap": whole-frame renders put T1 on a second stream and alternate between two tile stores and extent
// pools, so the point kernel of frame k+1 -- a latency chain whose wave slots drain from a quarter of its run on --
// runs beside the tile kernel and prefilter of frame k.  1: every whole frame that can; -1: by the streak of whole
// frames (rtr_overlap_policy.h); 0: never, and the second store and pool are given back.
// The front stream has the default priority: created with the lowest one, so that the context's or caller's stream wins
// dispatch, T1 ends later and the tile kernel gains nothing ("Overlap"; option "front_priority").
// With "tail_cus" = t > 0 (and "overlap" = 1) the two streams get disjoint CU masks instead (t CUs of every XCD for
// the tail, the rest for T1) so neither takes the other's wave slots.  The bit -> CU mapping of a
// mask is not documented for 8-XCD parts (XCD-interleaved or XCD-blocked); the pattern below
// gives every XCD exactly t tail CUs under both numberings.
static void overlap_teardown(rtr_ctx *c) {  // (both streams idle)
    if (c->masked_tail && c->stream == c->masked_tail) c->stream = c->own_stream;
    if (c->front) (void)hipStreamDestroy(c->front);
    if (c->masked_tail) (void)hipStreamDestroy(c->masked_tail);
    c->front = c->masked_tail = nullptr;
    for (auto &f : c->frame.fs) {
        if (f.binned) (void)hipEventDestroy(f.binned);
        if (f.consumed) (void)hipEventDestroy(f.consumed);
        f.binned = f.consumed = nullptr;
        f.consumed_valid = false;
    }
    if (c->joined) (void)hipEventDestroy(c->joined);
    c->joined = nullptr;
}

// the front stream and the events of the single frame's two sets, created once and kept (all or nothing)
static hipError_t overlap_streams(rtr_ctx *c) {
    if (c->front) return hipSuccess;
    hipError_t e = hipSuccess;
    if (c->ov.mode == 1 && c->opt_tail_cus > 0) {
        uint32_t tail[8] = {0}, head[8] = {0};
        for (int i = 0; i < 256; ++i) {
            int a = i % 8, b = (i / 8) % 4, x = i / 32;
            bool is_tail = b * 8 + (a + x) % 8 < c->opt_tail_cus;
            (is_tail ? tail : head)[i / 32] |= 1u << (i % 32);
        }
        e = hipExtStreamCreateWithCUMask(&c->front, 8, head);
        if (e == hipSuccess) e = hipExtStreamCreateWithCUMask(&c->masked_tail, 8, tail);
        if (e == hipSuccess && c->stream == c->own_stream) c->stream = c->masked_tail;
    } else if (c->opt_front_priority) {
        int least = 0, greatest = 0;  // (numerically, the least priority is the larger value)
        e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->front, hipStreamNonBlocking, c->opt_front_priority == 1 ? least : greatest);
    } else {
        e = hipStreamCreateWithFlags(&c->front, hipStreamNonBlocking);
    }
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {  // (the single frame's two sets)
        auto &f = c->frame.fs[k];
        e = hipEventCreateWithFlags(&f.binned, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&f.consumed, hipEventDisableTiming);
        f.consumed_valid = false;
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->joined, hipEventDisableTiming);
    if (e != hipSuccess) overlap_teardown(c);
    return e;
}

static int set_overlap(rtr_ctx *c, int value) {
    NEED(c, value >= -1 && value <= 1, "overlap: -1 (automatic), 0 or 1");
    if (value == c->ov.mode && value != 0) return RTR_OK;
    // (the peers of a sharded frame read THE exported tile store; alternating between two of them is for single-GPU frames)
    if (value == 1 && c->p2p.open) return fail(c, RTR_ERR_INVALID, "option overlap cannot be switched on while the peer-to-peer exchange is open (rtr_p2p_close first)");
    DevGuard g(c->device);
    HIP_TRY(c, sync_streams(c));
    (void)collect_timing(c);
    if (value == 1 && c->opt_tail_cus > 0) {
        int ncu = 0;
        HIP_TRY(c, hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device));
        if (ncu != 256) return fail(c, RTR_ERR_UNSUPPORTED, "tail_cus needs the 256-CU / 8-XCD part (device has %d CUs)", ncu);
    }
    overlap_teardown(c);  // (the streams of 1 and -1 differ with "tail_cus")
    c->ov.set_mode(value);
    if (value == 0) {  // the set the last frame did not use goes back -- unless the peers were given its handles
        auto &o = c->frame.fs[c->frame.cur ^ 1];
        if (!(c->frame.cur == 1 && (c->p2p.open || c->p2p.red))) {
            dfree(o.dyn); dfree(o.store.ext0); dfree(o.store.meta);
            o.dyn_cap = o.pool_n = 0;
            o.nst = o.ntiles = 0;
            o.consts = rtr::StoreConsts{};
            o.parity = 0;
            o.lean_pending = false;
        }
        return RTR_OK;
    }
    if (value == 1) {
        const hipError_t e = overlap_streams(c);
        if (e != hipSuccess) {
            c->ov.set_mode(0);
            return fail(c, RTR_ERR_HIP, "option overlap: creating the front stream failed: %s", hipGetErrorString(e));
        }
    }
    return RTR_OK;
}

// A whole frame that the policy wants overlapped and that does not follow an overlapped one: the streams, and in the
// automatic mode the second store and pool -- there a failure is no error, the context stays serial
static bool overlap_ready(rtr_ctx *c) {
    if (overlap_streams(c) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (c->ov.mode == 1) return true;  // (the sets are allocated by the frames that use them, failures are errors)
    auto &o = c->frame.fs[c->frame.cur ^ 1];
    const std::string err = c->err;
    if (ensure_pool(c, c->frame, o, 0) != RTR_OK || ensure_store(c, c->frame, o, 0, c->front) != RTR_OK) {
        (void)hipGetLastError();
        c->err = err;
        dfree(o.dyn); dfree(o.store.ext0); dfree(o.store.meta);
        o.dyn_cap = o.pool_n = 0;
        o.nst = o.ntiles = 0;
        o.consts = rtr::StoreConsts{};
        return false;
    }
    return true;
}

static int pack_cloud(rtr_ctx *c);

int rtr_set_option(rtr_ctx *c, const char *key, int value) {
    if (!c) return RTR_ERR_INVALID;
    // test aid: the value-th allocation attempted from now on fails, once (rtr_alloc_rule.h).  Process-wide, like the
    // counters: some allocation sites have no context at hand.  It touches nothing of the context, not even a streak of
    // whole frames, so that a test can arm it between two frames of one
    if (key && !strcmp(key, "debug_alloc_fail")) {
        NEED(c, value >= 0, "debug_alloc_fail must be >= 0 (0: off)");
        rtr::alloc_rule().arm(value);
        return RTR_OK;
    }
    c->ov.other_call();
    NEED(c, key != nullptr, "key is NULL");
    if (!strcmp(key, "mode")) {
        NEED(c, value == 0 || value == 1, "mode must be 0 or 1");
        c->opt_mode = value;
        c->list_valid = false;
        return RTR_OK;
    }
    if (!strcmp(key, "point_grid")) {
        NEED(c, value >= 1 && value <= 65535, "point_grid out of range");
        c->opt_grid = value;
        c->list_valid = false;
        return RTR_OK;
    }
    if (!strcmp(key, "split_threshold")) {  // 0: never split
        NEED(c, value >= 0, "split_threshold must be >= 0");
        c->opt_heavy = value;
        c->split_cooldown = kSplitCooldown;
        c->list_valid = false;
        return RTR_OK;
    }
#ifdef RTR_EXPERIMENT
    if (!strcmp(key, "xp")) {  // timing experiments: parts of T1 switched off, frames become wrong
        c->opt_xp = value;
        return RTR_OK;
    }
#endif
    if (!strcmp(key, "fill_shift")) {  // spacing of the tile stream counters: 4 << value bytes
        NEED(c, value >= -1 && value <= rtr::kFillShiftMax, "fill_shift must be in -1..6 (-1: automatic)");
        DevGuard g(c->device);
        HIP_TRY(c, sync_streams(c));
        c->opt_fill_shift = value;  // (the counters are all zero between frames: any spacing can follow any other)
        c->list_valid = false;
        return RTR_OK;
    }
    if (!strcmp(key, "debug_dyn_cap")) {  // test aid: a pool this small makes heavy tiles overflow it (error code 2)
        NEED(c, value >= -1, "debug_dyn_cap must be >= -1 (-1: off)");
        c->opt_debug_dyn_cap = value;
        c->list_valid = false;
        return RTR_OK;
    }
    if (!strcmp(key, "debug_extract_window")) {  // test aid: small clouds reach rtr_extract_points' multi-window path
        NEED(c, value == -1 || value >= 1, "debug_extract_window must be >= 1 (-1: off)");
        c->opt_debug_extract_window = value;
        return RTR_OK;
    }
    if (!strcmp(key, "debug_store_stamp")) {  // test aid: the 24-bit frame stamp's wrap (next_seq) within a few frames
        NEED(c, value >= 0 && value <= (int)rtr::kStampMask, "debug_store_stamp must be in 0..0xFFFFFF");
        // (forward only: a stamp moved backwards could make stale directory words current, which the library never does)
        for (const auto *t : {&c->frame, &c->views})
            for (const auto &f : t->fs)
                NEED(c, !f.store.ext0 || (uint32_t)value >= f.store.seq, "debug_store_stamp is below the stamp of a tile store (forward only)");
        for (auto *t : {&c->frame, &c->views})
            for (auto &f : t->fs)
                if (f.store.ext0) f.store.seq = (uint32_t)value;
        c->debug_store_stamp = (uint32_t)value;  // (host state only: the kernels get the stamp as an argument)
        return RTR_OK;
    }
    if (!strcmp(key, "debug_p2p_barrier")) {  // test aid: the barrier counter's wrap; read where the flag words are allocated (p2p_alloc)
        c->opt_debug_p2p_barrier = value;     // (-1: off; anything else is the counter's 32 bits)
        return RTR_OK;
    }
    if (!strcmp(key, "p2p_timeout_ms")) {
        NEED(c, value >= 1 && value <= 60000, "p2p_timeout_ms must be in 1..60000");
        c->opt_p2p_timeout_ms = value;
        return RTR_OK;
    }
    if (!strcmp(key, "phases")) {  // T1: wave groups that start at different places of the cloud (k_project_bin)
        NEED(c, value >= 0 && value <= 65535, "phases must be in 0..65535 (0: automatic)");
        c->opt_phases = value;
        c->list_valid = false;
        return RTR_OK;
    }
    if (!strcmp(key, "split_slice")) {
        NEED(c, value >= 1, "split_slice must be >= 1");
        c->opt_slice = value;
        c->split_cooldown = kSplitCooldown;
        c->list_valid = false;
        return RTR_OK;
    }
    if (!strcmp(key, "auto_reorder")) {
        NEED(c, value >= 0 && value <= 2, "auto_reorder must be 0 (never), 1 (always) or 2 (when the order is incoherent)");
        c->opt_auto_reorder = value;
        return RTR_OK;
    }
    if (!strcmp(key, "cull")) {
        c->opt_cull = value != 0;
        return RTR_OK;
    }
    if (!strcmp(key, "point_ids")) {  // read when a cloud is uploaded or sorted (rtr_point_pass)
        NEED(c, value == 0 || value == 1, "point_ids must be 0 or 1");
        c->opt_point_ids = value;
        return RTR_OK;
    }
    if (!strcmp(key, "lean")) {  // whole frames without T1's epilogue when nothing needs it (rtr_render)
        c->opt_lean = value != 0;
        return RTR_OK;
    }
    if (!strcmp(key, "lean_identity")) {  // lean frames: workgroup b = tile b when every tile workgroup is resident at once
        c->opt_lean_identity = value != 0;
        return RTR_OK;
    }
    if (!strcmp(key, "lean_early")) {  // lean frames: entries requested before the counters (tile_body); -1 = by the last frame
        NEED(c, value >= -1 && value <= 1, "lean_early: -1, 0 or 1");
        c->opt_lean_early = value;
        return RTR_OK;
    }
    if (!strcmp(key, "lane_test")) {  // T1: one point per lane first (k_project_bin); 0 = every point, as in round 3
        c->opt_lane_test = value != 0;
        c->list_valid = false;
        return RTR_OK;
    }
    if (!strcmp(key, "chunk_test")) {  // T1, packed clouds: the chunks' header boxes first (k_project_bin); 0 = as in round 4
        c->opt_chunk_test = value != 0;
        c->list_valid = false;
        return RTR_OK;
    }
    if (!strcmp(key, "pack")) {  // applies to the resident cloud at once, and to every later one
        NEED(c, value >= 0 && value <= 2, "pack must be 0 (never), 1 (when it pays) or 2 (always, verified)");
        const int before = c->opt_pack;
        c->opt_pack = value;
        DevGuard g(c->device);
        HIP_TRY(c, sync_streams(c));
        if (c->n == 0 || c->cap == 0) return RTR_OK;
        if (int rc = ensure_soa(c)) {  // (packing reads the fp32 arrays; "pack" = 0 leaves them as the resident form)
            c->opt_pack = before;  // (nothing has changed: the cloud stays in the form it has, under the option it had)
            return rc;
        }
        if (int rc = pack_cloud(c)) return rc;
        drop_soa(c);
        return RTR_OK;
    }
    if (!strcmp(key, "keep_soa")) {  // 1: the fp32 SoA arrays stay resident beside the packed form (12 B per point)
        c->opt_keep_soa = value != 0;
        DevGuard g(c->device);
        if (c->opt_keep_soa) return (c->cap && c->n) ? ensure_soa(c) : RTR_OK;
        drop_soa(c);
        return RTR_OK;
    }
    if (!strcmp(key, "pool_worst_case")) {  // 1: the extent pool is sized for the worst case (2 n entries) at once
        c->opt_pool_worst = value != 0;
        return RTR_OK;
    }
    if (!strcmp(key, "probe_variant")) {
        c->opt_probe = value;
        return RTR_OK;
    }
    if (!strcmp(key, "tail_cus")) {  // takes effect when "overlap" is switched on
        NEED(c, value >= 0 && value < 32, "tail_cus must be in 0..31 (CUs per XCD)");
        NEED(c, c->ov.mode != 1, "set tail_cus before overlap");
        c->opt_tail_cus = value;
        return RTR_OK;
    }
    if (!strcmp(key, "overlap")) return set_overlap(c, value);
    if (!strcmp(key, "front_priority")) {  // takes effect when the front stream is next created ("overlap")
        NEED(c, value >= 0 && value <= 2, "front_priority: 0 (default priority), 1 (lowest) or 2 (highest)");
        c->opt_front_priority = value;
        return RTR_OK;
    }
    if (!strcmp(key, "keep_accum")) {
        c->opt_keep_accum = value != 0;
        return RTR_OK;
    }
    return fail(c, RTR_ERR_INVALID, "unknown option '%s'", key);
}

int rtr_get_option(rtr_ctx *c, const char *key, int *value) {
    if (!c) return RTR_ERR_INVALID;
    NEED(c, key != nullptr && value != nullptr, "key / value is NULL");
    if (!strcmp(key, "mode")) *value = c->opt_mode;
    else if (!strcmp(key, "auto_reorder")) *value = c->opt_auto_reorder;
    else if (!strcmp(key, "reordered")) *value = c->reordered ? 1 : 0;
    else if (!strcmp(key, "selection")) *value = c->sel ? 1 : 0;  // a selection exists (rtr_select_points)
    else if (!strcmp(key, "voxel_keys_us")) *value = c->voxel_us[0];  // the last rtr_select_voxel_grid, stage by stage
    else if (!strcmp(key, "voxel_sort_us")) *value = c->voxel_us[1];
    else if (!strcmp(key, "voxel_heads_us")) *value = c->voxel_us[2];
    else if (!strcmp(key, "neighbours_keys_us")) *value = c->neighbours_us[0];  // the last rtr_select_neighbours, stage by stage
    else if (!strcmp(key, "neighbours_sort_us")) *value = c->neighbours_us[1];
    else if (!strcmp(key, "neighbours_count_us")) *value = c->neighbours_us[2];
    else if (!strcmp(key, "neighbours_pair_tests_k")) *value = c->neighbours_tests_k;
    else if (!strcmp(key, "near_given_us")) *value = c->near_us[0];  // the last rtr_select_near
    else if (!strcmp(key, "near_sweep_us")) *value = c->near_us[1];
    else if (!strcmp(key, "near_pair_tests_k")) *value = c->near_tests_k;
    else if (!strcmp(key, "near_chunks_skipped")) *value = c->near_chunks[0];
    else if (!strcmp(key, "near_chunks_decoded")) *value = c->near_chunks[1];
    else if (!strcmp(key, "nearest_given_us")) *value = c->nearest_us[0];  // the last rtr_nearest_points
    else if (!strcmp(key, "nearest_sweep_us")) *value = c->nearest_us[1];
    else if (!strcmp(key, "nearest_pair_tests_k")) *value = c->nearest_tests_k;
    else if (!strcmp(key, "nearest_chunks_skipped")) *value = c->nearest_chunks[0];
    else if (!strcmp(key, "nearest_chunks_decoded")) *value = c->nearest_chunks[1];
    else if (!strcmp(key, "nearest_k_given_us")) *value = c->nearest_k_us[0];  // the last rtr_nearest_k_points
    else if (!strcmp(key, "nearest_k_sweep_us")) *value = c->nearest_k_us[1];
    else if (!strcmp(key, "nearest_k_pair_tests_k")) *value = c->nearest_k_tests_k;
    else if (!strcmp(key, "nearest_k_chunks_skipped")) *value = c->nearest_k_chunks[0];
    else if (!strcmp(key, "nearest_k_chunks_decoded")) *value = c->nearest_k_chunks[1];
    else if (!strcmp(key, "nearest_k_cascades_k")) *value = c->nearest_k_cascades_k;
    else if (!strcmp(key, "clusters_keys_us")) *value = c->clusters_us[0];  // the last rtr_select_clusters
    else if (!strcmp(key, "clusters_sort_us")) *value = c->clusters_us[1];
    else if (!strcmp(key, "clusters_label_us")) *value = c->clusters_us[2];
    else if (!strcmp(key, "clusters_pair_tests_k")) *value = c->clusters_tests_k;
    else if (!strcmp(key, "plane_sample_us")) *value = c->plane_us[0];  // the last rtr_fit_plane
    else if (!strcmp(key, "plane_count_us")) *value = c->plane_us[1];
    else if (!strcmp(key, "point_keep")) *value = c->keep_up ? 1 : 0;  // a keep mask is set (rtr_set_point_keep)  // the resident cloud was sorted by the library
    else if (!strcmp(key, "order_ratio_ppm")) *value = (int)(c->order_ratio * 1e6f);  // chunk / cloud diagonal as uploaded
    else if (!strcmp(key, "cull")) *value = c->opt_cull;
    else if (!strcmp(key, "point_ids")) *value = c->opt_point_ids;
    else if (!strcmp(key, "lane_test")) *value = c->opt_lane_test;
    else if (!strcmp(key, "chunk_test")) *value = c->opt_chunk_test;
    else if (!strcmp(key, "phases")) *value = c->opt_phases;
    else if (!strcmp(key, "overlap")) *value = c->ov.mode;
    else if (!strcmp(key, "overlap_active")) *value = c->ov.active ? 1 : 0;  // the last whole frame ran overlapped
    else if (!strcmp(key, "front_priority")) *value = c->opt_front_priority;
    else if (!strcmp(key, "lean")) *value = c->opt_lean;
    else if (!strcmp(key, "lean_identity")) *value = c->opt_lean_identity;
    else if (!strcmp(key, "lean_early")) *value = c->opt_lean_early;
    else if (!strcmp(key, "p2p_open")) *value = c->p2p.open ? 1 : 0;  // the peers' buffers are mapped (rtr_p2p_open)
    else if (!strcmp(key, "keep_soa")) *value = c->opt_keep_soa;
    else if (!strcmp(key, "pool_worst_case")) *value = c->opt_pool_worst;
    else if (!strcmp(key, "views")) *value = c->jr.views.count;  // views of the last rtr_render_views
    else if (!strcmp(key, "resident_millibytes_per_point")) {
        // device memory this context holds for the cloud and its frames, per point: coordinates (fp32 SoA and / or packed
        // form), colours, chunk boxes and lane spreads, tile stores and extent pools, frame buffers
        const uint64_t nchunks = ((c->cap / 4) + 63) / 64;
        uint64_t b = (c->x ? 12 * c->cap : 0) + (c->rgba ? 4 * c->cap : 0) + nchunks * 28 +
                     (c->pk_hdr ? c->pk_bytes + (c->pk_units_cap - c->pk_units) * 32 + 64 : 0) +
                     (c->perm ? 4 * c->cap : 0) + (c->keep_up ? (c->n + 31) / 32 * 4 + nchunks * 33 + 4 : 0) +
                     (c->sel ? std::max<uint64_t>((c->n + 255) / 256, 1) * 32 + 32 : 0);
        const uint64_t npix = (uint64_t)c->W * c->H;
        for (const auto *t : {&c->frame, &c->views}) {
            for (const auto &f : t->fs) {
                b += f.dyn ? f.dyn_cap * 8 : 0;
                b += f.store.ext0 ? ((uint64_t)f.nst * rtr::kS0 + 16) * 8 + rtr::ts_meta_words(f.nst, f.ntiles) * 4 : 0;
            }
            b += t->cap ? npix * (16 + 1 + (uint64_t)t->cap * (4 + 3 + 10)) : 0;
        }
        *value = c->n ? (int)((b * 1000) / c->n > 0x7FFFFFFFull ? 0x7FFFFFFF : (b * 1000) / c->n) : 0;
    }
    else if (!strcmp(key, "pack")) *value = c->opt_pack;
    else if (!strcmp(key, "packed")) *value = c->pk_hdr ? 1 : 0;  // the point kernel reads the packed coordinates
    else if (!strcmp(key, "packed_millibytes_per_point"))         // its coordinate stream, headers included (12000 = raw)
        *value = c->pk_hdr && c->n ? (int)(c->pk_bytes * 1000 / c->n) : 12000;
    else if (!strcmp(key, "wide_chunks") || !strcmp(key, "wide_chunks_boxed")) {
        // chunks of the packed form with an axis of 32 bits / those of them whose header carries a box word (round 6).
        // Counted over the resident headers when asked, so every edit path is covered by construction.
        *value = 0;
        if (c->pk_hdr && c->n) {
            uint64_t *dev = nullptr, host[2] = {0, 0};
            hipError_t e = rtr::dev_malloc(&dev, sizeof host);
            if (e == hipSuccess) e = hipMemsetAsync(dev, 0, sizeof host, c->stream);
            if (e == hipSuccess) {
                rtr::launch_wide_counts(c->stream, c->pk_hdr, (((uint64_t)c->n + 3) / 4 + 63) / 64, dev);
                e = hipMemcpyAsync(host, dev, sizeof host, hipMemcpyDeviceToHost, c->stream);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            (void)rtr::dev_free(dev);
            if (e != hipSuccess) return fail(c, RTR_ERR_HIP, "wide_chunks: %s", hipGetErrorString(e));
            const uint64_t v = host[key[11] ? 1 : 0];
            *value = v > 0x7FFFFFFFull ? 0x7FFFFFFF : (int)v;
        }
    }
    else if (!strcmp(key, "keep_accum")) *value = c->opt_keep_accum;
    else if (!strcmp(key, "split_threshold")) *value = c->opt_heavy;
    else if (!strcmp(key, "split_slice")) *value = c->opt_slice;
    else if (!strcmp(key, "point_grid")) *value = c->opt_grid;
    else if (!strcmp(key, "debug_extract_window")) *value = c->opt_debug_extract_window;
    // (the allocation switch and counters of rtr_alloc_rule.h, process-wide; the counts saturate at INT_MAX)
    else if (!strcmp(key, "debug_alloc_fail")) *value = (int)std::min<int64_t>(rtr::alloc_rule().remaining(), 0x7FFFFFFF);
    else if (!strcmp(key, "debug_alloc_count"))
        *value = (int)std::min<uint64_t>(rtr::alloc_rule().attempts.load(std::memory_order_relaxed), 0x7FFFFFFFu);
    else if (!strcmp(key, "debug_alloc_live"))
        *value = (int)std::max<int64_t>(0, std::min<int64_t>(rtr::alloc_rule().live.load(std::memory_order_relaxed), 0x7FFFFFFF));
    // (while the exchange is open: the 32 bits of its barrier counter, the number of the last barrier queued)
    else if (!strcmp(key, "debug_p2p_barrier")) *value = c->p2p.open ? (int)c->p2p.seq : c->opt_debug_p2p_barrier;
    // (the stamp of the single frame's current store -- of its last frame, or what its first frame will start from)
    else if (!strcmp(key, "debug_store_stamp")) *value = (int)(c->F().store.ext0 ? c->F().store.seq : c->debug_store_stamp);
    else if (statistics_option(c, key, value)) return RTR_OK;  // (the keys of include/rtr_statistics.h, section 6n)
    else if (normals_option(c, key, value)) return RTR_OK;     // (the keys of include/rtr_normals.h, section 6o)
    else return fail(c, RTR_ERR_INVALID, "unknown option '%s'", key);
    return RTR_OK;
}

// ---- clip planes (rtr.h, section 6d) ------------------------------------------------
int rtr_set_clip_planes(rtr_ctx *c, int count, const float *planes) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, count >= 0 && count <= RTR_MAX_CLIP_PLANES, "clip planes: count outside 0..RTR_MAX_CLIP_PLANES");
    NEED(c, count == 0 || planes != nullptr, "clip planes: planes is NULL");
    rtr::Clip next{};
    for (int j = 0; j < count; ++j) {
        for (int k = 0; k < 4; ++k) {
            NEED(c, std::isfinite(planes[4 * j + k]), "clip planes: a coefficient is not finite");
            next.p[j][k] = planes[4 * j + k];
        }
        NEED(c, next.p[j][0] != 0.f || next.p[j][1] != 0.f || next.p[j][2] != 0.f, "clip planes: a = b = c = 0");
    }
    next.count = count;
    if (memcmp(&next, &c->clip, sizeof next) != 0) c->list_valid = false;  // (bins of other planes serve no later pass)
    c->clip = next;
    return RTR_OK;
}

int rtr_get_clip_planes(rtr_ctx *c, int *count, float *planes) {
    if (!c) return RTR_ERR_INVALID;
    NEED(c, count != nullptr, "count is NULL");
    NEED(c, c->clip.count == 0 || planes != nullptr, "planes is NULL");
    *count = c->clip.count;
    for (int j = 0; j < c->clip.count; ++j)
        for (int k = 0; k < 4; ++k) planes[4 * j + k] = c->clip.p[j][k];
    return RTR_OK;
}

int rtr_stream_probe(rtr_ctx *c, const float P[16]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, P != nullptr, "P is NULL");
    if (int rc = check_frame(c)) return rc;
    DevGuard g(c->device);
    if (int rc = ensure_soa(c)) return rc;
    { Timed t(c, RTR_K_PROBE); rtr::launch_stream_probe(c->stream, cloud_of(c), make_proj(P), c->W, c->H, c->frame.minmax, c->opt_probe); }
    return launch_check(c, "stream_probe");
}

int rtr_get_params(const rtr_ctx *c, rtr_params *p) {
    if (!c || !p) return RTR_ERR_INVALID;
    *p = c->prm;
    return RTR_OK;
}

static int switch_stream(rtr_ctx *c, hipStream_t s) {
    DevGuard g(c->device);
    HIP_TRY(c, sync_streams(c));
    (void)collect_timing(c);
    c->stream = s;
    return RTR_OK;
}

int rtr_set_stream(rtr_ctx *c, void *s) {  // NULL is HIP's default stream, a valid choice
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    return switch_stream(c, reinterpret_cast<hipStream_t>(s));
}

int rtr_reset_stream(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    return switch_stream(c, c->masked_tail ? c->masked_tail : c->own_stream);
}

// A device-to-host copy of a frame's results: queued again behind a repaired frame
struct Copy { void *host; const void *dev; size_t bytes; };
static hipError_t queue_copies(rtr_ctx *c, const Copy *cp, int n) {
    for (int i = 0; i < n; ++i)
        if (cp[i].host) {
            const hipError_t e = hipMemcpyAsync(cp[i].host, cp[i].dev, cp[i].bytes, hipMemcpyDeviceToHost, c->stream);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

static int queue_slot(rtr_ctx *c, const float P[16], int slot, int with_filter);
static int views_enqueue(rtr_ctx *c, int count, const float *P, int with_filter);

// After a synchronisation: the tile-store errors of target t.  They (entries dropped by T1: an extent that never
// appeared, an exhausted extent pool) reach the host through a mapped word that T1's epilogue writes; every call that
// has just synchronised reports and clears it -- a wrong frame is never returned as RTR_OK.  When the only error is an
// overflow of the ADAPTIVE extent pool (ensure_pool), the pool is worst-case sized from now on (and every frame still
// on its way to an async slot is marked stale: it was queued before the growth), and what the journal recorded for t
// is rendered again, once: with `slots` (rtr_wait) every stale slot in slot order, then the last whole frame and the
// point pass queued behind it -- or the last batch of views.  `own` (rtr_project): that frame instead of the
// journal's, whatever form it took.  `copies` are queued again behind them; one more synchronisation and check
// follow, without another try.
static int repair(rtr_ctx *c, rtr_ctx::Target &t, bool slots = false, const Copy *copies = nullptr, int ncopies = 0,
                  const rtr_ctx::Journal::Frames *own = nullptr) {
    auto &j = c->jr;
    const bool single = &t == &c->frame;
    const bool was_worst = t.pool_worst;  // (rtr_wait reads the word twice before it repeats anything)
    bool retry = false;
    auto check = [&](bool may_retry) -> int {
        const uint32_t e = __atomic_exchange_n(t.err_host, 0u, __ATOMIC_ACQUIRE);
        if (single && j.pass.unchecked) {  // (a point pass has read a frame: complete unless this word says otherwise)
            if (e != 0u) j.pass.invalid = true;  // (repeated below when it followed the frame repeated there)
            if (e != 0u || hipEventQuery(c->pp_done) == hipSuccess) j.pass.unchecked = false;
        }
        if (e == 0u) return RTR_OK;
        const bool grow = e == 2u && c->opt_debug_dyn_cap < 0 && !was_worst && t.fs[t.cur].dyn_cap < pool_worst_cap(c);
        if (grow && (single || may_retry)) {  // (the views' pools grow only with a batch to render again)
            t.pool_worst = true;  // (ensure_pool re-allocates before the next T1)
            for (int k = 0; single && k < RTR_ASYNC_SLOTS; ++k)
                if (c->ho[k].busy && !j.slot[k].sealed) j.slot[k].stale = true;
            if (may_retry) {
                retry = true;
                return RTR_OK;
            }
        }
        if (!single) {
            j.views.count = 0;
            return fail(c, RTR_ERR_INTERNAL, "tile store error 0x%x in a batch of views -- entries were dropped, the views are "
                        "incomplete: render the batch again", e);
        }
        if (grow)
            return fail(c, RTR_ERR_INTERNAL, "tile store error 0x2: the extent pool, sized by the frames seen so far, was too "
                        "small for a frame rendered since the last synchronising call -- entries were dropped; the pool is "
                        "worst-case sized from now on: render the frame again (option pool_worst_case = 1 sizes it so from "
                        "the start)");
        return fail(c, RTR_ERR_INTERNAL, "tile store error 0x%x: %s%s%s%s-- entries were dropped, frames rendered since the last "
                    "synchronising call are incomplete", e, (e & 1u) ? "a stream extent never appeared " : "",
                    (e & 2u) ? "the dynamic extent pool overflowed " : "",
                    (e & 4u) ? "a contested tile of a sharded frame had more stream pieces than its table holds " : "",
                    (e & 8u) ? "the split tiles' second phase gave up waiting for the first " : "");
    };
    if (int rc = check(single ? own || j.frame.count > 0 || slots : j.views.count > 0)) return rc;
    bool stale = false;
    for (int k = 0; slots && k < RTR_ASYNC_SLOTS; ++k) stale |= c->ho[k].busy && j.slot[k].stale;
    if (!retry && !stale) return RTR_OK;
    if (slots) {  // (rtr_wait has waited for its slots only: what was queued behind them is finished and checked too)
        HIP_TRY(c, sync_streams(c));
        if (int rc = check(true)) return rc;
    }
    // (every frame goes again with the clip planes it was issued with; the context's own come back afterwards)
    struct ClipScope {
        rtr_ctx *c;
        rtr::Clip keep;
        ~ClipScope() { c->clip = keep; }
    } clip_scope{c, c->clip};
    if (single) {
        const auto frame = own ? *own : j.frame;  // (the slots' frames below replace the record)
        const auto pass = j.pass;
        for (int k = 0; slots && k < RTR_ASYNC_SLOTS; ++k) {
            const auto f = j.slot[k];
            if (!c->ho[k].busy || !f.stale) continue;
            if (f.cloud != c->cloud_seq)
                return fail(c, RTR_ERR_INTERNAL, "rtr_wait: the frame of slot %d lost entries in an overflowing extent pool "
                            "and the cloud has been replaced since: it cannot be rendered again", k);
            c->clip = f.clip;
            if (int rc = queue_slot(c, f.P, k, f.filter)) return rc;
        }
        if (frame.count) {
            c->clip = frame.clip;
            if (int rc = rtr_render(c, frame.P, frame.filter)) return rc;
            c->clip = pass.clip;
            if (pass.behind)
                if (int rc = rtr_point_pass(c, pass.P, pass.what)) return rc;
        }
    } else {
        c->clip = j.views.clip;
        if (int rc = views_enqueue(c, j.views.count, j.views.P, j.views.filter)) return rc;
    }
    HIP_TRY(c, queue_copies(c, copies, ncopies));
    HIP_TRY(c, sync_streams(c));
    return check(false);
}

int rtr_synchronize(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    DevGuard g(c->device);
    HIP_TRY(c, sync_streams(c));
    if (int rc = repair(c, c->frame)) return rc;
    return repair(c, c->views);
}

}  // extern "C"

namespace {
// The packed form's invariants, each in one place (rtr::PackedXyz; `units`: 32-byte units of both plane streams).
// Resident bytes: blocks + headers
uint64_t pack_bytes(uint64_t units, uint64_t chunks) { return units * 32 + chunks * 32; }
// The spare bytes behind both plane streams read as zero: the last lanes' loads run into them
hipError_t zero_spare(hipStream_t s, uint32_t *planes, uint32_t *planes_b, uint64_t units) {
    const hipError_t e = hipMemsetAsync(planes + units * 2, 0, (rtr::pack_b_dwords(units) - units * 2) * 4, s);
    return e != hipSuccess ? e : hipMemsetAsync(planes_b + units * 6, 0, 64, s);
}
// The blocks of the chunks in front of a rebuilt window, `units` of them, into fresh planes (the A region's size
// changes, so the B region moves)
hipError_t copy_blocks(hipStream_t s, uint32_t *planes, uint32_t *planes_b, const rtr_ctx *c, uint64_t units) {
    const hipError_t e = d2d(s, planes, c->pk_planes, units * 2 * 4);
    return e != hipSuccess ? e : d2d(s, planes_b, c->pk_planes_b, units * 6 * 4);
}

// An upload-order bit-word argument (`words`, `nwords`; `fn` and `what` name the call and the argument in the messages):
// one bit per resident point, so nwords must be (n + 31) / 32, and a cloud the library sorted must have kept its
// permutation (need_upload_order with `or_else`) -- unless `order_checked_later`: the call asks that itself, behind its
// other arguments.  null_means_every: NULL with nwords 0 stands for every point and passes as it is.
int check_point_words(rtr_ctx *c, const char *fn, const char *what, const uint32_t *words, uint64_t nwords, bool null_means_every,
                      const char *or_else = "", bool order_checked_later = false) {
    if (!words && !(null_means_every && nwords == 0)) return fail(c, RTR_ERR_INVALID, "%s: %s is NULL", fn, what);
    if (!words) return RTR_OK;
    if (nwords != (c->n + 31) / 32)
        return fail(c, RTR_ERR_INVALID, "%s: nwords must be (n + 31) / 32 = %llu", fn, (unsigned long long)((c->n + 31) / 32));
    return order_checked_later ? RTR_OK : need_upload_order(c, "mapped", or_else);
}
}  // namespace

extern "C" {

// ---- keep mask (rtr.h, section 6e) ----------------------------------------------------
// Everything issued before is finished and checked first, as rtr_synchronize does, and also the async slots' frames a
// repair repeats (with the mask they were issued with): no journal entry then needs a copy of the mask.  The slots stay
// busy for rtr_wait, sealed: a later overflow does not make them stale.
static int complete_all(rtr_ctx *c) {
    HIP_TRY(c, sync_streams(c));
    if (int rc = repair(c, c->frame, true)) return rc;
    for (int k = 0; k < RTR_ASYNC_SLOTS; ++k)
        if (c->ho[k].busy) HIP_TRY(c, hipEventSynchronize(c->ho[k].done));
    if (int rc = repair(c, c->views)) return rc;
    for (int k = 0; k < RTR_ASYNC_SLOTS; ++k)
        if (c->ho[k].busy) c->jr.slot[k].sealed = true;
    return RTR_OK;
}

int rtr_set_point_keep(rtr_ctx *c, const uint32_t *words, uint64_t nwords) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    const bool clear = words == nullptr && nwords == 0;
    NEED(c, clear || c->n > 0, "rtr_set_point_keep: no cloud");
    if (int rc = check_point_words(c, "rtr_set_point_keep", "words", words, nwords, true)) return rc;
    DevGuard g(c->device);
    if (int rc = complete_all(c)) return rc;  // (frames issued before come out with the mask they were issued with)
    if (clear) {
        if (c->keep_up) c->list_valid = false;
        free_keep(c);
        return RTR_OK;
    }
    const uint64_t nchunks = (c->n + 255) / 256;
    DevBufs buf;
    uint32_t *up, *res = c->keep_res;
    uint8_t *sum = c->keep_sum;
    HIP_TRY(c, buf.get(&up, nwords * 4));
    // (the caller's words, host or device memory, into a new buffer: a failed copy leaves the old mask in force)
    HIP_TRY(c, hipMemcpyAsync(up, words, nwords * 4, hipMemcpyDefault, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!res) {
        HIP_TRY(c, buf.get(&res, nchunks * 32));
        HIP_TRY(c, buf.get(&sum, (nchunks + 3) & ~3ull));  // (read as whole dwords)
    }
    rtr::launch_keep_build(c->stream, up, c->reordered ? c->perm : nullptr, c->n, res, sum);
    HIP_TRY(c, sync_streams(c));
    if (int rc = launch_check(c, "keep mask")) return rc;
    buf.swap_in(c->keep_up, up); buf.swap_in(c->keep_res, res); buf.swap_in(c->keep_sum, sum);
    c->list_valid = false;  // (bins of another mask serve no later pass)
    return RTR_OK;
}

// ---- cloud -------------------------------------------------------------------------

// Option "auto_reorder" (after every upload / generation; the chunk bounds are current).  2 (default):
// sort when the 256-point chunks are not spatially compact -- mean chunk diagonal more than twice what
// an ideally ordered VOLUME cloud of this size would have, (256 / n)^(1/3) of the cloud's diagonal.
// A scanner's sweep order or the reference loader's Morton-like surfaces pass; a hash-ordered cloud
// (ratio ~1) and the reference's 0.25 m blocks that are unordered inside do not.  Frames never depend
// on the point order; rtr_download_points returns the resident (possibly sorted) order.
// Best effort: the sort works on scratch copies and only writes the cloud back at the very end, so a
// cloud too large for the scratch simply stays in the order it was uploaded in.
// Option "pack" (after every upload / generation / reorder): the tile-binned point kernel reads the
// coordinates from the lossless PackedXyz form when that is at least 1/8 smaller than the 12 B/pt SoA
// stream (spatially ordered clouds: 6-9 B/pt; a hash-ordered one stays raw).  The SoA arrays stay resident
// -- the atomic form, the phase calls with another matrix, rtr_download_points and the sort use them.
// Best effort: without memory for it the cloud simply stays unpacked.
static int pack_cloud(rtr_ctx *c) {
    free_pack(c);
    if (c->opt_pack == 0 || c->n == 0) return RTR_OK;
    const uint64_t n4 = (c->n + 3) / 4, nchunks = (n4 + 63) / 64;
    DevBufs buf;
    uint4 *hdr;
    uint32_t *planes, *cnt;
    uint64_t *tot;
    auto give_up = [&]() {  // (buf frees what was allocated)
        (void)hipGetLastError();
        return RTR_OK;
    };
    // (+ one zero header: the point kernel reads headers in pairs)
    if (buf.get(&hdr, (nchunks + 1) * 2 * sizeof(uint4)) != hipSuccess) return give_up();
    if (hipMemsetAsync(hdr + nchunks * 2, 0, 2 * sizeof(uint4), c->stream) != hipSuccess) return give_up();
    if (buf.get(&cnt, nchunks * sizeof(uint32_t)) != hipSuccess) return give_up();
    if (buf.get(&tot, 2 * sizeof(uint64_t)) != hipSuccess) return give_up();
    if (hipMemsetAsync(tot, 0, 2 * sizeof(uint64_t), c->stream) != hipSuccess) return give_up();
    const rtr::Cloud cl = cloud_of(c);
    rtr::pack_measure(c->stream, cl, hdr, cnt, tot);
    uint64_t host[2] = {0, 0};
    if (hipMemcpyAsync(host, tot, sizeof host, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return give_up();
    if (hipStreamSynchronize(c->stream) != hipSuccess) return give_up();
    const uint64_t bytes = pack_bytes(host[0], nchunks);
    if (c->opt_pack == 1 && bytes * 8 > n4 * 48 * 7) return give_up();  // saves less than 1/8 of the 12 B/pt stream
    // (one allocation: the A streams, 64 spare bytes, the B streams, 64 spare bytes -- the last lanes' loads run up to
    // 12 bytes past the last value of their stream)
    const uint64_t b_dw = rtr::pack_b_dwords(host[0]);
    if (buf.get(&planes, rtr::pack_total_dwords(host[0]) * 4) != hipSuccess) return give_up();
    if (zero_spare(c->stream, planes, planes + b_dw, host[0]) != hipSuccess) return give_up();
    rtr::pack_write(c->stream, cl, hdr, planes, planes + b_dw);
    if (c->opt_pack == 2) {
        rtr::pack_verify(c->stream, cl, hdr, planes, planes + b_dw, tot + 1);
        if (hipMemcpyAsync(host, tot, sizeof host, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return give_up();
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return give_up();
    if (c->opt_pack == 2 && host[1] != 0) {
        (void)give_up();
        return fail(c, RTR_ERR_HIP, "pack: %llu points decode to other coordinates", (unsigned long long)host[1]);
    }
    buf.swap_in(c->pk_hdr, hdr); buf.swap_in(c->pk_planes, planes);
    c->pk_planes_b = planes + b_dw;
    c->pk_bytes = bytes;
    c->pk_units = c->pk_units_cap = host[0];
    c->pk_hdr_chunks = nchunks;
    return RTR_OK;
}

static int auto_reorder(rtr_ctx *c) {
    c->reordered = false;
    dfree(c->perm);  // (a new cloud: upload order = resident order until it is sorted)
    c->order_ratio = 0.f;
    c->absmax[0] = c->absmax[1] = c->absmax[2] = __builtin_inff();  // (unknown: the lane test's margin step stays off)
    if (c->n < 1) return RTR_OK;
    float ratio = 0.f;  // measured under every policy: the point kernel has a form for incoherent clouds
    if (rtr::order_quality(c->stream, c->bounds, c->n, &ratio, c->absmax) != 0) {
        (void)hipGetLastError();
        c->absmax[0] = c->absmax[1] = c->absmax[2] = __builtin_inff();
        return RTR_OK;
    }
    bool want = c->opt_auto_reorder == 1;
    if (c->n >= (1u << 16)) {  // (tiny clouds render in microseconds whatever their order)
        c->order_ratio = ratio;
        if (c->opt_auto_reorder == 2) want = ratio > 2.0f * cbrtf(256.0f / (float)c->n);
    }
    if (c->n < 2 || !want) return RTR_OK;
    if (rtr_reorder_points(c) != RTR_OK) (void)hipGetLastError();
    return RTR_OK;
}

// Host AoS points into device SoA arrays through device staging pieces of 16 Mi points (AoS -> SoA on the GPU).  Between
// pieces only the context's stream is synchronised: both callers have drained every stream before (sync_streams /
// complete_all) and nothing here queues on another one, so waiting for the others too would wait for nothing.
static int stage_points(rtr_ctx *c, DevBufs &buf, const float *xyz, size_t xs, const uint8_t *rgb, size_t rs, uint64_t n,
                        float *x, float *y, float *z, uint32_t *rgba) {
    if (n == 0) return RTR_OK;
    const uint64_t piece = 1ull << 24;
    uint8_t *sx, *sc;
    HIP_TRY(c, buf.get(&sx, std::min(n, piece) * xs));
    HIP_TRY(c, buf.get(&sc, std::min(n, piece) * rs));
    for (uint64_t off = 0; off < n; off += piece) {
        const uint64_t cnt = std::min(n - off, piece);
        HIP_TRY(c, hipMemcpyAsync(sx, (const uint8_t *)xyz + off * xs, cnt * xs, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(sc, rgb + off * rs, cnt * rs, hipMemcpyHostToDevice, c->stream));
        rtr::launch_aos_to_soa(c->stream, sx, xs, sc, rs, cnt, x + off, y + off, z + off, rgba + off);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return RTR_OK;
}

// What every new cloud ends with (`what` filled its arrays): NaN padding, chunk boxes, options "auto_reorder" and "pack"
static int finish_new_cloud(rtr_ctx *c, const char *what) {
    rtr::launch_pad_nan(c->stream, c->x, c->y, c->z, c->rgba, c->n, (c->n + 3) & ~3ull);
    rtr::launch_chunk_bounds(c->stream, cloud_of(c), c->bounds, c->spread);
    HIP_TRY(c, sync_streams(c));
    if (int rc = launch_check(c, what)) return rc;
    free_pack(c);
    if (int rc = auto_reorder(c)) return rc;
    if (!c->pk_hdr)  // (a sort has packed already)
        if (int rc = pack_cloud(c)) return rc;
    drop_soa(c);
    return RTR_OK;
}

// What a cloud-replacing call falls back to when it fails after the previous cloud has begun to go (its arrays are freed
// or overwritten first, since two clouds may not fit): the context as an upload of 0 points leaves it -- no points, mask,
// selection, packed form, permutation or pools; the clip planes, options and frame resources stay.  The call's own
// error message is kept.  Should even the empty cloud's 16-byte arrays fail, the context is as rtr_create left it.
static void discard_cloud(rtr_ctx *c) {
    const std::string err = c->err;
    (void)sync_streams(c);
    free_cloud(c);
    if (alloc_cloud(c, 0) != RTR_OK || finish_new_cloud(c, "empty cloud") != RTR_OK) {
        (void)hipGetLastError();
        free_cloud(c);
        c->reordered = false;
        ++c->cloud_seq;
        c->jr.frame.count = 0;
        c->pp_vis_current = false;
    }
    c->jr.views.count = 0;
    c->err = err;
}

// alloc_cloud has failed: either nothing has changed (the old cloud, resident in packed form only, is intact; cap > 0)
// or the old cloud is gone
static int new_cloud_failed(rtr_ctx *c, int rc) {
    if (c->cap == 0) discard_cloud(c);
    return rc;
}

int rtr_upload_points(rtr_ctx *c, const float *xyz, size_t xs, const uint8_t *rgb, size_t rs, size_t n) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, n == 0 || (xyz && rgb), "xyz / rgb is NULL");
    NEED(c, xs >= 12 && xs % 4 == 0, "xyz_stride_bytes must be >= 12 and a multiple of 4");
    NEED(c, rs >= 3, "rgb_stride_bytes must be >= 3");
    NEED(c, n < (1ull << 32), "too many points for one context (point indices are 32-bit): shard the cloud");
    DevGuard g(c->device);
    HIP_TRY(c, sync_streams(c));
    if (int rc = alloc_cloud(c, n)) return new_cloud_failed(c, rc);
    DevBufs buf;
    if (int rc = stage_points(c, buf, xyz, xs, rgb, rs, n, c->x, c->y, c->z, c->rgba)) {
        discard_cloud(c);  // (the arrays hold some of the old cloud and some of the new)
        return rc;
    }
    return finish_new_cloud(c, "aos_to_soa");
}

int rtr_generate_synthetic(rtr_ctx *c, int scene, uint64_t seed, uint64_t first, uint64_t count, uint64_t total) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, scene == RTR_SCENE_UNIFORM_BOX || scene == RTR_SCENE_ROOM_SHELL, "unknown scene");
    NEED(c, first + count <= total, "first + count exceeds total");
    NEED(c, total < (1ull << 33), "total too large");
    NEED(c, count < (1ull << 32), "too many points for one context (point indices are 32-bit): shard the cloud");
    DevGuard g(c->device);
    HIP_TRY(c, sync_streams(c));
    if (int rc = alloc_cloud(c, count)) return new_cloud_failed(c, rc);
    rtr::launch_generate(c->stream, scene, seed, first, count, total, c->x, c->y, c->z, c->rgba);
    return finish_new_cloud(c, "generate");
}

// ---- editing the resident cloud (rtr.h, sections 2b - 2d) ---------------------------------------------------------
// rtr_append_points, rtr_remove_points and rtr_transform_points change the points of some 256-point chunks, so the
// per-chunk state of those chunks is rebuilt over a WINDOW: fp32 SoA scratch holding the chunks' new points, on which the
// upload's kernels run in their range forms (rtr_kernels.h) -- chunk boxes and lane spreads, packed headers (the scan
// continues from the first chunk's block offset) and blocks.  Each call builds its window in its own way (window_alloc,
// then its own kernels fill wx / wy / wz), measures it (window_measure), commits it and ends in cloud_edited.  Append
// and remove rebuild every chunk from c0 on and share commit_window; transform rebuilds chunks c0 .. c1, keeps the blocks
// behind them and has a commit of its own, from the same helpers (d2d, copy_blocks, zero_spare, pack_bytes).
struct Window {
    uint64_t c0 = 0, wn = 0, wpad = 0, wch = 0;  // first chunk; points, padded to a multiple of 4; chunks
    float *wx = nullptr, *wy = nullptr, *wz = nullptr;  // the points (NaN-padded by the caller)
    float *wb = nullptr, *wsp = nullptr;         // chunk boxes, lane spreads (window_measure)
    uint4 *whdr = nullptr;                       // packed: headers ...
    uint32_t *cnt = nullptr;                     // ... scratch of the measure, wch words (allocated unless the caller lends some) ...
    uint64_t first_unit = 0, units = 0;          // ... chunk c0's block offset, and the offset behind the window's last block
    rtr::Cloud cl{};                             // the view the range forms take: the cloud from chunk c0 on
};

// The resident cloud's settings over other coordinates: no colours, packed form or keep mask
static rtr::Cloud window_view(const rtr_ctx *c, const float *x, const float *y, const float *z, uint64_t n, const float *spread) {
    rtr::Cloud v = cloud_of(c);
    v.x = x, v.y = y, v.z = z, v.n = n, v.spread = spread;
    v.rgba = nullptr;
    v.pk = rtr::PackedXyz{nullptr, nullptr, nullptr};
    v.keep = rtr::Keep{nullptr, nullptr};
    return v;
}

// The counts of a window of wn points from chunk c0 on, and its point arrays for the caller to fill
static int window_alloc(rtr_ctx *c, DevBufs &buf, Window &w, uint64_t c0, uint64_t wn) {
    w.c0 = c0, w.wn = wn, w.wpad = (wn + 3) & ~3ull, w.wch = (wn + 255) / 256;
    HIP_TRY(c, buf.get(&w.wx, w.wpad * 4)); HIP_TRY(c, buf.get(&w.wy, w.wpad * 4)); HIP_TRY(c, buf.get(&w.wz, w.wpad * 4));
    return RTR_OK;
}

// The derived half of a window whose points are queued: boxes and spreads, and for a packed cloud the headers.  Chunk
// c0's block offset is read from its resident header -- except where the window begins a fresh chunk behind the cloud
// (an append to whole chunks: the zero pair there holds no offset), which starts at pk_units.  An empty window (a
// removal of whole trailing chunks) adds no unit.  units_dev: device word of the scan's total; old_end (transform): the
// block offset of the first resident chunk behind the window.  Synchronises; `what` names the launches in an error.
static int window_measure(rtr_ctx *c, DevBufs &buf, Window &w, uint64_t *units_dev, const char *what, uint64_t *old_end = nullptr) {
    hipStream_t s = c->stream;
    HIP_TRY(c, buf.get(&w.wb, w.wch * 6 * sizeof(float)));
    HIP_TRY(c, buf.get(&w.wsp, w.wch * sizeof(float)));
    w.cl = window_view(c, w.wx, w.wy, w.wz, w.wn, w.wsp);
    rtr::launch_chunk_bounds(s, w.cl, w.wb, w.wsp);
    if (c->pk_hdr) {
        const uint64_t nch = (c->n + 255) / 256, end = w.c0 + w.wch;
        uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0;
        const bool resident = w.c0 < nch, tail = old_end && end < nch;
        if (resident) HIP_TRY(c, hipMemcpyAsync(&h0, c->pk_hdr + 2 * w.c0 + 1, sizeof h0, hipMemcpyDeviceToHost, s));
        if (tail) HIP_TRY(c, hipMemcpyAsync(&h1, c->pk_hdr + 2 * end + 1, sizeof h1, hipMemcpyDeviceToHost, s));
        if (resident || tail) HIP_TRY(c, hipStreamSynchronize(s));
        w.first_unit = resident ? (((uint64_t)h0.y << 32) | h0.x) : c->pk_units;
        if (old_end) *old_end = tail ? (((uint64_t)h1.y << 32) | h1.x) : c->pk_units;
        w.units = w.first_unit;
        if (w.wn) {
            HIP_TRY(c, buf.get(&w.whdr, w.wch * 2 * sizeof(uint4)));
            if (!w.cnt) HIP_TRY(c, buf.get(&w.cnt, w.wch * sizeof(uint32_t)));
            rtr::pack_measure(s, w.cl, w.whdr, w.cnt, units_dev, w.first_unit);
            HIP_TRY(c, hipMemcpyAsync(&w.units, units_dev, sizeof w.units, hipMemcpyDeviceToHost, s));
        }
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return launch_check(c, what);
}

// Capacity rules of the resident arrays.  After an append: `have`, grown with 1/8 head-room when it is too small
static uint64_t grown(uint64_t have, uint64_t need) {
    if (need <= have) return have;
    const uint64_t g = have + have / 8;
    return g > need ? g : need;
}
// After a removal or a move: `have` unless it is too small or wastes more than 1/8
static uint64_t fitted(uint64_t have, uint64_t need) {
    const uint64_t fit = need + need / 8;
    return need > have ? fit : (have > fit ? fit : have);
}

// What rtr_append_points and rtr_remove_points hand to commit_window beside the window.  Their per-point arrays stand for
// the points from `at` on: the block behind the n0 resident points, or every survivor from chunk c0 on
struct Splice {
    uint64_t n1;                                // points afterwards
    uint64_t (*capacity)(uint64_t, uint64_t);   // grown / fitted
    uint64_t at;
    const uint32_t *rgba;                       // colours of points at .. at + rgba_n - 1 (zero up to the padded count behind them)
    uint64_t rgba_n;
    const uint32_t *perm;                       // upload indices of points at .. n1 - 1; null: the cloud keeps no permutation
    const uint32_t *renum_keep, *renum_scan;    // a removal with perm: its keep words and their popcount scan, by which the
                                                // upload indices of the points in front of `at` are renumbered (null: they stay)
    uint32_t *keep_up;                          // with a keep mask: its new upload-order words, a fresh buffer the caller filled
    uint64_t *bad;                              // option "pack" = 2: device counter of pack_verify (read by cloud_edited)
    const char *what;                           // names the launches in an error
};

// Splices a rebuilt window into the resident arrays: chunks [0, c0) stay, the window's chunks follow, n becomes n1.
// Three phases, and the boundary between the first two is the invariant: EVERY buffer that may fail to allocate is
// allocated before the first resident byte changes, so a failed call leaves the cloud as it was.  (1) The replacement
// of every array whose capacity rule asks for another size.  (2) Copies and kernels, queued in one order for both
// calls, writing into the replacements or -- from chunk c0 on only -- into the arrays that stay; then one
// synchronisation.  (3) The new arrays swapped in, the packed form's bookkeeping, the point count.
static int commit_window(rtr_ctx *c, DevBufs &buf, const Window &w, const Splice &e) {
    hipStream_t s = c->stream;
    const uint64_t c0 = w.c0, p0 = 256 * c0, nch1 = c0 + w.wch, n1 = e.n1, n1pad = (n1 + 3) & ~3ull;
    const bool packed = c->pk_hdr != nullptr;

    // (1) allocate
    const uint64_t cap1 = (e.capacity(c->cap, n1pad) + 3) & ~3ull, cch1 = (cap1 / 4 + 63) / 64;
    const bool realloc = cap1 != c->cap;
    float *x1 = c->x, *y1 = c->y, *z1 = c->z, *bounds1 = c->bounds, *spread1 = c->spread;
    uint32_t *rgba1 = c->rgba, *perm1 = e.perm ? c->perm : nullptr;
    if (realloc) {
        HIP_TRY(c, buf.get(&rgba1, cap1 * 4));
        HIP_TRY(c, buf.get(&bounds1, cch1 * 6 * sizeof(float)));
        HIP_TRY(c, buf.get(&spread1, cch1 * sizeof(float)));
        if (c->x) {
            HIP_TRY(c, buf.get(&x1, cap1 * 4)); HIP_TRY(c, buf.get(&y1, cap1 * 4)); HIP_TRY(c, buf.get(&z1, cap1 * 4));
        }
    }
    // (no perm yet: this block is the first one sorted; renum_keep: the indices in front of the window change as well, and
    // nothing in front of chunk c0 is written in place)
    if (e.perm && (realloc || !c->perm || e.renum_keep)) HIP_TRY(c, buf.get(&perm1, cap1 * 4));
    uint4 *hdr1 = c->pk_hdr;
    uint32_t *planes1 = c->pk_planes, *planes1_b = c->pk_planes_b;
    uint64_t hch1 = c->pk_hdr_chunks, ucap1 = c->pk_units_cap;
    if (packed) {  // (a removal's merged chunks may span wider boxes: its planes can grow as well as shrink)
        hch1 = e.capacity(c->pk_hdr_chunks, nch1);
        if (hch1 != c->pk_hdr_chunks) HIP_TRY(c, buf.get(&hdr1, (hch1 + 1) * 2 * sizeof(uint4)));  // (+ the zero pair: read in pairs)
        ucap1 = e.capacity(c->pk_units_cap, w.units);
        if (ucap1 != c->pk_units_cap) {
            HIP_TRY(c, buf.get(&planes1, rtr::pack_total_dwords(ucap1) * 4));
            planes1_b = planes1 + rtr::pack_b_dwords(ucap1);
        }
    }
    uint32_t *res1 = nullptr;
    uint8_t *sum1 = nullptr;
    if (e.keep_up) {
        HIP_TRY(c, buf.get(&res1, nch1 * 32));
        HIP_TRY(c, buf.get(&sum1, (nch1 + 3) & ~3ull));  // (read as whole dwords)
    }

    // (2) write: the resident prefix into replaced arrays, then the window's chunks from c0 on
    if (realloc) {
        HIP_TRY(c, d2d(s, rgba1, c->rgba, e.at * 4));
        HIP_TRY(c, d2d(s, bounds1, c->bounds, c0 * 6 * sizeof(float)));
        HIP_TRY(c, d2d(s, spread1, c->spread, c0 * sizeof(float)));
        if (c->x) {
            HIP_TRY(c, d2d(s, x1, c->x, p0 * 4)); HIP_TRY(c, d2d(s, y1, c->y, p0 * 4)); HIP_TRY(c, d2d(s, z1, c->z, p0 * 4));
        }
    }
    HIP_TRY(c, d2d(s, rgba1 + e.at, e.rgba, e.rgba_n * 4));
    if (n1pad > e.at + e.rgba_n) HIP_TRY(c, hipMemsetAsync(rgba1 + e.at + e.rgba_n, 0, (n1pad - e.at - e.rgba_n) * 4, s));
    if (x1) {
        HIP_TRY(c, d2d(s, x1 + p0, w.wx, w.wpad * 4)); HIP_TRY(c, d2d(s, y1 + p0, w.wy, w.wpad * 4));
        HIP_TRY(c, d2d(s, z1 + p0, w.wz, w.wpad * 4));
    }
    HIP_TRY(c, d2d(s, bounds1 + 6 * c0, w.wb, w.wch * 6 * sizeof(float)));
    HIP_TRY(c, d2d(s, spread1 + c0, w.wsp, w.wch * sizeof(float)));
    if (e.perm) {
        if (e.renum_keep) {  // (a sorted cloud: the chunks that stay hold indices above a removed one; into the fresh perm1)
            rtr::launch_remove_renumber(s, c->perm, e.at, e.renum_keep, e.renum_scan, perm1);
        } else if (perm1 != c->perm) {
            if (c->perm) HIP_TRY(c, d2d(s, perm1, c->perm, e.at * 4));
            else rtr::launch_iota(s, perm1, e.at);  // (the cloud was in upload order until this block's sort)
        }
        HIP_TRY(c, d2d(s, perm1 + e.at, e.perm, (n1 - e.at) * 4));
    }
    if (packed) {
        if (hdr1 != c->pk_hdr) HIP_TRY(c, d2d(s, hdr1, c->pk_hdr, c0 * 2 * sizeof(uint4)));
        HIP_TRY(c, d2d(s, hdr1 + 2 * c0, w.whdr, w.wch * 2 * sizeof(uint4)));
        HIP_TRY(c, hipMemsetAsync(hdr1 + 2 * nch1, 0, 2 * sizeof(uint4), s));  // (the zero pair sits behind the last chunk)
        if (planes1 != c->pk_planes) HIP_TRY(c, copy_blocks(s, planes1, planes1_b, c, w.first_unit));
        rtr::pack_write(s, w.cl, hdr1 + 2 * c0, planes1, planes1_b);
        HIP_TRY(c, zero_spare(s, planes1, planes1_b, w.units));
        if (c->opt_pack == 2) rtr::pack_verify(s, w.cl, hdr1 + 2 * c0, planes1, planes1_b, e.bad);
    }
    if (e.keep_up) {  // (resident words and summaries from chunk c0 on)
        HIP_TRY(c, d2d(s, res1, c->keep_res, c0 * 32));
        HIP_TRY(c, d2d(s, sum1, c->keep_sum, c0));
        rtr::launch_keep_build(s, e.keep_up, perm1, n1, res1, sum1, c0);
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = launch_check(c, e.what)) return rc;

    // (3) the new state
    buf.swap_in(c->rgba, rgba1); buf.swap_in(c->bounds, bounds1); buf.swap_in(c->spread, spread1);
    buf.swap_in(c->x, x1); buf.swap_in(c->y, y1); buf.swap_in(c->z, z1);
    if (e.perm) buf.swap_in(c->perm, perm1);
    c->cap = cap1;
    if (packed) {
        buf.swap_in(c->pk_hdr, hdr1); buf.swap_in(c->pk_planes, planes1);
        c->pk_planes_b = planes1_b;
        c->pk_units = w.units, c->pk_units_cap = ucap1, c->pk_hdr_chunks = hch1;
        c->pk_bytes = pack_bytes(w.units, nch1);
    }
    if (e.keep_up) { buf.swap_in(c->keep_up, e.keep_up); buf.swap_in(c->keep_res, res1); buf.swap_in(c->keep_sum, sum1); }
    c->n = n1;
    return RTR_OK;
}

// The cloud has changed: what was computed from the old one is dropped, what is measured over every chunk box is
// measured again.  resized (append, remove): upload indices or the point count changed too -- the selection goes, and
// the n-sized state (the peers' mappings of this rank's pools, the adaptive pool sizing) starts over; a move keeps all
// of that.  bad / which: option "pack" = 2, the commit's pack_verify counter and what it counted
// measure: order_quality's device scratch, which the caller allocated among its own buffers -- this function runs behind
// the commit and allocates nothing, so a failed allocation never reaches a caller as RTR_OK over an edited cloud
static int cloud_edited(rtr_ctx *c, bool resized, const uint64_t *bad, const char *which, void *measure) {
    if (resized) free_select(c);
    ++c->cloud_seq;
    c->list_valid = false;
    c->jr.frame.count = 0;
    c->jr.views.count = 0;
    c->pp_vis_current = false;
    c->split_cooldown = kSplitCooldown;
    if (resized) {
        if (c->p2p.open || c->p2p.red) p2p_release(c);  // (the peers map pools sized for the old cloud)
        reset_pool_sizing(c->frame);
        reset_pool_sizing(c->views);
    }
    {   // order measure and absmax over every chunk box: the lane test's margin steps and the incoherent form read them
        float ratio = 0.f;
        if (rtr::order_quality(c->stream, c->bounds, c->n, &ratio, c->absmax, measure) != 0) {
            (void)hipGetLastError();
            c->absmax[0] = c->absmax[1] = c->absmax[2] = __builtin_inff();
        }
        c->order_ratio = c->n >= (1u << 16) ? ratio : 0.f;
    }
    if (c->pk_hdr && c->opt_pack == 2) {
        uint64_t n_bad = 0;
        HIP_TRY(c, hipMemcpy(&n_bad, bad, sizeof n_bad, hipMemcpyDeviceToHost));
        if (n_bad) return fail(c, RTR_ERR_HIP, "pack: %llu %s decode to other coordinates", (unsigned long long)n_bad, which);
    }
    return RTR_OK;
}

// ---- appending (rtr.h, section 2b) ----------------------------------------------------
// The block goes behind the resident points.  Its first points may complete the last partial 256-point chunk c0, so the
// window holds chunk c0's resident points (copied, or decoded from the packed form when the SoA arrays are not
// resident) followed by the block.  commit_window with `grown`: the arrays grow with 1/8 head-room and never shrink.
// The block's colours and upload indices go behind the n0 resident ones; a block sorted on its own may give the cloud
// its first permutation; the new points are kept by a keep mask.
int rtr_append_points(rtr_ctx *c, const float *xyz, size_t xs, const uint8_t *rgb, size_t rs, size_t m) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, m == 0 || (xyz && rgb), "xyz / rgb is NULL");
    NEED(c, xs >= 12 && xs % 4 == 0, "xyz_stride_bytes must be >= 12 and a multiple of 4");
    NEED(c, rs >= 3, "rgb_stride_bytes must be >= 3");
    NEED(c, m < (1ull << 32) && c->n + m < (1ull << 32),
         "too many points for one context (point indices are 32-bit): shard the cloud");
    if (m == 0) return RTR_OK;
    if (c->n == 0) return rtr_upload_points(c, xyz, xs, rgb, rs, m);
    DevGuard g(c->device);
    if (int rc = complete_all(c)) return rc;  // (frames issued before come out with the cloud they were issued with)
    drop_soa(c);  // (SoA arrays decoded for a call in between are not kept: the window decodes what it needs)
    hipStream_t s = c->stream;
    const uint64_t n0 = c->n, n1 = n0 + m, c0 = n0 / 256, r = n0 - c0 * 256, m4 = (m + 3) & ~3ull;
    DevBufs buf;

    // the block: host -> device in pieces, AoS -> SoA (b*), NaN-padded to a multiple of 4
    float *bx, *by, *bz;
    uint32_t *bc, *bperm = nullptr;
    HIP_TRY(c, buf.get(&bx, m4 * 4)); HIP_TRY(c, buf.get(&by, m4 * 4)); HIP_TRY(c, buf.get(&bz, m4 * 4));
    HIP_TRY(c, buf.get(&bc, m4 * 4));
    if (int rc = stage_points(c, buf, xyz, xs, rgb, rs, m, bx, by, bz, bc)) return rc;
    rtr::launch_pad_nan(s, bx, by, bz, bc, m, m4);
    if (int rc = launch_check(c, "aos_to_soa")) return rc;

    // option "auto_reorder" on the block alone (auto_reorder's rule), never losing the order a keep mask needs
    bool sort = c->opt_auto_reorder == 1;
    if (c->opt_auto_reorder == 2 && m >= (1u << 16)) {
        float *bb, ratio = 0.f, am[3];
        HIP_TRY(c, buf.get(&bb, ((m + 255) / 256) * 6 * sizeof(float)));
        rtr::launch_chunk_bounds(s, window_view(c, bx, by, bz, m, nullptr), bb, nullptr);
        const int e = rtr::order_quality(s, bb, m, &ratio, am);
        if (e != 0) return fail(c, RTR_ERR_HIP, "block order measure failed: %s", hipGetErrorString((hipError_t)e));
        sort = ratio > 2.0f * cbrtf(256.0f / (float)m);
    }
    sort = sort && m >= 2 && !(c->keep_up && !c->reordered && !c->opt_point_ids);
    const bool with_perm = c->reordered ? c->perm != nullptr : (sort && c->opt_point_ids);
    if (with_perm) {  // upload indices of the block: n0 .. n1 - 1, sorted with it
        HIP_TRY(c, buf.get(&bperm, m * 4));
        rtr::launch_iota(s, bperm, m, n0);
    }
    if (sort) {
        const int e = rtr::reorder_morton(s, bx, by, bz, bc, m, bperm);
        if (e != 0) return fail(c, RTR_ERR_HIP, "block sort failed: %s", hipGetErrorString((hipError_t)e));
    }

    // the window: chunk c0's resident points, then the block
    Window w;
    if (int rc = window_alloc(c, buf, w, c0, r + m)) return rc;
    if (r) {
        if (c->x) {
            HIP_TRY(c, d2d(s, w.wx, c->x + c0 * 256, r * 4)); HIP_TRY(c, d2d(s, w.wy, c->y + c0 * 256, r * 4));
            HIP_TRY(c, d2d(s, w.wz, c->z + c0 * 256, r * 4));
        } else {  // (packed form only: chunk c0 alone is decoded, bit for bit; it writes whole quads, the block follows)
            rtr::unpack_to_soa(s, rtr::PackedXyz{c->pk_hdr + 2 * c0, c->pk_planes, c->pk_planes_b}, r, w.wx, w.wy, w.wz);
        }
    }
    HIP_TRY(c, d2d(s, w.wx + r, bx, m * 4)); HIP_TRY(c, d2d(s, w.wy + r, by, m * 4)); HIP_TRY(c, d2d(s, w.wz + r, bz, m * 4));
    rtr::launch_pad_nan(s, w.wx, w.wy, w.wz, nullptr, w.wn, w.wpad);
    uint64_t *tot = nullptr, *bad = nullptr;  // packed: the window's units, pack mismatches
    void *measure;  // (cloud_edited's scratch: allocated with the rest, before anything is committed)
    HIP_TRY(c, buf.get(&measure, rtr::order_quality_scratch_bytes()));
    if (c->pk_hdr) {
        HIP_TRY(c, buf.get(&tot, 2 * sizeof(uint64_t)));
        HIP_TRY(c, hipMemsetAsync(tot, 0, 2 * sizeof(uint64_t), s));
        bad = tot + 1;
    }
    if (int rc = window_measure(c, buf, w, tot, "append window")) return rc;

    uint32_t *up1 = nullptr;
    if (c->keep_up) {  // (the new points kept)
        HIP_TRY(c, buf.get(&up1, (n1 + 31) / 32 * 4));
        HIP_TRY(c, d2d(s, up1, c->keep_up, (n0 + 31) / 32 * 4));
        rtr::launch_keep_append(s, up1, n0, n1);
    }
    if (int rc = commit_window(c, buf, w, Splice{n1, grown, n0, bc, m, bperm, nullptr, nullptr, up1, bad, "append"})) return rc;
    c->reordered = c->reordered || sort;
    return cloud_edited(c, true, bad, "appended points", measure);
}

// ---- removing (rtr.h, section 2c) -------------------------------------------------------------------------------
// A stable compaction of the resident order.  One wave per chunk counts its survivors (through perm when the cloud is
// sorted) and names the first chunk c0 that loses a point; chunks before it stay where they are.  The window holds the
// survivors of the chunks from c0 on, compacted, with their colours and renumbered upload indices.  commit_window with
// `fitted`: arrays that would hold more than 1/8 head-room over the survivors are reallocated to that size.  A keep
// mask is compacted onto the survivors; a visibility mask much larger than they need is dropped.
int rtr_remove_points(rtr_ctx *c, const uint32_t *keep_words, uint64_t nwords) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->n > 0, "rtr_remove_points: no cloud");
    if (int rc = check_point_words(c, "rtr_remove_points", "keep_words", keep_words, nwords, false)) return rc;
    DevGuard g(c->device);
    if (int rc = complete_all(c)) return rc;  // (frames issued before come out with the cloud they were issued with)
    drop_soa(c);
    hipStream_t s = c->stream;
    const uint64_t n0 = c->n, nch0 = (n0 + 255) / 256;
    const uint32_t *perm0 = c->reordered ? c->perm : nullptr;
    DevBufs buf;

    // the caller's words (host or device memory), survivors per chunk, their exclusive scan, the first chunk losing one
    uint32_t *kw, *cnt, *dst, *scr;
    uint64_t *tot;
    HIP_TRY(c, buf.get(&kw, nwords * 4));
    HIP_TRY(c, buf.get(&cnt, nch0 * 4));
    HIP_TRY(c, buf.get(&dst, nch0 * 4));
    const uint64_t scr_words = std::max(rtr::scan_scratch_words(nch0), rtr::scan_scratch_words(nwords));
    HIP_TRY(c, buf.get(&scr, scr_words * 4));
    HIP_TRY(c, buf.get(&tot, 4 * sizeof(uint64_t)));  // first loss, survivors (then the window's units), kept words' total, pack mismatches
    void *measure;  // (cloud_edited's scratch: allocated with the rest, before anything is committed)
    HIP_TRY(c, buf.get(&measure, rtr::order_quality_scratch_bytes()));
    HIP_TRY(c, hipMemcpyAsync(kw, keep_words, nwords * 4, hipMemcpyDefault, s));
    HIP_TRY(c, hipMemsetAsync(tot, 0xFF, sizeof(uint64_t), s));
    HIP_TRY(c, hipMemsetAsync(tot + 1, 0, 3 * sizeof(uint64_t), s));
    rtr::launch_remove_count(s, kw, perm0, n0, cnt, tot);
    rtr::launch_scan_u32(s, cnt, nch0, 0, dst, scr, tot + 1);
    uint64_t head[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(head, tot, sizeof head, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = launch_check(c, "remove count")) return rc;
    const uint64_t n1 = head[1], c0 = head[0] < nch0 ? head[0] : nch0;
    // (the selection goes with every removal -- here where every point stays, with the cloud where none does, in
    // cloud_edited otherwise: behind the last allocation that can fail, so that a failed call leaves it in force.  The
    // caller's words are in kw: the selection's own buffer may have been passed)
    if (n1 == n0) {  // (every point stays: nothing else changes)
        free_select(c);
        return RTR_OK;
    }
    if (n1 == 0) {  // (no point stays: the context of an upload of 0 points)
        // (its 4-point arrays are allocated before the cloud is freed: a failed allocation leaves the cloud as it was;
        // the upload then finds them and allocates nothing)
        float *ex, *ey, *ez, *eb, *esp;
        uint32_t *ec;
        HIP_TRY(c, buf.get(&ex, 16)); HIP_TRY(c, buf.get(&ey, 16)); HIP_TRY(c, buf.get(&ez, 16));
        HIP_TRY(c, buf.get(&ec, 16)); HIP_TRY(c, buf.get(&eb, 6 * sizeof(float))); HIP_TRY(c, buf.get(&esp, sizeof(float)));
        free_cloud(c);
        buf.swap_in(c->x, ex); buf.swap_in(c->y, ey); buf.swap_in(c->z, ez); buf.swap_in(c->rgba, ec);
        buf.swap_in(c->bounds, eb); buf.swap_in(c->spread, esp);
        c->cap = 4;
        const float nx[4] = {0.f, 0.f, 0.f, 1.f};
        const uint8_t nc[4] = {0, 0, 0, 255};
        return rtr_upload_points(c, nx, 16, nc, 4, 0);
    }

    // the window: the survivors of chunks c0.., compacted (renumbered upload indices when the permutation is kept)
    Window w;
    uint32_t *wscan = nullptr, *wrgba, *wperm = nullptr;
    if (perm0 || c->keep_up) {
        HIP_TRY(c, buf.get(&wscan, nwords * 4));
        rtr::launch_scan_u32(s, kw, nwords, n0, wscan, scr, tot + 2);
    }
    if (int rc = window_alloc(c, buf, w, c0, n1 - 256 * c0)) return rc;
    w.cnt = cnt;  // (free again: the survivors' scan has read it)
    HIP_TRY(c, buf.get(&wrgba, w.wpad * 4));
    if (perm0) HIP_TRY(c, buf.get(&wperm, w.wpad * 4));
    rtr::launch_remove_compact(s, cloud_of(c), perm0, kw, wscan, dst, c0, w.wx, w.wy, w.wz, wrgba, wperm);
    rtr::launch_pad_nan(s, w.wx, w.wy, w.wz, wrgba, w.wn, w.wpad);
    if (int rc = window_measure(c, buf, w, tot + 1, "remove window")) return rc;

    uint32_t *up1 = nullptr;
    if (c->keep_up) {  // (old[keep] in upload order)
        HIP_TRY(c, buf.get(&up1, (n1 + 31) / 32 * 4));
        HIP_TRY(c, hipMemsetAsync(up1, 0, (n1 + 31) / 32 * 4, s));
        rtr::launch_remove_mask(s, kw, wscan, c->keep_up, n0, up1);
    }
    if (int rc = commit_window(c, buf, w, Splice{n1, fitted, 256 * c0, wrgba, w.wpad, wperm, perm0 ? kw : nullptr, wscan, up1, tot + 3, "remove"})) return rc;
    if (c->pp_vis && c->pp_vis_words > ((n1 + 31) / 32 > 8 ? (n1 + 31) / 32 : 8)) {  // (sized again by the next point pass)
        dfree(c->pp_vis);
        c->pp_vis_words = 0;
    }
    return cloud_edited(c, true, tot + 3, "points of the rebuilt chunks", measure);
}

// ---- moving and writing points (rtr.h, sections 2d and 2f) -------------------------------------------------------
// Points get new coordinates where they lie: upload indices, the resident order, the permutation and the keep mask stay.
// A selection pass names the first and last chunk holding a point that changes, c0 and c1; only chunks c0 .. c1 are
// rebuilt (rebuild_chunks).  `fill` queues the kernel that produces those chunks' new points (rtr_transform_points:
// the selected ones moved; rtr_write_points: the written ones taken from the caller's records) into the arrays it is
// handed, in_place or not.  An unpacked cloud is rebuilt in place (its SoA arrays, then the boxes of c0 .. c1).  A packed
// one gets a window: chunks c0 .. c1 decoded (read from the SoA arrays with "keep_soa" = 1) with the new points in.  Its
// commit is its own, because the blocks behind c1 are not decoded: when the window's units differ from the old ones by
// delta, the tail's A and B blocks move by delta (through a scratch copy, or into fresh planes when the capacity changes;
// `fitted`) and its headers' offsets with them.  Every buffer is allocated before the first resident byte changes, as in
// commit_window; `also` queues what else the call changes in the resident arrays (rtr_write_points: the colours) and
// runs in the commit phase, behind the last allocation.  tot: four device words -- the span (unused here), the window's
// units, pack_verify's mismatches.  The n-sized state stays: the callers end in cloud_edited without `resized`.
static int rebuild_chunks(rtr_ctx *c, DevBufs &buf, uint64_t c0, uint64_t c1, uint64_t *tot, const char *what,
                          const std::function<void(float *, float *, float *, bool)> &fill, const std::function<void()> &also) {
    hipStream_t s = c->stream;
    const uint64_t n = c->n, nch = (n + 255) / 256;
    const uint64_t p0 = 256 * c0, wn = std::min(n, 256 * (c1 + 1)) - p0;
    if (!c->pk_hdr) {  // (in place: nothing left to allocate)
        fill(c->x + p0, c->y + p0, c->z + p0, true);
        rtr::launch_chunk_bounds(s, window_view(c, c->x + p0, c->y + p0, c->z + p0, wn, c->spread + c0), c->bounds + 6 * c0,
                                 c->spread + c0);
        also();
        HIP_TRY(c, hipStreamSynchronize(s));
        return launch_check(c, what);
    }
    // the window: chunks c0 .. c1 with the new points in; old_end: the tail's first unit
    Window w;
    uint64_t old_end = 0;
    if (int rc = window_alloc(c, buf, w, c0, wn)) return rc;
    fill(w.wx, w.wy, w.wz, false);
    if (int rc = window_measure(c, buf, w, tot + 2, what, &old_end)) return rc;
    const uint64_t new_end = w.units, tail = c->pk_units - old_end, units1 = new_end + tail;
    const int64_t delta = (int64_t)(new_end - old_end);

    // every buffer the commit needs, before anything resident changes
    const uint64_t ucap1 = fitted(c->pk_units_cap, units1);
    uint32_t *planes1 = c->pk_planes, *planes1_b = c->pk_planes_b, *tmp = nullptr;
    if (ucap1 != c->pk_units_cap) {
        HIP_TRY(c, buf.get(&planes1, rtr::pack_total_dwords(ucap1) * 4));
        planes1_b = planes1 + rtr::pack_b_dwords(ucap1);
    } else if (delta != 0 && tail) {
        HIP_TRY(c, buf.get(&tmp, tail * 8 * 4));  // (the tail's A blocks, then its B blocks)
    }

    // commit: the tail's blocks to their new place, the window's headers and blocks, the tail's block offsets
    if (planes1 != c->pk_planes) {  // (fresh planes: the prefix and the tail are copied, nothing overlaps)
        HIP_TRY(c, copy_blocks(s, planes1, planes1_b, c, w.first_unit));
        HIP_TRY(c, d2d(s, planes1 + new_end * 2, c->pk_planes + old_end * 2, tail * 2 * 4));
        HIP_TRY(c, d2d(s, planes1_b + new_end * 6, c->pk_planes_b + old_end * 6, tail * 6 * 4));
    } else if (tmp) {  // (source and destination overlap: through the scratch copy)
        HIP_TRY(c, d2d(s, tmp, c->pk_planes + old_end * 2, tail * 2 * 4));
        HIP_TRY(c, d2d(s, tmp + tail * 2, c->pk_planes_b + old_end * 6, tail * 6 * 4));
        HIP_TRY(c, d2d(s, planes1 + new_end * 2, tmp, tail * 2 * 4));
        HIP_TRY(c, d2d(s, planes1_b + new_end * 6, tmp + tail * 2, tail * 6 * 4));
    }
    HIP_TRY(c, d2d(s, c->pk_hdr + 2 * c0, w.whdr, w.wch * 2 * sizeof(uint4)));
    rtr::launch_shift_units(s, c->pk_hdr, c1 + 1, nch, delta);
    rtr::pack_write(s, w.cl, c->pk_hdr + 2 * c0, planes1, planes1_b);
    HIP_TRY(c, zero_spare(s, planes1, planes1_b, units1));
    if (c->opt_pack == 2) rtr::pack_verify(s, w.cl, c->pk_hdr + 2 * c0, planes1, planes1_b, tot + 3);
    HIP_TRY(c, d2d(s, c->bounds + 6 * c0, w.wb, w.wch * 6 * sizeof(float)));
    HIP_TRY(c, d2d(s, c->spread + c0, w.wsp, w.wch * sizeof(float)));
    if (c->x) {  // ("keep_soa" = 1: the SoA arrays take the window as well)
        HIP_TRY(c, d2d(s, c->x + p0, w.wx, w.wpad * 4)); HIP_TRY(c, d2d(s, c->y + p0, w.wy, w.wpad * 4));
        HIP_TRY(c, d2d(s, c->z + p0, w.wz, w.wpad * 4));
    }
    also();
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = launch_check(c, what)) return rc;
    if (planes1 != c->pk_planes) {
        buf.swap_in(c->pk_planes, planes1);
        c->pk_planes_b = planes1_b;
        c->pk_units_cap = ucap1;
    }
    c->pk_units = units1;
    c->pk_bytes = pack_bytes(units1, nch);
    return RTR_OK;
}

// The first and last chunk holding a point of `sel` (upload-order words on the device; perm as for remove_gather) into
// c0 / c1; *any = false: no point is selected.  tot[0 .. 1]: device scratch of the span.
static int chunk_span(rtr_ctx *c, const uint32_t *sel, const uint32_t *perm, uint64_t *tot, const char *what, uint64_t *c0,
                      uint64_t *c1, bool *any) {
    hipStream_t s = c->stream;
    const uint64_t nch = (c->n + 255) / 256;
    HIP_TRY(c, hipMemsetAsync(tot, 0xFF, sizeof(uint64_t), s));
    HIP_TRY(c, hipMemsetAsync(tot + 1, 0, sizeof(uint64_t), s));
    rtr::launch_transform_span(s, sel, perm, c->n, tot);
    uint64_t span[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(span, tot, sizeof span, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = launch_check(c, what)) return rc;
    *any = span[0] < nch;
    *c0 = span[0], *c1 = span[1];
    return RTR_OK;
}

int rtr_transform_points(rtr_ctx *c, const float M[12], const uint32_t *select_words, uint64_t nwords) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->n > 0, "rtr_transform_points: no cloud");
    NEED(c, M != nullptr, "rtr_transform_points: M is NULL");
    for (int i = 0; i < 12; ++i) NEED(c, std::isfinite(M[i]), "rtr_transform_points: M has a non-finite coefficient");
    const bool every = select_words == nullptr && nwords == 0;
    if (int rc = check_point_words(c, "rtr_transform_points", "select_words", select_words, nwords, true,
                                   ", or move every point (select_words NULL)")) return rc;
    DevGuard g(c->device);
    if (int rc = complete_all(c)) return rc;  // (frames issued before come out with the cloud they were issued with)
    drop_soa(c);  // (SoA arrays decoded for a call in between are not kept: they would hold the old coordinates)
    hipStream_t s = c->stream;
    const uint64_t nch = (c->n + 255) / 256;
    const uint32_t *perm0 = c->reordered ? c->perm : nullptr;
    rtr::Affine A;
    memcpy(A.m, M, sizeof A.m);
    DevBufs buf;

    // the caller's words (host or device memory) and the span of the chunks holding a selected point
    uint32_t *sel = nullptr;
    uint64_t *tot;  // span (first, last chunk), window units, pack mismatches
    HIP_TRY(c, buf.get(&tot, 4 * sizeof(uint64_t)));
    void *measure;  // (cloud_edited's scratch: allocated with the rest, before anything is committed)
    HIP_TRY(c, buf.get(&measure, rtr::order_quality_scratch_bytes()));
    HIP_TRY(c, hipMemsetAsync(tot, 0, 4 * sizeof(uint64_t), s));
    uint64_t c0 = 0, c1 = nch - 1;
    if (!every) {
        HIP_TRY(c, buf.get(&sel, nwords * 4));
        HIP_TRY(c, hipMemcpyAsync(sel, select_words, nwords * 4, hipMemcpyDefault, s));
        bool any = false;
        if (int rc = chunk_span(c, sel, perm0, tot, "transform span", &c0, &c1, &any)) return rc;
        if (!any) return RTR_OK;  // (no point selected: nothing changes)
    }
    const rtr::Cloud cl = cloud_of(c);
    auto fill = [&](float *wx, float *wy, float *wz, bool in_place) {
        rtr::launch_transform_window(s, cl, perm0, sel, c0, c1, A, wx, wy, wz, in_place);
    };
    if (int rc = rebuild_chunks(c, buf, c0, c1, tot, "transform", fill, [] {})) return rc;
    return cloud_edited(c, false, tot + 3, "moved points", measure);
}

// ---- writing points back (rtr.h, section 2f) ------------------------------------------------------------------------
// rtr_extract_points' ranks over rtr_transform_points' commit.  The selection's popcount scan gives k and every selected
// point's rank; k_write_bits keeps the selection bits whose rank lies in [first, first + count) (for "every point" it
// synthesises the words first), and those bits are the selection everything behind works on: the span c0 .. c1, the window
// (rebuild_chunks with the caller's records as the source) and the colours (k_write_colors, queued in the commit phase:
// a call that fails to allocate has changed no colour).  Host records are copied to the device once, at the caller's
// stride, before anything resident changes.  A colour-only write rebuilds nothing: k_write_colors over the span.
int rtr_write_points(rtr_ctx *c, const uint32_t *select_words, uint64_t nwords, uint64_t first, uint64_t count, const float *xyz,
                     size_t xs, const uint8_t *rgb, size_t rs, uint64_t *total) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->n > 0, "rtr_write_points: no cloud");
    NEED(c, xyz || rgb, "rtr_write_points: nothing to write (xyz and rgb are both NULL)");
    const bool every = select_words == nullptr && nwords == 0;
    if (int rc = check_point_words(c, "rtr_write_points", "select_words", select_words, nwords, true, "", /*order_checked_later=*/true))
        return rc;
    NEED(c, !xyz || (xs >= 12 && xs % 4 == 0), "rtr_write_points: xyz_stride_bytes must be >= 12 and a multiple of 4");
    NEED(c, !rgb || rs >= 3 || rs == 0, "rtr_write_points: rgb_stride_bytes must be >= 3, or 0 for one record for every point");
    if (int rc = check_indexable(c)) return rc;
    if (!every)
        if (int rc = need_upload_order(c, "mapped", ", or write every point in the resident order (select_words NULL)")) return rc;
    DevGuard g(c->device);
    if (int rc = complete_all(c)) return rc;  // (frames issued before come out with the cloud they were issued with)
    hipStream_t s = c->stream;
    const uint64_t n = c->n, nw = (n + 31) / 32;
    const uint32_t *perm0 = c->reordered ? c->perm : nullptr;  // (sorted without point_ids, every point: rank = resident index)
    DevBufs buf;

    // the selection, its popcount scan and k, the number of selected points
    uint32_t *sel, *wscan, *selw;
    uint64_t *tot;  // span (first, last chunk), window units, pack mismatches, k
    uint64_t k = n;
    HIP_TRY(c, buf.get(&sel, nw * 4));
    HIP_TRY(c, buf.get(&wscan, nw * 4));
    HIP_TRY(c, buf.get(&selw, nw * 4));
    HIP_TRY(c, buf.get(&tot, 5 * sizeof(uint64_t)));
    void *measure;  // (cloud_edited's scratch: allocated with the rest, before anything is committed)
    HIP_TRY(c, buf.get(&measure, rtr::order_quality_scratch_bytes()));
    HIP_TRY(c, hipMemsetAsync(tot, 0, 5 * sizeof(uint64_t), s));
    if (!every) {
        uint32_t *scratch;
        HIP_TRY(c, buf.get(&scratch, rtr::scan_scratch_words(nw) * 4));
        HIP_TRY(c, hipMemcpyAsync(sel, select_words, nw * 4, hipMemcpyDefault, s));
        rtr::launch_scan_u32(s, sel, nw, n, wscan, scratch, tot + 4);
        HIP_TRY(c, hipMemcpyAsync(&k, tot + 4, sizeof k, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (int rc = launch_check(c, "write scan")) return rc;
    }
    if (total) *total = k;
    const uint64_t m = first < k ? std::min(count, k - first) : 0;
    if (m == 0) return RTR_OK;  // (a sizing call, or a window behind the selection: nothing changes)

    // the records on the device: only the bytes the call may read, a host stream copied once at the caller's stride
    const uint8_t *dxyz = (const uint8_t *)xyz, *drgb = rgb;
    if (xyz && !on_device(xyz)) {
        uint8_t *d;
        const size_t bytes = (m - 1) * xs + 12;
        HIP_TRY(c, buf.get(&d, bytes));
        HIP_TRY(c, hipMemcpyAsync(d, xyz, bytes, hipMemcpyHostToDevice, s));
        dxyz = d;
    }
    if (rgb && !on_device(rgb)) {
        uint8_t *d;
        const size_t bytes = (m - 1) * rs + 3;
        HIP_TRY(c, buf.get(&d, bytes));
        HIP_TRY(c, hipMemcpyAsync(d, rgb, bytes, hipMemcpyHostToDevice, s));
        drgb = d;
    }

    // the window's bits of the selection and the span of the chunks that hold them
    rtr::launch_write_bits(s, sel, wscan, n, every, first, m, selw);
    uint64_t c0 = 0, c1 = 0;
    bool any = false;
    if (int rc = chunk_span(c, selw, perm0, tot, "write span", &c0, &c1, &any)) return rc;
    if (!any) return RTR_OK;
    auto colours = [&] {
        if (drgb) rtr::launch_write_colors(s, perm0, selw, sel, wscan, n, c0, c1, drgb, rs, first, c->rgba);
    };
    if (!dxyz) {  // (colours only: no chunk box, header or packed block changes)
        colours();
        HIP_TRY(c, hipStreamSynchronize(s));
        if (int rc = launch_check(c, "write colours")) return rc;
        return cloud_edited(c, false, tot + 3, "written points", measure);
    }
    drop_soa(c);  // (SoA arrays decoded for a call in between are not kept: they would hold the old coordinates)
    const rtr::Cloud cl = cloud_of(c);
    auto fill = [&](float *wx, float *wy, float *wz, bool in_place) {
        rtr::launch_write_window(s, cl, perm0, selw, sel, wscan, c0, c1, dxyz, xs, first, wx, wy, wz, in_place);
    };
    if (int rc = rebuild_chunks(c, buf, c0, c1, tot, "write", fill, colours)) return rc;
    return cloud_edited(c, false, tot + 3, "written points", measure);
}

int rtr_reorder_points(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    DevGuard g(c->device);
    NEED(c, !c->keep_up || (c->opt_point_ids && (!c->reordered || c->perm)),
         "the cloud has a keep mask (rtr_set_point_keep), which a sort without option point_ids = 1 would lose: set "
         "point_ids = 1 before the upload, or clear the mask first");
    HIP_TRY(c, sync_streams(c));
    c->list_valid = false;
    c->pp_vis_current = false;
    if (int rc = ensure_soa(c)) return rc;
    // option "point_ids": the permutation travels with the points (starting from the identity while the cloud is in
    // upload order; a cloud sorted before without it has lost its upload order for good)
    // A failure up to and including the sort leaves the cloud as it was: the sort works on scratch copies and writes
    // nothing back before it has every one of them (rtr_reorder.hip), so what this call has made by then is taken back --
    // a permutation allocated here (it would stand filled with the identity beside `reordered` = 0), and the fp32
    // arrays decoded for the sort -- and a permutation that goes with this sort goes only behind it.
    const bool with_perm = c->opt_point_ids && (!c->reordered || c->perm);
    const bool perm_made = with_perm && !c->perm;
    auto as_it_was = [&]() {
        if (perm_made) dfree(c->perm);
        drop_soa(c);
    };
    if (perm_made) {
        const hipError_t ea = rtr::dev_malloc(&c->perm, c->cap * 4);
        if (ea != hipSuccess) {
            as_it_was();
            return fail(c, RTR_ERR_HIP, "rtr_reorder_points: allocating the permutation failed: %s", hipGetErrorString(ea));
        }
    }
    if (with_perm && !c->reordered) rtr::launch_iota(c->stream, c->perm, c->n);
    int e = rtr::reorder_morton(c->stream, c->x, c->y, c->z, c->rgba, c->n, with_perm ? c->perm : nullptr);
    if (e != 0) {
        (void)sync_streams(c);  // (the identity's launch may still be writing the permutation)
        as_it_was();
        return fail(c, RTR_ERR_HIP, "reorder failed: %s", hipGetErrorString((hipError_t)e));
    }
    if (!with_perm) dfree(c->perm);
    c->reordered = true;
    free_pack(c);
    rtr::launch_chunk_bounds(c->stream, cloud_of(c), c->bounds, c->spread);
    if (c->keep_up) rtr::launch_keep_build(c->stream, c->keep_up, c->perm, c->n, c->keep_res, c->keep_sum);  // (the mask follows)
    HIP_TRY(c, sync_streams(c));
    if (int rc = launch_check(c, "reorder")) return rc;
    if (int rc = pack_cloud(c)) return rc;
    drop_soa(c);
    return RTR_OK;
}

int rtr_num_points(const rtr_ctx *c, uint64_t *n) {
    if (!c || !n) return RTR_ERR_INVALID;
    *n = c->n;
    return RTR_OK;
}

int rtr_download_points(rtr_ctx *c, float *xyzw, uint8_t *rgba, uint64_t first, uint64_t count) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, xyzw && rgba, "output is NULL");
    NEED(c, first + count <= c->n, "range exceeds the resident cloud");
    if (count == 0) return RTR_OK;
    DevGuard g(c->device);
    if (int rc = ensure_soa(c)) return rc;  // (a cloud resident in packed form only is decoded for the copy, bit for bit)
    const uint64_t chunk = 1ull << 24;
    uint64_t m = count < chunk ? count : chunk;
    DevBufs buf;
    float *dx;
    uint8_t *dc;
    hipError_t ea = buf.get(&dx, m * 16);
    if (ea == hipSuccess) ea = buf.get(&dc, m * 4);
    if (ea != hipSuccess) {
        drop_soa(c);  // (decoded for this call only: a call that has run out of memory does not hold on to 12 B per point)
        return fail(c, RTR_ERR_HIP, "rtr_download_points: allocating the staging buffers failed: %s", hipGetErrorString(ea));
    }
    for (uint64_t off = 0; off < count; off += chunk) {
        uint64_t cnt = (count - off) < chunk ? (count - off) : chunk;
        uint64_t s0 = first + off;
        rtr::launch_soa_to_aos(c->stream, c->x + s0, c->y + s0, c->z + s0, c->rgba + s0, cnt, dx, dc);
        HIP_TRY(c, hipMemcpyAsync(xyzw + off * 4, dx, cnt * 16, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(rgba + off * 4, dc, cnt * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, sync_streams(c));
    }
    drop_soa(c);
    return launch_check(c, "soa_to_aos");
}

// ---- reading points back out (rtr.h, section 2e) ------------------------------------------------------------------
// Reads the cloud only, on the context's stream: one popcount scan of the selection words, then per internal window one
// launch of rtr::launch_extract, which decodes the chunks holding a point of the window and no others.  Device
// destinations are written by the kernel; host destinations go through a device staging window (at the caller's stride
// when every byte of a record is written -- 12 / 16 and 3 / 4 -- else tight, and the records are laid into the caller's
// memory by the host, so that the bytes between them stay).  No fp32 SoA is built for a packed-only cloud.
int rtr_extract_points(rtr_ctx *c, const uint32_t *select_words, uint64_t nwords, uint64_t first, uint64_t count, float *xyz,
                       size_t xs, uint8_t *rgb, size_t rs, uint32_t *indices, uint64_t *total) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->n > 0, "rtr_extract_points: no cloud");
    NEED(c, xyz || rgb || indices || total, "rtr_extract_points: nothing to produce (xyz, rgb, indices and total are all NULL)");
    const bool every = select_words == nullptr && nwords == 0;
    if (int rc = check_point_words(c, "rtr_extract_points", "select_words", select_words, nwords, true, "", /*order_checked_later=*/true))
        return rc;
    NEED(c, !xyz || (xs >= 12 && xs % 4 == 0), "rtr_extract_points: xyz_stride_bytes must be >= 12 and a multiple of 4");
    NEED(c, !rgb || rs >= 3, "rtr_extract_points: rgb_stride_bytes must be >= 3");
    if (int rc = check_indexable(c)) return rc;
    const bool lost_order = c->reordered && !c->perm;
    if (!every)
        if (int rc = need_upload_order(c, "mapped", ", or extract every point (select_words NULL)")) return rc;
    NEED(c, !(every && lost_order && indices),
         "the resident cloud was reordered without option point_ids = 1: every point comes out in the RESIDENT order and "
         "has no upload index, so indices must be NULL (set point_ids = 1 before the upload to get them)");
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const uint64_t n = c->n, nch = (n + 255) / 256;
    const uint32_t *perm = c->reordered ? c->perm : nullptr;
    DevBufs buf;

    // the selection's popcount scan and k, the number of selected points
    uint32_t *sel = nullptr, *wscan = nullptr;
    uint64_t k = n;
    if (!every) {
        uint32_t *scratch;
        uint64_t *tot;
        HIP_TRY(c, buf.get(&sel, nwords * 4));
        HIP_TRY(c, buf.get(&wscan, nwords * 4));
        HIP_TRY(c, buf.get(&scratch, rtr::scan_scratch_words(nwords) * 4));
        HIP_TRY(c, buf.get(&tot, sizeof(uint64_t)));
        HIP_TRY(c, hipMemcpyAsync(sel, select_words, nwords * 4, hipMemcpyDefault, s));
        rtr::launch_scan_u32(s, sel, nwords, n, wscan, scratch, tot);
        HIP_TRY(c, hipMemcpyAsync(&k, tot, sizeof k, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (int rc = launch_check(c, "extract scan")) return rc;
    }
    if (total) *total = k;
    const uint64_t produce = first < k ? std::min(count, k - first) : 0;
    if (produce == 0 || !(xyz || rgb || indices)) return RTR_OK;

    // the window: everything at once into device buffers, at most 2^24 points at a time through staging otherwise
    const bool xyz_dev = xyz && on_device(xyz), rgb_dev = rgb && on_device(rgb), idx_dev = indices && on_device(indices);
    const bool staged = (xyz && !xyz_dev) || (rgb && !rgb_dev) || (indices && !idx_dev);
    uint64_t win = produce;
    if (staged) win = std::min<uint64_t>(win, 1ull << 24);
    if (c->opt_debug_extract_window > 0) win = std::min<uint64_t>(win, (uint64_t)c->opt_debug_extract_window);
    // host streams whose records have gaps the call must not touch are staged tight and laid out by the host
    const bool xyz_gaps = xyz && !xyz_dev && xs != 12 && xs != 16, rgb_gaps = rgb && !rgb_dev && rs != 3 && rs != 4;
    const uint64_t sxs = xyz_gaps ? 12 : xs, srs = rgb_gaps ? 3 : rs;
    uint8_t *stx = nullptr, *stc = nullptr;
    uint32_t *sti = nullptr;
    if (xyz && !xyz_dev) HIP_TRY(c, buf.get(&stx, win * sxs + 16));
    if (rgb && !rgb_dev) HIP_TRY(c, buf.get(&stc, win * srs + 16));
    if (indices && !idx_dev) HIP_TRY(c, buf.get(&sti, win * 4));
    std::vector<uint8_t> bounce;
    if (xyz_gaps || rgb_gaps) bounce.resize(win * (xyz_gaps ? 12 : 3));

    const rtr::Cloud cl = cloud_of(c);
    rtr::ExtractArgs a{};
    a.pk = cl.pk;
    a.x4 = (const float4 *)cl.x, a.y4 = (const float4 *)cl.y, a.z4 = (const float4 *)cl.z;
    a.rgba4 = (const uint4 *)cl.rgba;
    a.perm = perm, a.sel = sel, a.wscan = wscan;
    a.n = n, a.total = k;
    for (uint64_t off = 0; off < produce; off += win) {
        const uint64_t w = std::min(win, produce - off);
        a.first = first + off, a.count = w;
        a.c0 = 0, a.c1 = nch;
        if (every && !perm) rtr::extract_all_chunks(a.first, w, &a.c0, &a.c1);
        a.xyz = !xyz ? nullptr : xyz_dev ? (uint8_t *)xyz + off * xs : stx;
        a.rgb = !rgb ? nullptr : rgb_dev ? rgb + off * rs : stc;
        a.idx = !indices ? nullptr : idx_dev ? indices + off : sti;
        a.xyz_stride = xyz_dev ? xs : sxs, a.rgb_stride = rgb_dev ? rs : srs;
        a.xyz_form = a.xyz_stride != 16 ? 0 : ((uintptr_t)a.xyz % 16 == 0 ? 2 : 1);
        a.rgb_form = a.rgb_stride != 4 ? 0 : ((uintptr_t)a.rgb % 4 == 0 ? 2 : 1);
        rtr::launch_extract(s, a);
        if (int rc = launch_check(c, "extract")) return rc;
        if (stx && !xyz_gaps) HIP_TRY(c, hipMemcpyAsync((uint8_t *)xyz + off * xs, stx, w * xs, hipMemcpyDeviceToHost, s));
        if (stc && !rgb_gaps) HIP_TRY(c, hipMemcpyAsync(rgb + off * rs, stc, w * rs, hipMemcpyDeviceToHost, s));
        if (sti) HIP_TRY(c, hipMemcpyAsync(indices + off, sti, w * 4, hipMemcpyDeviceToHost, s));
        if (xyz_gaps) {
            HIP_TRY(c, hipMemcpyAsync(bounce.data(), stx, w * 12, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            for (uint64_t j = 0; j < w; ++j) memcpy((uint8_t *)xyz + (off + j) * xs, bounce.data() + j * 12, 12);
        }
        if (rgb_gaps) {
            HIP_TRY(c, hipMemcpyAsync(bounce.data(), stc, w * 3, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            for (uint64_t j = 0; j < w; ++j) memcpy(rgb + (off + j) * rs, bounce.data() + j * 3, 3);
        }
        HIP_TRY(c, hipStreamSynchronize(s));  // (the staging window is reused; the call returns with the data in place)
    }
    return launch_check(c, "extract");
}

// ---- camera ------------------------------------------------------------------------

// project_cloud.cu:318 with project_cloud.h:50-59 and CameraCalibration.cpp:17-27:
// both glm transposes cancel, leaving P = K4 * E evaluated in fp32 (each entry the
// left-to-right sum of four separately rounded products), stored row-major.
int rtr_compose_projection(const double K[9], const double E[16], float P[16]) {
    if (!K || !E || !P) return RTR_ERR_INVALID;
    float K4[16] = {0}, Ef[16];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) K4[4 * r + q] = static_cast<float>(K[3 * r + q]);
    K4[15] = 1.0f;
    for (int i = 0; i < 16; ++i) Ef[i] = static_cast<float>(E[i]);
    for (int r = 0; r < 4; ++r)
        for (int q = 0; q < 4; ++q) {
            volatile float s = K4[4 * r + 0] * Ef[q];  // volatile: one rounding per op, no contraction
            volatile float t = K4[4 * r + 1] * Ef[4 + q];
            s = s + t;
            t = K4[4 * r + 2] * Ef[8 + q];
            s = s + t;
            t = K4[4 * r + 3] * Ef[12 + q];
            s = s + t;
            P[4 * r + q] = s;
        }
    return RTR_OK;
}

int rtr_set_resolution(rtr_ctx *c, int W, int H) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, W > 0 && H > 0 && (int64_t)W * H < (1ll << 31), "bad resolution");
    if (W == c->W && H == c->H) return RTR_OK;
    DevGuard g(c->device);
    HIP_TRY(c, sync_streams(c));
    free_frame(c);
    c->W = W; c->H = H;
    if (int rc = alloc_target(c, c->frame, 1)) {
        c->W = c->H = 0;
        return rc;
    }
    return RTR_OK;
}

// ---- phases ------------------------------------------------------------------------

int rtr_clear(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    if (int rc = check_frame(c)) return rc;
    DevGuard g(c->device);
    { Timed t(c, RTR_K_CLEAR); rtr::launch_clear(c->stream, c->frame.depth, c->frame.acc, (size_t)c->W * c->H); }
    return launch_check(c, "clear");
}

// The binned form keeps one LDS counter per screen tile (<= 4096 tiles: up to 3840 x 2160);
// larger frames fall back to the atomic form.
static bool use_tiles(const rtr_ctx *c) {
    return c->opt_mode == 1 && !c->force_atomic && rtr::tile_count(c->W, c->H) <= 4096;
}

// T1 of the tile-binned form: stream the cloud, append the in-frustum points to the tile store; its
// last workgroup writes the tile kernel's work list (and resets the tiles that will be split when
// the tile launches are the frame buffers' only writers: `clear_split`).
// With `overlapped` T1 goes to the front stream and fills the set the tail is NOT reading, so it
// runs beside T4 / the prefilter of the previous frame.
static int bin_points(rtr_ctx *c, const float P[16], bool overlapped, bool clear_split, bool no_split = false,
                      bool lean = false) {
    c->list_valid = false;
    c->last_lean = false;
    c->p2p.occ_current = false;
    c->p2p.occ_from_scan = false;
    hipStream_t s1 = c->stream;
    if (overlapped) {
        if (!c->ov.active) {  // (a streak begins: whatever the stream holds may still read either set)
            HIP_TRY(c, hipEventRecord(c->joined, c->stream));
            HIP_TRY(c, hipStreamWaitEvent(c->front, c->joined, 0));
        }
        c->frame.cur ^= 1;
        s1 = c->front;
        if (c->F().consumed_valid) HIP_TRY(c, hipStreamWaitEvent(c->front, c->F().consumed, 0));
    }
    if (int rc = ensure_pool(c, c->frame, c->F(), 0)) return rc;
    if (int rc = ensure_store(c, c->frame, c->F(), 0, s1)) return rc;
    auto &t = c->F().store;
    // (a lean frame's statistics are folded by the NEXT lean frame of its store: behind a bin with an epilogue that fold
    // would put the older frame's counts over the newer ones, so they are folded now)
    if (c->F().lean_pending && !lean) rtr::launch_lean_fold(s1, c->W, c->H, t, c->F().parity);
    c->F().lean_pending = lean;
    // (automatic: 8 bytes apart -- fewer cache lines for T1's epilogue to read and reset: -2 us on C3, -2.5 us on C2 --
    // unless tiles above the split threshold have been seen lately, where the claims of all waves queue on a dozen
    // counters and those want lines of their own; any spacing can follow any other, the counters are zero between frames)
    const bool heavy_seen = c->split_cooldown > 0 || __atomic_load_n(c->split_host, __ATOMIC_RELAXED) != 0u;
    t.fill_shift = c->opt_fill_shift >= 0 ? c->opt_fill_shift : (heavy_seen ? 4 : 1);
    if (int rc = next_seq(c, c->F(), s1)) return rc;
    bool binned_in_dispatch = false;
    {
        Timed tm(c, RTR_K_MIN_DEPTH, s1, true);
        // (a dispatch has one stop event: a bracketed T1 gives it to the bracket, and a lean frame of an empty cloud
        // launches nothing)
        binned_in_dispatch = (RTR_DISPATCH_EVENTS & 2) && overlapped && !tm.a && (c->n > 0 || !lean);
        rtr::launch_project_bin(s1, cloud_of(c), make_proj(P), c->W, c->H, t, c->opt_cull ? c->bounds : nullptr,
                                t1_flags(c, clear_split, no_split, lean), c->opt_phases, c->opt_xp, tm.a,
                                binned_in_dispatch ? c->F().binned : tm.b);
        c->p2p.occ_from_scan = c->p2p.open;
    }
    if (overlapped) {
        if (!binned_in_dispatch) HIP_TRY(c, hipEventRecord(c->F().binned, c->front));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->F().binned, 0));
    }
    memcpy(c->list_P, P, sizeof c->list_P);
    c->list_valid = true;
    return RTR_OK;
}

int rtr_min_depth_pass(rtr_ctx *c, const float P[16]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, P != nullptr, "P is NULL");
    if (int rc = check_frame(c)) return rc;
    DevGuard g(c->device);
    c->list_valid = false;
    c->jr.frame.count = 0;
    if (use_tiles(c)) {
        // (the phase calls' frames are consumed on the stream -- a sharded frame is reduced before anything synchronises
        // -- and no synchronising call can render them again: the extent pool is sized for the worst case at once)
        c->frame.pool_worst = true;
        if (int rc = bin_points(c, P, false, c->p2p.whole_frame)) return rc;
        Timed t(c, RTR_K_TILE);
        rtr::launch_tile(c->stream, 1, c->W, c->H, c->F().store, c->prm.depth_window, c->frame.depth, c->frame.acc, c->frame.img,
                         (c->p2p.whole_frame ? 6 : 0) | (c->F().parity << 4), nullptr);  // 2: only writer, 4: tiles without entries are not written
        mark_consumed(c);
    } else {
        if (int rc = ensure_soa(c)) return rc;
        Timed t(c, RTR_K_MIN_DEPTH);
        rtr::launch_min_depth(c->stream, cloud_of(c), make_proj(P), c->W, c->H, c->frame.depth);
    }
    return launch_check(c, "min_depth_pass");
}

int rtr_accumulate_pass(rtr_ctx *c, const float P[16]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, P != nullptr, "P is NULL");
    if (int rc = check_frame(c)) return rc;
    DevGuard g(c->device);
    // the bins are only usable for the matrix they were built with; otherwise re-project
    // the cloud like the reference does (render.cu:90-98)
    const bool use_bins = use_tiles(c) && c->list_valid && memcmp(c->list_P, P, sizeof c->list_P) == 0;
    c->p2p.acc_from_bins = use_bins && c->p2p.open && c->p2p.occ_current;
    if (c->p2p.whole_frame && !use_bins) return fail(c, RTR_ERR_INVALID, "rtr_p2p_render: the bins are not valid");
    if (use_bins) {
        // inside rtr_p2p_render with the default pyramid depth the tile kernel also emits the prefilter's
        // levels and min / max partials from the GLOBAL depth tile it has just loaded
        const rtr::TilePyr pyr = tile_pyr(c, c->frame, 0, c->p2p.whole_frame && c->p2p.pyramid_done);
        rtr::Sliced dsl{};
        if (c->p2p.whole_frame && c->p2p.depth_peers) {  // MIN over the occupying ranks' local depth, tile by tile
            dsl.src = c->p2p.depth;
            dsl.peers = c->p2p.world;
            dsl.occ_all = c->p2p.occ_all;
            dsl.out = c->p2p.red;  // (nobody reads `red` in this form; RTR_BUF_DEPTH is completed from it below)
            c->p2p.depth_in_red = true;
        } else if (c->p2p.whole_frame && c->p2p.depth_sliced) {
            dsl.src = c->p2p.reduced;
            dsl.chunk = p2p_slice(c).chunk;
        }
        c->p2p.depth_sliced = c->p2p.depth_peers = false;
        Timed t(c, RTR_K_TILE);
        rtr::launch_tile(c->stream, 2, c->W, c->H, c->F().store, c->prm.depth_window, c->frame.depth, c->frame.acc, c->frame.img,
                         c->p2p.whole_frame ? 6 : 0, pyr.enable ? &pyr : nullptr, (dsl.chunk || dsl.peers) ? &dsl : nullptr);
        mark_consumed(c);
    } else {
        if (int rc = ensure_soa(c)) return rc;
        Timed t(c, RTR_K_ACCUMULATE);
        rtr::launch_accumulate(c->stream, cloud_of(c), make_proj(P), c->W, c->H, c->frame.depth, c->frame.acc, c->prm.depth_window);
    }
    return launch_check(c, "accumulate_pass");
}

int rtr_resolve(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    if (int rc = check_frame(c)) return rc;
    DevGuard g(c->device);
    { Timed t(c, RTR_K_RESOLVE); rtr::launch_resolve(c->stream, c->frame.acc, c->frame.img, (size_t)c->W * c->H); }
    return launch_check(c, "resolve");
}

int rtr_resolve_range(rtr_ctx *c, const void *acc_dev, uint64_t first_pixel, uint64_t count) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    if (int rc = check_frame(c)) return rc;
    const uint64_t npix = (uint64_t)c->W * c->H;
    NEED(c, first_pixel % 4 == 0 && first_pixel + count <= npix, "bad pixel range (first must be a multiple of 4)");
    if (count == 0) return RTR_OK;
    DevGuard g(c->device);
    const uint32_t *src = acc_dev ? static_cast<const uint32_t *>(acc_dev) : c->frame.acc + first_pixel * 4;
    { Timed t(c, RTR_K_RESOLVE); rtr::launch_resolve(c->stream, src, c->frame.img + first_pixel * 3, (size_t)count); }
    return launch_check(c, "resolve_range");
}

static int filter_impl(rtr_ctx *c, int pyramid_parts, const rtr::Sliced *img_slices = nullptr,
                       const uint32_t *depth_src = nullptr) {
    if (int rc = check_frame(c)) return rc;
    DevGuard g(c->device);
    if (int rc = ensure_pyramid(c)) return rc;
    {
        Timed t(c, RTR_K_FILTER);
        rtr::launch_filter(c->stream, levels_of(c, c->frame, 0), c->frame.depth, c->frame.img, c->frame.mask, c->frame.tensor, c->frame.minmax, c->frame.part_min, c->frame.part_max,
                           c->W, c->H, c->prm.filter_strength, c->prm.gradient_threshold, pyramid_parts, img_slices,
                           depth_src);
    }
    return launch_check(c, "filter");
}

int rtr_filter(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    return filter_impl(c, 0);
}

// ---- whole frames ------------------------------------------------------------------

int rtr_render(rtr_ctx *c, const float P[16], int with_filter) {
    if (!c) return RTR_ERR_INVALID;
    NEED(c, P != nullptr, "P is NULL");
    if (int rc = check_frame(c)) return rc;
    c->jr.pass.behind = false;
    if (with_filter) {  // fail before touching the frame buffers
        DevGuard g(c->device);
        if (int rc = ensure_pyramid(c)) return rc;
    }
    int rc;
    bool fused = false;  // the tile launch has emitted the prefilter's pyramid
    if (use_tiles(c)) {  // one launch does clear + min + accumulate + resolve per tile
        DevGuard g(c->device);
        // (T1 beside the previous frame's tail must not touch the frame buffers: the split tiles' pixels are then
        // reset by a launch of their own on the tail's stream)
        bool overlapped = c->ov.frame(!c->p2p.open && (c->ov.mode == 1 || !c->p2p.red), with_filter != 0, c->W, c->H, c->cloud_seq);
        if (overlapped && !c->ov.active && !overlap_ready(c)) {
            c->ov.resources_failed();
            overlapped = false;
        }
        c->frame_overlapped = overlapped;
        bool split_launch = c->opt_heavy > 0;  // (split_threshold 0: nothing is ever split)
        if (split_launch) {
            if (__atomic_load_n(c->split_host, __ATOMIC_RELAXED) != 0u) c->split_cooldown = kSplitCooldown;
            split_launch = c->split_cooldown > 0;
            if (c->split_cooldown > 0) --c->split_cooldown;
        }
        // LEAN frames (rtr_kernels.h, ts_off_order): no split launch pending, no peers -- T1 ends without ticket and
        // epilogue, the tile workgroups read and reset the stream counters of the store they consume themselves.  The
        // parity is the store's: each of an overlapped streak's two stores sees every second frame
        const bool lean = c->opt_lean && !split_launch && !c->p2p.open;
        if ((rc = bin_points(c, P, overlapped, !overlapped, !split_launch, lean))) {
            c->frame_overlapped = false;
            c->ov.other_call();
            return rc;
        }
        if (lean) {
            c->F().parity ^= 1;
            c->last_lean = true;
        }
        if (overlapped && split_launch) rtr::launch_reset_split(c->stream, c->W, c->H, c->F().store, c->frame.depth, c->frame.acc);
        // with the default four levels the tile kernel also emits the prefilter's pyramid and
        // min / max partials (F1) while the finished depth tile is still in LDS
        fused = with_filter && c->prm.levels == 4;
        const rtr::TilePyr pyr = tile_pyr(c, c->frame, 0, fused);
        // (the store's last reader is the split launch where the frame has one)
        const hipEvent_t consumed = consumed_in_dispatch(c);
        {
            Timed t(c, RTR_K_TILE);
            rtr::launch_tile(c->stream, 0, c->W, c->H, c->F().store, c->prm.depth_window, c->frame.depth, c->frame.acc, c->frame.img,
                             c->opt_keep_accum | (lean ? lean_bits(c, c->frame) : 0) | (c->F().parity << 4), fused ? &pyr : nullptr,
                             nullptr, split_launch ? nullptr : consumed);
            if (lean) c->list_valid = false;  // (the tile launch has consumed and reset the stream counters)
            // tiles heavier than option "split_threshold" are split over several workgroups: a second launch takes
            // the minimum over each slice (they meet in the depth buffer), then -- behind a barrier over its 256
            // workgroups -- accumulates the slices against that minimum, and the last slice of each tile resolves it
            // (no work item on ordinary frames: its workgroups leave at once)
            if (split_launch)  // (skipped while no frame has had a tile above the threshold: see rtr_ctx::split_host)
                rtr::launch_tile(c->stream, 3, c->W, c->H, c->F().store, c->prm.depth_window, c->frame.depth, c->frame.acc, c->frame.img,
                                 c->opt_keep_accum, fused ? &pyr : nullptr, nullptr, consumed);
        }
        mark_consumed(c, consumed != nullptr);
        c->frame_overlapped = false;
        c->ov.frame_done(overlapped);
        if ((rc = launch_check(c, "tile frame"))) return rc;
        auto &rec = c->jr.frame;  // (what a synchronising call repeats if the adaptive pool overflowed)
        memcpy(rec.P, P, sizeof(float) * 16);
        rec.filter = with_filter;
        rec.count = 1;
        rec.clip = c->clip;
    } else {
        (void)c->ov.frame(false, false, c->W, c->H, c->cloud_seq);
        c->ov.frame_done(false);
        c->force_atomic = true;  // the phase calls below must not take the binned form either
        rc = rtr_clear(c);
        if (!rc) rc = rtr_min_depth_pass(c, P);
        if (!rc) rc = rtr_accumulate_pass(c, P);
        if (!rc) rc = rtr_resolve(c);
        c->force_atomic = false;
        if (rc) return rc;
    }
    if (with_filter) return filter_impl(c, fused ? rtr::tile_count(c->W, c->H) : 0);
    return RTR_OK;
}

static int frame_to_host(rtr_ctx *c, const float P[16], uint8_t *host_img, float *host_depth, int with_filter) {
    if (!c) return RTR_ERR_INVALID;
    if (!host_img && !host_depth) return fail(c, RTR_ERR_NO_OUTPUT, "both outputs are NULL (project_cloud.cu:270-273)");
    c->ov.other_call();
    if (int rc = rtr_render(c, P, with_filter)) return rc;
    DevGuard g(c->device);
    const size_t npix = (size_t)c->W * c->H;
    const Copy copies[2] = {{host_depth, c->frame.depth, npix * 4}, {host_img, c->frame.img, npix * 3}};
    HIP_TRY(c, queue_copies(c, copies, 2));
    HIP_TRY(c, sync_streams(c));
    rtr_ctx::Journal::Frames own;  // (after an overflow of the adaptive pool: this frame again, once)
    memcpy(own.P, P, sizeof(float) * 16);
    own.count = 1;
    own.filter = with_filter;
    own.clip = c->clip;
    return repair(c, c->frame, false, copies, 2, &own);
}

int rtr_project(rtr_ctx *c, const float P[16], uint8_t *host_img, float *host_depth) {
    return frame_to_host(c, P, host_img, host_depth, 0);
}

// ---- asynchronous host outputs ------------------------------------------------------------
// The reference's call shape pays kernels + 14.5 MB over PCIe per 1080p frame, one after the other
// (project_cloud.cu:302-309,424-431).  Here frame k's copies run on a second stream (the SDMA engines) beside
// frame k + 1's kernels: depth and image are snapshotted on the device first (two device copies, ~10 us), so the
// frame buffers are free again at once.

static int ensure_host_out(rtr_ctx *c) {
    if (!c->copy_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    const size_t npix = (size_t)c->W * c->H;
    for (auto &h : c->ho) {
        if (h.img) continue;
        // (a slot is complete or empty: h.img is what says it exists, so after a failure the slot holds nothing and the
        // next call makes it again.  Slots completed before stay)
        hipError_t e = rtr::host_malloc(&h.img, (npix * 3 + 15) & ~(size_t)15, hipHostMallocMapped);
        if (e == hipSuccess) e = rtr::host_malloc(&h.depth, (npix * 4 + 15) & ~(size_t)15, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&h.img_map, h.img, 0);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&h.depth_map, h.depth, 0);
        if (e == hipSuccess) e = rtr::dev_malloc(&h.dimg, (npix * 3 + 15) & ~(size_t)15);
        if (e == hipSuccess) e = rtr::dev_malloc(&h.ddepth, (npix * 4 + 15) & ~(size_t)15);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h.snap, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h.done, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)rtr::host_free(h.img); (void)rtr::host_free(h.depth);
            dfree(h.dimg); dfree(h.ddepth);
            if (h.snap) (void)hipEventDestroy(h.snap);
            if (h.done) (void)hipEventDestroy(h.done);
            h = rtr_ctx::HostOut{};
            return fail(c, RTR_ERR_HIP, "allocating the asynchronous host outputs failed: %s", hipGetErrorString(e));
        }
    }
    return RTR_OK;
}

int rtr_host_output_buffers(rtr_ctx *c, int slot, uint8_t **img, float **depth) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, slot >= 0 && slot < RTR_ASYNC_SLOTS, "slot out of range");
    if (int rc = check_frame(c)) return rc;
    DevGuard g(c->device);
    if (int rc = ensure_host_out(c)) return rc;
    if (img) *img = c->ho[slot].img;
    if (depth) *depth = c->ho[slot].depth;
    return RTR_OK;
}

// queues frame P into `slot`: render, snapshot on the device, copy to the pinned buffers on the copy stream
static int queue_slot(rtr_ctx *c, const float P[16], int slot, int with_filter) {
    auto &h = c->ho[slot];
    // (the slot's previous frame may still be on its way to the host: its snapshot must not be overwritten yet)
    if (h.busy) HIP_TRY(c, hipStreamWaitEvent(c->stream, h.done, 0));
    if (int rc = rtr_render(c, P, with_filter)) return rc;
    const size_t npix = (size_t)c->W * c->H;
    HIP_TRY(c, hipMemcpyAsync(h.ddepth, c->frame.depth, npix * 4, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h.dimg, c->frame.img, npix * 3, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(h.snap, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, h.snap, 0));
    rtr::launch_copy_to_host(c->copy_stream, h.ddepth, h.depth_map, npix * 4, h.dimg, h.img_map, npix * 3);
    HIP_TRY(c, hipEventRecord(h.done, c->copy_stream));
    auto &f = c->jr.slot[slot];
    memcpy(f.P, P, sizeof f.P);
    f.filter = with_filter;
    f.stale = false;
    f.sealed = false;
    f.cloud = c->cloud_seq;
    f.clip = c->clip;
    h.busy = true;
    return RTR_OK;
}

int rtr_project_async(rtr_ctx *c, const float P[16], int slot, int with_filter) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, P != nullptr, "P is NULL");
    NEED(c, slot >= 0 && slot < RTR_ASYNC_SLOTS, "slot out of range");
    if (int rc = check_frame(c)) return rc;
    DevGuard g(c->device);
    if (int rc = ensure_host_out(c)) return rc;
    return queue_slot(c, P, slot, with_filter);
}

int rtr_wait(rtr_ctx *c, int slot) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, slot >= -1 && slot < RTR_ASYNC_SLOTS, "slot out of range (-1: every slot)");
    DevGuard g(c->device);
    for (int k = 0; k < RTR_ASYNC_SLOTS; ++k)
        if ((slot < 0 || k == slot) && c->ho[k].busy) HIP_TRY(c, hipEventSynchronize(c->ho[k].done));
    const int rc = repair(c, c->frame, true);  // (after an overflow: the stale slots, then the last whole frame)
    // (a slot repeated there has queued its copies again, on the copy stream: they are finished before it is free)
    for (int k = 0; k < RTR_ASYNC_SLOTS; ++k)
        if ((slot < 0 || k == slot) && c->ho[k].busy) HIP_TRY(c, hipEventSynchronize(c->ho[k].done));
    for (int k = 0; k < RTR_ASYNC_SLOTS; ++k)
        if (slot < 0 || k == slot) c->ho[k].busy = false;
    return rc;
}

int rtr_project_filtered(rtr_ctx *c, const float P[16], uint8_t *host_img, float *host_depth) {
    return frame_to_host(c, P, host_img, host_depth, 1);
}

// ---- peer-to-peer exchange ------------------------------------------------------------

static int p2p_alloc_parts(rtr_ctx *c) {
    auto &q = c->p2p;
    const size_t npix = (size_t)c->W * c->H;
    if (!q.red) HIP_TRY(c, rtr::dev_malloc(&q.red, ((npix + 3) & ~(size_t)3) * sizeof(uint32_t)));
    if (!q.ximg) HIP_TRY(c, rtr::dev_malloc(&q.ximg, (npix * 3 + 15) & ~(size_t)15));
    if (!q.occ) HIP_TRY(c, rtr::dev_malloc(&q.occ, rtr::kP2POccBytes));
    if (!q.occ_all) HIP_TRY(c, rtr::dev_malloc(&q.occ_all, (size_t)rtr::kMaxPeers * rtr::kP2POccBytes));
    if (!q.flags) {
        HIP_TRY(c, rtr::dev_malloc_uncached(&q.flags, 4096));
        // (every word starts at the barrier number the exchange starts at -- 0, or option "debug_p2p_barrier" -- and is
        // filled HERE, before the handles leave rtr_p2p_export: a peer that opens first may already have written its
        // first barrier into them by the time this rank opens)
        // (the option is read HERE only: rtr_p2p_open starts the counter at what the words were filled with)
        if (c->opt_debug_p2p_barrier == -1) HIP_TRY(c, hipMemsetAsync(q.flags, 0, 4096, c->stream));
        else HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)q.flags, c->opt_debug_p2p_barrier, 4096 / 4, c->stream));
        q.start = c->opt_debug_p2p_barrier == -1 ? 0u : (uint32_t)c->opt_debug_p2p_barrier;
        HIP_TRY(c, sync_streams(c));
    }
    if (!q.status_host) HIP_TRY(c, mapped_word(&q.status_host, &q.status_dev));
    return RTR_OK;
}

// this rank's exchange buffers (per resolution), all or nothing: `red` is what says "exported" to the rest of the file
// (free_lists, ensure_pool, rtr_render's overlap condition) and rtr_p2p_open takes the set for complete, so after a
// failure none of them is kept and the next rtr_p2p_export makes them again
static int p2p_alloc(rtr_ctx *c) {
    const int rc = p2p_alloc_parts(c);
    if (rc != RTR_OK) p2p_release(c);
    return rc;
}

int rtr_p2p_export(rtr_ctx *c, rtr_p2p_handles *mine) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, mine != nullptr, "handles is NULL");
    if (int rc = check_frame(c)) return rc;
    static_assert(sizeof(hipIpcMemHandle_t) <= 64, "handle block too small");
    NEED(c, c->ov.mode != 1, "the peer-to-peer exchange needs option overlap off (the peers map ONE tile store)");
    DevGuard g(c->device);
    HIP_TRY(c, sync_streams(c));
    // (the owner-computes form reads the peers' tile stores: allocate this rank's now -- it is sized by the cloud, for
    // the worst case: a pool the peers have mapped must never move)
    c->frame.cur = 0;
    // (pool_worst is what makes ensure_pool size the pool for the worst case, so it is set ahead of that allocation; it
    // describes an exported pool, and an export that fails takes it back: later frames size their pool as before)
    const bool worst_before = c->frame.pool_worst;
    c->frame.pool_worst = true;
    int rc_alloc = ensure_pool(c, c->frame, c->F(), 0);
    if (!rc_alloc) rc_alloc = ensure_store(c, c->frame, c->F(), 0, c->stream);
    if (!rc_alloc) rc_alloc = p2p_alloc(c);
    if (rc_alloc) {
        c->frame.pool_worst = worst_before;
        return rc_alloc;
    }
    HIP_TRY(c, sync_streams(c));
    memset(mine, 0, sizeof *mine);
    void *bufs[9] = {c->frame.depth, c->frame.acc, c->p2p.ximg, c->p2p.red, c->p2p.flags, c->p2p.occ,
                     c->F().store.meta, c->F().store.ext0, c->F().dyn};
    unsigned char *dst[9] = {mine->depth, mine->accum, mine->image, mine->reduced, mine->flags, mine->tiles,
                             mine->store_meta, mine->store_ext0, mine->store_dyn};
    for (int k = 0; k < 9; ++k) {
        hipIpcMemHandle_t h;
        HIP_TRY(c, hipIpcGetMemHandle(&h, bufs[k]));
        memcpy(dst[k], &h, sizeof h);
    }
    return RTR_OK;
}

int rtr_p2p_open(rtr_ctx *c, int rank, int world, const rtr_p2p_handles *all) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, all != nullptr, "handles is NULL");
    NEED(c, world >= 1 && world <= RTR_P2P_MAX_RANKS && rank >= 0 && rank < world, "bad rank / world");
    if (int rc = check_frame(c)) return rc;
    DevGuard g(c->device);
    HIP_TRY(c, sync_streams(c));
    auto &q = c->p2p;
    NEED(c, q.red && q.ximg && q.flags && q.occ, "rtr_p2p_export has not been called for this resolution");
    NEED(c, !q.open, "already open (rtr_p2p_close first)");
    NEED(c, c->F().store.meta && c->F().store.ext0 && c->F().dyn, "the tile store changed since rtr_p2p_export (export again)");
    rtr::PeerSet *sets[9] = {&q.depth, &q.accum, &q.image, &q.reduced, &q.flags_of, &q.occ_of, &q.meta_of, &q.ext0_of, &q.dyn_of};
    void *own[9] = {c->frame.depth, c->frame.acc, q.ximg, q.red, q.flags, q.occ, c->F().store.meta, c->F().store.ext0, c->F().dyn};
    for (int r = 0; r < world; ++r) {
        const unsigned char *src[9] = {all[r].depth, all[r].accum, all[r].image, all[r].reduced, all[r].flags, all[r].tiles,
                                       all[r].store_meta, all[r].store_ext0, all[r].store_dyn};
        for (int k = 0; k < 9; ++k) {
            if (r == rank) {
                sets[k]->p[r] = own[k];
                continue;
            }
            hipIpcMemHandle_t h;
            memcpy(&h, src[k], sizeof h);
            void *ptr = nullptr;
            hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) {
                int rc = fail(c, RTR_ERR_HIP, "hipIpcOpenMemHandle (rank %d, buffer %d) failed: %s", r, k, hipGetErrorString(e));
                p2p_release(c);
                return rc;
            }
            q.opened[k][r] = ptr;
            sets[k]->p[r] = ptr;
        }
    }
    {   // the owner-computes form's pointer table, in device memory
        rtr::OwnedTab tab{};
        for (int r = 0; r < world; ++r) {
            tab.meta[r] = static_cast<const uint32_t *>(q.meta_of.p[r]);
            tab.ext0[r] = static_cast<const uint64_t *>(q.ext0_of.p[r]);
            tab.dyn[r] = static_cast<const uint64_t *>(q.dyn_of.p[r]);
            tab.depth[r] = static_cast<const uint32_t *>(q.depth.p[r]);
            tab.ximg[r] = static_cast<const uint8_t *>(q.image.p[r]);
        }
        hipError_t e = q.tab ? hipSuccess : rtr::dev_malloc(&q.tab, sizeof tab);
        if (e == hipSuccess) e = hipMemcpy(q.tab, &tab, sizeof tab, hipMemcpyHostToDevice);
        if (e != hipSuccess) {  // (as for a handle that does not open: the mappings made so far must not outlive the call)
            int rc = fail(c, RTR_ERR_HIP, "the peers' pointer table failed: %s", hipGetErrorString(e));
            p2p_release(c);
            return rc;
        }
    }
    q.rank = rank;
    q.world = world;
    q.seq = q.start;  // (0, or option "debug_p2p_barrier" as it was when this rank's flag words were filled)
    q.open = true;
    *q.status_host = 0;
    return RTR_OK;
}

int rtr_p2p_close(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    DevGuard g(c->device);
    HIP_TRY(c, sync_streams(c));
    p2p_release(c);
    return RTR_OK;
}

int rtr_p2p_status(rtr_ctx *c, uint32_t *barrier_timeouts) {
    if (!c || !barrier_timeouts) return RTR_ERR_INVALID;
    *barrier_timeouts = c->p2p.status_host ? *c->p2p.status_host : 0u;
    return RTR_OK;
}

namespace {
void p2p_barrier(rtr_ctx *c) {
    auto &q = c->p2p;
    const unsigned long long ticks = 100000ull * (unsigned long long)c->opt_p2p_timeout_ms;  // 100 MHz wall clock
    rtr::launch_p2p_sync(c->stream, q.flags, q.flags_of, q.rank, q.world, ++q.seq, q.status_dev, ticks);
}
}  // namespace

int rtr_p2p_min_depth(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    if (int rc = check_frame(c)) return rc;
    NEED(c, c->p2p.open, "rtr_p2p_open has not been called");
    DevGuard g(c->device);
    auto &q = c->p2p;
    const Slice s = p2p_slice(c);
    const size_t npix = (size_t)c->W * c->H;
    // which screen tiles this rank's frame touches at all (only known when it came from the bins)
    const bool binned = use_tiles(c) && c->list_valid;
    if (!(binned && q.occ_from_scan))  // otherwise the scan kernel of the tile sort has already written it
        rtr::launch_p2p_occupancy(c->stream, binned ? rtr::ts_tile_cnt(c->F().store) : nullptr, c->W, c->H, q.occ);
    q.occ_current = binned;
    q.acc_from_bins = false;
    p2p_barrier(c);  // every rank's local depth (and occupancy) is complete
    rtr::launch_p2p_depth_reduce(c->stream, q.depth, q.occ_of, q.red, s.first, s.count, q.world, c->W, c->H);
    p2p_barrier(c);  // every slice is reduced; nobody reads the local depth buffers any more
    if (q.whole_frame)
        q.depth_sliced = true;  // the accumulate launch reads the slices tile by tile and stores the result
    else
        rtr::launch_p2p_gather(c->stream, q.reduced, c->frame.depth, s.chunk * 4, npix * 4, -1);
    return launch_check(c, "p2p_min_depth");
}

int rtr_p2p_sum_resolve(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    if (int rc = check_frame(c)) return rc;
    NEED(c, c->p2p.open, "rtr_p2p_open has not been called");
    DevGuard g(c->device);
    auto &q = c->p2p;
    const Slice s = p2p_slice(c);
    const size_t npix = (size_t)c->W * c->H, nbytes = npix * 3;
    if (!q.acc_from_bins)  // accumulated by the atomic form (or no depth exchange before): nothing is known
        rtr::launch_p2p_occupancy(c->stream, nullptr, c->W, c->H, q.occ);
    p2p_barrier(c);  // every rank's accumulators are complete (and its reduced-depth slice has been read)
    rtr::launch_p2p_acc_resolve(c->stream, q.accum, q.occ_of, q.ximg, s.first, s.count, q.world, c->W, c->H);
    p2p_barrier(c);  // every image slice is resolved; nobody reads the accumulators any more
    if (q.whole_frame && q.pyramid_done)
        q.image_sliced = true;  // the fused prefilter reads the slices itself and writes RTR_BUF_IMAGE
    else
        rtr::launch_p2p_gather(c->stream, q.image, c->frame.img, s.chunk * 3, nbytes, -1);
    return launch_check(c, "p2p_sum_resolve");
}

int rtr_p2p_render(rtr_ctx *c, const float P[16], int with_filter) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, P != nullptr, "P is NULL");
    NEED(c, c->p2p.open, "rtr_p2p_open has not been called");
    if (with_filter) {  // fail before any rank enters a barrier the others would wait in
        DevGuard g(c->device);
        if (int rc = ensure_pyramid(c)) return rc;
    }
    // In the tile-binned form both tile launches of the frame visit every pixel, so they can be the
    // only writers of the depth buffer / accumulators (no clear, no read-modify-write), and the
    // accumulate launch -- which loads the GLOBAL depth tile -- can emit the prefilter's pyramid.
    auto &q = c->p2p;
    q.whole_frame = use_tiles(c);
    q.pyramid_done = q.whole_frame && with_filter && c->prm.levels == 4;
    int rc = q.whole_frame ? RTR_OK : rtr_clear(c);
    if (!rc) rc = rtr_min_depth_pass(c, P);
    if (!rc && q.whole_frame && c->list_valid && q.occ_from_scan) {
        // Tile-binned frame: ONE barrier (every rank's min pass and occupancy bitmap are complete; the same
        // launch gathers the bitmaps), then the accumulate launch takes the MIN over the occupying ranks' local
        // depth tile by tile -- no slice reduction, no second barrier (the barrier in front of the colour
        // exchange is what tells a rank that nobody reads its depth buffer any more).
        DevGuard g(c->device);
        q.occ_current = true;
        q.acc_from_bins = false;
        const unsigned long long ticks = 100000ull * (unsigned long long)c->opt_p2p_timeout_ms;
        rtr::launch_p2p_sync_gather(c->stream, q.flags, q.flags_of, q.rank, q.world, ++q.seq, q.status_dev, ticks, q.occ_of,
                                    q.occ_all);
        q.depth_peers = true;
        rc = launch_check(c, "p2p barrier");
    } else if (!rc) {
        rc = rtr_p2p_min_depth(c);
    }
    if (!rc) rc = rtr_accumulate_pass(c, P);
    if (!rc) rc = rtr_p2p_sum_resolve(c);
    const int parts = q.pyramid_done ? rtr::tile_count(c->W, c->H) : 0;
    rtr::Sliced isl{};
    if (q.image_sliced) {
        isl.src = q.image;
        isl.chunk = p2p_slice(c).chunk;
    }
    // One-barrier form: the completed depth lies in `red`.  Every rank is past its accumulate launch (the barriers
    // of the colour exchange), so nobody reads this rank's depth buffer any more: the fused prefilter reads `red`
    // and writes RTR_BUF_DEPTH; without a prefilter (or with another pyramid depth) a device copy completes it.
    const bool from_red = q.depth_in_red;
    const bool fused = with_filter && c->prm.levels == 4;
    q.whole_frame = q.pyramid_done = q.depth_sliced = q.depth_peers = q.image_sliced = q.depth_in_red = false;
    if (!rc && from_red && !fused) {
        DevGuard g(c->device);
        HIP_TRY(c, hipMemcpyAsync(c->frame.depth, q.red, (size_t)c->W * c->H * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    }
    if (!rc && with_filter) rc = filter_impl(c, parts, isl.chunk ? &isl : nullptr, (from_red && fused) ? q.red : nullptr);
    return rc;
}

// Owner-computes form of the sharded frame (rtr.h 5b): T1 -> barrier (+ every rank's occupancy bitmap) -> ONE fused tile
// launch over the tiles tile_owner() gives to this rank, reading the other occupying ranks' entries out of their tile
// stores -> barrier -> on the frame's owner only: collect the other ranks' tiles (+ pyramid) -> prefilter.  Six launches,
// two barriers, no MIN / SUM exchange; the next frame's first barrier is what keeps a rank from overwriting tiles the
// previous frame's owner is still collecting (that owner arrives at it only behind its collect and prefilter).
int rtr_p2p_render_owned(rtr_ctx *c, const float P[16], int with_filter, int frame_owner) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, P != nullptr, "P is NULL");
    NEED(c, c->p2p.open, "rtr_p2p_open has not been called");
    auto &q = c->p2p;
    NEED(c, frame_owner >= 0 && frame_owner < q.world, "frame_owner out of range");
    NEED(c, use_tiles(c), "the owner-computes form needs the tile-binned mode (option mode = 1, <= 4096 tiles)");
    NEED(c, c->ov.mode != 1, "the owner-computes form does not combine with option overlap");
    const bool mine = frame_owner == q.rank;
    DevGuard g(c->device);
    if (with_filter && mine)  // (fail before any rank enters a barrier the others would wait in)
        if (int rc = ensure_pyramid(c)) return rc;
    const bool fused = with_filter && c->prm.levels == 4;
    if (int rc = bin_points(c, P, false, false)) return rc;
    NEED(c, c->F().store.meta == q.meta_of.p[q.rank] && c->F().dyn == q.dyn_of.p[q.rank],
         "the tile store changed since rtr_p2p_export (export and open again)");
    const unsigned long long ticks = 100000ull * (unsigned long long)c->opt_p2p_timeout_ms;
    // every rank's stream lengths and occupancy bitmap are final (and gathered into local memory)
    rtr::launch_p2p_sync_gather(c->stream, q.flags, q.flags_of, q.rank, q.world, ++q.seq, q.status_dev, ticks, q.occ_of, q.occ_all);
    const rtr::TilePyr pyr = tile_pyr(c, c->frame, 0, mine && fused);
    rtr::Sliced dsl{};
    dsl.occ_all = q.occ_all;
    dsl.peers = q.world;
    dsl.rank = q.rank;
    dsl.tab = q.tab;
    {   // the frame's owner writes its tiles where the frame ends up; everybody else into the buffers the owner reads
        Timed t(c, RTR_K_TILE);
        rtr::launch_tile(c->stream, 4, c->W, c->H, c->F().store, c->prm.depth_window, c->frame.depth, c->frame.acc, mine ? c->frame.img : q.ximg,
                         c->opt_keep_accum, pyr.enable ? &pyr : nullptr, &dsl);
    }
    mark_consumed(c);
    p2p_barrier(c);  // every tile of the frame is final on the rank that produced it; nobody reads a tile store any more
    if (int rc = launch_check(c, "owned tile frame")) return rc;
    if (!mine) return RTR_OK;
    rtr::launch_p2p_collect(c->stream, c->W, c->H, q.tab, q.occ_all, q.world, q.rank, c->frame.depth, c->frame.img, pyr.enable ? &pyr : nullptr);
    if (int rc = launch_check(c, "collect")) return rc;
    if (with_filter) return filter_impl(c, pyr.enable ? rtr::tile_count(c->W, c->H) : 0);
    return RTR_OK;
}

// ---- point pass ----------------------------------------------------------------------
// Which points the frame in the depth buffer shows (rtr.h section 6b): one stream over the RESIDENT coordinates
// (rtr_kernels.hip, k_point_pass), queued behind the frame like the phase calls.  The ID buffer is cleared here, not by
// the frame; the visibility mask only when its bits go through the permutation (in upload order every word is stored).

int rtr_point_pass(rtr_ctx *c, const float P[16], int what) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, P != nullptr, "P is NULL");
    NEED(c, what >= 1 && what <= 3, "what must be a non-empty mask of RTR_POINTS_IDS (1) and RTR_POINTS_VISIBLE (2)");
    NEED(c, c->cap > 0, "no cloud: rtr_upload_points / rtr_generate_synthetic first");
    if (int rc = check_frame(c)) return rc;
    if (c->n >= (1ull << 32)) return fail(c, RTR_ERR_UNSUPPORTED, "point IDs are 32-bit: the cloud has %llu points", (unsigned long long)c->n);
    if (int rc = need_upload_order(c, "formed")) return rc;
    DevGuard g(c->device);
    const size_t npix = (size_t)c->W * c->H;
    const uint64_t words = (((c->n + 3) / 4 + 63) / 64) * 8;  // (8 per 256-point chunk: whole-chunk stores)
    if (!c->pp_done) HIP_TRY(c, hipEventCreateWithFlags(&c->pp_done, hipEventDisableTiming));
    // (a buffer of point IDs exists only once a pass has filled it: RTR_BUF_POINT_ID serves whatever pp_ids holds, so one
    // made here goes again when the call fails before its launch)
    const bool ids_made = (what & RTR_POINTS_IDS) && !c->pp_ids;
    if (ids_made) HIP_TRY(c, rtr::dev_malloc(&c->pp_ids, npix * 4));
    if ((what & RTR_POINTS_VISIBLE) && (!c->pp_vis || c->pp_vis_words < words)) {
        HIP_TRY(c, sync_streams(c));  // (a pass in flight may still write the old mask)
        dfree(c->pp_vis);
        // (the size and "current" describe the mask: without one, after a failure, they say so -- RTR_BUF_VISIBLE then
        // answers as before any pass -- and the size is set behind the allocation)
        c->pp_vis_words = 0;
        c->pp_vis_current = false;
        const uint64_t want = words > 8 ? words : 8;
        const hipError_t e = rtr::dev_malloc(&c->pp_vis, want * 4);
        if (e != hipSuccess) {
            if (ids_made) dfree(c->pp_ids);
            return fail(c, RTR_ERR_HIP, "rtr_point_pass: allocating the visibility mask failed: %s", hipGetErrorString(e));
        }
        c->pp_vis_words = want;
    }
    uint32_t *ids = (what & RTR_POINTS_IDS) ? c->pp_ids : nullptr, *vis = (what & RTR_POINTS_VISIBLE) ? c->pp_vis : nullptr;
    const uint32_t *perm = c->reordered ? c->perm : nullptr;
    if (ids) HIP_TRY(c, hipMemsetAsync(ids, 0xFF, npix * 4, c->stream));
    if (vis && (perm || words == 0)) HIP_TRY(c, hipMemsetAsync(vis, 0, c->pp_vis_words * 4, c->stream));
    rtr::launch_point_pass(c->stream, cloud_of(c), make_proj(P), c->W, c->H, c->frame.depth, c->prm.depth_window, ids, vis, perm);
    if (int rc = launch_check(c, "point_pass")) return rc;
    HIP_TRY(c, hipEventRecord(c->pp_done, c->stream));
    if (vis) c->pp_vis_current = true;
    auto &pass = c->jr.pass;  // (what a synchronising call repeats with the frame: repair)
    memcpy(pass.P, P, sizeof pass.P);
    pass.what = what;
    pass.behind = c->jr.frame.count > 0;
    pass.unchecked = true;
    pass.invalid = false;
    pass.clip = c->clip;
    return RTR_OK;
}

// ---- several views -----------------------------------------------------------------
// rtr_render_views (rtr.h, section 6c).  Binned batches: ONE point-kernel launch appends every view's points to that
// view's tile store (rtr::launch_project_bin_views), then per view a lean tile launch (and the prefilter) writes the
// view's slices of the batch buffers.  Every other form loops over the atomic form into the same slices.  Neither
// touches the single frame's target, its journal entries or the asynchronous slots.
// The views' extent pools are adaptive like the single frame's (sized by the densest frame or view seen); a batch that
// overflows one reports it through the views' own mapped word, and the next synchronising call (rtr_synchronize, a
// download of RTR_BUF_VIEW_*) sizes every view's pool for the worst case -- 16 B per point and view -- and repeats the
// batch (repair).

static bool views_binned(const rtr_ctx *c) {  // the binned form serves batches; the rest loop over the atomic form
    return c->opt_mode == 1 && rtr::tile_count(c->W, c->H) <= 4096 && !c->p2p.open && c->ov.mode != 1;
}

// buffers, scratch and (binned) tile stores / pools for `count` views at this resolution and cloud
static int ensure_views(rtr_ctx *c, int count, int with_filter) {
    auto &v = c->views;
    if (count > v.cap) {
        HIP_TRY(c, sync_streams(c));  // (a batch in flight may still write the old buffers)
        c->jr.views.count = 0;
        if (int rc = alloc_target(c, v, count)) return rc;
    }
    if (with_filter)
        if (int rc = ensure_levels(c, v)) return rc;
    auto &tab = c->vtab;
    if (!tab.host) {  // (all or nothing: tab.host is what says the three exist)
        hipError_t e = rtr::host_malloc(&tab.host, rtr::view_tab_bytes(), hipHostMallocDefault);
        if (e == hipSuccess) e = rtr::dev_malloc(&tab.dev, rtr::view_tab_bytes());
        if (e == hipSuccess) e = hipEventCreateWithFlags(&tab.copied, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)rtr::host_free(tab.host);
            dfree(tab.dev);
            if (tab.copied) (void)hipEventDestroy(tab.copied);
            tab = rtr_ctx::ViewTab{};
            return fail(c, RTR_ERR_HIP, "allocating the views' table failed: %s", hipGetErrorString(e));
        }
    }
    if (!views_binned(c)) return ensure_soa(c);
    for (int k = 0; k < count; ++k) {
        // (pools: the single frame's adaptive rule over the densest frame OR view seen)
        if (int rc = ensure_pool(c, v, v.fs[k], c->frame.entries_max)) return rc;
        if (int rc = ensure_store(c, v, v.fs[k], k, c->stream)) return rc;
    }
    return RTR_OK;
}

// the frame of view k: tile launch (binned) or the atomic form, then the prefilter, into the view's slices
static int views_enqueue(rtr_ctx *c, int count, const float *P, int with_filter) {
    auto &v = c->views;
    if (int rc = ensure_views(c, count, with_filter)) return rc;
    const size_t npix = (size_t)c->W * c->H;
    const bool binned = views_binned(c);
    const bool pyr_fused = binned && with_filter && c->prm.levels == 4;
    if (binned) {
        rtr::Proj proj[RTR_MAX_VIEWS];
        rtr::TileStore st[RTR_MAX_VIEWS];
        for (int k = 0; k < count; ++k) {
            v.fs[k].store.fill_shift = c->opt_fill_shift >= 0 ? c->opt_fill_shift : 1;
            if (int rc = next_seq(c, v.fs[k], c->stream)) return rc;
            proj[k] = make_proj(P + 16 * k);
            st[k] = v.fs[k].store;
        }
        if (count == 1) {  // (one view: the single frame's lean point kernel -- the table and the view loops cost ~15 us)
            Timed tm(c, RTR_K_MIN_DEPTH, c->stream, true);
            rtr::launch_project_bin(c->stream, cloud_of(c), proj[0], c->W, c->H, st[0], c->opt_cull ? c->bounds : nullptr,
                                    t1_flags(c, false, true, true), c->opt_phases, 0, tm.a, tm.b);
        } else {
            auto &tab = c->vtab;
            if (tab.pending) HIP_TRY(c, hipEventSynchronize(tab.copied));  // (the table's last copy has been read)
            {
                Timed tm(c, RTR_K_MIN_DEPTH, c->stream, true);
                HIP_TRY(c, rtr::launch_project_bin_views(c->stream, cloud_of(c), proj, st, count, c->W, c->H, tab.host,
                                                         tab.dev, c->opt_lane_test ? 0 : 4, c->opt_phases, tm.a, tm.b));
            }
            HIP_TRY(c, hipEventRecord(tab.copied, c->stream));
            tab.pending = true;
        }
        if (int rc = launch_check(c, "views point kernel")) return rc;
    }
    for (int k = 0; k < count; ++k) {
        uint32_t *depth = v.depth + (size_t)k * npix;
        uint8_t *img = v.img + (size_t)k * npix * 3;
        if (binned) {
            const rtr::TilePyr pyr = tile_pyr(c, v, k, pyr_fused);
            v.fs[k].parity ^= 1;
            Timed t(c, RTR_K_TILE);
            rtr::launch_tile(c->stream, 0, c->W, c->H, v.fs[k].store, c->prm.depth_window, depth, v.acc, img,
                             lean_bits(c, v) | (v.fs[k].parity << 4), pyr_fused ? &pyr : nullptr);
        } else {
            const rtr::Proj pk = make_proj(P + 16 * k);
            { Timed t(c, RTR_K_CLEAR); rtr::launch_clear(c->stream, depth, v.acc, npix); }
            { Timed t(c, RTR_K_MIN_DEPTH); rtr::launch_min_depth(c->stream, cloud_of(c), pk, c->W, c->H, depth); }
            { Timed t(c, RTR_K_ACCUMULATE); rtr::launch_accumulate(c->stream, cloud_of(c), pk, c->W, c->H, depth, v.acc, c->prm.depth_window); }
            { Timed t(c, RTR_K_RESOLVE); rtr::launch_resolve(c->stream, v.acc, img, npix); }
        }
        if (with_filter) {
            Timed t(c, RTR_K_FILTER);
            rtr::launch_filter(c->stream, levels_of(c, v, k), depth, img, v.mask, v.tensor + (size_t)k * npix * 5, v.minmax + 2 * k,
                               v.part_min, v.part_max, c->W, c->H, c->prm.filter_strength, c->prm.gradient_threshold,
                               pyr_fused ? rtr::tile_count(c->W, c->H) : 0);
        }
        if (int rc = launch_check(c, "views frame")) return rc;
    }
    return RTR_OK;
}

int rtr_render_views(rtr_ctx *c, int count, const float *P, int with_filter) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, count >= 1 && count <= RTR_MAX_VIEWS, "count must be in 1..RTR_MAX_VIEWS");
    NEED(c, P != nullptr, "P is NULL");
    NEED(c, c->cap > 0, "no cloud has been uploaded");
    NEED(c, c->W > 0 && c->H > 0, "rtr_set_resolution has not been called");
    NEED(c, (c->n + 255) / 256 < (1ull << 24), "rtr_render_views: more than 2^32 - 256 points");
    DevGuard g(c->device);
    if (with_filter)  // (before anything changes)
        if (int rc = check_prefilter(c)) return rc;
    auto &rec = c->jr.views;
    rec.count = 0;
    if (int rc = views_enqueue(c, count, P, with_filter)) return rc;
    memcpy(rec.P, P, sizeof(float) * 16 * (size_t)count);
    rec.filter = with_filter;
    rec.count = count;
    rec.clip = c->clip;
    return RTR_OK;
}

// ---- buffers -----------------------------------------------------------------------

int rtr_device_buffer(rtr_ctx *c, int which, void **ptr, size_t *bytes) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, ptr != nullptr, "dev_ptr is NULL");
    if (which != RTR_BUF_MINMAX && which != RTR_BUF_VIEW_MINMAX && which != RTR_BUF_POINT_KEEP && which != RTR_BUF_SELECTION)
        if (int rc = check_frame(c)) return rc;
    size_t npix = (size_t)c->W * c->H, b = 0;
    void *p = nullptr;
    switch (which) {
        case RTR_BUF_DEPTH: p = c->frame.depth; b = npix * 4; break;
        case RTR_BUF_ACCUM: p = c->frame.acc; b = npix * 16; break;
        case RTR_BUF_IMAGE: p = c->frame.img; b = npix * 3; break;
        case RTR_BUF_TENSOR: p = c->frame.tensor; b = npix * 10; break;
        case RTR_BUF_MASK: p = c->frame.mask; b = npix; break;
        case RTR_BUF_MINMAX: p = c->frame.minmax; b = 8; break;
        case RTR_BUF_POINT_ID:
            NEED(c, c->pp_ids != nullptr, "RTR_BUF_POINT_ID: no rtr_point_pass with RTR_POINTS_IDS at this resolution yet");
            p = c->pp_ids; b = npix * 4; break;
        case RTR_BUF_VISIBLE:
            NEED(c, c->pp_vis != nullptr && c->pp_vis_current, "RTR_BUF_VISIBLE: no rtr_point_pass with RTR_POINTS_VISIBLE for the resident cloud yet");
            p = c->pp_vis; b = (size_t)((c->n + 31) / 32) * 4; break;
        case RTR_BUF_VIEW_DEPTH: case RTR_BUF_VIEW_IMAGE: case RTR_BUF_VIEW_TENSOR: case RTR_BUF_VIEW_MINMAX: {
            NEED(c, c->jr.views.count > 0, "RTR_BUF_VIEW_*: no rtr_render_views at this resolution for the resident cloud yet");
            const size_t k = (size_t)c->jr.views.count;
            if (which == RTR_BUF_VIEW_DEPTH) p = c->views.depth, b = k * npix * 4;
            else if (which == RTR_BUF_VIEW_IMAGE) p = c->views.img, b = k * npix * 3;
            else if (which == RTR_BUF_VIEW_TENSOR) p = c->views.tensor, b = k * npix * 10;
            else p = c->views.minmax, b = k * 8;
            break;
        }
        case RTR_BUF_POINT_KEEP:
            NEED(c, c->keep_up != nullptr, "RTR_BUF_POINT_KEEP: no keep mask is set (rtr_set_point_keep)");
            p = c->keep_up; b = (size_t)((c->n + 31) / 32) * 4; break;
        case RTR_BUF_SELECTION:
            NEED(c, c->sel != nullptr, "RTR_BUF_SELECTION: no selection (rtr_select_points)");
            p = c->sel; b = (size_t)((c->n + 31) / 32) * 4; break;
        default: return fail(c, RTR_ERR_INVALID, "unknown buffer id %d", which);
    }
    *ptr = p;
    if (bytes) *bytes = b;
    return RTR_OK;
}

int rtr_download_buffer(rtr_ctx *c, int which, void *host, size_t bytes) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, host != nullptr, "host is NULL");
    void *p = nullptr; size_t b = 0;
    int rc = rtr_device_buffer(c, which, &p, &b);
    if (rc) return rc;
    NEED(c, bytes == b, "size mismatch");
    DevGuard g(c->device);
    const Copy copy{host, p, b};
    if (which >= RTR_BUF_VIEW_DEPTH && which <= RTR_BUF_VIEW_MINMAX) {  // (a batch: checked -- and repaired -- before the copy)
        HIP_TRY(c, sync_streams(c));
        if ((rc = repair(c, c->views))) return rc;
        HIP_TRY(c, queue_copies(c, &copy, 1));
        HIP_TRY(c, sync_streams(c));
        return RTR_OK;
    }
    HIP_TRY(c, queue_copies(c, &copy, 1));
    HIP_TRY(c, sync_streams(c));
    // (after an overflow of the adaptive pool: the frame and a point pass behind it again, then the copy)
    rc = repair(c, c->frame, false, &copy, 1);
    if (!rc && (which == RTR_BUF_POINT_ID || which == RTR_BUF_VISIBLE) && c->jr.pass.invalid)
        rc = fail(c, RTR_ERR_INTERNAL, "the last rtr_point_pass read a frame the tile store reported incomplete (the adaptive "
                  "extent pool overflowed and a later frame was rendered before a synchronising call): render the frame and "
                  "run the point pass again");
    return rc;
}

// ---- measurement -------------------------------------------------------------------

#ifdef RTR_EXPERIMENT
extern "C" int rtr_debug_stamps(rtr_ctx *c, unsigned long long out[64]) {  // timing-experiment builds only
    if (!c || !out || !c->F().store.meta) return RTR_ERR_INVALID;
    DevGuard g(c->device);
    HIP_TRY(c, hipMemcpyAsync(out, rtr::ts_dbg(c->F().store), 64 * 8, hipMemcpyDeviceToHost, c->stream));
    rtr::read_filter_stamps(c->stream, out + 24);  // (words 24..39: two workgroups of k_filter4; the second tile workgroup's stamps give way)
    HIP_TRY(c, hipMemsetAsync(rtr::ts_dbg(c->F().store) + 40, 0, 8 * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(rtr::ts_dbg(c->F().store) + 56, 0, 8 * 8, c->stream));  // (the per-wave maxima / sums of T1)
    HIP_TRY(c, sync_streams(c));
    return RTR_OK;
}
#endif

int rtr_frame_stats(rtr_ctx *c, uint32_t out[8]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, out != nullptr, "out is NULL");
    NEED(c, c->F().store.meta != nullptr, "no binned frame yet");
    DevGuard g(c->device);
    if (c->last_lean) rtr::launch_lean_fold(c->stream, c->W, c->H, c->F().store, c->F().parity);  // (lean frames fold lazily)
    HIP_TRY(c, hipMemcpyAsync(out, rtr::ts_hdr(c->F().store), 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_streams(c));
    return RTR_OK;
}

int rtr_timing_enable(rtr_ctx *c, int on) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    DevGuard g(c->device);
    (void)collect_timing(c);
    c->timing = on < 0 ? 0 : (on > 4 ? 1 : on);
    c->timing_tick = 0;
    return RTR_OK;
}

int rtr_timing_reset(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    DevGuard g(c->device);
    (void)collect_timing(c);
    for (int k = 0; k < RTR_K_COUNT; ++k) { c->total_ms[k] = 0; c->launches[k] = 0; }
    return RTR_OK;
}

int rtr_timing_get(rtr_ctx *c, int k, double *total_ms, uint64_t *launches) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, k >= 0 && k < RTR_K_COUNT, "bad kernel id");
    DevGuard g(c->device);
    if (int rc = collect_timing(c)) return rc;
    if (total_ms) *total_ms = c->total_ms[k];
    if (launches) *launches = c->launches[k];
    return RTR_OK;
}

}  // extern "C"
