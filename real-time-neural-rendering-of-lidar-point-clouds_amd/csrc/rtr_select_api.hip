// rtr_select_api.hip -- the selection and analysis calls of include/rtr.h (sections 6f - 6m), include/rtr_statistics.h
// (section 6n), include/rtr_normals.h (section 6o), include/rtr_register.h (section 6p) and include/rtr_segments.h (section 6q)
// on top of the kernels of
// rtr_cloud_kernels.hip, rtr_voxel.hip, rtr_neighbours.hip, rtr_clusters.hip, rtr_segments.hip, rtr_near.hip, rtr_nearest.hip, rtr_nearest_k.hip,
// rtr_statistical.hip, rtr_normals.hip, rtr_register.hip and rtr_planes.hip.  The rules the calls share are stated once each, in the helpers below; DESIGN.md ("The selection
// calls in their own file") has the order of events every call follows and why an error leaves the selection as it was.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/rtr_normals.h"
#include "../../include/rtr_register.h"
#include "../../include/rtr_segments.h"
#include "../../include/rtr_statistics.h"
#include "rtr_host.h"
#include "rtr_plane_fit.h"
#include "rtr_register_fit.h"
#include "rtr_register_kernels.h"
#include "rtr_segment_kernels.h"

int check_indexable(rtr_ctx *c) {
    if (c->n < (1ull << 32)) return RTR_OK;
    return fail(c, RTR_ERR_UNSUPPORTED, "point indices are 32-bit: the cloud has %llu points", (unsigned long long)c->n);
}

bool statistics_option(const rtr_ctx *c, const char *key, int *value) {
    const struct { const char *name; int value; } keys[] = {
        {"statistical_us0", c->statistical_us[0]}, {"statistical_us1", c->statistical_us[1]}, {"statistical_us2", c->statistical_us[2]},
        {"statistical_pair_tests_k", c->statistical_tests_k}, {"statistical_row_updates_k", c->statistical_updates_k}};
    for (const auto &k : keys) {
        if (strcmp(key, k.name) != 0) continue;
        *value = k.value;
        return true;
    }
    return false;
}

bool normals_option(const rtr_ctx *c, const char *key, int *value) {
    const struct { const char *name; int value; } keys[] = {
        {"normals_us0", c->normals_us[0]}, {"normals_us1", c->normals_us[1]}, {"normals_us2", c->normals_us[2]},
        {"normals_pair_tests_k", c->normals_tests_k}, {"normals_row_updates_k", c->normals_updates_k}};
    for (const auto &k : keys) {
        if (strcmp(key, k.name) != 0) continue;
        *value = k.value;
        return true;
    }
    return false;
}

namespace {
// One bit per point in whole 256-point chunks (launch_select_count, the select kernels' whole-chunk stores): 8 words per
// chunk, at least 8 -- the selection over the cloud, the near words over the given points
uint64_t sel_words(uint64_t n) { return std::max<uint64_t>((n + 255) / 256, 1) * 8; }

struct SelectOp { int base; bool outside; };  // an `op` argument taken apart: RTR_SELECT_REPLACE .. TOGGLE, RTR_SELECT_OUTSIDE
int check_select_op(rtr_ctx *c, const char *who, int op, SelectOp *o) {
    o->base = op & ~RTR_SELECT_OUTSIDE, o->outside = (op & RTR_SELECT_OUTSIDE) != 0;
    if (op >= 0 && (o->base <= RTR_SELECT_INTERSECT || o->base == RTR_SELECT_TOGGLE)) return RTR_OK;
    return fail(c, RTR_ERR_INVALID, "%s: unknown op", who);
}
// `count` finite `noun` ("points", "given points") have no cell of the neighbour grid
int fail_span(rtr_ctx *c, const char *who, const char *noun, uint64_t count) {
    return fail(c, RTR_ERR_UNSUPPORTED, "%s: %llu finite %s lie beyond the span of the internal grid (about 2^20 radius from the "
                "world origin on an axis)", who, (unsigned long long)count, noun);
}
int saturate_int(uint64_t x) { return (int)std::min<uint64_t>(x, 0x7FFFFFFF); }  // (the options are ints)
int saturate_k(uint64_t x) { return saturate_int(x / 1000); }                     // ... in thousands

// A selection that does not exist yet is empty.  reserve: its words and statistics, among the call's other allocations
// (nothing when it exists); create: once nothing but a launch can fail any more, the words zeroed on s and both arrays
// handed to the context (nothing when reserve took nothing)
struct NewSelection {
    uint32_t *w = nullptr;
    uint64_t *st = nullptr;
    int reserve(rtr_ctx *c, DevBufs &buf) {
        if (c->sel) return RTR_OK;
        HIP_TRY(c, buf.get(&w, sel_words(c->n) * 4));
        HIP_TRY(c, buf.get(&st, 4 * sizeof(uint64_t)));
        return RTR_OK;
    }
    int create(rtr_ctx *c, DevBufs &buf, hipStream_t s) {
        if (!w) return RTR_OK;
        HIP_TRY(c, hipMemsetAsync(w, 0, sel_words(c->n) * 4, s));
        buf.swap_in(c->sel, w); buf.swap_in(c->sel_stats, st);
        return RTR_OK;
    }
};

// The (key, value) pairs of `count` points on both sides of rtr_voxel.hip's sort (sorted: k1 / v1), its temporary, and --
// with_records -- a 16-byte record per point in upload-order slots (rec0) and gathered into sorted order (rec1).
// rtr_select_clusters takes the buffers that are dead by then, rec0 and k0, for its own arrays
struct KeyedScratch {
    uint64_t *k0, *k1;
    uint32_t *v0, *v1;
    float4 *rec0 = nullptr, *rec1 = nullptr;
    void *tmp;
    size_t tmp_bytes = 0;
    int alloc(rtr_ctx *c, DevBufs &buf, uint64_t count, bool with_records) {
        HIP_TRY(c, (hipError_t)rtr::voxel_sort_temp_bytes(std::max<uint64_t>(count, 1), &tmp_bytes));
        HIP_TRY(c, buf.get(&k0, count * 8));
        HIP_TRY(c, buf.get(&k1, count * 8));
        HIP_TRY(c, buf.get(&v0, count * 4));
        HIP_TRY(c, buf.get(&v1, count * 4));
        if (with_records) HIP_TRY(c, buf.get(&rec0, count * 16));
        if (with_records) HIP_TRY(c, buf.get(&rec1, count * 16));
        HIP_TRY(c, buf.get(&tmp, tmp_bytes));
        return RTR_OK;
    }
    hipError_t sort(hipStream_t s, uint64_t count) const {  // (nothing is queued for no pairs)
        return count ? (hipError_t)rtr::voxel_sort(s, tmp, tmp_bytes, k0, k1, v0, v1, count) : hipSuccess;
    }
};

struct EventSet {  // the stage boundaries of one call
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~EventSet() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    int create(rtr_ctx *c, int count) {
        for (int k = 0; k < count; ++k) HIP_TRY(c, hipEventCreate(&e[k]));
        return RTR_OK;
    }
    int record(rtr_ctx *c, int k, hipStream_t s) { HIP_TRY(c, hipEventRecord(e[k], s)); return RTR_OK; }
    // out[k] = the microseconds between events first + k and first + k + 1, rounded; behind the wait for the last of them
    int stage_us(rtr_ctx *c, int first, int count, int *out) {
        for (int k = 0; k < count; ++k) {
            float ms = 0.f;
            HIP_TRY(c, hipEventElapsedTime(&ms, e[first + k], e[first + k + 1]));
            out[k] = (int)(ms * 1000.f + 0.5f);
        }
        return RTR_OK;
    }
};

// The GIVEN points of rtr_select_near, rtr_nearest_points and rtr_nearest_k_points (rtr.h sections 6k - 6m): section 6h's
// key, sort and gather over a plain strided array in host or device memory.  alloc: the scratch, among the call's other allocations; run:
// everything up to the sorted records ks.k1 / ks.rec1 of the m points with a cell and their box, with ONE wait on the
// way, for the counters and the box: a finite point beyond the span fails the call there, before anything has changed.
// cn (device, 12 words): [0] non-finite given points, [1] those beyond the span, [2] the caller's, [4 .. 7] the sweep's,
// [8 .. 10] the box
struct GivenPoints {
    KeyedScratch ks;
    uint64_t *cn = nullptr;
    uint8_t *stage = nullptr;
    size_t gbytes = 0;
    uint64_t nonfinite = 0, m = 0;
    double glo[3] = {0, 0, 0}, ghi[3] = {0, 0, 0};
    int alloc(rtr_ctx *c, DevBufs &buf, const float *xyz, size_t xs, uint64_t count) {
        gbytes = count ? (size_t)(count - 1) * xs + 12 : 0;
        if (int rc = ks.alloc(c, buf, count, true)) return rc;
        HIP_TRY(c, buf.get(&cn, 12 * sizeof(uint64_t)));
        if (count && !on_device(xyz)) HIP_TRY(c, buf.get(&stage, gbytes));
        return RTR_OK;
    }
    int run(rtr_ctx *c, const char *who, hipStream_t s, const float *xyz, size_t xs, uint64_t count, float radius) {
        HIP_TRY(c, hipMemsetAsync(cn, 0, 12 * sizeof(uint64_t), s));
        HIP_TRY(c, hipMemsetAsync(cn + 8, 0xFF, 3 * sizeof(uint32_t), s));  // (box: the minima start at 2^32 - 1, the maxima at 0)
        const uint8_t *gxyz = (const uint8_t *)xyz;
        if (stage) {  // (the given points are read before the call returns: one copy at the caller's stride)
            HIP_TRY(c, hipMemcpyAsync(stage, xyz, gbytes, hipMemcpyHostToDevice, s));
            gxyz = stage;
        }
        rtr::launch_near_keys(s, gxyz, xs, count, radius, ks.k0, ks.v0, ks.rec0, cn, reinterpret_cast<uint32_t *>(cn + 8));
        if (int rc = launch_check(c, "given keys")) return rc;
        uint64_t host[12] = {};
        HIP_TRY(c, hipMemcpyAsync(host, cn, sizeof host, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (host[1]) return fail_span(c, who, "given points", host[1]);
        nonfinite = host[0], m = count - nonfinite;  // (the pairs with a cell sort to the front)
        HIP_TRY(c, ks.sort(s, count));
        rtr::launch_neighbour_gather(s, ks.v1, ks.rec0, m, ks.rec1);
        if (int rc = launch_check(c, "given gather")) return rc;
        if (m) {
            uint32_t box[6];
            memcpy(box, host + 8, sizeof box);
            rtr::near_box_from_keys(box, glo, ghi);
        }
        return RTR_OK;
    }
};

// selection := op(selection, hits), then its count into sel_stats[0]; `what` labels the combine launch
int selection_finish(rtr_ctx *c, hipStream_t s, const uint32_t *hit, uint64_t n, const SelectOp &op, const char *what) {
    rtr::launch_voxel_combine(s, hit, n, op.base, op.outside, c->sel);
    if (int rc = launch_check(c, what)) return rc;
    rtr::launch_select_count(s, c->sel, n, c->sel_stats);
    return launch_check(c, "select count");
}
}  // namespace

extern "C" {

// ---- selection (rtr.h, section 6f) ----------------------------------------------------
// One sweep over the resident coordinates on the context's stream (rtr::launch_select), nothing else read or written:
// the cloud's own planes and mask, the frames, their journal and the point pass's buffers stay as they are.
int rtr_select_points(rtr_ctx *c, int plane_count, const float *planes, const float *P, const int rect[4], int op,
                      uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_select_points: no cloud");
    NEED(c, plane_count >= 0 && plane_count <= RTR_MAX_CLIP_PLANES, "rtr_select_points: plane_count outside 0..RTR_MAX_CLIP_PLANES");
    NEED(c, plane_count == 0 || planes != nullptr, "rtr_select_points: planes is NULL");
    rtr::Clip clip{};
    for (int j = 0; j < plane_count; ++j) {
        for (int k = 0; k < 4; ++k) {
            NEED(c, std::isfinite(planes[4 * j + k]), "rtr_select_points: a coefficient is not finite");
            clip.p[j][k] = planes[4 * j + k];
        }
        NEED(c, clip.p[j][0] != 0.f || clip.p[j][1] != 0.f || clip.p[j][2] != 0.f, "rtr_select_points: a = b = c = 0");
    }
    clip.count = plane_count;
    if (P) {
        NEED(c, c->W > 0 && c->H > 0, "rtr_select_points: a rectangle needs a resolution (rtr_set_resolution)");
        NEED(c, rect != nullptr, "rtr_select_points: rect is NULL");
        NEED(c, 0 <= rect[0] && rect[0] < rect[2] && rect[2] <= c->W && 0 <= rect[1] && rect[1] < rect[3] && rect[3] <= c->H,
             "rtr_select_points: the rectangle must satisfy 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H");
    }
    SelectOp sop;
    if (int rc = check_select_op(c, "rtr_select_points", op, &sop)) return rc;
    if (int rc = check_indexable(c)) return rc;
    if (int rc = need_upload_order(c, "formed")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    DevBufs buf;
    NewSelection fresh;
    if (int rc = fresh.reserve(c, buf)) return rc;
    if (int rc = fresh.create(c, buf, s)) return rc;
    const uint32_t *perm = c->reordered ? c->perm : nullptr;
    if (perm && sop.base == RTR_SELECT_REPLACE) HIP_TRY(c, hipMemsetAsync(c->sel, 0, sel_words(c->n) * 4, s));
    if (stats) HIP_TRY(c, hipMemsetAsync(c->sel_stats, 0, 4 * sizeof(uint64_t), s));
    rtr::Proj proj{};
    if (P) proj = make_proj(P);
    rtr::launch_select(s, cloud_of(c), c->bounds, clip, P ? &proj : nullptr, c->W, c->H, rect, sop.base, sop.outside, c->sel, perm,
                       stats ? c->sel_stats : nullptr);
    if (int rc = launch_check(c, "select")) return rc;
    if (!stats) return RTR_OK;
    rtr::launch_select_count(s, c->sel, c->n, c->sel_stats);
    if (int rc = launch_check(c, "select count")) return rc;
    uint64_t out[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(out, c->sel_stats, sizeof out, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    memcpy(stats, out, sizeof out);
    return RTR_OK;
}

// ---- selection by a voxel grid (rtr.h, section 6g) ------------------------------------
// Keys in upload-order slots (rtr::launch_voxel_keys), rocPRIM's stable sort by key, the head of every run of equal keys
// into zeroed hit words, then selection := op(selection, hits).  The call waits for its work before the scratch goes.
// What rtr_select_points leaves alone stays as it is here too.
int rtr_select_voxel_grid(rtr_ctx *c, const float origin[3], const float cell[3], uint32_t min_count, int op, uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_select_voxel_grid: no cloud");
    NEED(c, origin != nullptr, "rtr_select_voxel_grid: origin is NULL");
    NEED(c, cell != nullptr, "rtr_select_voxel_grid: cell is NULL");
    rtr::VoxelGrid grid{};
    for (int k = 0; k < 3; ++k) {
        NEED(c, std::isfinite(origin[k]), "rtr_select_voxel_grid: origin is not finite");
        NEED(c, std::isfinite(cell[k]) && cell[k] > 0.f, "rtr_select_voxel_grid: cell must be finite and > 0");
        const float inv = 1.0f / cell[k];  // (one IEEE fp32 division: the build has no fast-math)
        NEED(c, std::isfinite(inv) && inv > 0.f, "rtr_select_voxel_grid: the reciprocal of cell is not finite and > 0 in fp32");
        grid.origin[k] = origin[k];
        grid.inv[k] = inv;
    }
    NEED(c, min_count >= 1u, "rtr_select_voxel_grid: min_count must be >= 1");
    SelectOp sop;
    if (int rc = check_select_op(c, "rtr_select_voxel_grid", op, &sop)) return rc;
    if (int rc = check_indexable(c)) return rc;
    if (int rc = need_upload_order(c, "formed")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const uint64_t n = c->n, nw = (n + 31) / 32;
    DevBufs buf;
    KeyedScratch ks;
    NewSelection fresh;
    EventSet ev;
    uint32_t *hit;
    if (int rc = ks.alloc(c, buf, n, false)) return rc;
    HIP_TRY(c, buf.get(&hit, nw * 4));
    if (int rc = fresh.reserve(c, buf)) return rc;
    if (int rc = ev.create(c, 4)) return rc;
    if (int rc = fresh.create(c, buf, s)) return rc;
    HIP_TRY(c, hipMemsetAsync(hit, 0, nw * 4, s));
    HIP_TRY(c, hipMemsetAsync(c->sel_stats, 0, 4 * sizeof(uint64_t), s));
    if (int rc = ev.record(c, 0, s)) return rc;
    rtr::launch_voxel_keys(s, cloud_of(c), c->reordered ? c->perm : nullptr, grid, ks.k0, ks.v0);
    if (int rc = launch_check(c, "voxel keys")) return rc;
    if (int rc = ev.record(c, 1, s)) return rc;
    HIP_TRY(c, ks.sort(s, n));
    if (int rc = ev.record(c, 2, s)) return rc;
    rtr::launch_voxel_heads(s, ks.k1, ks.v1, n, min_count, hit, c->sel_stats);
    if (int rc = launch_check(c, "voxel heads")) return rc;
    if (int rc = ev.record(c, 3, s)) return rc;
    if (int rc = selection_finish(c, s, hit, n, sop, "voxel combine")) return rc;
    uint64_t out[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(out, c->sel_stats, sizeof out, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // (always: the scratch goes with this call)
    if (int rc = ev.stage_us(c, 0, 3, c->voxel_us)) return rc;
    if (stats) memcpy(stats, out, sizeof out);
    return RTR_OK;
}

// ---- selection by neighbour count and by cluster (rtr.h, sections 6h and 6i) ----------
// rtr_select_voxel_grid's pattern with a neighbour search between the sort and the combine (rtr_neighbours.hip,
// rtr_clusters.hip).  Both calls share everything up to the work list (neighbour_search): it waits twice on the way --
// for the key sweep's two counters (a point beyond the span fails the call; the points with a cell are the first
// n - nonfinite sorted pairs) and for the number of occupied cells, which sizes the work list -- and both lie before the
// selection comes into existence or a word of it changes.
namespace {
struct NeighbourSearch {  // the scratch of one call and what the search found
    DevBufs buf;
    EventSet ev;
    KeyedScratch ks;
    uint64_t *cn;  // [0] non-finite points, [1] finite points beyond the span, [2] pair tests, [3] cells, [4] the list's cursor
    uint32_t *hit, *items;
    uint64_t n, m, cap;  // points, those of them with a cell (the first m sorted pairs), the work list's slots
};

// Allocates, sweeps, sorts, gathers and lists; leaves hit and sel_stats zeroed, the selection in existence and
// ev.e[0 .. 2] recorded (before the keys, behind them, behind the sort).  selects = false (rtr_estimate_normals, a pure
// analysis call): the selection and its statistics are neither created nor touched.
int neighbour_search(rtr_ctx *c, const char *who, float radius, NeighbourSearch &q, bool selects = true) {
    hipStream_t s = c->stream;
    const uint64_t n = c->n, nw = (n + 31) / 32;
    DevBufs &buf = q.buf;
    KeyedScratch &ks = q.ks;
    NewSelection fresh;
    if (int rc = ks.alloc(c, buf, n, true)) return rc;
    HIP_TRY(c, buf.get(&q.hit, nw * 4));
    HIP_TRY(c, buf.get(&q.cn, 5 * sizeof(uint64_t)));
    if (selects)
        if (int rc = fresh.reserve(c, buf)) return rc;
    if (int rc = q.ev.create(c, 4)) return rc;
    HIP_TRY(c, hipMemsetAsync(q.hit, 0, nw * 4, s));
    HIP_TRY(c, hipMemsetAsync(q.cn, 0, 5 * sizeof(uint64_t), s));
    if (int rc = q.ev.record(c, 0, s)) return rc;
    rtr::launch_neighbour_keys(s, cloud_of(c), c->reordered ? c->perm : nullptr, radius, ks.k0, ks.v0, ks.rec0, q.cn);
    if (int rc = launch_check(c, "neighbour keys")) return rc;
    if (int rc = q.ev.record(c, 1, s)) return rc;
    uint64_t host[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(host, q.cn, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (host[1]) return fail_span(c, who, "points", host[1]);
    const uint64_t nonfinite = host[0], m = n - nonfinite;  // (the pairs with a cell sort to the front)
    HIP_TRY(c, ks.sort(s, n));
    if (int rc = q.ev.record(c, 2, s)) return rc;
    rtr::launch_neighbour_gather(s, ks.v1, ks.rec0, m, ks.rec1);
    if (int rc = launch_check(c, "neighbour gather")) return rc;
    rtr::launch_neighbour_cells(s, ks.k1, m, q.cn + 3);
    if (int rc = launch_check(c, "neighbour cells")) return rc;
    HIP_TRY(c, hipMemcpyAsync(host + 3, q.cn + 3, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint64_t cap = std::min<uint64_t>(host[3] + m / 64, m);  // (a cell of len points: ceil(len / 64) <= 1 + len / 64 items, each of >= 1 point)
    HIP_TRY(c, buf.get(&q.items, cap * 80));
    if (selects) {
        if (int rc = fresh.create(c, buf, s)) return rc;
        HIP_TRY(c, hipMemsetAsync(c->sel_stats, 0, 4 * sizeof(uint64_t), s));
    }
    rtr::launch_neighbour_items(s, ks.k1, m, q.items, (uint32_t *)(q.cn + 4), cap);
    if (int rc = launch_check(c, "neighbour items")) return rc;
    q.n = n, q.m = m, q.cap = cap;
    return RTR_OK;
}

// selection := op(selection, hits), the count, the wait; out: the four statistics, *tests_k: the pair tests; us[0 .. 2]:
// the stage times between the search's events and ev.e[3], which the caller has recorded
int neighbour_finish(rtr_ctx *c, const char *what, NeighbourSearch &q, const SelectOp &op, uint64_t out[4], int us[3], int *tests_k) {
    hipStream_t s = c->stream;
    if (int rc = selection_finish(c, s, q.hit, q.n, op, what)) return rc;
    uint64_t tests = 0;
    HIP_TRY(c, hipMemcpyAsync(out, c->sel_stats, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&tests, q.cn + 2, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // (always: the scratch goes with this call)
    if (int rc = q.ev.stage_us(c, 0, 3, us)) return rc;
    *tests_k = saturate_k(tests);
    return RTR_OK;
}
}  // namespace

int rtr_select_neighbours(rtr_ctx *c, float radius, uint32_t min_neighbours, int op, uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_select_neighbours: no cloud");
    NEED(c, std::isfinite(radius) && radius > 0.f, "rtr_select_neighbours: radius must be finite and > 0");
    const float r2 = radius * radius;  // (one fp32 product: the build has no contraction and no fast-math)
    NEED(c, std::isnormal(r2), "rtr_select_neighbours: the square of radius is not a finite normal fp32 number");
    NEED(c, min_neighbours >= 1u, "rtr_select_neighbours: min_neighbours must be >= 1");
    SelectOp sop;
    if (int rc = check_select_op(c, "rtr_select_neighbours", op, &sop)) return rc;
    if (int rc = check_indexable(c)) return rc;
    if (int rc = need_upload_order(c, "formed")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    NeighbourSearch q;
    if (int rc = neighbour_search(c, "rtr_select_neighbours", radius, q)) return rc;
    rtr::launch_neighbour_count(s, q.ks.rec1, q.items, (const uint32_t *)(q.cn + 4), q.cap, r2, min_neighbours, q.hit, c->sel_stats, q.cn + 2);
    if (int rc = launch_check(c, "neighbour count")) return rc;
    if (int rc = q.ev.record(c, 3, s)) return rc;
    HIP_TRY(c, d2d(s, c->sel_stats + 3, q.cn, sizeof(uint64_t)));
    uint64_t out[4] = {0, 0, 0, 0};
    if (int rc = neighbour_finish(c, "neighbour combine", q, sop, out, c->neighbours_us, &c->neighbours_tests_k)) return rc;
    if (stats) memcpy(stats, out, sizeof out);
    return RTR_OK;
}

// ---- selection by connected cluster (rtr.h, section 6i) -------------------------------
// The union-find's four arrays (parent, size, smallest upload index, seed flag: n words each) live in the unsorted
// records' buffer, which is dead once the gather has run; the labels are written into the unsorted keys' buffer, dead
// since the sort, and copied to the caller's array -- host or device memory, told apart as rtr_extract_points does --
// once everything else has succeeded.
int rtr_select_clusters(rtr_ctx *c, float radius, uint32_t min_points, uint32_t max_points, int flags, int op, uint32_t *labels,
                        uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_select_clusters: no cloud");
    NEED(c, std::isfinite(radius) && radius > 0.f, "rtr_select_clusters: radius must be finite and > 0");
    const float r2 = radius * radius;  // (one fp32 product: the build has no contraction and no fast-math)
    NEED(c, std::isnormal(r2), "rtr_select_clusters: the square of radius is not a finite normal fp32 number");
    NEED(c, min_points >= 1u, "rtr_select_clusters: min_points must be >= 1");
    NEED(c, max_points == 0u || max_points >= min_points, "rtr_select_clusters: max_points must be 0 (unbounded) or >= min_points");
    NEED(c, (flags & ~RTR_CLUSTER_SEEDED) == 0, "rtr_select_clusters: unknown bits in flags");
    SelectOp sop;
    if (int rc = check_select_op(c, "rtr_select_clusters", op, &sop)) return rc;
    if (int rc = check_indexable(c)) return rc;
    if (int rc = need_upload_order(c, "formed")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const bool seeded = (flags & RTR_CLUSTER_SEEDED) != 0, labels_dev = labels && on_device(labels);
    NeighbourSearch q;
    if (int rc = neighbour_search(c, "rtr_select_clusters", radius, q)) return rc;
    const uint64_t n = q.n;
    uint32_t *parent = reinterpret_cast<uint32_t *>(q.ks.rec0), *size = parent + n, *minu = size + n, *seed = minu + n;
    uint32_t *lab = labels ? reinterpret_cast<uint32_t *>(q.ks.k0) : nullptr;
    rtr::launch_cluster_init(s, n, parent, size, minu, seed);
    if (int rc = launch_check(c, "cluster init")) return rc;
    rtr::launch_cluster_link(s, q.ks.rec1, q.items, (const uint32_t *)(q.cn + 4), q.cap, r2, parent, q.cn + 2);
    if (int rc = launch_check(c, "cluster link")) return rc;
    rtr::launch_cluster_flatten(s, q.ks.v1, n, seeded ? c->sel : nullptr, parent, size, minu, seed);
    if (int rc = launch_check(c, "cluster flatten")) return rc;
    rtr::launch_cluster_hits(s, q.ks.v1, n, parent, size, minu, seed, min_points, max_points, seeded, q.hit, lab, c->sel_stats);
    if (int rc = launch_check(c, "cluster hits")) return rc;
    if (int rc = q.ev.record(c, 3, s)) return rc;
    uint64_t out[4] = {0, 0, 0, 0};
    if (int rc = neighbour_finish(c, "cluster combine", q, sop, out, c->clusters_us, &c->clusters_tests_k)) return rc;
    if (lab) {  // (behind everything that can fail: the caller's array changes only when the call succeeds)
        HIP_TRY(c, hipMemcpyAsync(labels, lab, n * 4, labels_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    if (stats) memcpy(stats, out, sizeof out);
    return RTR_OK;
}

// ---- selection by smooth segment (rtr_segments.h, section 6q) -------------------------
// rtr_select_clusters' order of events with the normal test in the link (rtr_segments.hip).  The union-find's arrays and
// the labels live where section 6i keeps them; the normal records and the staging copies of inputs that lie in host
// memory are the only new scratch and are allocated BEFORE the search, so that the selection comes into existence
// behind the call's last allocation.  The stage times and the pair tests go to locals: the call has no option key.
int rtr_select_segments(rtr_ctx *c, float radius, float cos_angle, const float *normals, const float *curvature, float max_curvature,
                        uint32_t min_points, uint32_t max_points, int flags, int op, uint32_t *labels, uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_select_segments: no cloud");
    NEED(c, std::isfinite(radius) && radius > 0.f, "rtr_select_segments: radius must be finite and > 0");
    const float r2 = radius * radius;  // (one fp32 product: the build has no contraction and no fast-math)
    NEED(c, std::isnormal(r2), "rtr_select_segments: the square of radius is not a finite normal fp32 number");
    NEED(c, std::isfinite(cos_angle) && cos_angle > 0.f && cos_angle <= 1.f, "rtr_select_segments: cos_angle must be finite, > 0 and <= 1");
    NEED(c, normals != nullptr, "rtr_select_segments: normals is NULL");
    NEED(c, curvature == nullptr || !std::isnan(max_curvature), "rtr_select_segments: max_curvature is NaN with a curvature array");
    NEED(c, min_points >= 1u, "rtr_select_segments: min_points must be >= 1");
    NEED(c, max_points == 0u || max_points >= min_points, "rtr_select_segments: max_points must be 0 (unbounded) or >= min_points");
    NEED(c, (flags & ~(RTR_SEGMENT_SEEDED | RTR_SEGMENT_ORIENTED)) == 0, "rtr_select_segments: unknown bits in flags");
    SelectOp sop;
    if (int rc = check_select_op(c, "rtr_select_segments", op, &sop)) return rc;
    if (int rc = check_indexable(c)) return rc;
    if (int rc = need_upload_order(c, "formed")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const bool seeded = (flags & RTR_SEGMENT_SEEDED) != 0, oriented = (flags & RTR_SEGMENT_ORIENTED) != 0;
    const bool labels_dev = labels && on_device(labels);
    NeighbourSearch q;
    float4 *nrec;
    float *nstage = nullptr, *cstage = nullptr;
    HIP_TRY(c, q.buf.get(&nrec, c->n * 16));
    if (!on_device(normals)) HIP_TRY(c, q.buf.get(&nstage, c->n * 12));
    if (curvature && !on_device(curvature)) HIP_TRY(c, q.buf.get(&cstage, c->n * 4));
    if (int rc = neighbour_search(c, "rtr_select_segments", radius, q)) return rc;
    const uint64_t n = q.n;
    // (the inputs are read before the call returns: one copy each of those that lie in host memory)
    if (nstage) HIP_TRY(c, hipMemcpyAsync(nstage, normals, n * 12, hipMemcpyHostToDevice, s));
    if (cstage) HIP_TRY(c, hipMemcpyAsync(cstage, curvature, n * 4, hipMemcpyHostToDevice, s));
    uint32_t *parent = reinterpret_cast<uint32_t *>(q.ks.rec0), *size = parent + n, *minu = size + n, *seed = minu + n;
    uint32_t *lab = labels ? reinterpret_cast<uint32_t *>(q.ks.k0) : nullptr;
    rtr::launch_segment_gather(s, q.ks.v1, q.m, nstage ? nstage : normals, cstage ? cstage : curvature, max_curvature, nrec);
    if (int rc = launch_check(c, "segment gather")) return rc;
    rtr::launch_cluster_init(s, n, parent, size, minu, seed);
    if (int rc = launch_check(c, "segment init")) return rc;
    rtr::launch_segment_link(s, q.ks.rec1, nrec, q.items, (const uint32_t *)(q.cn + 4), q.cap, r2, cos_angle, oriented, parent, q.cn + 2);
    if (int rc = launch_check(c, "segment link")) return rc;
    rtr::launch_cluster_flatten(s, q.ks.v1, n, seeded ? c->sel : nullptr, parent, size, minu, seed);
    if (int rc = launch_check(c, "segment flatten")) return rc;
    rtr::launch_cluster_hits(s, q.ks.v1, n, parent, size, minu, seed, min_points, max_points, seeded, q.hit, lab, c->sel_stats);
    if (int rc = launch_check(c, "segment hits")) return rc;
    if (int rc = q.ev.record(c, 3, s)) return rc;
    uint64_t out[4] = {0, 0, 0, 0};
    int us[3] = {0, 0, 0}, tests_k = 0;  // (no option key reports them)
    if (int rc = neighbour_finish(c, "segment combine", q, sop, out, us, &tests_k)) return rc;
    if (lab) {  // (behind everything that can fail: the caller's array changes only when the call succeeds)
        HIP_TRY(c, hipMemcpyAsync(labels, lab, n * 4, labels_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    if (stats) memcpy(stats, out, sizeof out);
    return RTR_OK;
}

// ---- selection by mean neighbour distance (rtr_statistics.h, section 6n) --------------
// rtr_select_neighbours' order of events with rows in place of counts (rtr_statistical.hip): the means and the rows'
// lengths go to two scratch arrays in upload order, allocated with the sums' scratch BEFORE the search, so that the
// selection comes into existence behind the call's last allocation.  The two sums are waited for one after the other --
// the second needs mu --, the threshold is formed on the host, and the hits are combined as everywhere.  An output in
// host memory is staged in host memory, queued ahead of the combine, and handed over with moments and stats behind the
// last thing that can fail.
int rtr_select_statistical(rtr_ctx *c, uint32_t k, float radius, double std_mul, int flags, int op, float *mean_dist, uint32_t *found,
                           double moments[3], uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_select_statistical: no cloud");
    NEED(c, k >= 1u && k <= RTR_STAT_MAX_K, "rtr_select_statistical: k outside 1..RTR_STAT_MAX_K");
    NEED(c, std::isfinite(radius) && radius > 0.f, "rtr_select_statistical: radius must be finite and > 0");
    const float r2 = radius * radius;  // (one fp32 product: the build has no contraction and no fast-math)
    NEED(c, std::isnormal(r2), "rtr_select_statistical: the square of radius is not a finite normal fp32 number");
    NEED(c, (flags & ~RTR_STAT_THRESHOLD_GIVEN) == 0, "rtr_select_statistical: unknown bits in flags");
    const bool given = (flags & RTR_STAT_THRESHOLD_GIVEN) != 0;
    NEED(c, given || std::isfinite(std_mul), "rtr_select_statistical: std_mul must be finite");
    NEED(c, !given || moments != nullptr, "rtr_select_statistical: moments is NULL with RTR_STAT_THRESHOLD_GIVEN");
    NEED(c, !given || !std::isnan(moments[2]), "rtr_select_statistical: moments[2] (the threshold) is NaN with RTR_STAT_THRESHOLD_GIVEN");
    SelectOp sop;
    if (int rc = check_select_op(c, "rtr_select_statistical", op, &sop)) return rc;
    if (int rc = check_indexable(c)) return rc;
    if (int rc = need_upload_order(c, "formed")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const uint64_t n = c->n;
    const bool mean_dev = mean_dist && on_device(mean_dist), found_dev = found && on_device(found);
    std::vector<float> mean_host;
    std::vector<uint32_t> found_host;
    try {
        if (mean_dist && !mean_dev) mean_host.resize(n);
        if (found && !found_dev) found_host.resize(n);
    } catch (const std::bad_alloc &) {
        return fail(c, RTR_ERR_HIP, "rtr_select_statistical: no host memory for the staging copy of an output");
    }
    NeighbourSearch q;
    float *means;
    uint32_t *fnd;
    double *partial;
    uint64_t *red;  // [0] a sum (fp64 bits), [1] the points with a row, [2] the values written into rows
    HIP_TRY(c, q.buf.get(&means, n * 4));
    HIP_TRY(c, q.buf.get(&fnd, n * 4));
    HIP_TRY(c, q.buf.get(&partial, rtr::stat_partials(n) * sizeof(double)));
    HIP_TRY(c, q.buf.get(&red, 4 * sizeof(uint64_t)));
    if (int rc = neighbour_search(c, "rtr_select_statistical", radius, q)) return rc;
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)means, 0x7F800000, n, s));  // (the points no item holds: no row)
    HIP_TRY(c, hipMemsetAsync(fnd, 0, n * 4, s));
    HIP_TRY(c, hipMemsetAsync(red, 0, 4 * sizeof(uint64_t), s));
    rtr::launch_stat_rows(s, q.ks.rec1, q.items, (const uint32_t *)(q.cn + 4), q.cap, r2, k, means, fnd, q.cn + 2, red + 2);
    if (int rc = launch_check(c, "statistical rows")) return rc;
    rtr::launch_stat_sum(s, means, n, 0, 0.0, partial, reinterpret_cast<double *>(red), red + 1);
    if (int rc = launch_check(c, "statistical sum")) return rc;
    uint64_t h[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(h, red, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint64_t have = h[1];
    double S1, S2 = 0.0;
    memcpy(&S1, &h[0], sizeof S1);
    const double mu = have ? S1 / (double)have : 0.0;
    if (have >= 2) {
        rtr::launch_stat_sum(s, means, n, 1, mu, partial, reinterpret_cast<double *>(red), nullptr);
        if (int rc = launch_check(c, "statistical squares")) return rc;
        HIP_TRY(c, hipMemcpyAsync(&S2, red, sizeof S2, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    const double sigma = have >= 2 ? std::sqrt(S2 / (double)(have - 1)) : 0.0;
    const double spread = std_mul * sigma;  // (a product and a sum, each rounded: the build has no contraction)
    const double t = given ? moments[2] : mu + spread;
    rtr::launch_stat_hits(s, means, fnd, n, t, q.hit, c->sel_stats);
    if (int rc = launch_check(c, "statistical hits")) return rc;
    if (int rc = q.ev.record(c, 3, s)) return rc;
    HIP_TRY(c, d2d(s, c->sel_stats + 3, q.cn, sizeof(uint64_t)));
    uint64_t updates = 0;
    HIP_TRY(c, hipMemcpyAsync(&updates, red + 2, sizeof updates, hipMemcpyDeviceToHost, s));
    if (!mean_host.empty()) HIP_TRY(c, hipMemcpyAsync(mean_host.data(), means, n * 4, hipMemcpyDeviceToHost, s));
    if (!found_host.empty()) HIP_TRY(c, hipMemcpyAsync(found_host.data(), fnd, n * 4, hipMemcpyDeviceToHost, s));
    uint64_t out[4] = {0, 0, 0, 0};
    if (int rc = neighbour_finish(c, "statistical combine", q, sop, out, c->statistical_us, &c->statistical_tests_k)) return rc;
    c->statistical_updates_k = saturate_k(updates);
    out[2] -= q.n - q.m;  // (the hits kernel counts every point without a row: the non-finite ones are stats[3]'s)
    // behind everything else that can fail: the caller's arrays change only when the call succeeds
    if (mean_dev) HIP_TRY(c, hipMemcpyAsync(mean_dist, means, n * 4, hipMemcpyDeviceToDevice, s));
    if (found_dev) HIP_TRY(c, hipMemcpyAsync(found, fnd, n * 4, hipMemcpyDeviceToDevice, s));
    if (mean_dev || found_dev) HIP_TRY(c, hipStreamSynchronize(s));
    if (!mean_host.empty()) memcpy(mean_dist, mean_host.data(), n * 4);
    if (!found_host.empty()) memcpy(found, found_host.data(), n * 4);
    if (moments) moments[0] = mu, moments[1] = sigma, moments[2] = t;
    if (stats) memcpy(stats, out, sizeof out);
    return RTR_OK;
}

// ---- normals and curvature (rtr_normals.h, section 6o) --------------------------------
// rtr_select_statistical's order of events without a selection: the search neither creates nor touches it
// (neighbour_search with selects = false), the three outputs go to scratch arrays in upload order that are allocated
// BEFORE the search and preset to "no normal", the rows kernel fills them, and the caller's arrays -- host or device
// memory, each on its own -- are written behind the last thing that can fail.  Two waits on the way (the search's) and
// one at the end.
int rtr_estimate_normals(rtr_ctx *c, uint32_t k, float radius, int flags, const float viewpoint[3], float *normals, float *curvature,
                         uint32_t *found, uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_estimate_normals: no cloud");
    NEED(c, k >= 1u && k <= RTR_NORMAL_MAX_K, "rtr_estimate_normals: k outside 1..RTR_NORMAL_MAX_K");
    NEED(c, std::isfinite(radius) && radius > 0.f, "rtr_estimate_normals: radius must be finite and > 0");
    const float r2 = radius * radius;  // (one fp32 product: the build has no contraction and no fast-math)
    NEED(c, std::isnormal(r2), "rtr_estimate_normals: the square of radius is not a finite normal fp32 number");
    NEED(c, (flags & ~RTR_NORMAL_VIEWPOINT) == 0, "rtr_estimate_normals: unknown bits in flags");
    const bool towards = (flags & RTR_NORMAL_VIEWPOINT) != 0;
    NEED(c, !towards || viewpoint != nullptr, "rtr_estimate_normals: viewpoint is NULL with RTR_NORMAL_VIEWPOINT");
    NEED(c, !towards || (std::isfinite(viewpoint[0]) && std::isfinite(viewpoint[1]) && std::isfinite(viewpoint[2])),
         "rtr_estimate_normals: viewpoint has a non-finite component");
    if (int rc = check_indexable(c)) return rc;
    if (int rc = need_upload_order(c, "formed")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const uint64_t n = c->n;
    const bool normals_dev = normals && on_device(normals), curv_dev = curvature && on_device(curvature), found_dev = found && on_device(found);
    std::vector<float> normals_host, curv_host;
    std::vector<uint32_t> found_host;
    try {
        if (normals && !normals_dev) normals_host.resize(n * 3);
        if (curvature && !curv_dev) curv_host.resize(n);
        if (found && !found_dev) found_host.resize(n);
    } catch (const std::bad_alloc &) {
        return fail(c, RTR_ERR_HIP, "rtr_estimate_normals: no host memory for the staging copy of an output");
    }
    NeighbourSearch q;
    float *nrm, *curv;
    uint32_t *fnd;
    uint64_t *counts;  // [0] pair tests, [1] entries written into rows, [2] points with a normal, [3] normals negated
    HIP_TRY(c, q.buf.get(&nrm, n * 12));
    HIP_TRY(c, q.buf.get(&curv, n * 4));
    HIP_TRY(c, q.buf.get(&fnd, n * 4));
    HIP_TRY(c, q.buf.get(&counts, 4 * sizeof(uint64_t)));
    if (int rc = neighbour_search(c, "rtr_estimate_normals", radius, q, false)) return rc;
    HIP_TRY(c, hipMemsetAsync(nrm, 0, n * 12, s));  // (the points without a normal: (+0, +0, +0), +inf, and 0 where no item holds them)
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)curv, 0x7F800000, n, s));
    HIP_TRY(c, hipMemsetAsync(fnd, 0, n * 4, s));
    HIP_TRY(c, hipMemsetAsync(counts, 0, 4 * sizeof(uint64_t), s));
    rtr::launch_normal_rows(s, q.ks.rec1, q.items, (const uint32_t *)(q.cn + 4), q.cap, r2, k, towards ? viewpoint : nullptr, nrm, curv, fnd, counts);
    if (int rc = launch_check(c, "normal rows")) return rc;
    if (int rc = q.ev.record(c, 3, s)) return rc;
    uint64_t h[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(h, counts, sizeof h, hipMemcpyDeviceToHost, s));
    if (!normals_host.empty()) HIP_TRY(c, hipMemcpyAsync(normals_host.data(), nrm, n * 12, hipMemcpyDeviceToHost, s));
    if (!curv_host.empty()) HIP_TRY(c, hipMemcpyAsync(curv_host.data(), curv, n * 4, hipMemcpyDeviceToHost, s));
    if (!found_host.empty()) HIP_TRY(c, hipMemcpyAsync(found_host.data(), fnd, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // (always: the scratch goes with this call)
    if (int rc = q.ev.stage_us(c, 0, 3, c->normals_us)) return rc;
    c->normals_tests_k = saturate_k(h[0]);
    c->normals_updates_k = saturate_k(h[1]);
    // behind everything else that can fail: the caller's arrays change only when the call succeeds
    if (normals_dev) HIP_TRY(c, hipMemcpyAsync(normals, nrm, n * 12, hipMemcpyDeviceToDevice, s));
    if (curv_dev) HIP_TRY(c, hipMemcpyAsync(curvature, curv, n * 4, hipMemcpyDeviceToDevice, s));
    if (found_dev) HIP_TRY(c, hipMemcpyAsync(found, fnd, n * 4, hipMemcpyDeviceToDevice, s));
    if (normals_dev || curv_dev || found_dev) HIP_TRY(c, hipStreamSynchronize(s));
    if (!normals_host.empty()) memcpy(normals, normals_host.data(), n * 12);
    if (!curv_host.empty()) memcpy(curvature, curv_host.data(), n * 4);
    if (!found_host.empty()) memcpy(found, found_host.data(), n * 4);
    if (stats) stats[0] = h[2], stats[1] = q.m - h[2], stats[2] = q.n - q.m, stats[3] = h[3];  // (every finite point is on the list)
    return RTR_OK;
}

// ---- selection by distance to given points (rtr.h, section 6k) ------------------------
// The given points go through section 6h's key, sort and gather (GivenPoints: rtr_near.hip's k_near_keys over the plain
// strided array); the resident side is ONE sweep over the chunks that sorts and gathers nothing.  One wait on the way,
// for the given points' counters and box: a point beyond the span fails the call there, before anything has changed.  The
// caller's near words and stats are written last.
int rtr_select_near(rtr_ctx *c, const float *xyz, size_t xs, uint64_t count, float radius, int flags, int op, uint32_t *near_words,
                    uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_select_near: no cloud");
    NEED(c, std::isfinite(radius) && radius > 0.f, "rtr_select_near: radius must be finite and > 0");
    const float r2 = radius * radius;  // (one fp32 product: the build has no contraction and no fast-math)
    NEED(c, std::isnormal(r2), "rtr_select_near: the square of radius is not a finite normal fp32 number");
    NEED(c, count == 0 || xyz != nullptr, "rtr_select_near: xyz is NULL");
    NEED(c, xs >= 12 && xs % 4 == 0, "rtr_select_near: xyz_stride_bytes must be >= 12 and a multiple of 4");
    NEED(c, (flags & ~RTR_NEAR_GIVEN_ONLY) == 0, "rtr_select_near: unknown bits in flags");
    const bool given_only = (flags & RTR_NEAR_GIVEN_ONLY) != 0;
    SelectOp sop;
    if (int rc = check_select_op(c, "rtr_select_near", op, &sop)) return rc;
    NEED(c, !given_only || op == 0, "rtr_select_near: op must be 0 with RTR_NEAR_GIVEN_ONLY");
    NEED(c, !given_only || near_words != nullptr, "rtr_select_near: near_words is NULL with RTR_NEAR_GIVEN_ONLY");
    if (int rc = check_indexable(c)) return rc;
    if (count >= (1ull << 32)) return fail(c, RTR_ERR_UNSUPPORTED, "rtr_select_near: given indices are 32-bit: count is %llu", (unsigned long long)count);
    if (!given_only)  // (the near bits go by GIVEN index: they need no upload order)
        if (int rc = need_upload_order(c, "formed", ", or ask for the given side alone (flags = RTR_NEAR_GIVEN_ONLY)")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const uint64_t n = c->n, nw = (n + 31) / 32, gw = (count + 31) / 32;
    const uint64_t gwords = sel_words(count);  // (the near words, padded for launch_select_count)
    const bool near_dev = near_words && on_device(near_words);
    DevBufs buf;
    EventSet ev;
    GivenPoints gp;  // (cn[2]: the near bits)
    NewSelection fresh;
    uint32_t *hit = nullptr, *nearw = nullptr;
    if (int rc = gp.alloc(c, buf, xyz, xs, count)) return rc;
    uint64_t *cn = gp.cn;
    if (!given_only) HIP_TRY(c, buf.get(&hit, nw * 4));
    if (near_words) HIP_TRY(c, buf.get(&nearw, gwords * 4));
    if (!given_only)
        if (int rc = fresh.reserve(c, buf)) return rc;
    if (int rc = ev.create(c, 3)) return rc;
    if (hit) HIP_TRY(c, hipMemsetAsync(hit, 0, nw * 4, s));
    if (nearw) HIP_TRY(c, hipMemsetAsync(nearw, 0, gwords * 4, s));
    if (int rc = ev.record(c, 0, s)) return rc;
    if (int rc = gp.run(c, "rtr_select_near", s, xyz, xs, count, radius)) return rc;
    const uint64_t nonfinite = gp.nonfinite, m = gp.m;
    if (int rc = ev.record(c, 1, s)) return rc;
    if (int rc = fresh.create(c, buf, s)) return rc;
    if (!given_only) HIP_TRY(c, hipMemsetAsync(c->sel_stats, 0, 4 * sizeof(uint64_t), s));
    uint64_t sweep[4] = {0, 0, (n + 255) / 256, 0};  // (no given point has a cell: every chunk is decided without a launch)
    if (m) {
        rtr::launch_near_sweep(s, cloud_of(c), c->bounds, c->reordered ? c->perm : nullptr, gp.ks.k1, gp.ks.rec1, m, radius, r2, gp.glo, gp.ghi, hit,
                               nearw, cn + 4);
        if (int rc = launch_check(c, "near sweep")) return rc;
    }
    uint64_t out[4] = {0, 0, 0, nonfinite};
    if (!given_only) {
        if (int rc = selection_finish(c, s, hit, n, sop, "near combine")) return rc;
        HIP_TRY(c, hipMemcpyAsync(out, c->sel_stats, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    }
    if (nearw && count) {
        rtr::launch_select_count(s, nearw, count, cn + 2);
        if (int rc = launch_check(c, "near count")) return rc;
        HIP_TRY(c, hipMemcpyAsync(out + 2, cn + 2, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    }
    if (int rc = ev.record(c, 2, s)) return rc;
    if (m) HIP_TRY(c, hipMemcpyAsync(sweep, cn + 4, sizeof sweep, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // (always: the scratch goes with this call)
    out[1] = sweep[0];
    if (int rc = ev.stage_us(c, 0, 2, c->near_us)) return rc;
    c->near_tests_k = saturate_k(sweep[1]);
    c->near_chunks[0] = saturate_int(sweep[2]), c->near_chunks[1] = saturate_int(sweep[3]);
    if (near_words && gw) {  // (behind everything that can fail: the caller's words change only when the call succeeds)
        HIP_TRY(c, hipMemcpyAsync(near_words, nearw, gw * 4, near_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    if (stats) memcpy(stats, out, sizeof out);
    return RTR_OK;
}

// ---- the nearest resident point to each given point (rtr.h, section 6l) ---------------
// rtr_select_near's order of events with minima in place of bits (rtr_nearest.hip): the given points are keyed, sorted
// and gathered as there (GivenPoints), with the same wait and the same failure for a point beyond the span; the sweep
// fills one 64-bit slot per given point and, when a resident output is asked for, scratch copies of the two resident
// arrays.  The selection plays no part.  The caller's four arrays and stats are written last.
int rtr_nearest_points(rtr_ctx *c, const float *xyz, size_t xs, uint64_t count, float radius, int flags, uint32_t *given_index,
                       float *given_dist2, uint32_t *resident_index, float *resident_dist2, uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_nearest_points: no cloud");
    NEED(c, std::isfinite(radius) && radius > 0.f, "rtr_nearest_points: radius must be finite and > 0");
    const float r2 = radius * radius;  // (one fp32 product: the build has no contraction and no fast-math)
    NEED(c, std::isnormal(r2), "rtr_nearest_points: the square of radius is not a finite normal fp32 number");
    NEED(c, count == 0 || xyz != nullptr, "rtr_nearest_points: xyz is NULL");
    NEED(c, xs >= 12 && xs % 4 == 0, "rtr_nearest_points: xyz_stride_bytes must be >= 12 and a multiple of 4");
    NEED(c, flags == 0, "rtr_nearest_points: flags must be 0");
    if (int rc = check_indexable(c)) return rc;
    if (count >= (1ull << 32)) return fail(c, RTR_ERR_UNSUPPORTED, "rtr_nearest_points: given indices are 32-bit: count is %llu", (unsigned long long)count);
    if (int rc = need_upload_order(c, "returned")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const uint64_t n = c->n, n4 = (n + 3) & ~3ull;  // (the resident arrays hold whole quads)
    const bool want_res = resident_index || resident_dist2;
    DevBufs buf;
    EventSet ev;
    GivenPoints gp;  // (cn[2]: the given points with a nearest)
    uint64_t *slots;
    uint32_t *gi = nullptr, *gd = nullptr, *ri = nullptr, *rd = nullptr;
    if (int rc = gp.alloc(c, buf, xyz, xs, count)) return rc;
    uint64_t *cn = gp.cn;
    HIP_TRY(c, buf.get(&slots, count * 8));
    if (given_index) HIP_TRY(c, buf.get(&gi, count * 4));
    if (given_dist2) HIP_TRY(c, buf.get(&gd, count * 4));
    if (want_res) HIP_TRY(c, buf.get(&ri, n4 * 4));
    if (want_res) HIP_TRY(c, buf.get(&rd, n4 * 4));
    if (int rc = ev.create(c, 3)) return rc;
    if (count) HIP_TRY(c, hipMemsetAsync(slots, 0xFF, count * 8, s));
    if (want_res) {
        HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)ri, (int)RTR_NEAREST_NONE, n4, s));
        HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)rd, 0x7F800000, n4, s));
    }
    if (int rc = ev.record(c, 0, s)) return rc;
    if (int rc = gp.run(c, "rtr_nearest_points", s, xyz, xs, count, radius)) return rc;
    const uint64_t nonfinite = gp.nonfinite, m = gp.m;
    if (int rc = ev.record(c, 1, s)) return rc;
    uint64_t sweep[4] = {0, 0, (n + 255) / 256, 0};  // (no given point has a cell: every chunk is decided without a launch)
    if (m) {
        rtr::launch_nearest_sweep(s, cloud_of(c), c->bounds, c->reordered ? c->perm : nullptr, gp.ks.k1, gp.ks.rec1, m, radius, r2, gp.glo, gp.ghi,
                                  slots, ri, rd, cn + 4);
        if (int rc = launch_check(c, "nearest sweep")) return rc;
    }
    rtr::launch_nearest_unpack(s, slots, count, gi, gd, cn + 2);
    if (int rc = launch_check(c, "nearest unpack")) return rc;
    if (int rc = ev.record(c, 2, s)) return rc;
    uint64_t have = 0;
    HIP_TRY(c, hipMemcpyAsync(&have, cn + 2, sizeof have, hipMemcpyDeviceToHost, s));
    if (m) HIP_TRY(c, hipMemcpyAsync(sweep, cn + 4, sizeof sweep, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // (always: the scratch goes with this call)
    if (int rc = ev.stage_us(c, 0, 2, c->nearest_us)) return rc;
    c->nearest_tests_k = saturate_k(sweep[1]);
    c->nearest_chunks[0] = saturate_int(sweep[2]), c->nearest_chunks[1] = saturate_int(sweep[3]);
    // behind everything that can fail: the caller's arrays change only when the call succeeds
    struct Out { void *dst; const uint32_t *src; uint64_t words; };
    const Out outs[4] = {{given_index, gi, count}, {given_dist2, gd, count}, {resident_index, ri, n}, {resident_dist2, rd, n}};
    bool copied = false;
    for (const Out &o : outs) {
        if (!o.dst || !o.words) continue;
        HIP_TRY(c, hipMemcpyAsync(o.dst, o.src, o.words * 4, on_device(o.dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        copied = true;
    }
    if (copied) HIP_TRY(c, hipStreamSynchronize(s));
    const uint64_t out[4] = {have, sweep[0], nonfinite, 0};
    if (stats) memcpy(stats, out, sizeof out);
    return RTR_OK;
}

// ---- one registration step (rtr_register.h, section 6p) -------------------------------
// rtr_nearest_points' order of events around the same sweep, with no resident side: the given points go through the pose
// into scratch records (a host array is copied over first), GivenPoints keys, sorts and gathers THOSE, with its wait and
// its failure for a point beyond the span; behind the sweep one bit per winner goes into scratch words, their scan and
// one extract lay the winners' coordinates out by rank, and the two passes of sums follow, with a wait between them for
// the means.  The fit runs on the host (rtr_register_fit.h).  The selection plays no part; moments, step and stats are
// written last.
int rtr_register_points(rtr_ctx *c, const float *xyz, size_t xs, uint64_t count, float radius, int flags, const double pose[12],
                        const float *normals, double moments[RTR_REGISTER_MOMENTS], double step[12], uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_register_points: no cloud");
    NEED(c, std::isfinite(radius) && radius > 0.f, "rtr_register_points: radius must be finite and > 0");
    const float r2 = radius * radius;  // (one fp32 product: the build has no contraction and no fast-math)
    NEED(c, std::isnormal(r2), "rtr_register_points: the square of radius is not a finite normal fp32 number");
    NEED(c, count == 0 || xyz != nullptr, "rtr_register_points: xyz is NULL");
    NEED(c, xs >= 12 && xs % 4 == 0, "rtr_register_points: xyz_stride_bytes must be >= 12 and a multiple of 4");
    NEED(c, (flags & ~RTR_REGISTER_POINT_TO_PLANE) == 0, "rtr_register_points: unknown bits in flags");
    const bool plane = (flags & RTR_REGISTER_POINT_TO_PLANE) != 0;
    NEED(c, !plane || normals != nullptr, "rtr_register_points: normals is NULL with RTR_REGISTER_POINT_TO_PLANE");
    NEED(c, plane || normals == nullptr, "rtr_register_points: normals given without RTR_REGISTER_POINT_TO_PLANE");
    rtr::RegisterPose T{};
    if (pose) {
        for (int i = 0; i < 12; ++i) {
            NEED(c, std::isfinite(pose[i]), "rtr_register_points: pose has a non-finite entry");
            T.t[i] = pose[i];
        }
        T.given = 1;
    }
    if (int rc = check_indexable(c)) return rc;
    if (count >= (1ull << 32)) return fail(c, RTR_ERR_UNSUPPORTED, "rtr_register_points: given indices are 32-bit: count is %llu", (unsigned long long)count);
    if (int rc = need_upload_order(c, "matched")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const uint64_t n = c->n, nw = (n + 31) / 32, nch = (n + 255) / 256, nwin = std::min(count, n);
    const size_t gbytes = count ? (size_t)(count - 1) * xs + 12 : 0;
    const bool xyz_host = count && !on_device(xyz), normals_host = plane && !on_device(normals);
    DevBufs buf;
    GivenPoints gp;
    float4 *posed, *win;
    uint8_t *xstage = nullptr;
    float *nstage = nullptr;
    uint64_t *slots, *tot;
    uint32_t *wsel, *wscan, *scratch;
    double *partial, *red;
    HIP_TRY(c, buf.get(&posed, count * 16));
    if (xyz_host) HIP_TRY(c, buf.get(&xstage, gbytes));
    if (normals_host) HIP_TRY(c, buf.get(&nstage, n * 12));
    if (int rc = gp.alloc(c, buf, reinterpret_cast<const float *>(posed), 16, count)) return rc;
    uint64_t *cn = gp.cn;
    HIP_TRY(c, buf.get(&slots, count * 8));
    HIP_TRY(c, buf.get(&wsel, sel_words(n) * 4));
    HIP_TRY(c, buf.get(&wscan, sel_words(n) * 4));
    HIP_TRY(c, buf.get(&scratch, rtr::scan_scratch_words(nw) * 4));
    HIP_TRY(c, buf.get(&tot, sizeof(uint64_t)));
    HIP_TRY(c, buf.get(&win, nwin * 16));
    HIP_TRY(c, buf.get(&partial, rtr::register_chunks(count) * rtr::kRegPlaneSums * sizeof(double)));
    HIP_TRY(c, buf.get(&red, rtr::kRegPlaneSums * sizeof(double)));
    if (count) HIP_TRY(c, hipMemsetAsync(slots, 0xFF, count * 8, s));
    HIP_TRY(c, hipMemsetAsync(wsel, 0, sel_words(n) * 4, s));
    HIP_TRY(c, hipMemsetAsync(wscan, 0, sel_words(n) * 4, s));
    if (xstage) HIP_TRY(c, hipMemcpyAsync(xstage, xyz, gbytes, hipMemcpyHostToDevice, s));
    if (nstage) HIP_TRY(c, hipMemcpyAsync(nstage, normals, n * 12, hipMemcpyHostToDevice, s));
    rtr::launch_register_pose(s, xstage ? xstage : reinterpret_cast<const uint8_t *>(xyz), xs, count, T, posed);
    if (int rc = launch_check(c, "register pose")) return rc;
    if (int rc = gp.run(c, "rtr_register_points", s, reinterpret_cast<const float *>(posed), 16, count, radius)) return rc;
    const uint64_t nonfinite = gp.nonfinite, m = gp.m;
    if (m) {
        rtr::launch_nearest_sweep(s, cloud_of(c), c->bounds, c->reordered ? c->perm : nullptr, gp.ks.k1, gp.ks.rec1, m, radius, r2, gp.glo, gp.ghi,
                                  slots, nullptr, nullptr, cn + 4);
        if (int rc = launch_check(c, "register sweep")) return rc;
    }
    double mom[RTR_REGISTER_MOMENTS], sums[rtr::kRegPlaneSums] = {};
    rtr::RegisterSums a{};
    a.slots = slots, a.posed = posed, a.win = win, a.wsel = wsel, a.wscan = wscan, a.normals = nstage ? nstage : normals, a.count = count;
    if (m) {
        rtr::launch_register_mark(s, slots, count, wsel);
        if (int rc = launch_check(c, "register mark")) return rc;
        rtr::launch_scan_u32(s, wsel, nw, n, wscan, scratch, tot);
        if (int rc = launch_check(c, "register scan")) return rc;
        // every rank goes to its own slot: at most min(count, n) distinct winners.  The extract takes that bound as its total,
        // not the true number of winners, which lies in *tot on the device: reading it would cost one more wait.  The total
        // only closes the LAST chunk's run of ranks (extract_chunk_skip), so in upload order that one chunk is never left on
        // its two scan words and is gathered even when it holds no winner -- one chunk's bits per call, nothing decoded
        const rtr::Cloud cl = cloud_of(c);
        rtr::ExtractArgs e{};
        e.pk = cl.pk;
        e.x4 = (const float4 *)cl.x, e.y4 = (const float4 *)cl.y, e.z4 = (const float4 *)cl.z;
        e.rgba4 = (const uint4 *)cl.rgba;
        e.perm = c->reordered ? c->perm : nullptr, e.sel = wsel, e.wscan = wscan;
        e.n = n, e.total = nwin, e.c0 = 0, e.c1 = nch, e.first = 0, e.count = nwin;
        e.xyz = reinterpret_cast<uint8_t *>(win), e.xyz_stride = 16, e.xyz_form = 2;
        rtr::launch_extract(s, e);
        if (int rc = launch_check(c, "register extract")) return rc;
        rtr::launch_register_sums(s, a, plane, 0, partial, red);
        if (int rc = launch_check(c, "register sums")) return rc;
        HIP_TRY(c, hipMemcpyAsync(sums, red, 7 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    rtr::register_means(sums, mom);
    const int nsum = plane ? rtr::kRegPlaneSums : rtr::kRegPointSums;
    if (mom[0] > 0.0) {
        for (int i = 0; i < 6; ++i) a.mean[i] = mom[1 + i];
        rtr::launch_register_sums(s, a, plane, 1, partial, red);
        if (int rc = launch_check(c, "register moments")) return rc;
        HIP_TRY(c, hipMemcpyAsync(sums, red, nsum * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));  // (always: the scratch goes with this call)
    if (mom[0] > 0.0)
        for (int i = 0; i < nsum; ++i) mom[(plane ? 4 : 7) + i] = sums[i];  // (plane: the sums take qbar's place)
    double st[12];
    const bool degenerate = plane ? rtr::register_fit_plane(mom, st) : rtr::register_fit_point(mom, st);
    const uint64_t used = (uint64_t)mom[0];
    // behind everything that can fail: the caller's arrays change only when the call succeeds
    if (moments) memcpy(moments, mom, sizeof mom);
    if (step) memcpy(step, st, sizeof st);
    const uint64_t out[4] = {used, m - used, nonfinite, degenerate ? 1u : 0u};
    if (stats) memcpy(stats, out, sizeof out);
    return RTR_OK;
}

// ---- the k nearest resident points to each given point (rtr.h, section 6m) ------------
// rtr_nearest_points' order of events with a row of k slots per given point in place of one (rtr_nearest_k.hip).  The
// unpack kernel writes an output in device memory where it lies and one in host memory into a staging copy; it is the
// last thing queued that can fail, so the caller's arrays and stats change only when the call succeeds.
int rtr_nearest_k_points(rtr_ctx *c, const float *xyz, size_t xs, uint64_t count, float radius, uint32_t k, int flags, uint32_t *index,
                         float *dist2, uint32_t *found, uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    NEED(c, c->cap > 0, "rtr_nearest_k_points: no cloud");
    NEED(c, std::isfinite(radius) && radius > 0.f, "rtr_nearest_k_points: radius must be finite and > 0");
    const float r2 = radius * radius;  // (one fp32 product: the build has no contraction and no fast-math)
    NEED(c, std::isnormal(r2), "rtr_nearest_k_points: the square of radius is not a finite normal fp32 number");
    NEED(c, count == 0 || xyz != nullptr, "rtr_nearest_k_points: xyz is NULL");
    NEED(c, xs >= 12 && xs % 4 == 0, "rtr_nearest_k_points: xyz_stride_bytes must be >= 12 and a multiple of 4");
    NEED(c, k >= 1 && k <= RTR_NEAREST_MAX_K, "rtr_nearest_k_points: k outside 1..RTR_NEAREST_MAX_K");
    NEED(c, flags == 0, "rtr_nearest_k_points: flags must be 0");
    if (int rc = check_indexable(c)) return rc;
    if (count >= (1ull << 32)) return fail(c, RTR_ERR_UNSUPPORTED, "rtr_nearest_k_points: given indices are 32-bit: count is %llu", (unsigned long long)count);
    if (int rc = need_upload_order(c, "returned")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const uint64_t n = c->n, slots = count * k;
    DevBufs buf;
    EventSet ev;
    GivenPoints gp;
    uint64_t *rows, *tally;  // tally: the unpack's three counts, [3] the cascades
    struct Out { void *dst; uint32_t *dev; uint64_t words; };  // dev: where the unpack writes -- dst itself, or its staging copy
    Out outs[3] = {{index, nullptr, slots}, {dist2, nullptr, slots}, {found, nullptr, count}};
    if (int rc = gp.alloc(c, buf, xyz, xs, count)) return rc;
    uint64_t *cn = gp.cn;
    HIP_TRY(c, buf.get(&rows, slots * 8));
    HIP_TRY(c, buf.get(&tally, 4 * sizeof(uint64_t)));
    for (Out &o : outs) {
        if (!o.dst || !o.words) continue;
        if (on_device(o.dst)) o.dev = (uint32_t *)o.dst;
        else HIP_TRY(c, buf.get(&o.dev, o.words * 4));
    }
    if (int rc = ev.create(c, 3)) return rc;
    if (slots) HIP_TRY(c, hipMemsetAsync(rows, 0xFF, slots * 8, s));
    HIP_TRY(c, hipMemsetAsync(tally, 0, 4 * sizeof(uint64_t), s));
    if (int rc = ev.record(c, 0, s)) return rc;
    if (int rc = gp.run(c, "rtr_nearest_k_points", s, xyz, xs, count, radius)) return rc;
    const uint64_t nonfinite = gp.nonfinite, m = gp.m;
    if (int rc = ev.record(c, 1, s)) return rc;
    uint64_t sweep[4] = {0, 0, (n + 255) / 256, 0};  // (no given point has a cell: every chunk is decided without a launch)
    if (m) {
        rtr::launch_nearest_k_sweep(s, cloud_of(c), c->bounds, c->reordered ? c->perm : nullptr, gp.ks.k1, gp.ks.rec1, m, radius, r2, gp.glo, gp.ghi,
                                    rows, k, tally + 3, cn + 4);
        if (int rc = launch_check(c, "nearest k sweep")) return rc;
    }
    rtr::launch_nearest_k_unpack(s, rows, count, k, outs[0].dev, outs[1].dev, outs[2].dev, tally);
    if (int rc = launch_check(c, "nearest k unpack")) return rc;
    if (int rc = ev.record(c, 2, s)) return rc;
    uint64_t t[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(t, tally, sizeof t, hipMemcpyDeviceToHost, s));
    if (m) HIP_TRY(c, hipMemcpyAsync(sweep, cn + 4, sizeof sweep, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // (always: the scratch goes with this call)
    if (int rc = ev.stage_us(c, 0, 2, c->nearest_k_us)) return rc;
    bool copied = false;
    for (const Out &o : outs) {  // (behind everything else that can fail)
        if (!o.dev || o.dev == o.dst) continue;
        HIP_TRY(c, hipMemcpyAsync(o.dst, o.dev, o.words * 4, hipMemcpyDeviceToHost, s));
        copied = true;
    }
    if (copied) HIP_TRY(c, hipStreamSynchronize(s));
    c->nearest_k_tests_k = saturate_k(sweep[1]);
    c->nearest_k_chunks[0] = saturate_int(sweep[2]), c->nearest_k_chunks[1] = saturate_int(sweep[3]);
    c->nearest_k_cascades_k = saturate_k(t[3]);
    const uint64_t out[4] = {t[0], t[1], nonfinite, t[2]};
    if (stats) memcpy(stats, out, sizeof out);
    return RTR_OK;
}

// ---- counting points in bands, fitting a plane (rtr.h, section 6j) --------------------
// Both calls read the coordinates (and, flagged, the selection) and change nothing.  count_bands is the part they share:
// the counters, the selection in resident order when the cloud is sorted (rtr::launch_sel_gather into scratch, once per
// call), the passes of rtr::launch_count_bands, one copy and one wait.  Results reach the caller's arrays only on success.
namespace {
int check_bands_call(rtr_ctx *c, const char *who, int flags) {
    if (c->cap == 0) return fail(c, RTR_ERR_INVALID, "%s: no cloud", who);
    if ((flags & ~RTR_BANDS_SELECTED) != 0) return fail(c, RTR_ERR_INVALID, "%s: unknown bits in flags", who);
    return RTR_OK;
}
// counts[count] and st[4] (host, both written only on success) for `count` valid bands
int count_bands(rtr_ctx *c, uint32_t count, const float *bands, bool selected, uint64_t *counts, uint64_t st[4]) {
    hipStream_t s = c->stream;
    const uint64_t n = c->n, nch = (n + 255) / 256;
    std::vector<uint64_t> host(4 + (size_t)count, 0);
    if (selected && !c->sel) {  // (an empty population: every chunk is outside for every band)
        host[1] = nch * count;
    } else {
        DevBufs buf;
        uint64_t *dev;
        const uint32_t *res = nullptr;
        HIP_TRY(c, buf.get(&dev, host.size() * sizeof(uint64_t)));
        if (selected && c->reordered) {
            uint32_t *r;
            HIP_TRY(c, buf.get(&r, sel_words(n) * 4));
            rtr::launch_sel_gather(s, c->sel, c->perm, n, r);
            if (int rc = launch_check(c, "bands gather")) return rc;
            res = r;
        } else if (selected) {
            res = c->sel;  // (upload order is the resident order)
        }
        HIP_TRY(c, hipMemsetAsync(dev, 0, host.size() * sizeof(uint64_t), s));
        if (res) {
            rtr::launch_select_count(s, res, n, dev);
            if (int rc = launch_check(c, "bands population")) return rc;
        }
        rtr::launch_count_bands(s, cloud_of(c), c->bounds, bands, count, res, dev + 4, dev);
        if (int rc = launch_check(c, "count bands")) return rc;
        HIP_TRY(c, hipMemcpyAsync(host.data(), dev, host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));  // (always: the counts go to the host, the scratch with this call)
        if (!res) host[0] = n;
    }
    memcpy(counts, host.data() + 4, (size_t)count * sizeof(uint64_t));
    memcpy(st, host.data(), 4 * sizeof(uint64_t));
    return RTR_OK;
}
}  // namespace

int rtr_count_in_bands(rtr_ctx *c, uint32_t count, const float *bands, int flags, uint64_t *counts, uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    if (int rc = check_bands_call(c, "rtr_count_in_bands", flags)) return rc;
    NEED(c, count >= 1u && count <= RTR_MAX_BANDS, "rtr_count_in_bands: count outside 1..RTR_MAX_BANDS");
    NEED(c, bands != nullptr, "rtr_count_in_bands: bands is NULL");
    NEED(c, counts != nullptr, "rtr_count_in_bands: counts is NULL");
    for (uint32_t k = 0; k < count; ++k) {
        const float *b = bands + 5 * (size_t)k;
        for (int j = 0; j < 5; ++j) NEED(c, std::isfinite(b[j]), "rtr_count_in_bands: a value in bands is not finite");
        NEED(c, b[0] != 0.f || b[1] != 0.f || b[2] != 0.f, "rtr_count_in_bands: a band of bands has a = b = c = 0");
    }
    if (int rc = check_indexable(c)) return rc;
    const bool selected = (flags & RTR_BANDS_SELECTED) != 0;
    if (selected)
        if (int rc = need_upload_order(c, "read from the selection", " (flags = RTR_BANDS_SELECTED)")) return rc;
    DevGuard g(c->device);
    uint64_t st[4];
    std::vector<uint64_t> out(count);
    if (int rc = count_bands(c, count, bands, selected, out.data(), st)) return rc;
    memcpy(counts, out.data(), (size_t)count * sizeof(uint64_t));
    if (stats) memcpy(stats, st, sizeof st);
    return RTR_OK;
}

// The sample: ranks from rtr_plane_fit.h's sampler, their upload indices (flagged: through the selection words copied to
// the host and the prefix sums of their popcounts), one bit per distinct index into zeroed device words
// (rtr::launch_set_bits), and those points through rtr_extract_points -- in ascending index order, so a draw finds its
// coordinates by binary search among the sorted distinct indices.
int rtr_fit_plane(rtr_ctx *c, float dist, uint32_t iterations, uint64_t seed, int flags, float plane[4], uint64_t stats[4]) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    if (int rc = check_bands_call(c, "rtr_fit_plane", flags)) return rc;
    NEED(c, std::isfinite(dist) && dist >= 0.f, "rtr_fit_plane: dist must be finite and >= 0");
    NEED(c, iterations >= 1u && iterations <= RTR_MAX_BANDS, "rtr_fit_plane: iterations outside 1..RTR_MAX_BANDS");
    NEED(c, plane != nullptr, "rtr_fit_plane: plane is NULL");
    if (int rc = check_indexable(c)) return rc;
    if (int rc = need_upload_order(c, "sampled")) return rc;
    DevGuard g(c->device);
    hipStream_t s = c->stream;
    const auto t0 = std::chrono::steady_clock::now();
    const bool selected = (flags & RTR_BANDS_SELECTED) != 0;
    const uint64_t n = c->n, nw = (n + 31) / 32;
    uint64_t m = n;
    std::vector<uint32_t> selw, pre;  // flagged: the selection words and pre[w] = the selected points below word w
    if (selected) {
        m = 0;
        if (c->sel && nw) {
            selw.resize(nw), pre.resize(nw + 1);
            HIP_TRY(c, hipMemcpyAsync(selw.data(), c->sel, nw * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            pre[0] = 0;
            for (uint64_t w = 0; w < nw; ++w) pre[w + 1] = pre[w] + (uint32_t)__builtin_popcount(selw[w]);
            m = pre[nw];
        }
    }
    const uint32_t draws = 3u * iterations;
    std::vector<uint64_t> rank(draws), cnt;
    std::vector<uint32_t> idx(draws), uniq;
    std::vector<float> xyz, planes(4 * (size_t)iterations), bands;
    std::vector<uint32_t> cand;  // the non-degenerate candidates, ascending
    if (m >= 3) {
        for (uint32_t t = 0; t < draws; ++t) {
            rank[t] = rtr::plane_draw(seed, t) % m;
            uint32_t u = (uint32_t)rank[t];
            if (selected) {  // the rank-th set bit
                const uint64_t w = (uint64_t)(std::upper_bound(pre.begin(), pre.end(), (uint32_t)rank[t]) - pre.begin()) - 1;
                uint32_t bits = selw[w];
                for (uint32_t k = (uint32_t)rank[t] - pre[w]; k > 0; --k) bits &= bits - 1;
                u = (uint32_t)(32 * w) + (uint32_t)__builtin_ctz(bits);
            }
            idx[t] = u;
        }
        uniq = idx;
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        const uint64_t k = uniq.size();
        DevBufs buf;  // the sample's bits are set on the device: no word of them crosses the bus
        uint32_t *dw, *di;
        HIP_TRY(c, buf.get(&dw, nw * 4));
        HIP_TRY(c, buf.get(&di, k * 4));
        HIP_TRY(c, hipMemsetAsync(dw, 0, nw * 4, s));
        HIP_TRY(c, hipMemcpyAsync(di, uniq.data(), k * 4, hipMemcpyHostToDevice, s));
        rtr::launch_set_bits(s, di, k, dw);
        if (int rc = launch_check(c, "sample bits")) return rc;
        xyz.resize(3 * k);
        if (int rc = rtr_extract_points(c, dw, nw, 0, k, xyz.data(), 12, nullptr, 0, nullptr, nullptr)) return rc;
        for (uint32_t q = 0; q < iterations; ++q) {
            const float *p[3];
            for (int j = 0; j < 3; ++j)
                p[j] = xyz.data() + 3 * (size_t)(std::lower_bound(uniq.begin(), uniq.end(), idx[3 * q + j]) - uniq.begin());
            float band[5];
            if (!rtr::plane_candidate(p[0], p[1], p[2], &rank[3 * (size_t)q], &planes[4 * (size_t)q])) continue;
            rtr::plane_band(&planes[4 * (size_t)q], dist, band);
            if (!std::isfinite(band[3]) || !std::isfinite(band[4])) continue;
            cand.push_back(q);
            bands.insert(bands.end(), band, band + 5);
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
    uint64_t out[4] = {0, 0, 0, m};
    float win[4] = {0.f, 0.f, 0.f, 0.f};
    if (!cand.empty()) {
        uint64_t st[4];
        cnt.resize(cand.size());
        if (int rc = count_bands(c, (uint32_t)cand.size(), bands.data(), selected, cnt.data(), st)) return rc;
        size_t best = 0;
        for (size_t j = 1; j < cand.size(); ++j)
            if (cnt[j] > cnt[best]) best = j;  // (ties: the smallest c stays)
        out[0] = cnt[best], out[1] = cand.size(), out[2] = cand[best];
        memcpy(win, &planes[4 * (size_t)cand[best]], sizeof win);
    }
    const auto t2 = std::chrono::steady_clock::now();
    c->plane_us[0] = (int)std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
    c->plane_us[1] = (int)std::chrono::duration_cast<std::chrono::microseconds>(t2 - t1).count();
    memcpy(plane, win, sizeof win);
    if (stats) memcpy(stats, out, sizeof out);
    return RTR_OK;
}

int rtr_clear_selection(rtr_ctx *c) {
    if (!c) return RTR_ERR_INVALID;
    c->ov.other_call();
    DevGuard g(c->device);
    free_select(c);
    return RTR_OK;
}

}  // extern "C"
