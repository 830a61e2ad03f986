"""Every entry point of the library called while an overlapped streak (option "overlap", include/rtr.h) is still IN
FLIGHT: the point kernel of the streak's last frames sits on the front stream, their tile kernels and prefilters on the
context's stream, both held by a plug (streak_ctx.py), and the call under test arrives before any of them has run.  The
call must either drain both streams or queue strictly behind them.

One case: nine frames of warm-up (lean frames from there on), an unplugged streak of the same shape (everything
rtr_render allocates exists), the plugged streak of m = 3 or 4 frames (its last frame sits once in each tile store),
`assert not event.query()`, THE CALL, an unplugged streak of four frames.  Asserted for every case:
 (a) the snapshots of the plugged streak equal the oracle, bit for bit, on the cloud and state as they were when those
     frames were queued (depth, image, fp16 tensor, min / max words);
 (b) the call's own result against a plain host statement (numpy, the oracle, moved() of test_gpu_transform.py,
     select_ref.py, point_pass_ref.py, clip_keep);
 (c) the following streak reads overlap_active 0, 0, 1, 1, equals the oracle on the NEW state and reports no error.

The issue's pairs (pack 0 and back to 2, keep mask set then cleared, clip planes set then None, set_stream then
reset_stream) are each two kinds, run alone on a context prepared for the second half, and chained on one context in
test_paired_calls_on_one_context.  After reset_stream nothing can be cloned in stream order (the library's own stream
is no torch stream), so there (c) checks the buffers of the last following frame only.

The kinds are generators: what comes before their first `yield` prepares the arguments (before the plug is queued), the
engine asserts that the streak is in flight, and the next step makes the call and checks (b).

Which wait of csrc/rtr_api.hip a case pins -- remove it and the named assertion fails:
 - append / remove / transform, set_point_keep: complete_all -> sync_streams(front, then tail) before a window is
   committed or the mask rebuilt: (a), the queued frames would read rewritten chunks or the new mask; (c) for the
   `consumed` / `binned` events and the lean fold a half-drained store leaves behind.
 - upload_points, generate_synthetic, reorder_points, option "pack", set_resolution: sync_streams at the head of the
   call, before free_cloud / free_pack / free_frame: (a).
 - set_clip_planes, set_params, option "split_threshold": host state only, the queued launches carry their own
   arguments: (a) shows a launch that read the context late, (c) that the list of the old state was dropped.
 - point_pass, render_views, the phase calls, project_async: queued on the context's stream, which has waited for
   `binned` of every frame it completes, and returned from while the streak is still held (asserted: `_queued`): (b)
   reads the streak's LAST frame; (a) that nothing of theirs overtook the streak.  The first point pass of a context and
   the first batch of a view count allocate and drain both streams for that (sync_streams in rtr_point_pass /
   ensure_views): the kinds make one such call before the plug, and `point_pass_first_use` / `views_first_use` pin the
   draining first use by itself.
 - select_points, extract_points, download_points: queued on the context's stream like those, but they then WAIT for it
   (the statistics, the host copies; download_points ends each window with sync_streams): (b) reads the resident cloud.
 - project, frame_stats, download, synchronize, rtr_wait: sync_streams / repair behind their copies: (b).
 - set_stream / reset_stream: switch_stream drains both streams before the next frame runs on another stream: (a) for
   the snapshots, (c) for a frame that would otherwise start beside the old stream's tail.
 - close: rtr_destroy's sync_streams before anything is freed: (a).
 - an overflowing frame inside the plugged streak: complete_all's repair renders it again with the cloud and mask it
   was issued with, before the edit: the frame buffers after the call, and (c).

Measured on an MI355X (streak_ctx.py has the plug's figures: 0.37 ms to queue a streak, a plug of 60 ms = 143.5 M
cycles): the 170 cases of this module run in 15 s, the slowest in 0.5 s.  No case found a missing wait: the library is
unchanged."""
import numpy as np
import pytest

import point_pass_ref as ppr
import pool_overflow_scenes as sc
import select_ref
import test_gpu_transform as transform_tests
from streak_ctx import AUTO, Ctx, Scene

pytestmark = pytest.mark.gpu

PLANES = np.float32([[0.3, -0.2, 0.9, 0.35]])
RIGID = transform_tests.TRANSFORMS["rigid"]
NAMES = ("depth", "img", "tensor", "minmax")


# ---- the host model ------------------------------------------------------------------------------------------------
class State:
    """What the frames of a context show: the resident cloud in upload order, the keep mask and clip planes in force and
    the parameters; `ref` is the oracle's frame of it.  States are made once per (scene, lineage) and never changed; they
    hang on their Scene object and go with it."""

    def __init__(self, scene, tag, xyzw, rgba, keep=None, clip=None, params=None):
        self.scene, self.tag, self.xyzw, self.rgba, self.keep, self.clip, self.params = scene, tag, xyzw, rgba, keep, clip, params
        self._refs, self._serial = {}, {}

    @classmethod
    def base(cls, scene):
        states = scene.__dict__.setdefault("states", {})
        if "base" not in states:
            states["base"] = cls(scene, "base", scene.xyzw, scene.rgba)
        return states["base"]

    def but(self, op, **changes):
        """The state after `op` (a name that, with this state's lineage, fixes the changes)."""
        states, tag = self.scene.states, self.tag + "/" + op
        if tag not in states:
            f = dict(xyzw=self.xyzw, rgba=self.rgba, keep=self.keep, clip=self.clip, params=self.params)
            f.update(changes)
            states[tag] = State(self.scene, tag, **f)
        return states[tag]

    @property
    def n(self):
        return self.xyzw.shape[0]

    def shown(self):
        m = np.ones(self.n, bool) if self.keep is None else self.keep.copy()
        if self.clip is not None:
            m &= self.scene.pkg.clip_keep(self.clip, self.xyzw)
        return (self.xyzw, self.rgba) if m.all() else (np.ascontiguousarray(self.xyzw[m]), np.ascontiguousarray(self.rgba[m]))

    def _params(self):
        if self.params is None:
            return None
        prm = self.scene.orc.default_params()
        for k, v in self.params.items():
            setattr(prm, k, v)
        return prm

    def ref(self, P, filtered=True):
        key = (np.asarray(P, np.float32).tobytes(), bool(filtered))
        if key not in self._refs:
            orc, sc_ = self.scene.orc, self.scene
            xyzw, rgba = self.shown()
            r = orc.project(xyzw, rgba, P, sc_.W, sc_.H, self._params())
            out = {"depth": r["depth_bits"], "img": r["img"]}
            if filtered:
                f = orc.filter(r["depth_bits"], r["img"], self._params())
                out = {"depth": f["depth"].view(np.uint32), "img": f["img"], "tensor": f["tensor"], "minmax": f["minmax"],
                       "mask": f["mask"]}
            self._refs[key] = out
        return self._refs[key]


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.size == want.size and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape)
    g, w = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
    assert np.array_equal(g, w), (what, int((g != w).sum()), "bytes differ")


def check(frames, state, poses, flags, what):
    """The frames (Ctx.run / Ctx.frames) against the oracle on `state`, bit for bit."""
    flags = [flags] * len(poses) if isinstance(flags, bool) else flags
    assert len(frames) == len(poses)
    for k, (f, P, fl) in enumerate(zip(frames, poses, flags)):
        want = state.ref(P, fl)
        assert set(f) == set(NAMES if fl else NAMES[:2])
        for name, got in f.items():
            _same(got, want[name], (what, state.tag, "frame", k, name))


def _resident_is(c, state, what):
    """The resident cloud, read back in upload order, is the state's."""
    assert c.p.num_points == state.n, what
    xyz, rgb = c.p.extract_points()
    _same(xyz, state.xyzw, (what, "xyz"))
    _same(rgb, state.rgba, (what, "rgb"))


def _rows(xyzw, rgba):
    rec = np.concatenate([np.ascontiguousarray(xyzw, np.float32).view(np.uint32), np.ascontiguousarray(rgba).view(np.uint32)], axis=1)
    return rec[np.lexsort(rec.T)]


@pytest.fixture(scope="module")
def scenes(pkg, orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Scene(pkg, orc, name)
        return cache[name]
    return get


# ---- the calls under test ------------------------------------------------------------------------------------------
# kind(c, s, P_last) -> generator: prepare; yield; call + (b); yield (new state, how the following streak is rendered)
def k_append(c, s, P):
    xyz, rgb = s.scene.orc.generate("room_shell", 0xC0FFEE11, 0, 10_000, 10_000)
    new = s.but("append", xyzw=np.concatenate([s.xyzw, xyz]), rgba=np.concatenate([s.rgba, rgb]),
                keep=None if s.keep is None else np.concatenate([s.keep, np.ones(10_000, bool)]))
    yield
    c.p.append_points(xyz, rgb)
    _resident_is(c, new, "append")
    if new.keep is not None:
        assert np.array_equal(c.p.point_keep(), new.keep), "append"
    yield new, "run"


def _remove(name, mask_of):
    def kind(c, s, P):
        keep = mask_of(s.n)
        new = s.but(name, xyzw=np.ascontiguousarray(s.xyzw[keep]), rgba=np.ascontiguousarray(s.rgba[keep]),
                    keep=None if s.keep is None else s.keep[keep])
        yield
        c.p.remove_points(keep)
        _resident_is(c, new, name)
        if s.keep is not None:
            assert np.array_equal(c.p.point_keep(), new.keep), name
        yield new, "run"
    return kind


def _last_chunk(n):
    return n - n % 256 if n % 256 else n - 256


def _one(n):
    keep = np.zeros(n, bool)
    keep[n // 2] = True
    return keep


k_remove_random = _remove("remove_random", lambda n: np.random.default_rng(7).random(n) >= 0.3)
k_remove_tail = _remove("remove_tail", lambda n: np.arange(n) < _last_chunk(n))
k_remove_all_but_one = _remove("remove_all_but_one", _one)


def _transform(name, sel_of):
    def kind(c, s, P):
        sel = sel_of(s.n)
        new = s.but(name, xyzw=transform_tests.moved(s.xyzw, RIGID, sel))
        yield
        c.p.transform_points(RIGID, sel)
        _resident_is(c, new, name)
        yield new, "run"
    return kind


k_transform_all = _transform("transform_all", lambda n: None)
k_transform_quarter = _transform("transform_quarter", lambda n: np.arange(n) >= n - n // 4)


def _upload(name, size_of):
    def kind(c, s, P):
        m = size_of(s.n)
        xyz, rgb = s.scene.orc.generate("room_shell", 0xC0FFEE12, 0, m, m)
        new = s.but(name, xyzw=xyz, rgba=rgb, keep=None)
        yield
        c.p.upload_points(xyz, rgb)
        _resident_is(c, new, name)
        yield new, "run"
    return kind


k_upload_smaller = _upload("upload_smaller", lambda n: n // 2 + 1)
k_upload_larger = _upload("upload_larger", lambda n: n + n // 2 + 3)


def k_reorder(c, s, P):
    want = _rows(s.xyzw, s.rgba)
    yield
    c.p.reorder_points()
    assert c.p.get_option("reordered") == 1 and c.p.num_points == s.n
    assert np.array_equal(_rows(*c.p.download_points()), want)  # (the same points, in whatever order)
    yield s, "run"


def _pack(value):
    def kind(c, s, P):
        yield
        c.p.set_option("pack", value)
        assert c.p.get_option("pack") == value
        assert c.p.get_option("packed") == (1 if value == 2 else 0)
        _resident_is(c, s, ("pack", value))
        yield s, "run"
    return kind


def k_generate(c, s, P):
    xyz, rgb = s.scene.orc.generate("uniform_box", 0xC0FFEE13, 0, s.n, s.n)
    new = s.but("generate", xyzw=xyz, rgba=rgb, keep=None)
    want = _rows(xyz, rgb)
    yield
    c.p.generate_synthetic("uniform_box", 0xC0FFEE13, 0, s.n, s.n)
    assert c.p.num_points == s.n
    assert np.array_equal(_rows(*c.p.download_points()), want)  # (the library may have sorted it)
    yield new, "run"


def _half(n):
    return np.random.default_rng(11).random(n) < 0.5


def with_keep(c, s):
    keep = _half(s.n)
    c.p.set_point_keep(keep)
    return s.but("keep_set", keep=keep)


def k_keep_set(c, s, P):
    keep = _half(s.n)
    new = s.but("keep_set", keep=keep)
    yield
    c.p.set_point_keep(keep)
    assert np.array_equal(c.p.point_keep(), keep)
    yield new, "run"


def k_keep_clear(c, s, P):
    new = s.but("keep_clear", keep=None)
    yield
    c.p.set_point_keep(None)
    assert c.p.point_keep() is None
    yield new, "run"


def with_clip(c, s):
    c.p.set_clip_planes(PLANES)
    return s.but("clip_set", clip=PLANES)


def k_clip_set(c, s, P):
    new = s.but("clip_set", clip=PLANES)
    assert 0 < new.shown()[0].shape[0] < s.shown()[0].shape[0]  # (the plane cuts the cloud)
    yield
    c.p.set_clip_planes(PLANES)
    assert np.array_equal(c.p.clip_planes(), PLANES)
    yield new, "run"


def k_clip_clear(c, s, P):
    new = s.but("clip_clear", clip=None)
    yield
    c.p.set_clip_planes(None)
    assert c.p.clip_planes().shape == (0, 4)
    yield new, "run"


def k_params(c, s, P):
    prm = {"depth_window": 0.05, "filter_strength": 1.1}
    new = s.but("params", params=prm)
    yield
    c.p.set_params(**prm)
    got = c.p.params
    assert (got.depth_window, got.filter_strength) == (np.float32(0.05), np.float32(1.1)) and got.levels == 4
    yield new, "run"


def k_split_threshold(c, s, P):
    yield
    c.p.set_option("split_threshold", 64)
    assert c.p.get_option("split_threshold") == 64
    stats = yield s, "run"
    assert stats["split_tiles"] > 0, stats  # (the following streak really went through the split launch)


def k_resolution(c, s, P):
    W, H = s.scene.W, s.scene.H
    yield
    c.resolution(320, 240)
    c.resolution(W, H)
    assert (c.p.W, c.p.H) == (W, H) and tuple(c.bufs["depth"].shape) == (H, W)
    yield s, "run"


def _queued(c, what):
    """Directly behind a call that must QUEUE behind the streak: the streak's first frame is still held by the plug.  (A
    call that drained instead took another path than the one its case is there for.)"""
    assert not c.first.query(), (what, "the call drained the streak: the queue-behind path was not taken")


def _point_pass(first_use):
    def kind(c, s, P):
        xyzw, _ = s.shown()
        assert xyzw is s.xyzw  # (IDs are upload indices: no mask or plane in these cases)
        e_ids, e_vis = ppr.point_pass(s.scene.orc, s.xyzw, P, s.scene.W, s.scene.H, s.ref(P)["depth"])
        L = c.pkg._lib
        if not first_use:
            # (a context's first pass allocates its buffers and drains both streams for that, rtr_point_pass: one pass
            # before the plug, so that the call under test only queues its kernel on the context's stream)
            c.p.point_pass(s.scene.poses[8])
            c.p.synchronize()
        yield
        c.p.point_pass(P)
        if not first_use:
            _queued(c, "point_pass")
        ids, vis = c.p.download(L.BUF_POINT_ID), c.p.download(L.BUF_VISIBLE)
        assert np.array_equal(ids, e_ids), ("ids", int((ids != e_ids).sum()))
        assert np.array_equal(vis, e_vis), "visible"
        yield s, "run"
    return kind


def k_select(c, s, P):
    sc_, L = s.scene, c.pkg._lib
    rect = (sc_.W // 4, sc_.H // 4, 3 * sc_.W // 4, 3 * sc_.H // 4)
    inside = select_ref.inside(sc_.pkg, sc_.orc, s.xyzw, PLANES, P, rect, sc_.W, sc_.H)
    assert 0 < inside.sum() < s.n
    yield
    stats = c.p.select_points(planes=PLANES, P=P, rect=rect)
    assert stats[0] == inside.sum(), (stats, int(inside.sum()))
    assert c.p.selection() is not None
    assert np.array_equal(c.p.download(L.BUF_SELECTION), select_ref.words(inside))
    yield s, "run"


def k_extract(c, s, P):
    sel = np.arange(s.n) % 3 == 0
    yield
    xyz, rgb = c.p.extract_points()
    _same(xyz, s.xyzw, "extract all xyz")
    _same(rgb, s.rgba, "extract all rgb")
    xyz, rgb, idx = c.p.extract_points(sel, indices=True)
    _same(xyz, s.xyzw[sel], "extract selection xyz")
    _same(rgb, s.rgba[sel], "extract selection rgb")
    assert np.array_equal(idx, np.flatnonzero(sel))
    yield s, "run"


def k_download_points(c, s, P):
    yield
    xyz, rgb = c.p.download_points()
    _same(xyz, s.xyzw, "download_points xyz")
    _same(rgb, s.rgba, "download_points rgb")
    yield s, "run"


def _views(first_use):
    def kind(c, s, P):
        L = c.pkg._lib
        Ps = np.stack(s.scene.poses[7:9])
        want = [s.ref(p) for p in Ps]
        if not first_use:
            # (the first batch of a count allocates the views' buffers, stores and pools and drains both streams for
            # that, ensure_views: one batch of the same count before the plug)
            c.p.render_views(np.stack(s.scene.poses[5:7]), True)
            c.p.synchronize()
        yield
        c.p.render_views(Ps, True)
        if not first_use:
            _queued(c, "render_views")
        _views_are(c, L, want)
        yield s, "run"
    return kind


def _views_are(c, L, want):
    for which, name in ((L.BUF_VIEW_DEPTH, "depth"), (L.BUF_VIEW_IMAGE, "img"), (L.BUF_VIEW_TENSOR, "tensor"), (L.BUF_VIEW_MINMAX, "minmax")):
        got = c.p.download(which)
        for v in range(2):
            _same(got[v], want[v][name], ("view", v, name))


def k_phases(c, s, P):
    L = c.pkg._lib
    P2 = s.scene.poses[8]
    want = s.ref(P2)
    yield
    c.p.clear(); c.p.min_depth_pass(P2); c.p.accumulate_pass(P2); c.p.resolve(); c.p.filter()
    _queued(c, "phase calls")
    for which, name in ((L.BUF_DEPTH, "depth"), (L.BUF_IMAGE, "img"), (L.BUF_TENSOR, "tensor"), (L.BUF_MINMAX, "minmax"), (L.BUF_MASK, "mask")):
        _same(c.p.download(which), want[name], ("phases", name))
    yield s, "run"


def k_project(c, s, P):
    P2 = s.scene.poses[8]
    yield
    img, depth = c.p.project(P2)
    _same(depth, s.ref(P2, False)["depth"], "project depth")
    _same(img, s.ref(P2, False)["img"], "project image")
    img, depth = c.p.project(P2, filtered=True)
    _same(depth, s.ref(P2)["depth"], "project_filtered depth")
    _same(img, s.ref(P2)["img"], "project_filtered image")
    _same(c.p.download(c.pkg._lib.BUF_TENSOR), s.ref(P2)["tensor"], "project_filtered tensor")
    yield s, "run"


def k_project_async(c, s, P):
    P2 = s.scene.poses[8]
    img, depth = c.p.host_output_buffers(0)  # (allocates the slots: before the plug)
    yield
    c.p.project_async(P2, 0, filtered=True)
    _queued(c, "project_async")
    c.p.wait_outputs(0)
    _same(depth, s.ref(P2)["depth"], "slot depth")
    _same(img, s.ref(P2)["img"], "slot image")
    yield s, "run"


def _serial_stats(c, s, P):
    """(entries, colour_chunks, errors) of P's frame in a serial context (option "overlap" = 0) past its warm-up."""
    key, _serial = np.asarray(P, np.float32).tobytes(), s._serial
    if key not in _serial:
        assert s.tag == "base"
        ser = Ctx(c.pkg, s.scene, {"overlap": 0})
        try:
            ser.run(s.scene.poses, True)
            ser.p.synchronize()
            ser.p.render(P, True)
            st = ser.p.frame_stats()
            _serial[key] = (st["entries"], st["colour_chunks"], st["errors"])
        finally:
            ser.close()
    return _serial[key]


def k_frame_stats(c, s, P):
    want = _serial_stats(c, s, P)
    assert want[0] > 0 and want[2] == 0
    yield
    st = c.p.frame_stats()
    assert (st["entries"], st["colour_chunks"], st["errors"]) == want, (st, want)
    yield s, "run"


def k_download(c, s, P):
    L = c.pkg._lib
    want = s.ref(P)
    yield
    for which, name in ((L.BUF_DEPTH, "depth"), (L.BUF_IMAGE, "img"), (L.BUF_TENSOR, "tensor"), (L.BUF_MINMAX, "minmax"), (L.BUF_MASK, "mask")):
        _same(c.p.download(which), want[name], ("download", name))
    yield s, "run"


def k_set_stream(c, s, P):
    st2 = c.torch.cuda.Stream(device=0)
    yield
    c.p.set_stream(st2.cuda_stream)
    c.st = st2  # (the following streak and its clones run there; nothing here has synchronised the old stream)
    yield s, "run"


def k_reset_stream(c, s, P):
    yield
    c.p.reset_stream()
    # (the library's own stream is no torch stream and the ABI hands out no handle to it, so nothing can be cloned in
    # stream order there: of the following streak (c) checks overlap_active of all four frames, but only the LAST
    # frame's buffers, downloaded behind a synchronisation)
    yield s, "host"


def k_synchronize(c, s, P):
    yield
    c.p.synchronize()
    for name in NAMES:  # (no copy queued by the library: the frame buffers as they are)
        _same(c.bufs[name].cpu().numpy(), s.ref(P)[name], ("behind synchronize", name))
    yield s, "run"


def k_close(c, s, P):
    yield
    c.close()  # (Projector.close is idempotent -- it clears its handle -- so the test's own close() in `finally` is a no-op)
    yield s, "fresh"


# name -> (what puts the context into its starting state or None, the kind, context options)
KINDS = {
    # calls that rewrite or free what the running point kernel reads
    "append": (None, k_append, {}), "remove_random": (None, k_remove_random, {}), "remove_tail": (None, k_remove_tail, {}),
    "remove_all_but_one": (None, k_remove_all_but_one, {}), "transform_all": (None, k_transform_all, {}),
    "transform_quarter": (None, k_transform_quarter, {}), "upload_smaller": (None, k_upload_smaller, {}),
    "upload_larger": (None, k_upload_larger, {}), "reorder": (None, k_reorder, {}), "pack_0": (None, _pack(0), {"pack": 2}),
    "pack_2": (None, _pack(2), {"pack": 0}), "generate": (None, k_generate, {}),
    # calls that change state queued frames must not see
    "keep_set": (None, k_keep_set, {}), "keep_clear": (with_keep, k_keep_clear, {}), "clip_set": (None, k_clip_set, {}),
    "clip_clear": (with_clip, k_clip_clear, {}), "params": (None, k_params, {}), "split_threshold": (None, k_split_threshold, {}),
    "resolution": (None, k_resolution, {}),
    # calls that queue or read behind the streak
    "point_pass": (None, _point_pass(False), {}), "point_pass_first_use": (None, _point_pass(True), {}), "select": (None, k_select, {}), "extract": (None, k_extract, {}),
    "download_points": (None, k_download_points, {}), "views": (None, _views(False), {}),
    "views_first_use": (None, _views(True), {}), "phases": (None, k_phases, {}),
    "project": (None, k_project, {}), "project_async": (None, k_project_async, {}), "frame_stats": (None, k_frame_stats, {}),
    "download": (None, k_download, {}), "set_stream": (None, k_set_stream, {}), "reset_stream": (None, k_reset_stream, {}),
    "synchronize": (None, k_synchronize, {}),
    # tear-down
    "close": (None, k_close, {}),
}
SUBSET = ("append", "remove_random", "transform_quarter", "keep_set", "point_pass")


# ---- the engine ----------------------------------------------------------------------------------------------------
def plugged_step(c, s, m, kind, what, mode=-1):
    """The unplugged streak, the plugged one, the assertion, the call, (a) and (c); -> the state after the call."""
    scene = s.scene
    poses, follow = scene.poses[:m], scene.poses[4:8]
    want = AUTO[:m] if mode < 0 else [1] * m
    active, frames = c.run(poses, True)  # (the same shape unplugged: whatever rtr_render allocates now exists)
    assert active == want, (what, active)
    check(frames, s, poses, True, (what, "unplugged"))
    c.p.synchronize()
    g = kind(c, s, poses[-1])
    next(g)
    active, event, snaps = c.run_plugged(poses, True)
    assert active == want, (what, active)
    assert not event.query() and not c.first.query(), (what, "the streak had left the queue before the call under test: the case has tested nothing")
    new, how = next(g)  # THE CALL UNDER TEST, and (b)
    check(Ctx.frames(event, snaps), s, poses, True, (what, "(a)"))
    want = AUTO[:4] if mode < 0 else [1] * 4
    if how == "run":
        active, frames = c.run(follow, True)
        check(frames, new, follow, True, (what, "(c)"))
    elif how == "host":
        active = []
        for P in follow:
            c.p.render(P, True)
            active.append(c.p.get_option("overlap_active"))
        c.p.synchronize()
        L = c.pkg._lib
        last = dict(zip(NAMES, (c.p.download(w) for w in (L.BUF_DEPTH, L.BUF_IMAGE, L.BUF_TENSOR, L.BUF_MINMAX))))
        check([last], new, follow[-1:], True, (what, "(c)"))
    else:
        assert how == "fresh"
        c2 = Ctx(c.pkg, scene)
        try:
            active, frames = c2.run(follow, True)
            check(frames, new, follow, True, (what, "(c)"))
            assert c2.p.frame_stats()["errors"] == 0
        finally:
            c2.close()
    assert active == want, (what, "(c)", active)
    if how != "fresh":
        stats = c.p.frame_stats()
        assert stats["errors"] == 0, (what, stats)
        try:
            g.send(stats)
        except StopIteration:
            pass
    return new


def _warm_up(c, s, frames=9):
    """Nine frames: past the split launch's grace period (eight frames), lean frames from here on."""
    active, got = c.run(s.scene.poses[:frames], True)
    check(got, s, s.scene.poses[:frames], True, "warm-up")
    c.p.synchronize()


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("shape", ["96x64", "208x112"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_call_behind_a_streak_in_flight(pkg, scenes, kind, shape, m):
    scene = scenes(shape)
    setup, fn, options = KINDS[kind]
    c = Ctx(pkg, scene, options)
    try:
        s = State.base(scene)
        if setup:
            s = setup(c, s)
        _warm_up(c, s)
        plugged_step(c, s, m, fn, (kind, shape, m))
    finally:
        c.close()


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", SUBSET)
def test_call_behind_a_streak_that_is_not_lean_yet(pkg, scenes, kind, m):
    """A fresh context: with the unplugged streak four frames of warm-up, so the plugged streak's frames are frames
    5 .. 8 of the cloud at the most -- the split launch is still on, the frames have T1's epilogue and the reset of the
    split tiles' pixels sits on the tail stream."""
    scene = scenes("208x112")
    c = Ctx(pkg, scene)
    try:
        s = State.base(scene)
        _warm_up(c, s, 4 - m)  # (m = 3: one frame; m = 4: none -- plugged_step's unplugged streak is the rest)
        plugged_step(c, s, m, KINDS[kind][1], (kind, "not lean", m))
    finally:
        c.close()


@pytest.mark.parametrize("kind", SUBSET)
def test_call_behind_a_streak_with_explicit_overlap(pkg, scenes, kind):
    """Option "overlap" = 1: every frame overlaps and `consumed` is recorded behind every reader."""
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = State.base(scene)
        _warm_up(c, s)
        plugged_step(c, s, 4, KINDS[kind][1], (kind, "overlap = 1"), mode=1)
    finally:
        c.close()


@pytest.mark.parametrize("variant", ["plain", "sorted", "keep"])
def test_plugged_steps_in_a_row(pkg, scenes, variant):
    """One context: streak -> remove -> streak -> transform -> streak -> append, every streak plugged and in flight; on
    a cloud the library sorted (upload-order indices through the permutation) and with a keep mask in force (compacted
    by the removal, extended by the append)."""
    scene = scenes("640x480")
    c = Ctx(pkg, scene, {"auto_reorder": 1, "point_ids": 1} if variant == "sorted" else {})
    try:
        assert c.p.get_option("reordered") == (1 if variant == "sorted" else 0)
        s = State.base(scene)
        if variant == "keep":
            s = with_keep(c, s)
        _warm_up(c, s)
        for m, name in ((3, "remove_random"), (4, "transform_quarter"), (3, "append")):
            s = plugged_step(c, s, m, KINDS[name][1], (variant, name, m))
    finally:
        c.close()


PAIRS = {"pack_0_then_2": ("pack_0", "pack_2"), "keep_then_clear": ("keep_set", "keep_clear"),
         "clip_then_none": ("clip_set", "clip_clear"), "set_then_reset_stream": ("set_stream", "reset_stream")}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_paired_calls_on_one_context(pkg, scenes, pair):
    """The issue's pairs as it words them, on ONE context with two plugged streaks: the second call undoes the first
    behind a streak that ran under it -- reset_stream comes behind a streak on the second torch stream set_stream
    switched to.  (test_call_behind_a_streak_in_flight runs each half alone, on a context prepared for it.)"""
    scene = scenes("208x112")
    first, second = PAIRS[pair]
    c = Ctx(pkg, scene, KINDS[first][2])
    try:
        s = State.base(scene)
        _warm_up(c, s)
        s = plugged_step(c, s, 3, KINDS[first][1], (pair, first))
        plugged_step(c, s, 4, KINDS[second][1], (pair, second))
    finally:
        c.close()


MIXED = [bool(int(f)) for f in "1110111100111"]


@pytest.mark.parametrize("mode", [-1, 1])
@pytest.mark.parametrize("shape", ["96x64", "208x112"])
def test_mixed_prefilter_behind_a_plug(pkg, scenes, shape, mode):
    """Frames with and without the prefilter in one plugged run.  Automatic: a frame without it is serial and the count
    starts again; "overlap" = 1: every frame overlaps.  Every frame exact."""
    scene = scenes(shape)
    s = State.base(scene)
    poses = [scene.poses[k % len(scene.poses)] for k in range(len(MIXED))]
    want, streak = [], 0
    for f in MIXED:  # (rtr_overlap_policy.h: engaged from the third consecutive frame with the prefilter on)
        streak = streak + 1 if f else 0
        want.append(1 if mode == 1 or streak >= 3 else 0)
    c = Ctx(pkg, scene, {"overlap": mode})
    try:
        _warm_up(c, s)
        for f in (True, False):  # (both forms unplugged: the pyramid and the second set exist)
            c.run(scene.poses[:4], f)
            c.p.synchronize()
        active, event, snaps = c.run_plugged(poses, MIXED)
        assert active == want, active
        assert not event.query() and not c.first.query(), "the run had finished before the call under test: the case has tested nothing"
        c.p.synchronize()
        check(Ctx.frames(event, snaps), s, poses, MIXED, ("mixed", shape, mode))
        assert c.p.frame_stats()["errors"] == 0
    finally:
        c.close()


# ---- an overflowing frame inside the plugged streak ----------------------------------------------------------------
class _Big:
    """pool_overflow_scenes' cloud as a Scene for State and Ctx."""

    def __init__(self, pkg, orc):
        self.pkg, self.orc, self.W, self.H = pkg, orc, sc.W, sc.H
        self.xyzw, self.rgba = sc.cloud(orc)
        self.n = self.xyzw.shape[0]
        self.P_one = sc.p_one(orc)[0]
        self.poses = [pkg.orbit_projection(k, sc.W, sc.H) for k in sc.ORDINARY[:4]] + [pkg.orbit_projection(3, sc.W, sc.H)]


@pytest.fixture(scope="module")
def big(pkg, orc):
    return _Big(pkg, orc)


@pytest.mark.parametrize("call", ["remove_points", "set_point_keep"])
@pytest.mark.parametrize("before", [2, 3])
def test_pool_overflow_behind_a_plug(pkg, orc, big, before, call):
    """test_pool_overflow_inside_a_streak's scene: the frame that overflows the adaptive extent pool is the third or
    fourth of a plugged streak, and the call that meets it edits the cloud or sets a mask.  The repair replays the frame
    with the cloud and mask it was issued with -- the frame buffers hold the OLD state's frame after the call -- and the
    next streak shows the new state."""
    L = pkg._lib
    s = State.base(big)
    keep = np.arange(big.n) % 16 != 1  # (a sixteenth: under the head-room at which a removal reallocates the arrays)
    new = s.but("remove", xyzw=np.ascontiguousarray(s.xyzw[keep]), rgba=np.ascontiguousarray(s.rgba[keep])) \
        if call == "remove_points" else s.but("keep", keep=keep)
    c = Ctx(pkg, big, upload=False)
    try:
        sc.prepare(pkg, orc, c.p, big.xyzw, big.rgba, "late")
        c.resolution(sc.W, sc.H)
        ordinary = big.poses[:before]
        active, frames = c.run(ordinary + big.poses[before:before + 1], True)  # (the same shape with an ordinary last frame)
        assert active == AUTO[:before + 1]
        c.p.synchronize()
        start = sc.footprint(c.p) * big.n  # (millibytes, with the second tile store and pool of the overlapped frames)
        active, event, snaps = c.run_plugged(ordinary + [big.P_one], True)
        assert active == AUTO[:before + 1]
        assert not event.query() and not c.first.query(), "the streak had finished before the call under test: the case has tested nothing"
        if call == "remove_points":
            c.p.remove_points(keep)
        else:
            c.p.set_point_keep(keep)
        after = sc.footprint(c.p) * c.p.num_points
        # (pool_overflow_scenes.assert_overflowed in bytes -- a removal changes the point count, and the second store
        # is resident here: the pool of the set that took the repaired frame has grown to the worst case)
        assert after - start >= sc.JUMP_MB * big.n, ("the pool did not grow: no overflow", start, after)
        check(Ctx.frames(event, snaps)[:before], s, ordinary, True, ("overflow", "(a)"))
        for which, name in ((L.BUF_DEPTH, "depth"), (L.BUF_IMAGE, "img"), (L.BUF_TENSOR, "tensor"), (L.BUF_MINMAX, "minmax")):
            _same(c.p.download(which), s.ref(big.P_one)[name], ("the repaired frame", name))
        if call == "remove_points":
            assert c.p.num_points == new.n
        else:
            assert np.array_equal(c.p.point_keep(), keep)
        # (ordinary poses: a removal sizes the adaptive pool again, and nothing here would repair a second overflow)
        follow = [big.poses[0], big.poses[1], big.poses[4], big.poses[2]]
        active, frames = c.run(follow, True)
        assert active == AUTO[:4]
        check(frames, new, follow, True, ("overflow", "(c)"))
        assert c.p.frame_stats()["errors"] == 0
    finally:
        c.close()
