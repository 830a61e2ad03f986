"""Overlapped frames whose two events ride on dispatch packets (csrc/rtr_api.hip: consumed_in_dispatch, bin_points): the
tile launch -- the split launch where the frame has one -- signals the store's `consumed` event and an unbracketed T1
signals `binned`, instead of an event packet of their own behind the launch.  What must not change is the order the
events stand for: T1 of frame k + 2 must not write a store before the tile launch of frame k has read it, and the tile
launch of frame k must not read before T1 of frame k has ended.

Reference: a second context with option "overlap" = 0 renders the same pose list, and depth, image and tensor of every
frame are compared bit for bit.  Three passes per case:
  cold    a streak on the fresh context, the frame buffers cloned on its stream between the renders (no library call in
          between): the first eight frames of a cloud keep the split launch, so `consumed` rides on k_tile_split
  serial  both contexts render pose by pose and download after each frame (a download drains: no streak survives)
  warm    the streak again (lean frames now, both stores, both parities), every clone compared, then ONE download of the
          last frame.

Shapes: a 300 000-point room_shell at 256x160 (8x10 tiles of 32x16) with four pyramid levels, and 250x150 for a ragged
last tile column and row -- the prefilter needs W % 2^levels == 0, so that shape runs it with levels = 1 (the unfused
prefilter behind the tile launch).
Poses: the room seen from outside, alternately in the left upper and the right lower two thirds of the frame (a dozen of
the 80 tiles in common; the right lower view reaches the last tile column and row), every pose shifted by another pixel:
a store read after it was overwritten, or before T1 had finished, gives the other view's tiles, and a stale frame gives
a shifted one.  `_serial` asserts that neighbouring frames differ.  The heaviest tile holds 19 000 entries, below the
default split threshold, so warm frames are lean."""
import numpy as np
import pytest

from streak_ctx import AUTO, Ctx

pytestmark = pytest.mark.gpu

N_POINTS = 300_000
N_FRAMES = 12


class World:
    """What streak_ctx.Ctx needs of a scene (a cloud and a frame size) and the two-view pose list."""

    def __init__(self, pkg, orc, W, H):
        self.W, self.H = W, H
        self.xyzw, self.rgba = orc.generate("room_shell", 0xC0FFEE17, 0, N_POINTS, N_POINTS)
        self.extra = orc.generate("room_shell", 0xC0FFEE18, 0, 20_000, 20_000)
        E = np.eye(4)
        E[2, 3] = 14.0  # (the room is x, z in [-4, 4], y in [-1.5, 1.5]: its front face is 10 m away)
        self.poses = []
        for k in range(N_FRAMES):
            left = k % 2 == 0
            K = [[0.8 * W, 0, (0.32 if left else 0.68) * W + k // 2], [0, 2.2 * H, (0.34 if left else 0.66) * H - k // 2], [0, 0, 1]]
            self.poses.append(pkg.compose_projection(K, E))


@pytest.fixture(scope="module")
def worlds(pkg, orc):
    cache = {}

    def get(W=256, H=160):
        if (W, H) not in cache:
            cache[(W, H)] = World(pkg, orc, W, H)
        return cache[(W, H)]
    return get


def _grab(c, filtered):
    L = c.pkg._lib
    f = {"depth": c.p.download(L.BUF_DEPTH), "img": c.p.download(L.BUF_IMAGE)}
    if filtered:
        f["tensor"] = c.p.download(L.BUF_TENSOR)
    return f


def _streak(c, poses, flags):
    """Renders back to back, cloning the frame buffers on the context's stream -> overlap_active per frame, the frames."""
    active, snaps = [], []
    for P, f in zip(poses, flags):
        c.p.render(P, bool(f))
        active.append(c.p.get_option("overlap_active"))
        with c.torch.cuda.stream(c.st):
            snaps.append({k: c.bufs[k].clone() for k in (("depth", "img", "tensor") if f else ("depth", "img"))})
    c.st.synchronize()
    return active, [{k: v.cpu().numpy() for k, v in s.items()} for s in snaps]


def _same(got, want, what):
    for name, g in got.items():
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(want[name])
        assert g.nbytes == w.nbytes, (what, name, g.shape, w.shape)
        diff = g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8)
        assert not diff.any(), (what, name, int(diff.sum()), "bytes differ")


def _serial(a, b, poses, flags, what):
    """Both contexts pose by pose, a download after every frame -> the serial context's frames."""
    ref = []
    for k, (P, f) in enumerate(zip(poses, flags)):
        a.p.render(P, bool(f))
        b.p.render(P, bool(f))
        ref.append(_grab(b, f))
        _same(_grab(a, f), ref[-1], (what, "serial pass", k))
    for k in range(1, len(ref)):  # (the poses must tell the frames apart)
        assert not np.array_equal(ref[k]["depth"], ref[k - 1]["depth"]) and not np.array_equal(ref[k]["img"], ref[k - 1]["img"]), k
    return ref


def _three_passes(a, b, poses, flags, want_active, what):
    cold_active, cold = _streak(a, poses, flags)
    assert cold_active == want_active, (what, "cold", cold_active)
    ref = _serial(a, b, poses, flags, what)
    for k, f in enumerate(cold):
        _same(f, ref[k], (what, "cold streak", k))
    for rep in range(2):  # (twice: the second streak starts on the store the first one ended on or on the other one)
        active, warm = _streak(a, poses, flags)
        assert active == want_active, (what, "warm", rep, active)
        for k, f in enumerate(warm):
            _same(f, ref[k], (what, "warm streak", rep, k))
        _same(_grab(a, flags[-1]), ref[-1], (what, "last frame downloaded", rep))
    return ref


def _pair(pkg, world, options, levels=4):
    a = Ctx(pkg, world, options)
    try:
        b = Ctx(pkg, world, dict(options, overlap=0))
    except BaseException:
        a.close()
        raise
    if levels != 4:
        a.p.set_params(levels=levels)
        b.p.set_params(levels=levels)
    return a, b


ALL = [1] * N_FRAMES


@pytest.mark.parametrize("overlap", [1, -1])
def test_filtered_streak_equals_serial(pkg, worlds, overlap):
    w = worlds()
    a, b = _pair(pkg, w, {"overlap": overlap})
    try:
        want = [1] * N_FRAMES if overlap == 1 else (AUTO + [1] * N_FRAMES)[:N_FRAMES]
        _three_passes(a, b, w.poses, ALL, want, ("overlap", overlap))
        st = a.p.frame_stats()
        assert st["errors"] == 0 and st["split_tiles"] == 0, st  # (the warm streaks were lean frames)
        assert a.p.get_option("lean") == 1
    finally:
        a.close()
        b.close()


def test_ragged_last_tile(pkg, worlds):
    """250x150: the last tile column holds 26 of 32 pixels and the last row 6 of 16; one pyramid level, so the prefilter
    is a launch of its own behind the tile launch that carries `consumed`."""
    w = worlds(250, 150)
    a, b = _pair(pkg, w, {"overlap": 1}, levels=1)
    try:
        _three_passes(a, b, w.poses, ALL, [1] * N_FRAMES, "250x150")
        assert a.p.frame_stats()["errors"] == 0
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_timing_modes_mix_bracketed_and_plain_t1(pkg, worlds, mode):
    """Modes 1 and 2 bracket every T1 (the bracket owns the dispatch's stop event: `binned` is recorded), 3 every fourth
    and 4 every second (recorded and dispatch-borne `binned` in one streak), 0 none."""
    w = worlds()
    a, b = _pair(pkg, w, {"overlap": 1})
    try:
        a.p.timing_enable(mode)
        _three_passes(a, b, w.poses, ALL, [1] * N_FRAMES, ("timing", mode))
        t = a.p.timing()
        launches = t["min_depth"][1]
        # 12 cold + 12 serial + 2 x 12 warm frames = 48 T1 launches since timing_enable
        assert launches == {0: 0, 1: 48, 2: 48, 3: 12, 4: 24}[mode], (mode, t)
        assert a.p.frame_stats()["errors"] == 0
    finally:
        a.close()
        b.close()


def test_split_launch_carries_consumed(pkg, worlds):
    """Tiles above 64 entries are split: every frame has the split launch, the store's last reader."""
    w = worlds()
    a, b = _pair(pkg, w, {"overlap": 1, "split_threshold": 64, "split_slice": 48})
    try:
        _three_passes(a, b, w.poses, ALL, [1] * N_FRAMES, "split")
        st = a.p.frame_stats()
        assert st["errors"] == 0 and st["split_tiles"] > 0 and st["split_items"] > 0, st
    finally:
        a.close()
        b.close()


def test_frame_without_prefilter_inside_a_streak(pkg, worlds):
    w = worlds()
    a, b = _pair(pkg, w, {"overlap": 1})
    try:
        flags = [1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1]
        _three_passes(a, b, w.poses, flags, [1] * N_FRAMES, "unfiltered frames")
        assert a.p.frame_stats()["errors"] == 0
    finally:
        a.close()
        b.close()


def test_streak_ended_and_reengaged(pkg, worlds):
    """frame_stats drains; set_clip_planes changes host state only.  Both end the streak, and the automatic mode engages
    again at the third frame behind each."""
    w = worlds()
    planes = np.float32([[0.3, -0.2, 0.9, 0.35]])
    a, b = _pair(pkg, w, {"overlap": -1})
    try:
        b.p.render(w.poses[-1], True)
        unclipped = _grab(b, True)
        ref = []
        for k, P in enumerate(w.poses):
            if k == 9:
                b.p.set_clip_planes(planes)
            b.p.render(P, True)
            ref.append(_grab(b, True))
        assert not np.array_equal(ref[-1]["depth"], unclipped["depth"])  # (the plane cuts the room)
        for run in range(2):  # (the first run's frames keep the split launch, the second's are lean)
            a.p.set_clip_planes(None)
            active, f0 = _streak(a, w.poses[:5], [1] * 5)
            assert active == AUTO[:5]
            assert a.p.frame_stats()["errors"] == 0
            assert a.p.get_option("overlap_active") == 0
            active, f1 = _streak(a, w.poses[5:9], [1] * 4)
            assert active == AUTO[:4]
            a.p.set_clip_planes(planes)
            assert a.p.get_option("overlap_active") == 0
            active, f2 = _streak(a, w.poses[9:], [1] * 3)
            assert active == AUTO[:3]
            for k, f in enumerate(f0 + f1 + f2):
                _same(f, ref[k], ("re-engaged", run, k))
            _same(_grab(a, True), ref[-1], ("re-engaged", run, "last"))
    finally:
        a.close()
        b.close()


def test_point_pass_and_project_async_behind_a_streak(pkg, worlds):
    """Both are queued behind frames whose events rode on dispatches: the point pass reads the store and the frame, the
    asynchronous frame renders once more and copies out."""
    w = worlds()
    L = pkg._lib
    a, b = _pair(pkg, w, {"overlap": 1, "point_ids": 1})
    try:
        for run in range(2):
            b.p.render(w.poses[10], True)
            b.p.point_pass(w.poses[10])
            want_ids, want_vis = b.p.download(L.BUF_POINT_ID), b.p.download(L.BUF_VISIBLE)
            active, _ = _streak(a, w.poses[:11], [1] * 11)
            assert active == [1] * 11
            a.p.point_pass(w.poses[10])
            assert np.array_equal(a.p.download(L.BUF_POINT_ID), want_ids), run
            assert np.array_equal(a.p.download(L.BUF_VISIBLE), want_vis), run
            assert (want_ids != L.NO_POINT).sum() > 1000 and want_vis.any()

            b.p.project_async(w.poses[7], 0, True)
            b.p.wait_outputs(0)
            want_img, want_depth = (x.copy() for x in b.p.host_output_buffers(0))
            active, _ = _streak(a, w.poses[:7], [1] * 7)
            assert active == [1] * 7
            a.p.project_async(w.poses[7], 0, True)
            a.p.wait_outputs(0)
            img, depth = a.p.host_output_buffers(0)
            assert np.array_equal(img, want_img) and np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)), run
            _same(_grab(a, True), _grab(b, True), ("project_async", run))
        assert a.p.frame_stats()["errors"] == 0
    finally:
        a.close()
        b.close()


def test_first_frames_after_set_resolution_and_append(pkg, worlds):
    """Both reallocate the tile stores: the streak behind them starts on fresh stores whose `consumed` events must not
    stand for launches over the old ones."""
    w = worlds()
    a, b = _pair(pkg, w, {"overlap": 1})
    try:
        ref = _three_passes(a, b, w.poses, ALL, [1] * N_FRAMES, "before")
        a.resolution(128, 96)
        a.p.render(pkg.orbit_projection(3, 128, 96), True)  # (a frame at the other size, still queued)
        a.resolution(w.W, w.H)
        active, frames = _streak(a, w.poses, ALL)
        assert active == [1] * N_FRAMES
        for k, f in enumerate(frames):
            _same(f, ref[k], ("after set_resolution", k))
        for c in (a, b):  # (behind a streak still in flight on a)
            c.p.append_points(*w.extra)
        active, frames = _streak(a, w.poses, ALL)
        assert active == [1] * N_FRAMES
        ref2 = _serial(a, b, w.poses, ALL, "appended")
        assert not np.array_equal(ref2[0]["depth"], ref[0]["depth"])
        for k, f in enumerate(frames):
            _same(f, ref2[k], ("after append_points", k))
        assert a.p.frame_stats()["errors"] == 0
    finally:
        a.close()
        b.close()
