"""Option "overlap" in its automatic mode (include/rtr.h; csrc/rtr_overlap_policy.h): from the third consecutive
rtr_render with the prefilter of a context on, the point kernel of frame k + 1 runs on a second stream and into a second
tile store beside the tail of frame k, and overlapped frames are lean frames like serial ones, with the lean parity kept
per store.  Frames without the prefilter stay serial in the automatic mode (they lose by overlapping) and overlap with
an explicit 1.

Every frame of every run is compared bit for bit with the oracle: depth, image and, with the prefilter, the fp16 tensor
and the min / max words.  A frame in the middle of a streak cannot be downloaded without ending the streak, so the
context renders on a torch stream and the frame buffers are cloned on that stream between the renders (no library
call in between: `overlap_active` is read through rtr_get_option, which leaves the streak alone).

Small shapes on purpose: 50 k - 300 k point rooms at 96x64 (3x2 tiles), 200x120 and 208x112 (no multiples of 32; the
prefilter needs a multiple of 16, so only the second has it) and 640x480;
runs of 9 frames with distinct orbit poses, twice -- a fresh cloud's first eight frames keep the split launch and so are
not lean, the second run's are, and each store's parity turns over twice in it."""
import numpy as np
import pytest

import pool_overflow_scenes as sc
from streak_ctx import AUTO, SHAPES, Ctx, Scene, _exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(pkg, orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Scene(pkg, orc, name)
        return cache[name]
    return get


def _cases():
    return [(s, f) for s in SHAPES for f in (False, True) if f <= SHAPES[s][3]]


@pytest.mark.parametrize("shape,filtered", _cases())
def test_default_context_engages_at_the_third_frame(pkg, scenes, shape, filtered):
    """With the prefilter: 0, 0, 1, 1, ...; without it the automatic mode never engages."""
    sc_ = scenes(shape)
    c = Ctx(pkg, sc_)
    try:
        assert c.p.get_option("overlap") == -1 and c.p.get_option("overlap_active") == 0
        for run in range(2):  # (the first run: split launch on, not lean; the second: lean frames)
            active, frames = c.run(sc_.poses, filtered)
            assert active == (AUTO if filtered else [0] * len(AUTO)), (run, active)
            _exact(frames, sc_, sc_.poses, filtered, (shape, filtered, run))
            assert c.p.frame_stats()["errors"] == 0
            assert c.p.get_option("overlap_active") == 0  # (the statistics call ended the streak)
    finally:
        c.close()


@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("shape,filtered", _cases())
def test_explicit_settings_override(pkg, scenes, shape, filtered, value):
    sc_ = scenes(shape)
    c = Ctx(pkg, sc_, {"overlap": value})
    try:
        for run in range(2):
            active, frames = c.run(sc_.poses, filtered)
            assert active == [value] * len(sc_.poses), (run, active)
            _exact(frames, sc_, sc_.poses, filtered, (shape, filtered, value, run))
            c.p.synchronize()
        # ... and switching inside a context: 1 -> auto -> 0 -> auto
        auto = AUTO[:4] if filtered else [0] * 4  # (without the prefilter the automatic mode stays serial)
        for value2, want in ((-1, auto), (0, [0] * 4), (-1, auto), (1, [1] * 4)):
            c.p.set_option("overlap", value2)
            active, frames = c.run(sc_.poses[:4], filtered)
            assert active == want, (value2, active)
            _exact(frames, sc_, sc_.poses[:4], filtered, (shape, filtered, value, "then", value2))
    finally:
        c.close()


@pytest.mark.parametrize("shape", ["96x64", "640x480"])
def test_frame_stats_of_an_overlapped_lean_frame(pkg, scenes, shape):
    """The statistics of the LAST frame, whichever store it went to: equal to the serial context's for every length of
    streak from 3 to 6 (both stores, both parities).  The poses' entry counts differ, so a fold of the wrong store or
    parity shows."""
    sc_ = scenes(shape)
    serial, auto = Ctx(pkg, sc_, {"overlap": 0}), Ctx(pkg, sc_)
    try:
        for c in (serial, auto):  # (past the split launch's grace period: lean frames from here on)
            c.run(sc_.poses, True)
            c.p.synchronize()
        want = []
        for P in sc_.poses:
            serial.p.render(P, True)
            st = serial.p.frame_stats()
            want.append((st["entries"], st["colour_chunks"], st["errors"]))
        assert len({w[0] for w in want}) == len(want), ("the poses must differ in their entry counts", want)
        for m in (3, 4, 5, 6, 9):
            active, _ = auto.run(sc_.poses[:m], True)
            assert active == AUTO[:m]
            st = auto.p.frame_stats()
            assert (st["entries"], st["colour_chunks"], st["errors"]) == want[m - 1], (m, st, want[m - 1])
    finally:
        serial.close()
        auto.close()


@pytest.mark.parametrize("kind", ["frame_stats", "point_pass", "clip", "append", "resolution", "download", "views"])
def test_streak_interrupted_and_rearmed(pkg, orc, scenes, kind):
    """Frames 1-4, another call, frames 5-7, another call, frames 8-9: every frame exact, and the streak counts from one
    again behind each interruption.  Run twice (the second time with lean frames)."""
    sc_ = scenes("640x480")
    W, H = sc_.W, sc_.H
    extra = orc.generate("room_shell", 0xC0FFEE11, 0, 40_000, 40_000)
    planes = np.float32([[0.3, -0.2, 0.9, 0.35]])
    c = Ctx(pkg, sc_, {"point_ids": 1} if kind == "point_pass" else {})  # (IDs of a sorted cloud need its permutation)
    try:
        cloud, tag = (sc_.xyzw, sc_.rgba), "base"
        for run in range(2):
            parts = ((0, 4), (4, 7), (7, 9))
            for i, (a, b) in enumerate(parts):
                poses = sc_.poses[a:b]
                active, frames = c.run(poses, True)
                assert active == AUTO[: b - a], (kind, run, i, active)
                shown = cloud
                if kind == "clip" and i == 1:  # (the middle part is rendered through the plane)
                    keep = pkg.clip_keep(planes, cloud[0])
                    shown, tag_ = (cloud[0][keep], cloud[1][keep]), tag + "+clip"
                else:
                    tag_ = tag
                _exact(frames, sc_, poses, True, (kind, run, i), shown, tag_)
                if i == 2:
                    break
                if kind == "frame_stats":
                    assert c.p.frame_stats()["errors"] == 0
                elif kind == "point_pass":
                    c.p.point_pass(poses[-1])
                elif kind == "clip":
                    c.p.set_clip_planes(planes if i == 0 else None)
                elif kind == "append":
                    lo = (2 * run + i) * 10_000
                    c.p.append_points(extra[0][lo:lo + 10_000], extra[1][lo:lo + 10_000])
                    cloud = (np.concatenate([cloud[0], extra[0][lo:lo + 10_000]]), np.concatenate([cloud[1], extra[1][lo:lo + 10_000]]))
                    tag = "base+%d" % (lo + 10_000)
                elif kind == "resolution":
                    c.resolution(320, 240)
                    c.resolution(W, H)
                elif kind == "download":
                    got = c.p.download(pkg._lib.BUF_DEPTH)
                    assert np.array_equal(got, sc_.ref(poses[-1], True, shown, tag_)["depth"])
                else:
                    c.p.render_views(np.stack(sc_.poses[:2]), True)
                assert c.p.get_option("overlap_active") == 0
            c.p.synchronize()
    finally:
        c.close()


def test_split_tiles_inside_a_streak(pkg, scenes):
    """Tiles above "split_threshold": the split launch and the reset of the split tiles' pixels (on the tail's stream)
    run inside the streak, and those frames are not lean.  Then the threshold goes back up inside the same context:
    the lean frames that follow fold their statistics into stores whose last frames had an epilogue."""
    sc_ = scenes("96x64")
    c = Ctx(pkg, sc_, {"split_threshold": 64, "split_slice": 48})
    try:
        for run in range(2):
            active, frames = c.run(sc_.poses, True)
            assert active == AUTO, active
            _exact(frames, sc_, sc_.poses, True, ("split", run))
            st = c.p.frame_stats()
            assert st["errors"] == 0 and st["split_tiles"] > 0, st
        c.p.set_option("split_threshold", 32768)
        c.p.set_option("split_slice", 16384)
        for run in range(3):  # (eight more frames keep the split launch, then lean ones)
            active, frames = c.run(sc_.poses, True)
            assert active == AUTO, active
            _exact(frames, sc_, sc_.poses, True, ("unsplit", run))
            c.p.synchronize()  # (ends the streak)
        st = c.p.frame_stats()
        assert st["errors"] == 0 and st["split_tiles"] == 0, st
    finally:
        c.close()


@pytest.fixture(scope="module")
def overflow_world(pkg, orc):
    xyzw, rgba = sc.cloud(orc)
    P = sc.p_one(orc)[0]
    r = orc.project(xyzw, rgba, P, sc.W, sc.H)
    f = orc.filter(r["depth_bits"], r["img"])
    P2 = pkg.orbit_projection(3, sc.W, sc.H)
    r2 = orc.project(xyzw, rgba, P2, sc.W, sc.H)
    f2 = orc.filter(r2["depth_bits"], r2["img"])
    return xyzw, rgba, P, f, P2, f2


@pytest.mark.parametrize("before", [2, 3])
def test_pool_overflow_inside_a_streak(pkg, orc, overflow_world, before):
    """The frame that overflows the adaptive extent pool is the third or fourth of a streak -- it runs overlapped, into
    either store.  The synchronising call repairs THAT frame; the frames behind it are exact."""
    xyzw, rgba, P, rf, P2, r2 = overflow_world
    L = pkg._lib
    p = pkg.Projector(0)
    try:
        start = sc.prepare(pkg, orc, p, xyzw, rgba, "late")
        for k in sc.ORDINARY[:before]:
            p.render(pkg.orbit_projection(k, sc.W, sc.H), True)
        assert p.get_option("overlap_active") == (1 if before >= 3 else 0)
        p.render(P, True)
        assert p.get_option("overlap_active") == 1
        p.synchronize()
        sc.assert_overflowed(p, start, before)
        assert np.array_equal(p.download(L.BUF_DEPTH), rf["depth"].view(np.uint32))
        assert np.array_equal(p.download(L.BUF_IMAGE), rf["img"])
        assert np.array_equal(p.download(L.BUF_TENSOR).reshape(5, sc.H, sc.W), rf["tensor"])
        sc.no_errors(p)
        for k in range(4):  # a streak behind the repair
            p.render(P, True)
        p.render(P2, True)
        assert p.get_option("overlap_active") == 1
        assert np.array_equal(p.download(L.BUF_DEPTH), r2["depth"].view(np.uint32))
        assert np.array_equal(p.download(L.BUF_IMAGE), r2["img"])
        assert np.array_equal(p.download(L.BUF_TENSOR).reshape(5, sc.H, sc.W), r2["tensor"])
        sc.no_errors(p)
    finally:
        p.close()


def test_p2p_open_on_a_default_context(pkg, scenes):
    """The exchange opens under the default (only an explicit 1 is refused); the automatic mode is inactive while it
    is open -- the peers map ONE tile store -- and comes back when it is closed."""
    sc_ = scenes("640x480")
    c = Ctx(pkg, sc_)
    try:
        active, frames = c.run(sc_.poses[:4], True)
        assert active == AUTO[:4]
        c.p.p2p_open(0, 1, [c.p.p2p_export()])
        assert c.p.get_option("p2p_open") == 1 and c.p.get_option("overlap") == -1
        with pytest.raises(pkg.RtrError):
            c.p.set_option("overlap", 1)
        active, frames = c.run(sc_.poses[:5], True)
        assert active == [0] * 5, active
        _exact(frames, sc_, sc_.poses[:5], True, "open")
        c.p.p2p_render(sc_.poses[5], False)
        c.p.synchronize()
        assert np.array_equal(c.p.download(pkg._lib.BUF_DEPTH), sc_.ref(sc_.poses[5], False)["depth"])
        c.p.p2p_close()
        active, frames = c.run(sc_.poses[:5], True)
        assert active == AUTO[:5], active
        _exact(frames, sc_, sc_.poses[:5], True, "closed")
    finally:
        c.close()


def test_two_default_contexts_alternate(pkg, scenes):
    """Two contexts with streaks of their own, rendering in turn: both engage, both stay exact."""
    import torch
    a_s, b_s = scenes("640x480"), scenes("96x64")
    a, b = Ctx(pkg, a_s), Ctx(pkg, b_s)
    try:
        for run in range(2):
            act = {a: [], b: []}
            snaps = {a: [], b: []}
            for k in range(9):
                for c, s in ((a, a_s), (b, b_s)):
                    c.p.render(s.poses[k], True)
                    act[c].append(c.p.get_option("overlap_active"))
                    with torch.cuda.stream(c.st):
                        snaps[c].append({n: c.bufs[n].clone() for n in ("depth", "img", "tensor", "minmax")})
            for c, s in ((a, a_s), (b, b_s)):
                c.st.synchronize()
                assert act[c] == AUTO, act[c]
                frames = []
                for sn in snaps[c]:
                    f = {n: v.cpu().numpy() for n, v in sn.items()}
                    f["depth"], f["minmax"] = f["depth"].view(np.uint32), f["minmax"].view(np.uint32)
                    f["tensor"] = f["tensor"].view(np.uint16).reshape(5, s.H, s.W)
                    frames.append(f)
                _exact(frames, s, s.poses, True, ("two contexts", run))
                c.p.synchronize()
    finally:
        a.close()
        b.close()
