"""-m gpu: the tile store's 24-bit frame stamp through its wrap (csrc/rtr_stamp_rule.h, next_seq() in rtr_api.hip).

A context reaches the wrap after 2^24 frames into one store; option "debug_store_stamp" (a test aid, include/rtr.h)
puts a store a few frames short of it.  Every case renders through the wrap and at least four frames beyond it, compares
EVERY frame with the oracle bit for bit -- depth, image and, where filtered, the five tensor planes, mask and min / max
-- and asserts from read-backs that the wrap took place (the stamp read through rtr_get_option drops from 0xFFFFFF to 1
and is never 0) and that dynamic extents were in use after it (frame_stats against the oracle's own counts per tile:
tests/stamp_wrap_scenes.py, pinned without a GPU by test_stamp_wrap_host.py).  Alternating poses load different tiles in
consecutive frames, so a directory word that survived the wrap, or was cleared too late, shows as a wrong frame.

The sharded cases (a store the peers have mapped) are in test_gpu_p2p.py."""
import numpy as np
import pytest

import point_pass_ref as ppr
import pool_overflow_scenes as po
import stamp_wrap_scenes as sw
from streak_ctx import Ctx, _exact

pytestmark = pytest.mark.gpu

W, H = sw.W, sw.H
TOP = sw.STAMP_MAX
NPOSES = len(sw.POSE_SPECS)


class World:
    """The cloud, its poses, the oracle's frames and counts: computed once per module, never changed.  (`ref` has the
    signature of streak_ctx.Scene.ref, `cloud` included: streak_ctx._exact calls it with all four arguments.)"""

    def __init__(self, pkg, orc):
        self.pkg, self.orc = pkg, orc
        self.W, self.H, self.n, self.can_filter = W, H, sw.N, True
        self.xyzw, self.rgba = sw.cloud(orc)
        self.poses = [sw.pose(orc, i) for i in range(NPOSES)]
        self.edit = sw.edited_cloud(orc)
        self._refs, self._counts = {}, {}

    def _cloud(self, tag):
        return (self.xyzw, self.rgba) if tag == "base" else self.edit[2]

    def ref(self, P, filtered, cloud=None, tag="base"):
        key = (np.asarray(P, np.float32).tobytes(), bool(filtered), tag)
        if key not in self._refs:
            xyzw, rgba = cloud if cloud is not None else self._cloud(tag)
            r = self.orc.project(xyzw, rgba, P, W, H)
            out = {"depth": r["depth_bits"], "img": r["img"]}
            if filtered:
                f = self.orc.filter(r["depth_bits"], r["img"])
                out = {"depth": f["depth"].view(np.uint32), "img": f["img"], "tensor": f["tensor"], "minmax": f["minmax"],
                       "mask": f["mask"]}
            self._refs[key] = out
        return self._refs[key]

    def counts(self, i, tag="base"):
        if (i, tag) not in self._counts:
            c = sw.tile_counts(self.orc, *self._cloud(tag), self.poses[i])
            assert sw.uses_dynamic_extents(c), (i, tag, c)
            self._counts[(i, tag)] = c
        return self._counts[(i, tag)]


@pytest.fixture(scope="module")
def world(pkg, orc):
    return World(pkg, orc)


def _context(pkg, world, options=(), point_ids=True):
    p = pkg.Projector(0)
    try:
        for k, v in dict(options).items():
            p.set_option(k, v)
        p.upload_points(world.xyzw, world.rgba, point_ids=point_ids)  # (uniform_box is sorted by the library)
        p.set_resolution(W, H)
    except BaseException:
        p.close()
        raise
    return p


def _same_frame(pkg, p, want, filtered, what):
    """The frame in the context's buffers ≡ the oracle's."""
    L = pkg._lib
    got = {"depth": p.download(L.BUF_DEPTH), "img": p.download(L.BUF_IMAGE)}
    if filtered:
        got.update(tensor=p.download(L.BUF_TENSOR).reshape(5, H, W), mask=p.download(L.BUF_MASK), minmax=p.download(L.BUF_MINMAX))
    for name, g in got.items():
        w = np.asarray(want[name])
        assert g.shape == w.shape and np.array_equal(g, w.view(g.dtype)), (what, name, int((g != w.view(g.dtype)).sum()))


def _dynamic_extents_in_use(p, counts, what):
    """The frame just rendered held what the oracle counts: more than 8192 entries in at least two storage tiles."""
    st = p.frame_stats()
    assert st["errors"] == 0, (what, st)
    assert st["entries"] == int(counts.sum()) and st["heaviest_tile"] == sw.heaviest_tile(counts), (what, st, counts)
    assert sw.uses_dynamic_extents(counts) and st["heaviest_tile"] > sw.DYN2


def _stamp(p):
    return p.get_option("debug_store_stamp")


# ---- serial single frames --------------------------------------------------------------------------------------------

CONFIGS = {
    "tile": {},
    "tile-lean0": {"lean": 0},
    "tile-split": {"split_threshold": 64, "split_slice": 48},  # (split tiles are live at the wrap)
    "tile-packed": {"pack": 2},
    "two-pass": {"mode": 0},                                    # (no store: the option must be harmless)
}


@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "filtered"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_serial_frames_through_the_wrap(pkg, orc, world, config, filtered):
    """Three frames up to 0xFFFFFF, the frame that wraps, five beyond; the point pass behind the first frame after the
    wrap.  Unfiltered cases set the stamp into a store that has rendered frames with stamps 1 and 2 -- their directory
    words are what the clear at the wrap must remove --, filtered ones before the store exists."""
    binned = config != "two-pass"
    p = _context(pkg, world, CONFIGS[config])
    try:
        k = 0
        if not filtered:
            for k in (0, 1):
                p.render(world.poses[k], filtered)
                _same_frame(pkg, p, world.ref(world.poses[k], filtered), filtered, (config, "warm-up", k))
            assert _stamp(p) == (2 if binned else 0)
            k = 3  # (the frames that take stamps 1 and 2 again see other poses than the warm-up's: its words are stale)
        p.set_option("debug_store_stamp", TOP - 3)
        assert _stamp(p) == TOP - 3
        seen = []
        for j in range(9):
            i = (k + j) % NPOSES
            P = world.poses[i]
            p.render(P, filtered)
            seen.append(_stamp(p))
            _same_frame(pkg, p, world.ref(P, filtered), filtered, (config, "frame", j, seen))
            if binned and j >= 3:
                _dynamic_extents_in_use(p, world.counts(i), (config, j))
                if config == "tile-split":
                    assert p.frame_stats()["split_tiles"] >= 2
            if j == 3:  # the first frame after the wrap: per-pixel point IDs and per-point visibility behind it
                p.point_pass(P)
                ids, vis = p.download(pkg._lib.BUF_POINT_ID), p.download(pkg._lib.BUF_VISIBLE)
                e_ids, e_vis = ppr.point_pass(orc, world.xyzw, P, W, H, world.ref(P, filtered)["depth"])
                assert np.array_equal(ids, e_ids) and np.array_equal(vis, e_vis), (config, "point pass")
                assert _stamp(p) == seen[-1]  # (it renders nothing)
        want = [TOP - 2, TOP - 1, TOP, 1, 2, 3, 4, 5, 6] if binned else [TOP - 3] * 9
        assert seen == want, (config, seen)
    finally:
        p.close()


# ---- an overlapped streak --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [-1, 1])
def test_both_stores_wrap_inside_an_overlapped_streak(pkg, world, overlap):
    """One streak of 18 filtered frames, cloned on the context's stream between the renders and compared after ONE
    synchronisation.  Each of the single frame's two stores sees every second frame, so they wrap on different frames;
    the clear of a store's directory runs on the front stream, behind the tail that last read that store and beside the
    tail of the other one.  The option call ends a streak, so the stamp is set before this one begins -- after a warm-up
    streak, so that both stores exist and take it."""
    c = Ctx(pkg, world, {"overlap": overlap})
    try:
        warm = [world.poses[j % NPOSES] for j in range(5)]
        active, frames = c.run(warm, True)
        assert active[-1] == 1
        _exact(frames, world, warm, True, ("warm-up", overlap))
        c.p.set_option("debug_store_stamp", TOP - 4)  # both stores: four more frames each, the fifth wraps
        assert c.p.get_option("overlap_active") == 0
        order = [(3 * j) % NPOSES for j in range(18)]  # (neither consecutive frames nor a store's consecutive frames repeat a pose)
        poses = [world.poses[i] for i in order]
        act, seen, snaps = [], [], []
        for P in poses:
            c.p.render(P, True)
            act.append(c.p.get_option("overlap_active"))
            seen.append(_stamp(c.p))  # (rtr_get_option leaves the streak alone: the stamp of the store this frame took)
            with c.torch.cuda.stream(c.st):
                snaps.append({k: c.bufs[k].clone() for k in ("depth", "img", "tensor", "minmax")})
        ev = c.torch.cuda.Event()
        ev.record(c.st)
        _exact(Ctx.frames(ev, snaps), world, poses, True, ("streak", overlap, seen))
        assert 0 not in seen and all(1 <= s <= TOP for s in seen), seen
        wraps = [j for j, s in enumerate(seen) if s == 1]
        tops = [j for j, s in enumerate(seen) if s == TOP]
        assert len(wraps) == 2 and wraps[1] > wraps[0], (seen, wraps)      # each store wrapped, on its own frame
        assert len(tops) == 2 and tops[0] < wraps[0] and tops[1] < wraps[1], (seen, tops, wraps)  # ... each from 0xFFFFFF
        assert act[wraps[0] - 1] == 1 and all(a == 1 for a in act[wraps[0] - 1:]), (act, wraps)  # the streak was active throughout
        assert len(seen) - wraps[1] >= 5 and act[-1] == 1
        # the last frame's store, read back: dynamic extents in use after both wraps
        _dynamic_extents_in_use(c.p, world.counts(order[-1]), ("streak", overlap))
    finally:
        c.close()


# ---- view batches ----------------------------------------------------------------------------------------------------

def _same_views(pkg, p, world, idx, what):
    L = pkg._lib
    depth, img = p.download(L.BUF_VIEW_DEPTH), p.download(L.BUF_VIEW_IMAGE)
    tensor, minmax = p.download(L.BUF_VIEW_TENSOR), p.download(L.BUF_VIEW_MINMAX)
    for v, i in enumerate(idx):
        want = world.ref(world.poses[i], True)
        assert np.array_equal(depth[v], want["depth"]), (what, "view", v, "depth")
        assert np.array_equal(img[v], want["img"]), (what, "view", v, "img")
        assert np.array_equal(tensor[v], np.asarray(want["tensor"]).view(np.uint16)), (what, "view", v, "tensor")
        assert np.array_equal(minmax[v], want["minmax"]), (what, "view", v, "minmax")
        assert sw.uses_dynamic_extents(world.counts(i))  # (every view's store: the oracle's counts for its pose)


@pytest.mark.parametrize("when", ["first-use", "after-a-batch"])
def test_view_batches_through_the_wrap(pkg, world, when):
    """Batches of three filtered views, one single frame after each batch.  The views' stores take one stamp per batch,
    the single frame's store one per frame, and the option gives all of them the same stamp, so they wrap in the same
    round: the single frame's stamp is read back directly, the views' stores through the option's forward-only rule
    (a value is accepted only if NO store of the context is ahead of it).
    first-use: the stamp is set before the views' stores exist; after-a-batch: into stores that have rendered one."""
    p = _context(pkg, world)
    try:
        def round_(b, what):
            idx = [(b + v) % NPOSES for v in range(3)]
            p.render_views([world.poses[i] for i in idx], True)
            _same_views(pkg, p, world, idx, (when, what, b))
            i = (b + 3) % NPOSES
            p.render(world.poses[i], True)
            _same_frame(pkg, p, world.ref(world.poses[i], True), True, (when, what, b, "single frame"))
            return i

        if when == "after-a-batch":
            round_(4, "warm-up")
            assert _stamp(p) == 1
        p.set_option("debug_store_stamp", TOP - 2)
        seen = []
        for b in range(7):
            i = round_(b, "round")
            seen.append(_stamp(p))
            if b == 0:  # the views' stores are at 0xFFFFFE like the single frame's: a step back is refused for them all
                with pytest.raises(pkg.RtrError) as e:
                    p.set_option("debug_store_stamp", TOP - 2)
                assert e.value.code == pkg._lib.RTR_ERR_INVALID and _stamp(p) == TOP - 1
            if b >= 2:
                _dynamic_extents_in_use(p, world.counts(i), (when, b))
                # every store of the context -- the three views' too -- is at or below the single frame's small stamp
                p.set_option("debug_store_stamp", seen[-1])
        assert seen == [TOP - 1, TOP, 1, 2, 3, 4, 5], (when, seen)
    finally:
        p.close()


# ---- a pool overflow at the wrap -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def overflow_world(pkg, orc):
    xyzw, rgba = po.cloud(orc)
    P1 = po.p_one(orc, sw.OVERFLOW_CX)[0]   # every point an entry, half of them in each of two storage tiles
    P2 = pkg.orbit_projection(3, po.W, po.H)
    refs = {}
    for name, P in (("one", P1), ("orbit", P2)):
        r = orc.project(xyzw, rgba, P, po.W, po.H)
        f = orc.filter(r["depth_bits"], r["img"])
        refs[name] = {False: {"depth": r["depth_bits"], "img": r["img"]},
                      True: {"depth": f["depth"].view(np.uint32), "img": f["img"], "tensor": f["tensor"]}}
    counts = sw.tile_counts(orc, xyzw, rgba, P1, po.W, po.H)
    assert sw.uses_dynamic_extents(counts) and int(counts.sum()) == po.N
    return xyzw, rgba, {"one": P1, "orbit": P2}, refs, counts


def test_pool_overflow_on_the_frame_that_wraps(pkg, orc, overflow_world):
    """pool_overflow_scenes' late overflow: ten ordinary frames size the adaptive pool and take the store to 0xFFFFFF;
    the next frame takes the wrapped stamp 1 AND overflows the pool, so the synchronising call grows the pool and
    renders it again, with stamp 2, into a directory that holds the words of the incomplete attempt."""
    xyzw, rgba, P, refs, counts = overflow_world
    L = pkg._lib
    p = pkg.Projector(0)
    try:
        before = po.prepare(pkg, orc, p, xyzw, rgba, "late", {"debug_store_stamp": TOP - len(po.ORDINARY)})
        assert _stamp(p) == TOP

        def same(name, filtered, what):
            want = refs[name][filtered]
            assert np.array_equal(p.download(L.BUF_DEPTH), want["depth"]), (what, "depth")
            assert np.array_equal(p.download(L.BUF_IMAGE), want["img"]), (what, "img")
            if filtered:
                assert np.array_equal(p.download(L.BUF_TENSOR).reshape(5, po.H, po.W), want["tensor"]), (what, "tensor")

        p.render(P["one"], False)
        assert _stamp(p) == 1             # the wrap took place ...
        p.synchronize()                   # ... and the frame is repeated here
        po.assert_overflowed(p, before, "the frame that wraps")
        assert _stamp(p) == 2
        same("one", False, "repeated frame")
        st = p.frame_stats()
        assert st["errors"] == 0 and st["entries"] == po.N and st["heaviest_tile"] == sw.heaviest_tile(counts) > sw.DYN2, st
        for j, (name, filtered) in enumerate((("one", True), ("orbit", False), ("one", False), ("orbit", True))):
            p.render(P[name], filtered)
            p.synchronize()
            same(name, filtered, ("beyond the wrap", j))
            assert p.frame_stats()["errors"] == 0 and _stamp(p) == 3 + j
    finally:
        p.close()


# ---- edits across the wrap -------------------------------------------------------------------------------------------

def test_append_and_remove_between_the_last_stamp_and_the_first(pkg, world):
    """rtr_append_points and rtr_remove_points between the frame with stamp 0xFFFFFF and the one that wraps: the store
    survives both (its stamp reads 0xFFFFFF after them), the pool is re-sized for the new point count."""
    (ax, ac), keep, _ = world.edit
    p = _context(pkg, world)
    try:
        p.set_option("debug_store_stamp", TOP - 2)
        seen = []
        for i in (0, 1):
            p.render(world.poses[i], True)
            seen.append(_stamp(p))
            _same_frame(pkg, p, world.ref(world.poses[i], True), True, ("before the edits", i))
        _dynamic_extents_in_use(p, world.counts(1), "before the edits")
        p.append_points(ax, ac)
        p.remove_points(keep)
        assert p.num_points == int(keep.sum())
        seen.append(_stamp(p))
        for j in range(5):
            i = j % 2
            filtered = j != 1
            p.render(world.poses[i], filtered)
            seen.append(_stamp(p))
            _same_frame(pkg, p, world.ref(world.poses[i], filtered, tag="edited"), filtered, ("after the edits", j, seen))
            _dynamic_extents_in_use(p, world.counts(i, "edited"), ("after the edits", j))
        assert seen == [TOP - 1, TOP, TOP, 1, 2, 3, 4, 5], seen
    finally:
        p.close()


# ---- the option's contract -------------------------------------------------------------------------------------------

def test_option_contract(pkg, world):
    L = pkg._lib
    p = pkg.Projector(0)
    try:
        assert _stamp(p) == 0
        p.set_option("debug_store_stamp", 5)          # no store yet: the stamp its first frame starts from
        assert _stamp(p) == 5
        p.upload_points(world.xyzw, world.rgba)
        p.set_resolution(W, H)
        assert _stamp(p) == 5
        P = world.poses[0]
        p.render(P, False)
        assert _stamp(p) == 6
        for bad in (3, 5, -1, TOP + 1):               # backwards, or outside 24 bits: refused, nothing changed
            with pytest.raises(pkg.RtrError) as e:
                p.set_option("debug_store_stamp", bad)
            assert e.value.code == L.RTR_ERR_INVALID
            assert _stamp(p) == 6
        p.render(P, False)
        assert _stamp(p) == 7                          # (nothing changed: the next frame took the next stamp)
        _same_frame(pkg, p, world.ref(P, False), False, "after the refused values")
        p.set_option("debug_store_stamp", 7)          # the current value: accepted
        # calls that render nothing leave the stamp alone
        p.synchronize()
        p.frame_stats()
        p.download(L.BUF_DEPTH)
        p.get_option("overlap_active")
        p.set_option("lean", 0)
        p.set_option("lean", 1)
        assert _stamp(p) == 7
        # stores created later start from the value set: the views' stores
        p.set_option("debug_store_stamp", 100)
        assert _stamp(p) == 100
        p.render_views([world.poses[1], world.poses[2]], False)
        assert _stamp(p) == 100                        # (the single frame's store rendered nothing)
        with pytest.raises(pkg.RtrError):
            p.set_option("debug_store_stamp", 100)    # the views' stores are at 101: one step back for them
        p.set_option("debug_store_stamp", 101)
        p.set_option("debug_store_stamp", TOP)        # the largest value: the next frame wraps at once
        p.render(P, True)
        assert _stamp(p) == 1
        _same_frame(pkg, p, world.ref(P, True), True, "wrapped at once")
        _dynamic_extents_in_use(p, world.counts(0), "wrapped at once")
    finally:
        p.close()
