"""Selecting one point per voxel-grid cell on the GPU (include/rtr.h section 6g): rtr_select_voxel_grid's words and all
four statistics compared exactly (np.array_equal) with the numpy float32 reference of tests/voxel_ref.py -- in every
form the cloud can take, at ragged point counts, on duplicated points whatever the resident order, on special
coordinates and the grid's 2^20 boundary, with every op chained between rtr_select_points calls; the words fed to
rtr_remove_points / rtr_set_point_keep and the facade's thin against an upload of A[hit] and the oracle, frame for
frame; what the call must leave alone; the error paths."""
import ctypes as C

import numpy as np
import pytest

import select_ref as sr
import voxel_ref as vr
from test_gpu_select import FORMS, _new, _sel, _specials

pytestmark = pytest.mark.gpu

ORIGIN = (0.013, -0.4, 0)
CELLS = {"0.05": 0.05, "0.25": 0.25, "aniso": (0.25, 0.5, 0.125), "1000": 1000}
MIN_COUNTS = (1, 2, 3, 257)
SCENES = (("room_shell", 150_001), ("uniform_box", 160_003))
# what the reference gives these inputs (cells, cells with >= 2, >= 3 points): spread enough that neither "all" nor
# "nothing" passes for any of them
SPREAD = {("room_shell", "0.05"): (82_922, 46_515, 16_149), ("room_shell", "0.25"): (4_113, 4_086, 4_066),
          ("uniform_box", "0.05"): (151_998, 7_737, 261), ("uniform_box", "0.25"): (13_501, 13_331, 13_200)}


@pytest.fixture(scope="module")
def clouds(orc):
    """scene -> (xyzw, rgba, {(cell name, origin) -> voxel_ref.runs}): computed once, never changed."""
    out = {}
    for scene, n in SCENES:
        xyzw, rgba = orc.generate(scene, 41, 0, n, n)
        grids = {(name, ORIGIN): vr.runs(xyzw, cell, ORIGIN) for name, cell in CELLS.items()}
        grids[("0.25", (0, 0, 0))] = vr.runs(xyzw, 0.25)
        out[scene] = (xyzw, rgba, grids)
    return out


def test_the_reference_spreads_these_inputs(clouds):
    for (scene, name), want in SPREAD.items():
        of = clouds[scene][2][(name, ORIGIN)]
        assert tuple(vr.select(None, None, None, mc, of)[1][1] for mc in (1, 2, 3)) == want, (scene, name)
        assert vr.select(None, None, None, 257, of)[1][1] == 0
    for scene, _ in SCENES:
        of = clouds[scene][2][("1000", ORIGIN)]
        assert [vr.select(None, None, None, mc, of)[1][:2] for mc in MIN_COUNTS] == [(8, 8)] * 4, scene


def _check(pkg, p, n, want, ref_stats, st, what):
    assert st == (int(want.sum()),) + tuple(ref_stats), (what, st, ref_stats)
    assert np.array_equal(_sel(pkg, p, n), want), what


@pytest.mark.parametrize("form", sorted(FORMS))
def test_words_and_stats_match_the_reference_in_every_form(pkg, clouds, form):
    options, sort = FORMS[form]
    both = 0
    for scene, n in SCENES:
        xyzw, rgba, grids = clouds[scene]
        opts = dict(options)
        if scene == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            if form == "sorted":
                assert p.get_option("reordered") == 1
            for (name, origin), of in grids.items():
                for mc in MIN_COUNTS:
                    hit, ref = vr.select(None, None, None, mc, of)
                    # both hits and misses wherever some cell is full: a kernel returning all or nothing cannot pass
                    assert hit.any() == (ref[1] > 0) and not hit.all(), (scene, name, mc)
                    both += bool(hit.any())
                    for outside in (False, True):
                        st = p.select_voxel_grid(CELLS[name], origin, mc, outside=outside)
                        _check(pkg, p, n, hit != outside, ref, st, (form, scene, name, origin, mc, outside))
                        if not outside:
                            assert st[0] == st[2] + (st[3] if mc == 1 else 0)
        finally:
            p.close()
    assert both >= 2 * (3 * 5 + 1)  # (min_count 1, 2, 3 of every grid, 257 at cell 1000, in both scenes)


def test_ragged_counts(pkg, orc):
    for n in (1, 255, 256, 257, 4099):
        xyzw, rgba = orc.generate("room_shell", 100 + n, 0, n, n)
        hit1, ref1 = vr.select(xyzw, 0.25, ORIGIN, 1)
        hit2, ref2 = vr.select(xyzw, 0.25, ORIGIN, 2)
        hit3, ref3 = vr.select(xyzw, (0.5, 0.25, 1.0), ORIGIN, 1)
        assert n < 255 or (0 < hit2.sum() < hit1.sum() < n)
        for options, sort in (({}, False), ({"pack": 0}, False), ({"point_ids": 1}, True)):
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                sel = np.zeros(n, bool)
                for cell, mc, op, outside, hit, ref in ((0.25, 1, "replace", False, hit1, ref1), (0.25, 2, "toggle", True, hit2, ref2),
                                                        ((0.5, 0.25, 1.0), 1, "add", True, hit3, ref3), (0.25, 2, "toggle", False, hit2, ref2),
                                                        (0.25, 1, "replace", True, hit1, ref1), (0.25, 1, "toggle", True, hit1, ref1),
                                                        (0.25, 2, "intersect", True, hit2, ref2)):
                    sel = sr.combine(op, sel, hit != outside)
                    st = p.select_voxel_grid(cell, ORIGIN, mc, op=op, outside=outside)
                    _check(pkg, p, n, sel, ref, st, (n, options, cell, mc, op, outside))  # (_sel: no bit at or past n)
            finally:
                p.close()


def test_duplicates_keep_the_smallest_index_in_every_resident_order(pkg, orc):
    n = 80_001
    xyzw, rgba = orc.generate("room_shell", 7, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[5000:5100] = xyzw[:100]
    xyzw[70_000:70_100] = xyzw[:100]
    got = {form: _new(pkg, options, xyzw, rgba, sort=sort)
           for form, (options, sort) in (("packed", ({}, False)), ("unpacked", ({"pack": 0}, False)), ("sorted", ({"point_ids": 1}, True)))}
    try:
        assert got["sorted"].get_option("reordered") == 1 and got["packed"].get_option("reordered") == 0
        assert got["packed"].get_option("packed") == 1 and got["unpacked"].get_option("packed") == 0
        for cell in (1e-4, 0.05):
            for mc in (1, 2, 3, 4):
                hit, ref = vr.select(xyzw, cell, ORIGIN, mc)
                assert not hit[5000:5100].any() and not hit[70_000:70_100].any()  # (never a later copy)
                if cell == 1e-4:  # (cells so small that only the copies share one: three points each)
                    assert hit[:100].all() == (mc <= 3) and hit[:100].any() == (mc <= 3)
                # (the resident order of the sorted context differs: its keys went through the scatter)
                for form, p in got.items():
                    st = p.select_voxel_grid(cell, ORIGIN, mc)
                    _check(pkg, p, n, hit, ref, st, (form, cell, mc))
                words = [p.download(pkg._lib.BUF_SELECTION) for p in got.values()]
                assert np.array_equal(words[0], words[1]) and np.array_equal(words[0], words[2])
    finally:
        for p in got.values():
            p.close()


def _special_cloud(orc, axis):
    f = np.float32
    n = 4099
    xyzw, rgba = orc.generate("room_shell", 300 + axis, 0, n, n)
    xyzw = xyzw.copy()
    edge = f([-262144.0, 262144.0, np.nextafter(f(262144), f(0)), np.nextafter(f(-262144), f(-np.inf)), 262143.75])
    sp = np.concatenate([_specials(), edge])  # (cell 0.25, origin 0: t = 4 x exactly, 2^20 at x = 262144)
    rng = np.random.default_rng(axis)
    at = rng.choice(np.arange(300, 1500), 3 * sp.size, replace=False)  # (chunks 1 .. 5: the others stay narrow)
    xyzw[at, axis] = np.tile(sp, 3)
    xyzw[at[:sp.size], (axis + 1) % 3] = 0.1  # (one copy of each special in a cell of its own choosing ...)
    for k in range(3):  # (... and two more that share cells pairwise)
        if k != axis:
            xyzw[at[sp.size:], k] = 0.3
    return xyzw, rgba, at, sp


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_special_coordinates_and_the_grid_boundary(pkg, orc, axis):
    xyzw, rgba, at, sp = _special_cloud(orc, axis)
    n = xyzw.shape[0]
    ok, _ = vr.cells(xyzw, 0.25)
    v = xyzw[:, axis]
    with np.errstate(invalid="ignore"):
        want_out = ~np.isfinite(v) | (np.abs(v) >= 3e38) | (v >= 262144) | (v < -262144)
    assert np.array_equal(~ok, want_out) and want_out.sum() == 3 * 9  # (+-1e30, +-3.4e38, +-inf, NaN, 2^20, below -2^20)
    for options in ({"auto_reorder": 0}, {"auto_reorder": 0, "pack": 2}, {"auto_reorder": 0, "pack": 0}, {"point_ids": 1}):
        p = _new(pkg, options, xyzw, rgba, sort="point_ids" in options)
        try:
            for mc in (1, 2):
                hit, ref = vr.select(xyzw, 0.25, (0, 0, 0), mc)
                st = p.select_voxel_grid(0.25, min_count=mc)
                _check(pkg, p, n, hit, ref, st, (axis, options, mc))
                got = _sel(pkg, p, n)
                assert st[3] == 27 and (got[~ok].all() if mc == 1 else not got[~ok].any())
                st = p.select_voxel_grid(0.25, min_count=mc, outside=True)
                _check(pkg, p, n, ~hit, ref, st, (axis, options, mc, "outside"))
        finally:
            p.close()


@pytest.mark.parametrize("form", ["default", "sorted"])
def test_ops_chained_with_select_points(pkg, orc, form):
    options, sort = FORMS[form]
    n = 70_003
    xyzw, rgba = orc.generate("room_shell", 23, 0, n, n)
    f3 = xyzw[:, :3]
    lo, hi = f3.min(axis=0) - 1, (f3.min(axis=0) + f3.max(axis=0)) / 2 + np.float32(0.013)
    planes = pkg.clip_box_planes(lo, hi)
    box = pkg.clip_keep(planes, xyzw)
    v1, r1 = vr.select(xyzw, 0.05, ORIGIN, 1)
    v2, r2 = vr.select(xyzw, 0.05, ORIGIN, 2)
    v3, r3 = vr.select(xyzw, 0.25, ORIGIN, 3)
    p = _new(pkg, options, xyzw, rgba, sort=sort)
    try:
        sel = box.copy()
        assert p.select_points(planes=planes)[0] == int(sel.sum())
        for cell, mc, op, outside, hit, ref in ((0.05, 1, "intersect", False, v1, r1), (0.05, 2, "add", True, v2, r2),
                                                (0.25, 3, "toggle", False, v3, r3), (0.05, 1, "subtract", False, v1, r1)):
            sel = sr.combine(op, sel, hit != outside)
            st = p.select_voxel_grid(cell, ORIGIN, mc, op=op, outside=outside)
            _check(pkg, p, n, sel, ref, st, (form, cell, mc, op))
            assert 0 < sel.sum() < n
        sel = sr.combine("add", sel, box)  # (... and rtr_select_points goes on from the voxel call's words)
        assert p.select_points(planes=planes, op="add")[0] == int(sel.sum())
        assert np.array_equal(_sel(pkg, p, n), sel)
        # the combining ops on a selection that does not exist yet: it counts as empty; stats=False still waits
        for op, want in (("add", v1), ("subtract", np.zeros(n, bool)), ("intersect", np.zeros(n, bool)), ("toggle", v1)):
            p.clear_selection()
            assert p.select_voxel_grid(0.05, ORIGIN, op=op, stats=False) is None
            assert np.array_equal(_sel(pkg, p, n), want), op
    finally:
        p.close()


def _frames(pkg, p, Ps):
    L = pkg._lib
    out = []
    for k, P in enumerate(Ps):
        img, depth = p.project(P, filtered=k % 2 == 1)
        frame = {"depth": depth.view(np.uint32).copy(), "image": img.copy(), "tensor": None, "ids": None}
        if k % 2 == 1:
            frame["tensor"] = p.download(L.BUF_TENSOR).copy()
        else:  # (the point pass of the unfiltered frame)
            p.point_pass(P)
            frame["ids"], frame["visible"] = p.download(L.BUF_POINT_ID).copy(), sr.unpack(p.download(L.BUF_VISIBLE), p.num_points)
        out.append(frame)
    return out


def _same_frames(a, b, what, index_of=None):
    """index_of: a's point index of every point of b (a shows b's points under a keep mask)."""
    for k, (fa, fb) in enumerate(zip(a, b)):
        for name in ("depth", "image", "tensor"):
            if fa[name] is not None:
                assert np.array_equal(fa[name], fb[name]), (what, k, name)
        if fa["ids"] is None:
            continue
        ids_b, vis_b = fb["ids"], fb["visible"]
        if index_of is not None:
            none = ids_b == 0xFFFFFFFF
            ids_b = np.where(none, ids_b, index_of[np.where(none, 0, ids_b)]).astype(np.uint32)
            full = np.zeros(fa["visible"].size, bool)
            full[index_of] = vis_b
            vis_b = full
        assert np.array_equal(fa["ids"], ids_b), (what, k, "ids")
        assert np.array_equal(fa["visible"], vis_b), (what, k, "visible")


@pytest.mark.parametrize("form", ["default", "sorted"])
def test_the_words_thin_the_cloud(pkg, orc, form):
    options, sort = FORMS[form]
    n, W, H = 120_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 52, 0, n, n)
    hit, ref = vr.select(xyzw, 0.05, ORIGIN)
    assert n // 4 < hit.sum() < 3 * n // 4
    Ps = [pkg.orbit_projection(k, W, H) for k in (5, 130, 420, 777)]
    b = _new(pkg, {}, xyzw[hit], rgba[hit], W, H)
    try:
        want = _frames(pkg, b, Ps)
        for k, P in enumerate(Ps):  # (the second context is the oracle's cloud A[hit])
            r = orc.project(xyzw[hit], rgba[hit], P, W, H)
            if k % 2 == 1:
                f = orc.filter(r["depth_bits"], r["img"])
                r = {"depth_bits": f["depth"].view(np.uint32), "img": f["img"]}
            assert np.array_equal(want[k]["depth"], r["depth_bits"]) and np.array_equal(want[k]["image"], r["img"]), (form, k)
        # as the keep words of remove_points
        a = _new(pkg, options, xyzw, rgba, W, H, sort=sort)
        try:
            assert a.select_voxel_grid(0.05, ORIGIN) == (int(hit.sum()),) + ref
            a.remove_points(a.selection())
            assert a.num_points == int(hit.sum()) and a.selection() is None
            _same_frames(_frames(pkg, a, Ps), want, (form, "remove"))
        finally:
            a.close()
        # through set_point_keep: hidden, not removed
        a = _new(pkg, options, xyzw, rgba, W, H, sort=sort)
        try:
            a.select_voxel_grid(0.05, ORIGIN, stats=False)
            a.set_point_keep(a.selection())
            assert np.array_equal(a.point_keep(), hit) and a.num_points == n
            _same_frames(_frames(pkg, a, Ps), want, (form, "keep"), np.flatnonzero(hit))
        finally:
            a.close()
    finally:
        b.close()


@pytest.mark.parametrize("point_ids", [False, True])
def test_facade_thin(pkg, orc, point_ids):
    n, W, H = 100_003, 320, 240
    xyzw, rgba = orc.generate("room_shell", 64, 0, n, n)
    hit, _ = vr.select(xyzw, 0.08)
    hit3, _ = vr.select(xyzw, (0.08, 0.1, 0.2), ORIGIN, 3)
    assert 0 < hit3.sum() < hit.sum() < n
    cal, E = pkg.benchmark_calibration(W, H), pkg.orbit_pose(300)
    pc = pkg.ProjectCloud(xyzw, rgba, reorder=point_ids, point_ids=point_ids)
    assert pc.selectVoxelGrid((0.08, 0.1, 0.2), ORIGIN, min_count=3) == int(hit3.sum()) == pc.selectedCount()
    assert pc.selectVoxelGrid(0.08, outside=True, op="add") == int((hit3 | ~hit).sum())
    assert pc.thin(0.08) == int(hit.sum()) == pc.projector.num_points
    assert pc.projector.selection() is None and pc.selectedCount() == 0
    color, depth = np.empty((H, W, 3), np.uint8), np.empty((H, W), np.float32)
    assert pc.computeRGBD(cal, E, color, depth) == 1
    r = orc.project(xyzw[hit], rgba[hit], orc.compose_projection(cal.getIntrinsicsMatrix(), E), W, H)
    assert np.array_equal(depth.view(np.uint32), r["depth_bits"])
    assert pc.thin(0.08) == int(hit.sum())  # (already thin: nothing goes)


def test_the_call_moves_nothing_else(pkg, orc):
    L = pkg._lib
    n, W, H = 150_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 88, 0, n, n)
    P, P2 = pkg.orbit_projection(40, W, H), pkg.orbit_projection(41, W, H)
    keep = np.arange(n) % 3 != 0
    planes = np.float32([[0, 0, 1, 100], [1, 0, 0, 50]])
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        def state():
            return [p.download(b).copy() for b in (L.BUF_DEPTH, L.BUF_IMAGE, L.BUF_TENSOR, L.BUF_VISIBLE, L.BUF_POINT_ID, L.BUF_POINT_KEEP)] + \
                   [p.clip_planes(), p.frame_stats(), p.get_option("p2p_open"), p.get_option("packed"), p.get_option("reordered"),
                    p.get_option("point_keep"), p.num_points]

        def same(a, b):
            return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

        p.set_clip_planes(planes)
        p.set_point_keep(keep)
        p.p2p_open(0, 1, [p.p2p_export()])  # (the one-rank form of test_gpu_p2p.py: a rank maps its own buffers)
        p.p2p_render(P, True)
        p.point_pass(P)
        before = state()
        want = None
        for kw in (dict(cell=0.05), dict(cell=(0.25, 0.5, 0.125), origin=ORIGIN, min_count=2, op="add"),
                   dict(cell=0.25, op="toggle", outside=True, stats=False)):
            hit, ref = vr.select(xyzw, kw["cell"], kw.get("origin", (0, 0, 0)), kw.get("min_count", 1))
            want = sr.combine(kw.get("op", "replace"), want, hit != kw.get("outside", False)) if want is not None else hit
            p.select_voxel_grid(**kw)
            assert np.array_equal(_sel(pkg, p, n), want), kw  # (the clip planes and the keep mask in force play no part)
        assert same(before, state()) and p.get_option("p2p_open") == 1
        p.p2p_close()
        p.set_clip_planes(None)
        p.set_point_keep(None)
        # issued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.select_voxel_grid(0.05, ORIGIN, 2)
        p.wait_outputs(0)
        r = orc.project(xyzw, rgba, P2, W, H)
        assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(img, r["img"])
    finally:
        p.close()


def test_errors_leave_the_selection_intact(pkg, orc):
    L = pkg._lib
    n = 20_001
    xyzw, rgba = orc.generate("room_shell", 4, 0, n, n)
    f = np.float32
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    zero, cell = f([0, 0, 0]), f([0.25, 0.25, 0.25])
    fresh = pkg.Projector(0)
    try:
        with pytest.raises(pkg.RtrError) as e:
            fresh.select_voxel_grid(0.25)
        assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        want, _ = vr.select(xyzw, 0.05, ORIGIN, 2)
        p.select_voxel_grid(0.05, ORIGIN, 2)
        lib, ctx = p._lib, p._ctx
        bad = [(None, vp(cell), 1, 0, "origin"), (vp(zero), None, 1, 0, "cell"), (vp(zero), vp(cell), 0, 0, "min_count")]
        for v in (np.nan, np.inf, -np.inf):
            for k in range(3):
                o = zero.copy(); o[k] = v
                bad.append((vp(o), vp(cell), 1, 0, "origin", o))
        den = np.array([1], np.uint32).view(f)[0]  # (its reciprocal overflows)
        for v in (0.0, -0.0, -0.25, np.nan, np.inf, den):
            for k in range(3):
                c3 = cell.copy(); c3[k] = v
                bad.append((vp(zero), vp(c3), 1, 0, "cell", c3))
        for op in (-1, 9, 10, 11, 13, 16, 32):
            bad.append((vp(zero), vp(cell), 1, op, "op"))
        for case in bad:
            st = np.full(4, 77, np.uint64)
            assert lib.rtr_select_voxel_grid(ctx, case[0], case[1], case[2], case[3], vp(st)) == L.RTR_ERR_INVALID, case
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_select_voxel_grid" in text and case[4] in text, (case, text)
            assert np.array_equal(_sel(pkg, p, n), want), case
            assert (st == 77).all(), case
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        with pytest.raises(pkg.RtrError) as e:
            p.select_voxel_grid(0.25)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert np.array_equal(_sel(pkg, p, n), want)
        # an error on a context without a selection makes none
        p.clear_selection()
        assert lib.rtr_select_voxel_grid(ctx, vp(zero), vp(cell), 0, 0, None) == L.RTR_ERR_INVALID and p.selection() is None
    finally:
        p.close()
