"""Selecting resident points on the GPU (include/rtr.h section 6f): rtr_select_points' words compared exactly
(np.array_equal) with the references of tests/select_ref.py -- camera.clip_keep in numpy float32 for the planes, the
oracle's projection for the rectangle -- in every form the cloud can take; every op, chained; the statistics and the
three-way chunk decision; the words fed back to rtr_remove_points / rtr_transform_points / rtr_set_point_keep and the
facade's removeSelected / hideSelected / transformSelected against an upload of the numpy-edited cloud, frame for frame;
what a selection must leave alone; the life of the buffer and the error paths."""
import ctypes as C

import numpy as np
import pytest

import select_ref as sr

pytestmark = pytest.mark.gpu

OPS = ("replace", "add", "subtract", "intersect", "toggle")
FORMS = {"default": ({}, False), "pack0": ({"pack": 0}, False), "pack2": ({"pack": 2}, False),
         "hash_unpacked": ({"auto_reorder": 0}, False), "sorted": ({"point_ids": 1}, True)}


def _specials():  # (the specials of test_clip_host.py)
    f = np.float32
    den = np.array([1, 0x80000001, 0x007FFFFF, 0x807FFFFF], np.uint32).view(np.float32)
    return np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 0.5, -2.0, 1e30, -1e30, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan,
                                     np.nextafter(f(1), f(2)), np.nextafter(f(1), f(0)), np.nextafter(f(-1), f(0))],
                                    np.float32), den])


def _new(pkg, options, xyzw, rgba, W=64, H=48, sort=False):
    p = pkg.Projector(0)
    for k, v in options.items():
        p.set_option(k, v)
    p.upload_points(xyzw, rgba)
    if sort:
        p.reorder_points()
    p.set_resolution(W, H)
    return p


def _octant(xyzw):
    f = xyzw[np.isfinite(xyzw[:, :3]).all(axis=1), :3]
    lo, hi = f.min(axis=0), f.max(axis=0)
    return lo - 1, (lo + hi) / 2 + np.float32(0.013)


def _regions(pkg, xyzw):
    f = np.float32
    lo, hi = _octant(xyzw)
    return {"octant": pkg.clip_box_planes(lo, hi),
            "oblique": f([[0.3, -0.2, 0.9, 0.35], [-0.7, 0.1, 0.2, 1.3]]),
            "half": f([[1, 0, 0, 0]]),
            "keep_all": f([[0, 0, 1, 100]]),
            "keep_none": f([[0, 0, 1, -100]]),
            "none": None}


def _sel(pkg, p, n):
    w = p.download(pkg._lib.BUF_SELECTION)
    assert w.shape == ((n + 31) // 32,)
    if n % 32:
        assert w[-1] >> (n % 32) == 0, "bits past n"
    return sr.unpack(w, n)


def _chunks(n):
    return (n + 255) // 256


def _check(pkg, p, n, want, st, what):
    assert st[0] == int(want.sum()), (what, st)
    assert st[1] + st[2] + st[3] == _chunks(n), (what, st)
    if n:
        assert np.array_equal(_sel(pkg, p, n), want), what


@pytest.mark.parametrize("form", sorted(FORMS))
def test_planes_match_clip_keep_in_every_form(pkg, orc, form):
    options, sort = FORMS[form]
    for scene, n in (("room_shell", 150_001), ("uniform_box", 160_003)):
        xyzw, rgba = orc.generate(scene, 41, 0, n, n)
        opts = dict(options)
        if scene == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            if form == "hash_unpacked" and scene == "uniform_box":
                assert p.get_option("reordered") == 0 and p.get_option("packed") == 0
            for name, planes in _regions(pkg, xyzw).items():
                want = sr.inside(pkg, orc, xyzw, planes)
                for outside in (False, True):
                    st = p.select_points(planes=planes, outside=outside)
                    _check(pkg, p, n, want != outside, st, (form, scene, name, outside))
                    if name == "none":
                        assert st[0] == (0 if outside else n)
        finally:
            p.close()


def test_ragged_counts(pkg, orc):
    for n in (0, 1, 255, 256, 257, 4099):
        xyzw, rgba = orc.generate("room_shell", 100 + n, 0, n, n) if n else (np.zeros((0, 4), np.float32), np.zeros((0, 4), np.uint8))
        for options, sort in (({}, False), ({"pack": 2}, False), ({"pack": 0}, False), ({"point_ids": 1}, True)):
            p = _new(pkg, options, xyzw, rgba, sort=sort and n > 0)
            try:
                sel = np.zeros(n, bool)
                for k, (name, op, outside) in enumerate((("half", "replace", False), ("oblique", "add", True), ("none", "toggle", False),
                                                         ("keep_all", "intersect", False), ("half", "subtract", True))):
                    planes = _regions(pkg, xyzw if n else np.zeros((1, 4), np.float32))[name]
                    hit = sr.inside(pkg, orc, xyzw, planes) != outside
                    sel = sr.combine(op, sel, hit)
                    st = p.select_points(planes=planes, op=op, outside=outside)
                    _check(pkg, p, n, sel, st, (n, options, name, op))
            finally:
                p.close()


def test_upload_plus_two_appends(pkg, orc):
    n = 90_001
    xyzw, rgba = orc.generate("room_shell", 9, 0, n, n)
    cuts = (0, 40_000, 40_300, n)
    for options in ({}, {"pack": 0}, {"point_ids": 1, "auto_reorder": 1}):
        p = _new(pkg, options, xyzw[:cuts[1]], rgba[:cuts[1]])
        try:
            p.select_points(planes=_regions(pkg, xyzw)["half"])
            for a, b in zip(cuts[1:-1], cuts[2:]):
                p.append_points(xyzw[a:b], rgba[a:b])
                assert p.selection() is None and p.get_option("selection") == 0
            for name, planes in _regions(pkg, xyzw).items():
                st = p.select_points(planes=planes)
                _check(pkg, p, n, sr.inside(pkg, orc, xyzw, planes), st, (options, name))
        finally:
            p.close()


def test_special_coordinates_on_box_faces(pkg, orc):
    rng = np.random.default_rng(17)
    sp = _specials()
    finite = sp[np.isfinite(sp)]
    n = 6000
    for trial in range(6):
        lo, hi = rng.choice(finite, 3), rng.choice(finite, 3)
        lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
        pts = rng.choice(sp, (n, 3))
        faces = rng.integers(0, 4, (n, 3))
        near = np.nextafter(np.where(faces == 1, lo[None, :], hi[None, :]).astype(np.float32),
                            np.float32(np.inf) * np.where(rng.random((n, 3)) < 0.5, -1, 1).astype(np.float32))
        pts = np.where(faces == 1, lo[None, :], np.where(faces == 2, hi[None, :], np.where(faces == 3, near, pts))).astype(np.float32)
        if trial % 2:  # (chunks of equal points: boxes that the headers decide, a face value throughout)
            pts = np.repeat(pts[: n // 256 + 1], 256, axis=0)[:n]
            pts[3 * 256:4 * 256, 0] = np.nan
        xyzw = np.concatenate([pts, np.ones((n, 1), np.float32)], axis=1)
        rgba = rng.integers(0, 256, (n, 4), dtype=np.uint8)
        planes = pkg.clip_box_planes(lo, hi)
        want = np.all((lo[None, :] <= pts) & (pts <= hi[None, :]), axis=1)
        assert np.array_equal(want, pkg.clip_keep(planes, pts))
        nan = np.isnan(pts).any(axis=1)
        assert nan.any() and not want[nan].any()
        for options in ({"auto_reorder": 0}, {"auto_reorder": 0, "pack": 2}, {"auto_reorder": 0, "pack": 0}):
            p = _new(pkg, options, xyzw, rgba)
            try:
                for outside in (False, True):
                    st = p.select_points(planes=planes, outside=outside)
                    _check(pkg, p, n, want != outside, st, (trial, options, outside))
                    got = _sel(pkg, p, n)
                    assert got[nan].all() if outside else not got[nan].any()  # (NaN: never inside, always hit by OUTSIDE)
            finally:
                p.close()


@pytest.mark.parametrize("form", ["default", "pack0", "sorted"])
def test_every_op_chained_over_three_calls(pkg, orc, form):
    options, sort = FORMS[form]
    n, W, H = 70_003, 64, 48
    xyzw, rgba = orc.generate("room_shell", 23, 0, n, n)
    reg = _regions(pkg, xyzw)
    P = pkg.orbit_projection(7, W, H)
    rect = (5, 3, 50, 40)
    p = _new(pkg, options, xyzw, rgba, W, H, sort=sort)
    try:
        in_a = sr.inside(pkg, orc, xyzw, reg["octant"])
        in_b = sr.inside(pkg, orc, xyzw, reg["oblique"])
        in_c = sr.inside(pkg, orc, xyzw, None, P, rect, W, H)
        for op2 in OPS:
            for out2 in (False, True):
                for op3, out3 in ((OPS[(OPS.index(op2) + 1) % 5], not out2), ("intersect", out2)):
                    sel = in_a.copy()
                    st = p.select_points(planes=reg["octant"], op="replace")
                    _check(pkg, p, n, sel, st, (form, "first"))
                    sel = sr.combine(op2, sel, in_b != out2)
                    st = p.select_points(planes=reg["oblique"], op=op2, outside=out2)
                    _check(pkg, p, n, sel, st, (form, op2, out2))
                    sel = sr.combine(op3, sel, in_c != out3)
                    st = p.select_points(P=P, rect=rect, op=op3, outside=out3)
                    _check(pkg, p, n, sel, st, (form, op2, out2, op3, out3))
        # the combining ops on a selection that does not exist yet: it counts as empty
        for op, want in (("add", in_a), ("subtract", np.zeros(n, bool)), ("intersect", np.zeros(n, bool)), ("toggle", in_a)):
            p.clear_selection()
            _check(pkg, p, n, want, p.select_points(planes=reg["octant"], op=op), (form, "fresh", op))
        # stats=False queues the call; the words are the same
        assert p.select_points(planes=reg["oblique"], stats=False) is None
        assert np.array_equal(_sel(pkg, p, n), in_b)
    finally:
        p.close()


def test_stats_show_all_three_chunk_decisions(pkg, orc):
    n = 1_000_000
    xyzw, rgba = orc.generate("room_shell", 0xC0FFEE03, 0, n, n)
    p = _new(pkg, {"auto_reorder": 0}, xyzw, rgba)
    try:
        assert p.get_option("packed") == 1 and p.get_option("reordered") == 0
        lo, hi = _octant(xyzw)
        planes = pkg.clip_box_planes(lo, hi)
        want = pkg.clip_keep(planes, xyzw)
        st = p.select_points(planes=planes)
        print("octant box on room_shell 1e6: selected %d, chunks outside %d, inside %d, decoded %d" % st)
        _check(pkg, p, n, want, st, "octant")
        assert st[1] > 0 and st[2] > 0 and st[3] > 0  # (a build that decodes every chunk would pass the comparison alone)
        st = p.select_points(planes=planes, outside=True)
        _check(pkg, p, n, ~want, st, "octant outside")
        assert st[1] > 0 and st[2] > 0 and st[3] > 0
        assert p.select_points()[1:] == (0, _chunks(n), 0)  # (no region: every chunk inside, none decoded)
    finally:
        p.close()


@pytest.mark.parametrize("form", ["default", "pack0", "sorted"])
def test_rectangle_matches_the_oracle(pkg, orc, form):
    options, sort = FORMS[form]
    for (W, H), n, rects in (((64, 48), 60_001, ((0, 0, 64, 48), (10, 5, 11, 6), (0, 20, 64, 21), (30, 0, 64, 48), (63, 47, 64, 48))),
                             ((1920, 1080), 400_003, ((0, 0, 1920, 1080), (600, 300, 1300, 800), (0, 0, 1, 1080), (1900, 1000, 1920, 1080)))):
        xyzw, rgba = orc.generate("room_shell", 77, 0, n, n)
        p = _new(pkg, options, xyzw, rgba, W, H, sort=sort)
        try:
            for k in (3, 250, 611):
                P = pkg.orbit_projection(k, W, H)
                pix = sr.pixels(orc, xyzw, P, W, H)
                for rect in rects:
                    x0, y0, x1, y1 = rect
                    want = (pix >= 0) & (pix % W >= x0) & (pix % W < x1) & (pix // W >= y0) & (pix // W < y1)
                    st = p.select_points(P=P, rect=rect)
                    _check(pkg, p, n, want, st, (form, W, k, rect))
                    assert st[2] == 0  # (a rectangle never decides a chunk inside on its box)
                # the full frame selects exactly the points a frame accepts
                p.project(P)
                assert p.select_points(P=P, rect=(0, 0, W, H))[0] == p.frame_stats()["entries"] == int((pix >= 0).sum())
                # a rectangle with planes in one call = the AND of the two selections
                planes = _regions(pkg, xyzw)["oblique"]
                rect = (0, 0, W, H) if k == 3 else rects[1]
                st = p.select_points(planes=planes, P=P, rect=rect)
                both = _sel(pkg, p, n)
                p.select_points(planes=planes)
                p.select_points(P=P, rect=rect, op="intersect")
                assert np.array_equal(both, _sel(pkg, p, n)) and st[0] == int(both.sum())
                assert np.array_equal(both, sr.inside(pkg, orc, xyzw, planes, P, rect, W, H))
        finally:
            p.close()


def _frames(pkg, p, Ps):
    L = pkg._lib
    out = []
    for k, P in enumerate(Ps):
        img, depth = p.project(P, filtered=k % 2 == 1)
        out.append((depth.view(np.uint32).copy(), img.copy(), p.download(L.BUF_TENSOR).copy() if k % 2 == 1 else None))
    return out


def _same_frames(a, b, what):
    for k, (fa, fb) in enumerate(zip(a, b)):
        for name, xa, xb in zip(("depth", "image", "tensor"), fa, fb):
            if xa is not None:
                assert np.array_equal(xa, xb), (what, k, name)


def _moved(xyzw, M, sel):
    m = np.asarray(M, np.float64)[:3].astype(np.float32)
    out = xyzw.copy()
    x, y, z = out[sel, 0].copy(), out[sel, 1].copy(), out[sel, 2].copy()
    for r in range(3):
        out[sel, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    return out


M_RIGID = np.array([[np.cos(0.05), -np.sin(0.05), 0, 0.3], [np.sin(0.05), np.cos(0.05), 0, -0.2], [0, 0, 1, 0.1], [0, 0, 0, 1]])


@pytest.mark.parametrize("form", ["default", "pack0", "sorted"])
def test_selection_feeds_the_editing_calls(pkg, orc, form):
    options, sort = FORMS[form]
    n, W, H = 120_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 52, 0, n, n)
    lo, hi = _octant(xyzw)
    planes = pkg.clip_box_planes(lo, hi)
    inside = pkg.clip_keep(planes, xyzw)
    assert 0 < inside.sum() < n
    Ps = [pkg.orbit_projection(k, W, H) for k in (5, 130, 420, 777)]
    # remove_points(selection()) after an OUTSIDE box selection: the inside of the box is deleted
    a = _new(pkg, options, xyzw, rgba, W, H, sort=sort)
    b = _new(pkg, {}, xyzw[~inside], rgba[~inside], W, H)
    try:
        a.select_points(planes=planes, outside=True)
        a.remove_points(a.selection())
        assert a.num_points == int((~inside).sum()) and a.selection() is None
        _same_frames(_frames(pkg, a, Ps), _frames(pkg, b, Ps), (form, "remove"))
    finally:
        a.close(); b.close()
    # transform_points(M, selection()), then set_point_keep(selection())
    a = _new(pkg, options, xyzw, rgba, W, H, sort=sort)
    moved = _moved(xyzw, M_RIGID, inside)
    b = _new(pkg, {}, moved, rgba, W, H)
    c = _new(pkg, {}, moved[inside], rgba[inside], W, H)
    try:
        a.select_points(planes=planes)
        a.transform_points(M_RIGID, a.selection())
        assert np.array_equal(_sel(pkg, a, n), inside)  # (the selection stays)
        _same_frames(_frames(pkg, a, Ps), _frames(pkg, b, Ps), (form, "transform"))
        a.set_point_keep(a.selection())
        assert np.array_equal(a.point_keep(), inside) and np.array_equal(_sel(pkg, a, n), inside)
        _same_frames(_frames(pkg, a, Ps), _frames(pkg, c, Ps), (form, "keep"))
    finally:
        a.close(); b.close(); c.close()


@pytest.mark.parametrize("point_ids", [False, True])
def test_facade_selected_calls(pkg, orc, point_ids):
    n, W, H = 100_003, 320, 240
    xyzw, rgba = orc.generate("room_shell", 64, 0, n, n)
    lo, hi = _octant(xyzw)
    inside = pkg.clip_keep(pkg.clip_box_planes(lo, hi), xyzw)
    half = pkg.clip_keep(np.float32([[1, 0, 0, 0]]), xyzw)
    cal = pkg.benchmark_calibration(W, H)
    Es = [pkg.orbit_pose(k) for k in (5, 300, 650)]

    def frames(pc):
        out = []
        for k, E in enumerate(Es):
            color, depth = np.empty((H, W, 3), np.uint8), np.empty((H, W), np.float32)
            fn = pc.computeFilteredRGBD if k % 2 else pc.computeRGBD
            assert fn(cal, E, color, depth) == 1
            out.append((depth.view(np.uint32).copy(), color, None))
        return out

    def cloud(x, c):
        return pkg.ProjectCloud(x, c, reorder=point_ids, point_ids=point_ids)

    pc = cloud(xyzw, rgba)
    assert pc.selectedCount() == 0
    assert pc.selectBox(lo, hi) == int(inside.sum()) == pc.selectedCount()
    assert pc.selectPlanes(np.float32([[1, 0, 0, 0]]), op="intersect") == int((inside & half).sum())
    sel = inside & half
    E = Es[0]
    pix = sr.pixels(orc, xyzw, pkg.compose_projection(cal.getIntrinsicsMatrix(), E), W, H)
    in_rect = (pix >= 0) & (pix % W >= 40) & (pix % W < 200) & (pix // W >= 30) & (pix // W < 220)
    assert pc.selectRect(cal, E, 40, 30, 200, 220, op="add") == int((sel | in_rect).sum())
    sel |= in_rect
    # hideSelected: the mask becomes everything but the selection, which stays
    pc.hideSelected()
    assert pc.selectedCount() == int(sel.sum())
    assert np.array_equal(pc.projector.point_keep(), ~sel)
    _same_frames(frames(pc), frames(cloud(xyzw[~sel], rgba[~sel])), "hideSelected")
    pc.clearPointKeep()
    # transformSelected: the selection stays on the same vertices
    pc.transformSelected(M_RIGID)
    moved = _moved(xyzw, M_RIGID, sel)
    assert pc.selectedCount() == int(sel.sum())
    assert np.array_equal(_sel(pkg, pc.projector, n), sel)
    _same_frames(frames(pc), frames(cloud(moved, rgba)), "transformSelected")
    # removeSelected: gone, and so is the selection
    pc.removeSelected()
    assert pc.projector.num_points == int((~sel).sum()) and pc.projector.selection() is None and pc.selectedCount() == 0
    _same_frames(frames(pc), frames(cloud(moved[~sel], rgba[~sel])), "removeSelected")
    pc.removeSelected()  # (nothing selected: nothing removed)
    assert pc.projector.num_points == int((~sel).sum())
    pc.clearSelection()


def test_a_selection_moves_nothing_else(pkg, orc):
    L = pkg._lib
    n, W, H = 150_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 88, 0, n, n)
    reg = _regions(pkg, xyzw)
    P, P2 = pkg.orbit_projection(40, W, H), pkg.orbit_projection(41, W, H)
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        def state():
            return [p.download(b).copy() for b in (L.BUF_DEPTH, L.BUF_IMAGE, L.BUF_TENSOR, L.BUF_VISIBLE, L.BUF_POINT_ID)] + \
                   [p.frame_stats(), p.get_option("p2p_open")]

        def same(a, b):
            return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

        p.p2p_open(0, 1, [p.p2p_export()])  # (the one-rank form of test_gpu_p2p.py: a rank maps its own buffers)
        assert p.get_option("p2p_open") == 1
        p.p2p_render(P, True)
        p.point_pass(P)
        before = state()
        for kw in (dict(planes=reg["octant"]), dict(P=P2, rect=(10, 10, 300, 200), op="add"), dict(planes=reg["half"], op="toggle", stats=False)):
            p.select_points(**kw)
        assert same(before, state()) and p.get_option("p2p_open") == 1
        p.p2p_close()
        # queued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.select_points(planes=reg["oblique"], stats=False)
        p.select_points(P=P, rect=(0, 0, W, H), op="intersect")
        p.wait_outputs(0)
        ref = orc.project(xyzw, rgba, P2, W, H)
        assert np.array_equal(depth.view(np.uint32), ref["depth_bits"]) and np.array_equal(img, ref["img"])
        # the context's own clip planes and keep mask play no part
        want = sr.inside(pkg, orc, xyzw, reg["octant"])
        p.set_clip_planes(reg["keep_none"])
        p.set_point_keep(np.arange(n) % 3 == 0)
        _check(pkg, p, n, want, p.select_points(planes=reg["octant"]), "clip planes and keep mask in force")
        assert np.array_equal(p.clip_planes(), reg["keep_none"]) and np.array_equal(p.point_keep(), np.arange(n) % 3 == 0)
    finally:
        p.close()


def test_life_of_the_buffer(pkg, orc):
    L = pkg._lib
    n, W, H = 100_001, 64, 48
    xyzw, rgba = orc.generate("room_shell", 3, 0, n, n)
    reg = _regions(pkg, xyzw)
    want = sr.inside(pkg, orc, xyzw, reg["octant"])
    p = _new(pkg, {"point_ids": 1}, xyzw, rgba, W, H)
    try:
        def gone():
            assert p.get_option("selection") == 0 and p.selection() is None
            with pytest.raises(pkg.RtrError) as e:
                p.device_buffer(L.BUF_SELECTION)
            assert e.value.code == L.RTR_ERR_INVALID

        gone()
        m0 = p.get_option("resident_millibytes_per_point")
        p.select_points(planes=reg["octant"])
        m1 = p.get_option("resident_millibytes_per_point")
        cost = (_chunks(n) * 32 + 32) * 1000 / n  # (8 words per chunk and the four statistics words)
        assert abs((m1 - m0) - cost) <= 1
        assert p.get_option("selection") == 1
        buf = p.selection()
        assert buf.shape == ((n + 31) // 32,) and buf.typestr == "<u4"
        # survives: set_resolution, clip planes, keep mask, reorder, transform (the bits stay on the same upload indices)
        p.set_resolution(320, 240)
        p.set_clip_planes(reg["half"])
        p.set_point_keep(np.arange(n) % 2 == 0)
        p.reorder_points()
        assert p.get_option("reordered") == 1
        p.transform_points(M_RIGID, np.arange(n) < n // 2)
        assert np.array_equal(_sel(pkg, p, n), want) and p.get_option("selection") == 1
        # ... and a selection of the sorted cloud still goes by upload index
        moved = _moved(xyzw, M_RIGID, np.arange(n) < n // 2)
        _check(pkg, p, n, sr.inside(pkg, orc, moved, reg["oblique"]), p.select_points(planes=reg["oblique"]), "sorted, moved")
        m2 = p.get_option("resident_millibytes_per_point")
        p.clear_selection()
        gone()
        assert abs((m2 - p.get_option("resident_millibytes_per_point")) - cost) <= 1
        p.set_point_keep(None)
        for drop in ("upload", "append", "remove", "generate"):
            p.select_points(planes=reg["half"])
            assert p.get_option("selection") == 1
            if drop == "upload":
                p.upload_points(xyzw, rgba)
            elif drop == "append":
                p.append_points(xyzw[:100], rgba[:100])
            elif drop == "remove":
                p.remove_points(np.arange(p.num_points) % 5 != 0)
            else:
                p.generate_synthetic("room_shell", 5, 0, 5000, 5000)
            gone()
    finally:
        p.close()


def test_errors_leave_the_selection_intact(pkg, orc):
    L = pkg._lib
    n, W, H = 20_001, 64, 48
    xyzw, rgba = orc.generate("room_shell", 4, 0, n, n)
    reg = _regions(pkg, xyzw)
    f = np.float32
    P = pkg.orbit_projection(1, W, H)
    fresh = pkg.Projector(0)
    try:
        with pytest.raises(pkg.RtrError) as e:  # (no cloud)
            fresh.select_points()
        assert e.value.code == L.RTR_ERR_INVALID
        fresh.upload_points(xyzw, rgba)
        with pytest.raises(pkg.RtrError) as e:  # (P without a resolution)
            fresh.select_points(P=P, rect=(0, 0, 1, 1))
        assert e.value.code == L.RTR_ERR_INVALID and fresh.selection() is None
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        want = sr.inside(pkg, orc, xyzw, reg["oblique"])
        p.select_points(planes=reg["oblique"])
        lib, ctx = p._lib, p._ctx
        good = np.ascontiguousarray(reg["half"])
        Pm = np.ascontiguousarray(P, np.float32).reshape(16)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rect = lambda *r: np.array(r, np.int32)  # noqa: E731
        nine = np.zeros((9, 4), f) + f([1, 0, 0, 0])
        bad = [(9, vp(nine), None, None, 0), (-1, vp(good), None, None, 0), (1, None, None, None, 0),
               (1, vp(f([[np.nan, 0, 1, 0]])), None, None, 0), (1, vp(f([[1, 0, 0, np.inf]])), None, None, 0),
               (1, vp(f([[0, 0, 0, 1]])), None, None, 0), (0, None, vp(Pm), None, 0)]
        for r in ((-1, 0, 10, 10), (0, 0, 0, 10), (5, 5, 5, 6), (10, 0, 5, 10), (0, 0, W + 1, H), (0, 0, W, H + 1), (0, 10, 10, 10), (0, -1, 10, 10)):
            rr = rect(*r)
            bad.append((0, None, vp(Pm), vp(rr), 0, rr))
        for op in (-1, 9, 10, 11, 13, 16, 32):
            bad.append((1, vp(good), None, None, op))
        for case in bad:
            k, pl, Pp, rc, op = case[:5]
            st = np.zeros(4, np.uint64)
            assert lib.rtr_select_points(ctx, k, pl, Pp, rc, op, vp(st)) == L.RTR_ERR_INVALID, case
            assert np.array_equal(_sel(pkg, p, n), want), case
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        with pytest.raises(pkg.RtrError) as e:
            p.select_points(planes=reg["half"])
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert np.array_equal(_sel(pkg, p, n), want)
    finally:
        p.close()
