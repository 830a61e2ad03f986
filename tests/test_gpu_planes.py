"""Counting points in bands and fitting the dominant plane on the GPU (include/rtr.h section 6j): rtr_count_in_bands'
counts and statistics and rtr_fit_plane's plane, count and statistics compared exactly (np.array_equal, ==) with the
numpy references of tests/planes_ref.py, in every form the cloud can take; band counts around the pass width; ragged
sizes and non-finite points; RTR_BANDS_SELECTED after several kinds of selection; what both calls must leave alone; the
error paths.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import planes_ref as pr
import select_ref as sr
import voxel_ref as vr
from test_gpu_select import FORMS, _new, _sel, _specials

pytestmark = pytest.mark.gpu

B = 64  # the pass width (csrc/rtr_kernels.h, kBandPass)
COUNTS = (1, B - 1, B, B + 1, 2 * B + 1, 4096)
SCENES = (("room_shell", 150_001), ("uniform_box", 160_003))
FIT_SEED = 3  # (test_the_fit_cloud_and_seed_are_fair checks on the CPU that the reference alone finds the plane with it)


def _chunks(n):
    return (n + 255) // 256


def _mix(xyzw, rng, count):
    """`count` distinct bands: thin ones through three cloud points, 2 cm and 5 cm ones, slabs that swallow or miss the
    cloud, axis-aligned ones whose faces are the faces of upload-order chunk boxes, and oblique ones of every width."""
    f = np.float32
    xyz = xyzw[:, :3]
    n = len(xyz)
    out = [f([0, 0, 1, 1000, 1000]), f([0, 0, 1, -1000, 2000]), f([0.6, 0, -0.8, 500, 500]), f([1, 0, 0, -900, 901])]
    for c in rng.choice(max(_chunks(n) - 1, 1), min(12, max(_chunks(n) - 1, 1)), replace=False) if n >= 256 else ():  # (whole chunks)
        blk = xyz[256 * c:256 * c + 256]
        for a in range(3):
            e = np.zeros(3, f)
            e[a] = 1
            out.append(f([e[0], e[1], e[2], -blk[:, a].min(), blk[:, a].max()]))
    while len(out) < count:
        i = rng.choice(n, 3, replace=False)
        pl = pr.candidate(xyz[i[0]], xyz[i[1]], xyz[i[2]], [0, 1, 2])
        if pl is None:
            continue
        dist = f([0, 0.02, 0.05, 0.02, 0.05, 0.3])[len(out) % 6]
        out.append(pr.band_of(pl, dist))
        if len(out) % 7 == 0:  # (the walls and the floor: axis-aligned 2 cm / 5 cm bands through a cloud point)
            e = np.zeros(3, f)
            e[len(out) % 3] = 1
            out.append(pr.band_of(f([e[0], e[1], e[2], -xyz[i[0], len(out) % 3]]), dist))
    return np.array(out[:count], f)


@pytest.fixture(scope="module")
def clouds(orc):
    """Per scene: the cloud, 4096 bands drawn from 448 distinct ones (the first 2 B + 1 are distinct) and their counts."""
    out = {}
    for scene, n in SCENES:
        rng = np.random.default_rng(n)
        xyzw, rgba = orc.generate(scene, 41, 0, n, n)
        pool = _mix(xyzw, rng, 448)
        ref = pr.counts(xyzw[:, :3], pool)
        pick = np.concatenate([np.arange(2 * B + 1), rng.integers(0, 448, 4096 - 2 * B - 1)])
        out[scene] = (xyzw, rgba, pool[pick], ref[pick])
    return out


def test_the_reference_spreads_these_bands(clouds):
    for scene, n in SCENES:
        xyzw, _, bands, ref = clouds[scene]
        assert ref[0] == n and ref[1] == 0 and ref[2] == n  # (the slabs)
        assert ref[3] == 0 and (ref[:2 * B + 1] == 0).sum() < 40 and len(set(ref[:2 * B + 1].tolist())) > 60
        assert ref[4] >= 256  # (a chunk-box band holds its chunk at least)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_counts_and_stats_match_the_reference_in_every_form(pkg, clouds, form):
    options, sort = FORMS[form]
    for scene, n in SCENES:
        xyzw, rgba, bands, ref = clouds[scene]
        opts = dict(options)
        if scene == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            packed = p.get_option("packed")
            total = np.zeros(4, np.uint64)
            for nb in COUNTS:
                counts, st = p.count_in_bands(bands[:nb])
                assert np.array_equal(counts, ref[:nb]), (form, scene, nb, np.flatnonzero(counts != ref[:nb])[:5])
                assert st[0] == n and st[1] + st[2] + st[3] == _chunks(n) * nb, (form, scene, nb, st)
                if not packed:
                    assert st[2] == 0  # (a box of the fp32 form may hide a NaN: never inside)
                total += np.uint64(st)
            if packed:
                assert total[1] > 0 and total[2] > 0 and total[3] > 0, (form, scene, total)
            assert np.array_equal(p.count_in_bands(bands[:B + 1], stats=False), ref[:B + 1])
            assert p.selection() is None
            for k in (0, 1, 4, 5, 6, 16, 17, 18, 19, 20, 40, 41, 60, 64, 100, 128):  # rtr_select_points on the same two planes
                st = p.select_points(planes=pr.two_planes(bands[k]))
                assert st[0] == ref[k], (form, scene, k, st)
        finally:
            p.close()


def _special_cloud(orc, n, seed):
    rng = np.random.default_rng(seed)
    xyzw, rgba = orc.generate("room_shell", 100 + n, 0, n, n)
    sp = _specials()
    rows = rng.choice(n, max(1, n // 6), replace=False)
    xyzw[rows, rng.integers(0, 3, rows.size)] = rng.choice(sp, rows.size)
    if n >= 255:
        xyzw[7, :3] = [np.nan, 0.5, 0.5]  # (a NaN in a chunk whose other points lie well inside the slabs)
        xyzw[200, :3] = [0.5, np.inf, 0.5]
    return xyzw, rgba


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_ragged_sizes_and_non_finite_points(pkg, orc, n):
    xyzw, rgba = _special_cloud(orc, n, n)
    rng = np.random.default_rng(n + 1)
    clean = xyzw[np.isfinite(xyzw[:, :3]).all(axis=1) & (np.abs(xyzw[:, :3]) < 100).all(axis=1)]
    src = clean if len(clean) >= 3 else np.float32([[0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0, 1]])
    bands = np.concatenate([np.float32([[0, 0, 1, 1000, 1000], [1, 0, 0, 1e30, 1e30], [0, 1, 0, 3e38, 3e38], [0, 0, 1, -1000, 2000],
                                        [1, 1, 1, 50, 50]]), _mix(src, rng, 70)[-61:]])
    ref = pr.counts(xyzw[:, :3], bands)
    bad = ~np.isfinite(xyzw[:, :3]).all(axis=1)
    assert ref[0] <= n - np.isnan(xyzw[:, :3]).any(axis=1).sum() and (n < 255 or bad.sum() >= 2)
    for b in bands:
        assert not pr.in_band(xyzw[:, :3], b)[np.isnan(xyzw[:, :3]).any(axis=1)].any()
    cut = np.float32([[0.3, -0.2, 0.9, -(0.3 * src[0, 0] - 0.2 * src[0, 1] + 0.9 * src[0, 2])]])
    sel = sr.inside(pkg, orc, xyzw, cut)
    ref_sel = pr.counts(xyzw[:, :3], bands, sel)
    for options, sort in (({}, False), ({"pack": 0}, False), ({"point_ids": 1}, True)):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for nb in (1, 5, len(bands)):
                counts, st = p.count_in_bands(bands[:nb])
                assert np.array_equal(counts, ref[:nb]), (n, options, nb)
                assert st[0] == n and st[1] + st[2] + st[3] == _chunks(n) * nb
                if options.get("pack") == 0:
                    assert st[2] == 0
            # the flag on the same sizes: the points on one side of an oblique plane through the cloud
            assert p.select_points(planes=cut)[0] == int(sel.sum())
            counts, st = p.count_in_bands(bands, selected=True)
            assert np.array_equal(counts, ref_sel), (n, options)
            assert st[0] == int(sel.sum()) and st[1] + st[2] + st[3] == _chunks(n) * len(bands)
            assert np.array_equal(_sel(pkg, p, n), sel)
        finally:
            p.close()


def test_selected_population_after_several_selections(pkg, orc):
    n, W, H = 150_001, 160, 120
    xyzw, rgba = orc.generate("room_shell", 41, 0, n, n)
    rng = np.random.default_rng(8)
    bands = np.concatenate([np.float32([[0, 0, 1, 1000, 1000]]), _mix(xyzw, rng, 99)])
    P = pkg.orbit_projection(12, W, H)
    ref_all = pr.counts(xyzw[:, :3], bands)
    for form in ("default", "pack0", "sorted"):
        options, sort = FORMS[form]
        p = _new(pkg, options, xyzw, rgba, W, H, sort=sort)
        try:
            # no selection at all: an empty population, and none is created
            counts, st = p.count_in_bands(bands, selected=True)
            assert not counts.any() and st == (0, _chunks(n) * len(bands), 0, 0) and p.selection() is None
            # a rectangle on the screen: most chunks hold no selected point
            got = p.select_points(P=P, rect=(40, 30, 100, 90))
            sel = _sel(pkg, p, n)
            assert 0 < got[0] == sel.sum() < n // 2
            counts, st = p.count_in_bands(bands, selected=True)
            assert np.array_equal(counts, pr.counts(xyzw[:, :3], bands, sel)), form
            assert st[0] == int(sel.sum()) and st[1] + st[2] + st[3] == _chunks(n) * len(bands)
            if p.get_option("reordered") == 0:  # (upload order is the resident order: the empty chunks are known)
                pad = np.concatenate([sel, np.zeros(-n % 256, bool)]).reshape(-1, 256)
                empty = int((~pad.any(axis=1)).sum())
                assert empty > 10 and st[1] >= empty * len(bands)
                one = p.count_in_bands(bands[:1], selected=True)[1]  # (the slab that swallows the cloud: outside = empty)
                assert one[1] == empty and one[1] + one[2] + one[3] == _chunks(n)
            assert np.array_equal(p.count_in_bands(bands, stats=False), ref_all)  # (without the flag: everything)
            assert np.array_equal(_sel(pkg, p, n), sel)
            # a voxel selection
            hit, _ = vr.select(xyzw, 0.07)
            p.select_voxel_grid(0.07)
            counts, st = p.count_in_bands(bands, selected=True)
            assert np.array_equal(counts, pr.counts(xyzw[:, :3], bands, hit)) and st[0] == int(hit.sum()), form
            # an empty selection
            assert p.select_points(planes=np.float32([[0, 0, 1, -100]]))[0] == 0
            counts, st = p.count_in_bands(bands, selected=True)
            assert not counts.any() and st == (0, _chunks(n) * len(bands), 0, 0)
        finally:
            p.close()
    # a cloud sorted without point_ids: the flag is refused, the plain call works
    p = _new(pkg, {}, xyzw, rgba, W, H, sort=True)
    try:
        assert p.get_option("reordered") == 1
        with pytest.raises(pkg.RtrError) as e:
            p.count_in_bands(bands, selected=True)
        assert e.value.code == pkg._lib.RTR_ERR_INVALID and "point_ids" in str(e.value)
        counts, st = p.count_in_bands(bands)
        assert np.array_equal(counts, ref_all) and st[0] == n
    finally:
        p.close()


# ---- the fit ------------------------------------------------------------------------------------------------------------
def _fit_cloud():
    rng = np.random.default_rng(77)
    n = 100_003
    on = rng.random(n) < 0.6
    xyz = rng.uniform([-4, -3, 0], [4, 3, 2.5], (n, 3)).astype(np.float32)
    xyz[on, 2] = np.float32(0.3) + rng.uniform(-0.01, 0.01, int(on.sum())).astype(np.float32)
    xyzw = np.concatenate([xyz, np.ones((n, 1), np.float32)], axis=1)
    rgba = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    rgba[:, 3] = 255
    return xyzw, rgba, on


@pytest.fixture(scope="module")
def fit_case():
    xyzw, rgba, on = _fit_cloud()
    plane, st = pr.fit(xyzw, np.float32(0.03), 128, FIT_SEED)
    rest = ~pr.in_band(xyzw[:, :3], pr.band_of(plane, np.float32(0.03)))
    plane2, st2 = pr.fit(xyzw, np.float32(0.03), 128, FIT_SEED, rest)
    return xyzw, rgba, on, plane, st, rest, plane2, st2


def test_the_fit_cloud_and_seed_are_fair(fit_case):
    """The reference alone, on the CPU: at the pinned seed the winner holds the generated plane."""
    xyzw, rgba, on, plane, st, rest, plane2, st2 = fit_case
    assert st[0] >= 0.9 * on.sum() and st[3] == len(xyzw) and st[1] > 100
    assert plane[2] > 0.999 and abs(plane[3] + 0.3) < 0.01
    assert st2[3] == int(rest.sum()) and 0 < st2[0] < st[0] // 10


@pytest.mark.parametrize("form", ["default", "pack0", "sorted"])
def test_fit_matches_the_reference_bit_for_bit(pkg, fit_case, form):
    xyzw, rgba, on, plane, st, rest, plane2, st2 = fit_case
    options, sort = FORMS[form]
    n, dist = len(xyzw), np.float32(0.03)
    p = _new(pkg, dict(options, point_ids=1), xyzw, rgba, sort=sort)
    try:
        got, inliers, gst = p.fit_plane(dist, 128, FIT_SEED)
        assert np.array_equal(got.view(np.uint32), plane.view(np.uint32)) and gst == st and inliers == st[0], (form, got, gst, plane, st)
        assert inliers >= 0.9 * on.sum()
        assert p.selection() is None  # (no selection was created)
        # peeled: everything outside the winner's band, then the fit among the selected points
        two = pr.two_planes(pr.band_of(got, dist))
        assert p.select_points(planes=two)[0] == inliers
        assert p.select_points(planes=two, outside=True)[0] == n - inliers
        got2, inliers2, gst2 = p.fit_plane(dist, 128, FIT_SEED, selected=True)
        assert np.array_equal(got2.view(np.uint32), plane2.view(np.uint32)) and gst2 == st2, (form, got2, gst2, plane2, st2)
        assert np.array_equal(_sel(pkg, p, n), rest)
        # other shapes of the call
        for kw in (dict(dist=0.03, iterations=1, seed=9), dict(dist=0, iterations=40, seed=1), dict(dist=0.05, iterations=B + 1, seed=(1 << 64) - 1)):
            want, wst = pr.fit(xyzw, np.float32(kw["dist"]), kw["iterations"], kw["seed"])
            got, _, gst = p.fit_plane(**kw)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and gst == wst, (form, kw, gst, wst)
    finally:
        p.close()


def test_every_candidate_degenerate(pkg, orc):
    L = pkg._lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    xyzw, rgba = orc.generate("room_shell", 5, 0, 500, 500)
    same = np.repeat(xyzw[:1], 500, axis=0)
    for pts, m in ((xyzw[:2], 2), (same, 500), (xyzw[:1], 1)):
        p = _new(pkg, {}, pts, rgba[:len(pts)])
        try:
            plane, st = np.full(4, 7, np.float32), np.full(4, 7, np.uint64)
            assert p._lib.rtr_fit_plane(p._ctx, 0.03, 32, 0, 0, vp(plane), vp(st)) == L.RTR_OK
            assert not plane.any() and list(st) == [0, 0, 0, m]
            assert pr.fit(pts, 0.03, 32)[1] == (0, 0, 0, m)
            with pytest.raises(RuntimeError, match="degenerate"):
                p.fit_plane(0.03, 32)
        finally:
            p.close()
    # a population of fewer than three selected points
    p = _new(pkg, {}, xyzw, rgba)
    try:
        p.select_points(planes=np.float32([[0, 0, 1, -100]]))
        plane, st = np.full(4, 7, np.float32), np.full(4, 7, np.uint64)
        assert p._lib.rtr_fit_plane(p._ctx, 0.03, 32, 0, L.BANDS_SELECTED, vp(plane), vp(st)) == L.RTR_OK
        assert not plane.any() and list(st) == [0, 0, 0, 0]
        p.clear_selection()
        assert p._lib.rtr_fit_plane(p._ctx, 0.03, 32, 0, L.BANDS_SELECTED, vp(plane), vp(st)) == L.RTR_OK
        assert not plane.any() and list(st) == [0, 0, 0, 0] and p.selection() is None
    finally:
        p.close()


# ---- side effects and errors ----------------------------------------------------------------------------------------------
def test_the_calls_move_nothing(pkg, orc):
    L = pkg._lib
    n, W, H = 150_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 88, 0, n, n)
    P, P2 = pkg.orbit_projection(40, W, H), pkg.orbit_projection(41, W, H)
    keep = np.arange(n) % 3 != 0
    planes = np.float32([[0, 0, 1, 100], [1, 0, 0, 50]])
    rng = np.random.default_rng(3)
    bands = _mix(xyzw, rng, 70)
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        def state():
            return [p.download(b).copy() for b in (L.BUF_DEPTH, L.BUF_IMAGE, L.BUF_TENSOR, L.BUF_VISIBLE, L.BUF_POINT_ID, L.BUF_POINT_KEEP,
                                                   L.BUF_SELECTION)] + \
                   [p.clip_planes(), p.frame_stats(), p.get_option("p2p_open"), p.get_option("packed"), p.get_option("reordered"),
                    p.get_option("point_keep"), p.get_option("selection"), p.num_points]

        def same(a, b):
            return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

        p.set_clip_planes(planes)
        p.set_point_keep(keep)
        sel = sr.inside(pkg, orc, xyzw, np.float32([[1, 0, 0, 0.2]]))
        p.select_points(planes=np.float32([[1, 0, 0, 0.2]]))
        p.p2p_open(0, 1, [p.p2p_export()])  # (the one-rank form of test_gpu_p2p.py: a rank maps its own buffers)
        p.p2p_render(P, True)
        p.point_pass(P)
        before = state()
        # (the clip planes and the keep mask in force play no part)
        assert np.array_equal(p.count_in_bands(bands, stats=False), pr.counts(xyzw[:, :3], bands))
        assert np.array_equal(p.count_in_bands(bands, selected=True)[0], pr.counts(xyzw[:, :3], bands, sel))
        for selected in (False, True):
            want, wst = pr.fit(xyzw, np.float32(0.02), 24, 6, sel if selected else None)
            got, _, gst = p.fit_plane(0.02, 24, 6, selected=selected)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and gst == wst
        assert same(before, state()) and p.get_option("p2p_open") == 1
        p.p2p_close()
        p.set_clip_planes(None)
        p.set_point_keep(None)
        # issued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.count_in_bands(bands)
        p.fit_plane(0.02, 24, 6)
        p.wait_outputs(0)
        r = orc.project(xyzw, rgba, P2, W, H)
        assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(img, r["img"])
    finally:
        p.close()


def test_errors_leave_everything_untouched(pkg, orc):
    L = pkg._lib
    n = 20_001
    xyzw, rgba = orc.generate("room_shell", 4, 0, n, n)
    f = np.float32
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = f([[0, 0, 1, 0.5, 0.5], [1, 0, 0, 0.25, 0.75]])
    fresh = pkg.Projector(0)
    try:
        for call in (lambda: fresh.count_in_bands(good), lambda: fresh.fit_plane(0.03)):
            with pytest.raises(pkg.RtrError) as e:
                call()
            assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        want = sr.inside(pkg, orc, xyzw, np.float32([[1, 0, 0, 0.2]]))
        p.select_points(planes=np.float32([[1, 0, 0, 0.2]]))
        lib, ctx = p._lib, p._ctx
        big = np.tile(good[:1], (L.MAX_BANDS + 1, 1))
        bad = [(0, vp(good), 0, True, "count"), (L.MAX_BANDS + 1, vp(big), 0, True, "count"), (2, None, 0, True, "bands"),
               (2, vp(good), 0, False, "counts"), (2, vp(good), 2, True, "flags"), (2, vp(good), 3, True, "flags"),
               (2, vp(good), -1, True, "flags")]
        for v in (np.nan, np.inf, -np.inf):
            for k in range(5):
                b = good.copy(); b[1, k] = v
                bad.append((2, vp(b), 0, True, "bands", b))
        z = good.copy(); z[1, :3] = [0, -0.0, 0]
        bad.append((2, vp(z), 0, True, "a = b = c = 0", z))
        for case in bad:
            counts, st = np.full(8, 77, np.uint64), np.full(4, 77, np.uint64)
            assert lib.rtr_count_in_bands(ctx, case[0], case[1], case[2], vp(counts) if case[3] else None, vp(st)) == L.RTR_ERR_INVALID, case
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_count_in_bands" in text and case[4] in text, (case, text)
            assert (counts == 77).all() and (st == 77).all(), case
        for dist, it, flags, has_plane, name in ((-0.01, 8, 0, True, "dist"), (np.nan, 8, 0, True, "dist"), (np.inf, 8, 0, True, "dist"),
                                                 (0.03, 0, 0, True, "iterations"), (0.03, L.MAX_BANDS + 1, 0, True, "iterations"),
                                                 (0.03, 8, 2, True, "flags"), (0.03, 8, -1, True, "flags"), (0.03, 8, 0, False, "plane")):
            plane, st = np.full(4, 77, np.float32), np.full(4, 77, np.uint64)
            assert lib.rtr_fit_plane(ctx, dist, it, 0, flags, vp(plane) if has_plane else None, vp(st)) == L.RTR_ERR_INVALID, name
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_fit_plane" in text and name in text, (name, text)
            assert (plane == 77).all() and (st == 77).all(), name
        assert np.array_equal(_sel(pkg, p, n), want)
        # a cloud sorted without point_ids has lost its upload order: the flag and the sampler need it
        p.reorder_points()
        for call in (lambda: p.count_in_bands(good, selected=True), lambda: p.fit_plane(0.03), lambda: p.fit_plane(0.03, selected=True)):
            with pytest.raises(pkg.RtrError) as e:
                call()
            assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert np.array_equal(p.count_in_bands(good, stats=False), pr.counts(xyzw[:, :3], good))
        assert np.array_equal(_sel(pkg, p, n), want)
    finally:
        p.close()
