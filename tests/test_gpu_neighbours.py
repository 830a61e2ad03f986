"""Selecting by neighbour count on the GPU (include/rtr.h section 6h): rtr_select_neighbours' words and all four
statistics compared exactly (np.array_equal) with the numpy float32 reference of tests/neighbours_ref.py -- in every
form the cloud can take, at ragged point counts with every op chained between rtr_select_points and
rtr_select_voxel_grid calls, on pairs exactly at and one ulp beyond the radius, on coincident piles, on special
coordinates and beyond the grid's span, whatever the resident order; the words fed to rtr_remove_points /
rtr_set_point_keep and the facade's removeOutliers against an upload of A[hit] and the oracle, frame for frame; what the
call must leave alone; the error paths."""
import ctypes as C

import numpy as np
import pytest

import neighbours_cases as nc
import neighbours_ref as nr
import select_ref as sr
import voxel_ref as vr
from test_gpu_select import FORMS, _new, _sel
from test_gpu_voxel import _frames, _same_frames

pytestmark = pytest.mark.gpu

f32 = np.float32
THREE_FORMS = (("packed", {}, False), ("unpacked", {"pack": 0}, False), ("sorted", {"point_ids": 1}, True))


@pytest.fixture(scope="module")
def clouds(orc):
    """scene -> (xyzw, rgba, {radius -> neighbours_ref.counts}): computed once, never changed."""
    out = {}
    for scene, (n, radii) in nc.SCENES.items():
        xyzw, rgba = orc.generate(scene, nc.SEED, 0, n, n)
        out[scene] = (xyzw, rgba, {r: nr.counts(xyzw, r) for r in radii})
    return out


def _check(pkg, p, n, want, ref_stats, st, what):
    assert st == (int(want.sum()),) + tuple(ref_stats), (what, st, ref_stats)
    assert np.array_equal(_sel(pkg, p, n), want), what


@pytest.mark.parametrize("form", sorted(FORMS))
def test_words_and_stats_match_the_reference_in_every_form(pkg, clouds, form):
    options, sort = FORMS[form]
    for scene, (n, radii) in nc.SCENES.items():
        xyzw, rgba, cnts = clouds[scene]
        opts = dict(options)
        if scene == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            if form == "sorted":
                assert p.get_option("reordered") == 1
            for r in radii:
                for k, pinned in zip(nc.KS, nc.PINS[(scene, r)]):
                    hit, ref = nr.select(xyzw, r, k, cnts[r])
                    assert ref[0] == pinned  # (test_neighbours_host.py: pinned and spread without a GPU)
                    for outside in (False, True):
                        st = p.select_neighbours(r, k, outside=outside)
                        _check(pkg, p, n, hit != outside, ref, st, (form, scene, r, k, outside))
            assert p.get_option("neighbours_keys_us") > 0 and p.get_option("neighbours_sort_us") > 0
            assert p.get_option("neighbours_count_us") > 0
        finally:
            p.close()


def _ragged(orc, n):
    rng = np.random.default_rng(100 + n)
    xyzw, rgba = orc.generate("room_shell", 100 + n, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = (rng.normal(size=(n, 3)) * (0.1 if n <= 2 else 0.5)).astype(f32)
    return xyzw, rgba, (0.35 if n <= 257 else 0.12)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4099])
def test_ragged_counts_and_every_op_between_other_selections(pkg, orc, n):
    xyzw, rgba, r = _ragged(orc, n)
    cnt = nr.counts(xyzw, r)
    nb = {k: nr.select(xyzw, r, k, cnt) for k in (1, 2, 5)}
    assert n < 63 or 0 < nb[5][0].sum() < nb[2][0].sum() < nb[1][0].sum() < n
    assert n != 2 or nb[1][0].all()
    planes = f32([[1, 0, 0, 0.05]])
    half = pkg.clip_keep(planes, xyzw)
    vox, _ = vr.select(xyzw, 0.25, (0.013, -0.4, 0), 1)
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            sel = np.zeros(n, bool)
            for step in (("nb", 1, "replace", False), ("planes", "add"), ("nb", 2, "toggle", True), ("voxel", "subtract"),
                         ("nb", 5, "add", False), ("nb", 1, "intersect", True), ("planes", "toggle"), ("nb", 2, "subtract", False),
                         ("voxel", "add"), ("nb", 5, "intersect", False), ("nb", 2, "replace", True), ("nb", 1, "toggle", False)):
                if step[0] == "planes":
                    sel = sr.combine(step[1], sel, half)
                    assert p.select_points(planes=planes, op=step[1])[0] == int(sel.sum())
                elif step[0] == "voxel":
                    sel = sr.combine(step[1], sel, vox)
                    assert p.select_voxel_grid(0.25, (0.013, -0.4, 0), op=step[1])[0] == int(sel.sum())
                else:
                    _, k, op, outside = step
                    hit, ref = nb[k]
                    sel = sr.combine(op, sel, hit != outside)
                    st = p.select_neighbours(r, k, op=op, outside=outside)
                    _check(pkg, p, n, sel, ref, st, (n, name, step))  # (_sel: no bit at or past n)
                    continue
                assert np.array_equal(_sel(pkg, p, n), sel), (n, name, step)
            # the combining ops on a selection that does not exist yet: it counts as empty; stats=False still waits
            for op, want in (("add", nb[1][0]), ("subtract", np.zeros(n, bool)), ("intersect", np.zeros(n, bool)), ("toggle", nb[1][0])):
                p.clear_selection()
                assert p.select_neighbours(r, 1, op=op, stats=False) is None
                assert np.array_equal(_sel(pkg, p, n), want), op
        finally:
            p.close()


def _edge_cloud():
    """Isolated pairs at radius 13/256 (exact in fp32, as is its square): along an axis at exactly the radius (hit) and one
    ulp of the coordinate further -- two where the difference rounds back -- (miss); on the diagonal (3, 4, 12) / 256,
    whose d2 is exactly r2 (hit), and with its long component an ulp longer (miss); and diagonals whose rounded d2 is
    r2 (hit) and exactly one ulp of d2 more (miss).  120 offsets per lane, 47/256 apart, from -11 to +11, one pair across coordinate 0 and one ending
    on it: whatever the cell edge is, many pairs straddle a cell face.  Returns xyz, radius, the expected hit."""
    r = f32(13 / 256)
    pts, want = [], []
    lane = 0
    for a in range(3):
        for diag in (False, True):
            for miss in (False, True):
                lane += 1
                for g in range(120):
                    A = np.zeros(3, f32)
                    A[a] = f32((g - 60) * 47 / 256 - (6 if g % 2 == 0 else 0) / 256)
                    A[(a + 1) % 3] = f32(4 * lane)
                    A[(a + 2) % 3] = f32(-3)
                    sign = f32(1 if g % 4 < 2 else -1)
                    B = A.copy()
                    if diag:
                        B[a] = A[a] + sign * f32(12 / 256)
                        B[(a + 1) % 3] += f32(3 / 256) * sign
                        B[(a + 2) % 3] -= f32(4 / 256)
                    else:
                        B[a] = A[a] + sign * r
                    while miss and nr._d2(A, B) <= nr.r2_of(r):  # (one ulp of B; two where fp32 cannot tell the first)
                        B[a] = np.nextafter(B[a], f32(np.inf) * sign)
                    pts += [A, B]
                    want += [not miss, not miss]
        # d2 one ulp over r2: the 4/256 component longer by 3 * 2^-29 adds 6 * 2^-35 to the sum, 0.75 ulp of r2 (every
        # other operation is exact); the fine component starts at 0, where fp32 resolves it
        for miss in (False, True):
            for g in range(120):
                A = np.zeros(3, f32)
                A[a] = f32((g - 60) * 47 / 256 - (1 if g % 2 == 0 else 0) / 256)
                A[(a + 2) % 3] = f32(-9 if miss else -6)
                sign = f32(1 if g % 4 < 2 else -1)
                B = A.copy()
                B[a] = A[a] + sign * f32(3 / 256)
                B[(a + 1) % 3] = sign * (f32(2.0 ** -6) + (f32(3 * 2.0 ** -29) if miss else f32(0)))
                B[(a + 2) % 3] = A[(a + 2) % 3] - sign * f32(12 / 256)
                pts += [A, B]
                want += [not miss, not miss]
    return np.array(pts, f32), r, np.array(want)


def test_the_threshold_is_exact_on_both_sides(pkg, orc):
    xyz, r, want = _edge_cloud()
    n = xyz.shape[0]
    cnt = nr.counts_brute(xyz, r)
    assert np.array_equal(cnt, want.astype(np.int64))  # (the reference: every pair alone, a neighbour or none)
    d2 = nr._d2(xyz[0::2], xyz[1::2])
    r2 = nr.r2_of(r)
    assert (d2[want[0::2]] == r2).all() and (d2[~want[0::2]] > r2).all()
    assert (d2[~want[0::2]] == np.nextafter(r2, f32(1))).sum() >= 360  # (... 360 of them by one ulp of d2 itself)
    assert (xyz[0::2].min(axis=1)[want[0::2]] < 0).any() and (np.sign(xyz[0::2]) != np.sign(xyz[1::2])).any()
    xyzw, rgba = orc.generate("room_shell", 9, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = xyz
    hit, ref = nr.select(xyzw, r, 1, cnt)
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(pkg, p, n, hit, ref, p.select_neighbours(r, 1), name)
            _check(pkg, p, n, ~hit, ref, p.select_neighbours(r, 1, outside=True), name)
            assert p.select_neighbours(r, 2)[:3] == (0, 0, int((~hit).sum()))
        finally:
            p.close()


def test_coincident_piles(pkg, orc):
    n = 3000 + 65 + 500
    xyzw, rgba = orc.generate("room_shell", 12, 0, n, n)
    xyzw = xyzw.copy()
    rng = np.random.default_rng(2)
    at = rng.permutation(n)
    big, small = at[:3000], at[3000:3065]
    xyzw[big, :3] = f32([0.7, -0.3, 1.9])
    xyzw[small, :3] = f32([-2.5, 0.25, -0.004])
    rest = at[3065:]
    xyzw[rest, :3] = (rng.uniform(-1, 1, (500, 3)) * [50, 50, 50] + [100, 0, 0]).astype(f32)  # (far from both, sparse)
    r = 0.01
    cnt = nr.counts_brute(xyzw, r)
    assert (cnt[big] == 2999).all() and (cnt[small] == 64).all() and cnt[rest].max() == 0
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for k in (1, 64, 65, 2999, 3000):
                hit, ref = nr.select(xyzw, r, k, cnt)
                assert hit[big].all() == (k <= 2999) and hit[small].all() == (k <= 64) and not hit[rest].any()
                _check(pkg, p, n, hit, ref, p.select_neighbours(r, k), (name, k))
                assert ref[1] == 500
        finally:
            p.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_special_coordinates(pkg, orc, axis):
    n = 4099
    xyzw, rgba = orc.generate("room_shell", 300 + axis, 0, n, n)
    xyzw = xyzw.copy()
    rng = np.random.default_rng(axis)
    at = rng.choice(np.arange(300, 1500), 12, replace=False)
    xyzw[at[:9], axis] = np.tile(f32([np.nan, np.inf, -np.inf]), 3)
    xyzw[at[3:6], (axis + 1) % 3] = xyzw[at[3], (axis + 1) % 3]  # (three of them also share their other coordinates)
    xyzw[at[3:6], (axis + 2) % 3] = xyzw[at[3], (axis + 2) % 3]
    bad = np.zeros(n, bool)
    bad[at[:9]] = True
    r = 0.15
    cnt = nr.counts(xyzw, r)
    assert (cnt[bad] == 0).all()
    far = {"1e30": 1e30, "-1e30": -1e30, "FLT_MAX": np.finfo(f32).max, "-FLT_MAX": -np.finfo(f32).max, "beyond": 2.0 ** 20 * r * 1.0011,
           "-beyond": -(2.0 ** 20) * r * 1.0011}
    for name, options, sort in THREE_FORMS + (("hash", {"auto_reorder": 0, "pack": 2}, False),):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for k in (1, 3):
                hit, ref = nr.select(xyzw, r, k, cnt)
                assert 0 < hit.sum() < n - 9 and ref[2] == 9
                st = p.select_neighbours(r, k)
                _check(pkg, p, n, hit, ref, st, (axis, name, k))
                assert not _sel(pkg, p, n)[bad].any()
                st = p.select_neighbours(r, k, outside=True)
                _check(pkg, p, n, ~hit, ref, st, (axis, name, k, "outside"))
                assert _sel(pkg, p, n)[bad].all()
        finally:
            p.close()
    # a coordinate within 2^20 radius of the origin is inside the span; a finite one beyond the span fails the call
    edge = xyzw.copy()
    edge[at[9], axis], edge[at[10], axis] = f32(2.0 ** 20 * r), f32(-(2.0 ** 20) * r)
    with np.errstate(invalid="ignore"):
        cnt_edge = nr.counts_brute(edge, r)
    p = _new(pkg, {}, edge, rgba)
    try:
        hit, ref = nr.select(edge, r, 1, cnt_edge)
        _check(pkg, p, n, hit, ref, p.select_neighbours(r, 1), (axis, "edge of the span"))
    finally:
        p.close()
    for what, v in far.items():
        moved = xyzw.copy()
        moved[at[11], axis] = f32(v)
        p = _new(pkg, {}, moved, rgba)
        try:
            want, _ = vr.select(moved, 0.25)
            p.select_voxel_grid(0.25, stats=False)
            with pytest.raises(pkg.RtrError) as e:
                p.select_neighbours(r, 1)
            assert e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED and "span" in str(e.value), what
            assert np.array_equal(_sel(pkg, p, n), want) and p.get_option("selection") == 1, what
            p.clear_selection()
            with pytest.raises(pkg.RtrError):
                p.select_neighbours(r, 1, op="add")
            assert p.get_option("selection") == 0 and p.selection() is None, what
        finally:
            p.close()


def test_same_words_in_every_resident_order(pkg, orc):
    n = 40_001
    xyzw, rgba = orc.generate("room_shell", 7, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[5000:5100] = xyzw[:100]
    xyzw[35_000:35_100] = xyzw[:100]
    got = {name: _new(pkg, options, xyzw, rgba, sort=sort) for name, options, sort in THREE_FORMS}
    try:
        assert got["sorted"].get_option("reordered") == 1 and got["packed"].get_option("reordered") == 0
        assert got["packed"].get_option("packed") == 1 and got["unpacked"].get_option("packed") == 0
        for r in (1e-4, 0.07):
            cnt = nr.counts(xyzw, r)
            assert (cnt[:100] >= 2).all() and (cnt[5000:5100] >= 2).all()  # (the copies are neighbours of each other)
            for k in (1, 2, 3, 4):
                hit, ref = nr.select(xyzw, r, k, cnt)
                if r == 1e-4:  # (a radius so small that only the copies have neighbours: two each)
                    assert hit.sum() == (300 if k <= 2 else 0)
                for name, p in got.items():
                    _check(pkg, p, n, hit, ref, p.select_neighbours(r, k), (name, r, k))
                words = [p.download(pkg._lib.BUF_SELECTION) for p in got.values()]
                assert np.array_equal(words[0], words[1]) and np.array_equal(words[0], words[2])
    finally:
        for p in got.values():
            p.close()


@pytest.mark.parametrize("form", ["default", "sorted"])
def test_the_words_clean_the_cloud(pkg, orc, form):
    options, sort = FORMS[form]
    n, W, H = 120_001, 320, 240
    r, k = 0.05, 3
    xyzw, rgba = orc.generate("room_shell", 52, 0, n, n)
    hit, ref = nr.select(xyzw, r, k)
    assert n // 4 < hit.sum() < 3 * n // 4
    Ps = [pkg.orbit_projection(j, W, H) for j in (5, 130, 420, 777)]
    b = _new(pkg, {}, xyzw[hit], rgba[hit], W, H)
    try:
        want = _frames(pkg, b, Ps)
        # the oracle on A[hit], at 64 x 48
        small = pkg.orbit_projection(130, 64, 48)
        b.set_resolution(64, 48)
        img, depth = b.project(small, filtered=False)
        o = orc.project(xyzw[hit], rgba[hit], small, 64, 48)
        assert np.array_equal(depth.view(np.uint32), o["depth_bits"]) and np.array_equal(img, o["img"])
        # the outliers' words, complemented on the device, as the keep words of remove_points
        a = _new(pkg, options, xyzw, rgba, W, H, sort=sort)
        try:
            assert a.select_neighbours(r, k, outside=True) == (int((~hit).sum()),) + ref
            assert a.select_points(op="toggle")[0] == int(hit.sum())  # (no region: every point is inside)
            a.remove_points(a.selection())
            assert a.num_points == int(hit.sum()) and a.selection() is None
            _same_frames(_frames(pkg, a, Ps), want, (form, "remove"))
        finally:
            a.close()
        # through set_point_keep: hidden, not removed
        a = _new(pkg, options, xyzw, rgba, W, H, sort=sort)
        try:
            a.select_neighbours(r, k, outside=True, stats=False)
            a.select_points(op="toggle", stats=False)
            a.set_point_keep(a.selection())
            assert np.array_equal(a.point_keep(), hit) and a.num_points == n
            _same_frames(_frames(pkg, a, Ps), want, (form, "keep"), np.flatnonzero(hit))
        finally:
            a.close()
        # the facade's removeOutliers
        pc = pkg.ProjectCloud(xyzw, rgba, reorder=sort, point_ids=sort)
        assert pc.selectNeighbours(r, k) == int(hit.sum()) == pc.selectedCount()
        assert pc.removeOutliers(r, k) == int((~hit).sum()) and pc.projector.num_points == int(hit.sum())
        assert pc.projector.selection() is None and pc.selectedCount() == 0
        pc.projector.set_resolution(W, H)
        _same_frames(_frames(pkg, pc.projector, Ps), want, (form, "removeOutliers"))
    finally:
        b.close()


def test_the_call_moves_nothing_else(pkg, orc):
    L = pkg._lib
    n, W, H = 60_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 88, 0, n, n)
    P, P2 = pkg.orbit_projection(40, W, H), pkg.orbit_projection(41, W, H)
    keep = np.arange(n) % 3 != 0
    planes = f32([[0, 0, 1, 100], [1, 0, 0, 50]])
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        def state():
            return [p.download(b).copy() for b in (L.BUF_DEPTH, L.BUF_IMAGE, L.BUF_TENSOR, L.BUF_VISIBLE, L.BUF_POINT_ID, L.BUF_POINT_KEEP)] + \
                   [p.clip_planes(), p.frame_stats(), p.get_option("p2p_open"), p.get_option("packed"), p.get_option("reordered"),
                    p.get_option("point_keep"), p.num_points, p.get_option("resident_millibytes_per_point")]

        def same(a, b):
            return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

        p.set_clip_planes(planes)
        p.set_point_keep(keep)
        p.p2p_open(0, 1, [p.p2p_export()])  # (the one-rank form of test_gpu_p2p.py: a rank maps its own buffers)
        p.p2p_render(P, True)
        p.point_pass(P)
        p.select_points(stats=False)  # (the selection's own words count as resident: they exist before the first call)
        before = state()
        want = None
        for kw in (dict(radius=0.07, min_neighbours=2), dict(radius=0.12, min_neighbours=9, op="add"),
                   dict(radius=0.07, min_neighbours=4, op="toggle", outside=True, stats=False)):
            hit, _ = nr.select(xyzw, kw["radius"], kw["min_neighbours"])
            assert 0 < hit.sum() < n
            want = sr.combine(kw.get("op", "replace"), want, hit != kw.get("outside", False)) if want is not None else hit
            p.select_neighbours(**kw)
            assert np.array_equal(_sel(pkg, p, n), want), kw  # (the clip planes and the keep mask in force play no part)
        assert same(before, state()) and p.get_option("p2p_open") == 1
        p.p2p_close()
        p.set_clip_planes(None)
        p.set_point_keep(None)
        # issued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.select_neighbours(0.07, 2)
        p.wait_outputs(0)
        o = orc.project(xyzw, rgba, P2, W, H)
        assert np.array_equal(depth.view(np.uint32), o["depth_bits"]) and np.array_equal(img, o["img"])
    finally:
        p.close()


def test_errors_leave_the_selection_intact(pkg, orc):
    L = pkg._lib
    n = 20_001
    xyzw, rgba = orc.generate("room_shell", 4, 0, n, n)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    fresh = pkg.Projector(0)
    try:
        with pytest.raises(pkg.RtrError) as e:
            fresh.select_neighbours(0.25, 1)
        assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        want, _ = nr.select(xyzw, 0.1, 2)
        assert 0 < want.sum() < n
        p.select_neighbours(0.1, 2)
        lib, ctx = p._lib, p._ctx
        den = np.array([1], np.uint32).view(f32)[0]
        bad = [(v, 1, 0, "radius") for v in (0.0, -0.0, -0.25, np.nan, np.inf, -np.inf)]
        bad += [(v, 1, 0, "square of radius") for v in (float(den), 1e-20, 1e-30, 2e19, 3e38)]  # (r2 subnormal, 0 or infinite)
        bad += [(0.1, 0, 0, "min_neighbours")]
        bad += [(0.1, 1, op, "op") for op in (-1, 9, 10, 11, 13, 16, 32)]
        for case in bad:
            st = np.full(4, 77, np.uint64)
            assert lib.rtr_select_neighbours(ctx, case[0], case[1], case[2], vp(st)) == L.RTR_ERR_INVALID, case
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_select_neighbours" in text and case[3] in text, (case, text)
            assert np.array_equal(_sel(pkg, p, n), want) and p.get_option("selection") == 1, case
            assert (st == 77).all(), case
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        with pytest.raises(pkg.RtrError) as e:
            p.select_neighbours(0.1, 2)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert np.array_equal(_sel(pkg, p, n), want)
        # an error on a context without a selection makes none
        p.clear_selection()
        assert lib.rtr_select_neighbours(ctx, 0.1, 0, 0, None) == L.RTR_ERR_INVALID and p.selection() is None
        assert p.get_option("selection") == 0
    finally:
        p.close()
