"""Selecting by distance to given points on the GPU (include/rtr.h section 6k): rtr_select_near's words, near words and
all four statistics compared exactly (np.array_equal) with the numpy float32 reference of tests/near_ref.py -- in every
form the cloud can take, with and without the near words (the early-exit path), at ragged point counts on both sides
with every op chained between rtr_select_points and rtr_select_voxel_grid calls, on pairs exactly at and one ulp beyond
the radius, on special coordinates, across the edge of the grid's span, whatever the order of the given points and
wherever they lie (host or device memory, tight or float4); chunks far from every given point are never decoded; the
given-only form and appendNewPoints; what the call must leave alone; the error paths."""
import ctypes as C

import numpy as np
import pytest

import near_cases as nc
import near_ref as nr
import select_ref as sr
import voxel_ref as vr
from test_gpu_neighbours import THREE_FORMS, _edge_cloud
from test_gpu_select import FORMS, _new, _sel
from test_near_host import span_edge_pairs

pytestmark = pytest.mark.gpu

f32 = np.float32


def _chunks(n):
    return (n + 255) // 256


def _check(pkg, p, n, G, want_sel, hit, near, got, what, with_near=True):
    st, bits = got if with_near else (got, None)
    assert st == nr.stats(hit, near if with_near else None, G, want_sel), (what, st)
    assert np.array_equal(_sel(pkg, p, n), want_sel), what
    if with_near:
        assert bits.dtype == bool and np.array_equal(bits, near), what
    assert p.get_option("near_chunks_skipped") + p.get_option("near_chunks_decoded") == _chunks(n), what


@pytest.fixture(scope="module")
def cases(orc):
    """scene -> (xyzw, rgba); case -> (given, hit, near): computed once, never changed."""
    clouds, ref = {}, {}
    for scene, n in nc.SCENES.items():
        clouds[scene] = orc.generate(scene, nc.SEED, 0, n, n)
        second = orc.generate(scene, nc.GIVEN_SEED, 0, n, n)[0]
        for case in nc.CASES:
            if case[0] == scene:
                G = np.ascontiguousarray(nc.given(case, second))
                hit, near = nr.near_bucket(clouds[scene][0], G, case[2])
                assert (G.shape[0], int(hit.sum()), int(near.sum())) == case[3:]  # (test_near_host.py: by brute force, and spread)
                ref[case] = (G, hit, near)
    return clouds, ref


@pytest.mark.parametrize("form", sorted(FORMS))
def test_words_near_words_and_stats_match_the_reference_in_every_form(pkg, cases, form):
    options, sort = FORMS[form]
    clouds, ref = cases
    for scene, n in nc.SCENES.items():
        xyzw, rgba = clouds[scene]
        opts = dict(options)
        if scene == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            if form == "sorted":
                assert p.get_option("reordered") == 1
            first = True
            for case in nc.CASES:
                if case[0] != scene:
                    continue
                G, hit, near = ref[case]
                for outside in (False, True):
                    got = p.select_near(G if outside else np.ascontiguousarray(G[:, :3]), case[2], outside=outside, near=True)  # (float4 and tight rows)
                    _check(pkg, p, n, G, hit != outside, hit, near, got, (form, case, outside))
                    assert p.get_option("near_given_us") > 0 and p.get_option("near_sweep_us") > 0
                    assert p.get_option("near_pair_tests_k") > 0 and p.get_option("near_chunks_decoded") > 0
                if first:  # the early-exit path: without the near words the resident words are the same
                    first = False
                    p.clear_selection()
                    st = p.select_near(G, case[2])
                    _check(pkg, p, n, G, hit, hit, None, st, (form, case, "no near words"), with_near=False)
        finally:
            p.close()


def _ragged(orc, n, count):
    rng = np.random.default_rng(1000 * n + count)
    xyzw, rgba = orc.generate("room_shell", 100 + n, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = (rng.normal(size=(n, 3)) * (0.1 if n <= 2 else 0.5)).astype(f32)
    r = 0.35 if n <= 257 else 0.12
    # the given points: half of them beside a resident point, half anywhere
    G = np.where((np.arange(count) % 2 == 0)[:, None], xyzw[rng.integers(0, n, count), :3] + rng.normal(0, r / 2, (count, 3)),
                 rng.normal(size=(count, 3)) * 1.0).astype(f32)
    return xyzw, rgba, r, G


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4099])
def test_ragged_counts_and_every_op_between_other_selections(pkg, orc, n):
    planes = f32([[1, 0, 0, 0.05]])
    some_hit = some_miss = False
    for count in (0, 1, 63, 64, 65, 257):
        xyzw, rgba, r, G = _ragged(orc, n, count)
        hit, near = nr.near_brute(xyzw, G, r)
        some_hit, some_miss = some_hit or hit.any(), some_miss or not hit.all()
        assert count < 63 or n < 63 or (0 < hit.sum() < n and 0 < near.sum() < count)
        half = pkg.clip_keep(planes, xyzw)
        vox, _ = vr.select(xyzw, 0.25, (0.013, -0.4, 0), 1)
        for name, options, sort in THREE_FORMS:
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                sel = np.zeros(n, bool)
                for step in (("near", "replace", False), ("planes", "add"), ("near", "toggle", True), ("voxel", "subtract"),
                             ("near", "add", False), ("near", "intersect", True), ("planes", "toggle"), ("near", "subtract", False),
                             ("voxel", "add"), ("near", "intersect", False), ("near", "replace", True), ("near", "toggle", False)):
                    if step[0] == "planes":
                        sel = sr.combine(step[1], sel, half)
                        assert p.select_points(planes=planes, op=step[1])[0] == int(sel.sum())
                    elif step[0] == "voxel":
                        sel = sr.combine(step[1], sel, vox)
                        assert p.select_voxel_grid(0.25, (0.013, -0.4, 0), op=step[1])[0] == int(sel.sum())
                    else:
                        _, op, outside = step
                        sel = sr.combine(op, sel, hit != outside)
                        got = p.select_near(G, r, op=op, outside=outside, near=True)
                        _check(pkg, p, n, G, sel, hit, near, got, (n, count, name, step))  # (_sel: no bit at or past n)
                        continue
                    assert np.array_equal(_sel(pkg, p, n), sel), (n, count, name, step)
                # the combining ops on a selection that does not exist yet: it counts as empty; stats=False still waits
                for op, want in (("add", hit), ("subtract", np.zeros(n, bool)), ("intersect", np.zeros(n, bool)), ("toggle", hit),
                                 ("replace", hit)):
                    p.clear_selection()
                    assert p.select_near(G, r, op=op, stats=False) is None
                    assert p.get_option("selection") == 1, "created"  # (count == 0 with REPLACE: an empty selection, created)
                    assert np.array_equal(_sel(pkg, p, n), want), (op, count)
            finally:
                p.close()
    assert some_hit and (some_miss or n <= 2)


def test_the_threshold_is_exact_on_both_sides(pkg, orc):
    xyz, r, want = _edge_cloud()  # (test_gpu_neighbours: 2160 isolated pairs at, and one ulp beyond, the radius)
    ends = (xyz[0::2], xyz[1::2])
    want = want[0::2]
    assert want.sum() * 2 == want.size == 2160
    for a, g in ((0, 1), (1, 0)):  # (the direction of the subtraction does not matter)
        A, G = ends[a], np.ascontiguousarray(ends[g])
        n = A.shape[0]
        hit, near = nr.near_brute(A, G, r)
        assert np.array_equal(hit, want) and np.array_equal(near, want)  # (every pair alone: near or not)
        xyzw, rgba = orc.generate("room_shell", 9, 0, n, n)
        xyzw = xyzw.copy()
        xyzw[:, :3] = A
        for name, options, sort in THREE_FORMS:
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                _check(pkg, p, n, G, hit, hit, near, p.select_near(G, r, near=True), (name, a))
                _check(pkg, p, n, G, ~hit, hit, near, p.select_near(G, r, outside=True, near=True), (name, a))
                _check(pkg, p, n, G, hit, hit, None, p.select_near(G, r), (name, a), with_near=False)
            finally:
                p.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_special_coordinates_on_either_side(pkg, orc, axis):
    n, m = 4099, 600
    xyzw, rgba = orc.generate("room_shell", 300 + axis, 0, n, n)
    xyzw = xyzw.copy()
    rng = np.random.default_rng(axis)
    at = rng.choice(np.arange(300, 1500), 16, replace=False)
    big = np.finfo(f32).max
    xyzw[at[:9], axis] = np.tile(f32([np.nan, np.inf, -np.inf]), 3)
    xyzw[at[9:13], axis] = f32([1e30, -1e30, big, -big])  # (finite and far beyond the span: legal on the resident side)
    G = (xyzw[rng.choice(np.arange(1500, n), m, replace=False), :3] + rng.normal(0, 0.05, (m, 3))).astype(f32)  # (beside ordinary points)
    G[:9] = xyzw[at[:9], :3]  # coincident with the non-finite resident points: near nothing all the same
    G[9:12, (axis + 1) % 3] = f32([np.nan, np.inf, -np.inf])
    G[12] = xyzw[at[14], :3]  # coincident with a finite resident point: near it, there is no self-exclusion
    r = 0.15
    hit, near = nr.near_brute(xyzw, G, r)
    bad = np.zeros(n, bool)
    bad[at[:13]] = True
    assert not hit[bad].any() and not near[:12].any() and near[12] and hit[at[14]] and 0 < hit.sum() < n and 0 < near.sum() < m
    for name, options, sort in THREE_FORMS + (("hash", {"auto_reorder": 0, "pack": 2}, False),):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            got = p.select_near(G, r, near=True)
            _check(pkg, p, n, G, hit, hit, near, got, (axis, name))
            assert got[0][3] == 12
            got = p.select_near(G, r, outside=True, near=True)
            _check(pkg, p, n, G, ~hit, hit, near, got, (axis, name, "outside"))
            assert _sel(pkg, p, n)[bad].all()
            # given points that are all non-finite: nothing is near anything
            st, bits = p.select_near(G[:12], r, near=True)
            assert st == (0, 0, 0, 12) and not bits.any() and p.get_option("near_chunks_skipped") == _chunks(n)
        finally:
            p.close()
    # a finite GIVEN coordinate beyond the span fails the call before anything changes
    far = {"1e30": 1e30, "FLT_MAX": big, "-FLT_MAX": -big, "beyond": 2.0 ** 20 * r * 1.0011, "-beyond": -(2.0 ** 20) * r * 1.0011}
    p = _new(pkg, {}, xyzw, rgba)
    try:
        want, _ = vr.select(xyzw, 0.25)
        for what, v in far.items():
            moved = G.copy()
            moved[77, axis] = f32(v)
            p.select_voxel_grid(0.25, stats=False)
            with pytest.raises(pkg.RtrError) as e:
                p.select_near(moved, r, near=True)
            assert e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED and "span" in str(e.value), what
            assert np.array_equal(_sel(pkg, p, n), want) and p.get_option("selection") == 1, what
            p.clear_selection()
            with pytest.raises(pkg.RtrError):
                p.select_near(moved, r, op="add")
            assert p.get_option("selection") == 0 and p.selection() is None, what
        # a given coordinate within 2^20 radius of the origin is inside the span
        edge = G.copy()
        edge[77, axis], edge[78, axis] = f32(2.0 ** 20 * r), f32(-(2.0 ** 20) * r)
        h2, n2 = nr.near_brute(xyzw, edge, r)
        _check(pkg, p, n, edge, h2, h2, n2, p.select_near(edge, r, near=True), (axis, "edge of the span"))
    finally:
        p.close()


@pytest.mark.parametrize("radius", [0.05, 1.0, 0.37])
def test_resident_points_across_the_edge_of_the_span(pkg, orc, radius):
    A, G, (qa, qg) = span_edge_pairs(radius)  # (test_near_host.py: the reference on them)
    n = A.shape[0]
    hit, near = nr.near_brute(A, G, radius)
    beyond = ((qa < -(2 ** 20 - 1)) | (qa > 2 ** 20 - 2)).any(axis=1)
    assert (hit & beyond).any() and (~hit & beyond).any()
    xyzw, rgba = orc.generate("room_shell", 5, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = A
    G = np.ascontiguousarray(G)
    for name, options, sort in THREE_FORMS + (("hash", {"auto_reorder": 0, "pack": 2}, False),):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(pkg, p, n, G, hit, hit, near, p.select_near(G, radius, near=True), (name, radius))
            _check(pkg, p, n, G, hit, hit, None, p.select_near(G, radius), (name, radius), with_near=False)
        finally:
            p.close()
    # one resident point per chunk beyond the span, the chunks' boxes reaching across its edge: a larger cloud around them
    m = 4099
    more, rgba = orc.generate("room_shell", 6, 0, m, m)
    more = more.copy()
    more[::41][:n, :3] = A
    h2, n2 = nr.near_brute(more, G, radius)
    assert np.array_equal(h2[::41][:n], hit)
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, more, rgba, sort=sort)
        try:
            _check(pkg, p, m, G, h2, h2, n2, p.select_near(G, radius, near=True), (name, radius, "mixed"))
        finally:
            p.close()


def test_chunks_far_from_the_given_points_are_never_decoded(pkg, orc):
    n = 120_001
    xyzw, rgba = orc.generate("room_shell", 7, 0, n, n)
    centre = xyzw[777, :3]
    G = np.ascontiguousarray(xyzw[np.linalg.norm(xyzw[:, :3] - centre, axis=1) < 0.4, :3] + f32(0.003))
    two = np.concatenate([G, G[:50] - 2 * (centre - xyzw[:, :3].mean(axis=0))]).astype(f32)  # (a second spot: the box between is empty)
    r = 0.03
    for given in (G, two):
        hit, near = nr.near_bucket(xyzw, given, r)
        assert 0 < hit.sum() < n // 20 and near.sum() > 0
        for name, options, sort in (("sorted", {"point_ids": 1}, True), ("sorted_unpacked", {"point_ids": 1, "pack": 0}, True)):
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                _check(pkg, p, n, given, hit, hit, near, p.select_near(given, r, near=True), name)
                skipped, decoded = p.get_option("near_chunks_skipped"), p.get_option("near_chunks_decoded")
                # the given points fill a ball of radius 0.4 (and a second, smaller spot) of a room of 8 x 3 x 8, and the chunks
                # of a Morton-sorted cloud are compact: most of them are nowhere near
                assert decoded >= 1 and skipped > 0.5 * _chunks(n), (name, skipped, decoded)
            finally:
                p.close()


def test_the_order_and_the_memory_of_the_given_points_do_not_matter(pkg, orc):
    import torch
    L = pkg._lib
    n, m = 40_001, 3001
    xyzw, rgba = orc.generate("room_shell", 7, 0, n, n)
    G = np.ascontiguousarray(orc.generate("room_shell", 8, 0, n, n)[0][:m])
    G[100:200] = G[:100]  # (copies: each has its own bit)
    r = 0.06
    hit, near = nr.near_bucket(xyzw, G, r)
    assert 0.05 * n < hit.sum() < 0.95 * n and 0.05 * m < near.sum() < 0.95 * m
    perm = np.random.default_rng(1).permutation(m)
    got = {name: _new(pkg, options, xyzw, rgba, sort=sort) for name, options, sort in THREE_FORMS}
    try:
        for name, p in got.items():
            _check(pkg, p, n, G, hit, hit, near, p.select_near(G, r, near=True), name)
            st, bits = p.select_near(G[perm], r, near=True)
            assert np.array_equal(bits, near[perm]) and np.array_equal(_sel(pkg, p, n), hit), name
            # device memory: the given points as a torch tensor, float4 rows and tight ones
            for rows in (torch.from_numpy(G).cuda(), torch.from_numpy(np.ascontiguousarray(G[:, :3])).cuda()):
                p.clear_selection()
                _check(pkg, p, n, G, hit, hit, near, p.select_near(rows, r, near=True), (name, "device"))
            # the near words into device memory, over the C ABI
            dev = torch.full(((m + 31) // 32 + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            st = np.zeros(4, np.uint64)
            assert p._lib.rtr_select_near(p._ctx, C.c_void_p(G.ctypes.data), 16, m, r, 0, 0, C.c_void_p(dev.data_ptr()),
                                          st.ctypes.data_as(C.c_void_p)) == L.RTR_OK
            words = dev.cpu().numpy().view(np.uint32)
            assert np.array_equal(words[:-1], nr.words(near)) and words[-1] == 0x5A5A5A5A, name
            assert tuple(int(v) for v in st) == nr.stats(hit, near, G, hit)
        words = [p.download(L.BUF_SELECTION) for p in got.values()]
        assert np.array_equal(words[0], words[1]) and np.array_equal(words[0], words[2])
    finally:
        for p in got.values():
            p.close()


def test_given_only_and_append_new_points(pkg, orc):
    n, m = 30_001, 4003
    xyzw, rgba = orc.generate("room_shell", 15, 0, n, n)
    g2, c2 = orc.generate("room_shell", 16, 0, n, n)
    G, Gc = np.ascontiguousarray(g2[:m]), np.ascontiguousarray(c2[:m])
    r = 0.05
    hit, near = nr.near_bucket(xyzw, G, r)
    assert 0.05 * m < near.sum() < 0.95 * m
    # a cloud sorted WITHOUT point_ids: the given side needs no upload order, the resident side does
    p = _new(pkg, {}, xyzw, rgba, sort=True)
    try:
        assert p.get_option("reordered") == 1
        st, bits = p.select_near(G, r, given_only=True)
        assert st == (0, 0, int(near.sum()), 0) and np.array_equal(bits, near)
        assert p.get_option("selection") == 0 and p.selection() is None  # (neither read, changed nor created)
        with pytest.raises(pkg.RtrError) as e:
            p.select_near(G, r)
        assert e.value.code == pkg._lib.RTR_ERR_INVALID and "point_ids" in str(e.value) and p.get_option("selection") == 0
    finally:
        p.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        # the keep mask, the clip planes and the selection play no part on the given side, and stay
        keep = np.arange(n) % 3 != 0
        p.set_point_keep(keep)
        p.set_clip_planes(f32([[1, 0, 0, 0]]))
        p.select_points(planes=f32([[0, 1, 0, 0]]), stats=False)
        before = _sel(pkg, p, n)
        assert 0 < before.sum() < n
        assert np.array_equal(p.select_near(G, r, given_only=True, stats=False), near)
        assert np.array_equal(_sel(pkg, p, n), before) and np.array_equal(p.point_keep(), keep)
    finally:
        p.close()
    for form in ("default", "sorted"):
        options, sort = FORMS[form]
        pc = pkg.ProjectCloud(xyzw, rgba, reorder=sort, point_ids=sort)
        assert pc.selectNear(G, r) == int(hit.sum()) == pc.selectedCount()
        assert np.array_equal(pc.projector.download(pkg._lib.BUF_SELECTION), nr.words(hit))
        new = int((~near).sum())
        assert pc.appendNewPoints(G, Gc, r) == new and pc.projector.num_points == n + new
        xyz, rgb = pc.projector.extract_points()[:2]
        assert np.array_equal(np.ascontiguousarray(xyz[n:, :3]).view(np.uint32), np.ascontiguousarray(G[~near, :3]).view(np.uint32))
        assert np.array_equal(rgb[n:, :3], Gc[~near, :3]) and np.array_equal(np.ascontiguousarray(xyz[:n, :3]), xyzw[:, :3])
        # the scan again adds nothing, and leaves the selection alone
        pc.selectNear(G[:10], r)
        sel = pc.projector.download(pkg._lib.BUF_SELECTION).copy()
        assert pc.appendNewPoints(G, Gc, r) == 0 and pc.projector.num_points == n + new
        assert np.array_equal(pc.projector.download(pkg._lib.BUF_SELECTION), sel)


def test_the_call_moves_nothing_else(pkg, orc):
    L = pkg._lib
    n, W, H = 60_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 88, 0, n, n)
    G = np.ascontiguousarray(orc.generate("room_shell", 89, 0, n, n)[0][:5003])
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
        for kw in (dict(radius=0.05), dict(radius=0.09, op="add", near=True), dict(radius=0.05, op="toggle", outside=True, stats=False),
                   dict(radius=0.07, given_only=True)):
            hit, near = nr.near_bucket(xyzw, G, kw["radius"])
            assert 0 < hit.sum() < n
            if not kw.get("given_only"):
                want = sr.combine(kw.get("op", "replace"), want, hit != kw.get("outside", False)) if want is not None else hit
            got = p.select_near(G, **kw)
            if kw.get("near") or kw.get("given_only"):
                assert np.array_equal(got[1], near), kw  # (every resident point counts, hidden and clipped ones too)
            assert np.array_equal(_sel(pkg, p, n), want), kw  # (the clip planes and the keep mask in force play no part)
        assert same(before, state()) and p.get_option("p2p_open") == 1
        p.p2p_close()
        p.set_clip_planes(None)
        p.set_point_keep(None)
        # issued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.select_near(G, 0.05)
        p.wait_outputs(0)
        o = orc.project(xyzw, rgba, P2, W, H)
        assert np.array_equal(depth.view(np.uint32), o["depth_bits"]) and np.array_equal(img, o["img"])
    finally:
        p.close()


def test_errors_leave_everything_intact(pkg, orc):
    L = pkg._lib
    n, m = 20_001, 1001
    xyzw, rgba = orc.generate("room_shell", 4, 0, n, n)
    G = np.ascontiguousarray(orc.generate("room_shell", 3, 0, n, n)[0][:m, :3])
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    fresh = pkg.Projector(0)
    try:
        with pytest.raises(pkg.RtrError) as e:
            fresh.select_near(G, 0.25)
        assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        want, _ = nr.near_bucket(xyzw, G, 0.1)
        assert 0 < want.sum() < n
        p.select_near(G, 0.1)
        lib, ctx = p._lib, p._ctx
        den = np.array([1], np.uint32).view(f32)[0]
        words = np.full((m + 31) // 32, 0x77777777, np.uint32)
        # (xyz, stride, count, radius, flags, op, near words, what the message names)
        bad = [(G, 12, m, v, 0, 0, words, "radius") for v in (0.0, -0.0, -0.25, np.nan, np.inf, -np.inf)]
        bad += [(G, 12, m, v, 0, 0, words, "square of radius") for v in (float(den), 1e-20, 1e-30, 2e19, 3e38)]
        bad += [(None, 12, m, 0.1, 0, 0, words, "xyz is NULL")]
        bad += [(G, s, m, 0.1, 0, 0, words, "xyz_stride_bytes") for s in (0, 4, 8, 11, 13, 14, 18)]
        bad += [(G, 12, m, 0.1, f, 0, words, "flags") for f in (2, 3, 4, -1, 1 << 16)]
        bad += [(G, 12, m, 0.1, 0, op, words, "op") for op in (-1, 9, 10, 11, 13, 16, 32)]
        bad += [(G, 12, m, 0.1, L.NEAR_GIVEN_ONLY, op, words, "RTR_NEAR_GIVEN_ONLY") for op in (1, 2, 3, 4, 8)]
        bad += [(G, 12, m, 0.1, L.NEAR_GIVEN_ONLY, 0, None, "near_words is NULL")]
        for case in bad:
            st = np.full(4, 77, np.uint64)
            rc = lib.rtr_select_near(ctx, vp(case[0]), case[1], case[2], case[3], case[4], case[5], vp(case[6]), vp(st))
            assert rc == L.RTR_ERR_INVALID, case[1:6]
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_select_near" in text and case[7] in text, (case[1:6], text)
            assert np.array_equal(_sel(pkg, p, n), want) and p.get_option("selection") == 1, case[1:6]
            assert (st == 77).all() and (words == 0x77777777).all(), case[1:6]
        # 2^32 given points or more
        st = np.full(4, 77, np.uint64)
        assert lib.rtr_select_near(ctx, vp(G), 12, 2 ** 32, 0.1, 0, 0, vp(words), vp(st)) == L.RTR_ERR_UNSUPPORTED
        assert np.array_equal(_sel(pkg, p, n), want) and (st == 77).all() and (words == 0x77777777).all()
        # count == 0: xyz may be NULL, nothing is near anything
        assert lib.rtr_select_near(ctx, None, 12, 0, 0.1, 0, 0, None, vp(st)) == L.RTR_OK
        assert tuple(st) == (0, 0, 0, 0) and not _sel(pkg, p, n).any() and p.get_option("near_chunks_skipped") == _chunks(n)
        p.select_near(G, 0.1)
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        with pytest.raises(pkg.RtrError) as e:
            p.select_near(G, 0.1)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert np.array_equal(_sel(pkg, p, n), want)
        # an error on a context without a selection makes none
        p.clear_selection()
        assert lib.rtr_select_near(ctx, vp(G), 12, m, -1.0, 0, 0, None, None) == L.RTR_ERR_INVALID and p.selection() is None
        assert p.get_option("selection") == 0
    finally:
        p.close()
