"""Selecting by connected cluster on the GPU (include/rtr.h section 6i): rtr_select_clusters' words, labels (into host and
into device memory) and all four statistics compared exactly (np.array_equal) with the numpy float32 reference of
tests/clusters_ref.py -- in every form the cloud can take, at ragged point counts with every op chained between
rtr_select_points and rtr_select_neighbours calls, seeded by a plane's selection, on long chains whose sorted order is
not their chain order, on a link one ulp too long, on coincident piles, on special coordinates and beyond the grid's
span, whatever the resident order; the facade's removeSmallClusters against an upload of A[hit] and the oracle, frame
for frame; what the call must leave alone; the error paths."""
import ctypes as C

import numpy as np
import pytest

import clusters_cases as cc
import clusters_ref as cr
import neighbours_ref as nr
import select_ref as sr
from test_gpu_select import FORMS, _new, _sel
from test_gpu_voxel import _frames, _same_frames

pytestmark = pytest.mark.gpu

f32 = np.float32
THREE_FORMS = (("packed", {}, False), ("unpacked", {"pack": 0}, False), ("sorted", {"point_ids": 1}, True))
STEP = f32(13 / 256)  # exact in fp32, as is its square


@pytest.fixture(scope="module")
def clouds(orc):
    """scene -> (xyzw, rgba, {radius -> clusters_ref.labels}): computed once, never changed."""
    out = {}
    for scene, (n, radii) in cc.SCENES.items():
        xyzw, rgba = orc.generate(scene, cc.SEED, 0, n, n)
        radii = radii + tuple(case[1] for case in (cc.EVERYTHING, cc.NOTHING) if case[0] == scene and case[1] not in radii)
        out[scene] = (xyzw, rgba, {r: cr.labels(xyzw, r) for r in radii})
    return out


def _want(lab, window, outside=False, seeds=None):
    """(the hits after OUTSIDE, stats[1..3])"""
    hit = cr.hits(lab, window[0], window[1], seeds)
    return hit != outside, cr.stats(lab, hit)


def _check(pkg, p, n, sel, ref_stats, st, what):
    assert st == (int(sel.sum()),) + tuple(ref_stats), (what, st, ref_stats)
    assert np.array_equal(_sel(pkg, p, n), sel), what


def _device_labels(p, n, radius, window, fill=0xDEADBEEF):
    """rtr_select_clusters with labels in device memory (a torch tensor): (return code, the labels read back)"""
    import torch
    t = torch.full((max(n, 1),), fill - 2 ** 32, dtype=torch.int32, device="cuda:0")
    rc = p._lib.rtr_select_clusters(p._ctx, radius, window[0], window[1], 0, 0, C.c_void_p(t.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, t.cpu().numpy().view(np.uint32)[:n]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_words_labels_and_stats_match_the_reference_in_every_form(pkg, clouds, form):
    options, sort = FORMS[form]
    for scene, (n, radii) in cc.SCENES.items():
        xyzw, rgba, labs = clouds[scene]
        opts = dict(options)
        if scene == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            if form == "sorted":
                assert p.get_option("reordered") == 1
            for r in radii:
                lab = labs[r]
                pins = cc.PINS[(scene, r)]
                for window, pinned in zip(cc.WINDOWS, pins[3]):
                    for outside in (False, True):
                        sel, ref = _want(lab, window, outside)
                        assert ref[0] == pins[0] and ref[2] == pins[2] and (outside or int(sel.sum()) == pinned)
                        if window == cc.WINDOWS[1]:  # (labels into host memory)
                            st, got = p.select_clusters(r, *window, outside=outside, labels=True)
                            assert got.dtype == np.uint32 and np.array_equal(got, lab), (form, scene, r)
                        else:
                            st = p.select_clusters(r, *window, outside=outside)
                        _check(pkg, p, n, sel, ref, st, (form, scene, r, window, outside))
                rc, got = _device_labels(p, n, r, cc.WINDOWS[2])  # (labels into device memory)
                assert rc == 0 and np.array_equal(got, lab), (form, scene, r, "device labels")
                assert np.array_equal(_sel(pkg, p, n), _want(lab, cc.WINDOWS[2])[0])
            for case in (cc.EVERYTHING, cc.NOTHING):
                if case[0] != scene:
                    continue
                lab = labs[case[1]]
                sel, ref = _want(lab, case[2:])
                assert (ref[0], ref[2], int(sel.sum())) == cc.NAMED_PINS[case]
                st, got = p.select_clusters(case[1], case[2], case[3], labels=True)
                _check(pkg, p, n, sel, ref, st, (form, case))
                assert np.array_equal(got, lab), (form, case)
                _check(pkg, p, n, ~sel, ref, p.select_clusters(case[1], case[2], case[3], outside=True), (form, case, "outside"))
            for key in ("clusters_keys_us", "clusters_sort_us", "clusters_label_us", "clusters_pair_tests_k"):
                assert p.get_option(key) > 0, key
        finally:
            p.close()


def _ragged(orc, n):
    rng = np.random.default_rng(100 + n)
    xyzw, rgba = orc.generate("room_shell", 100 + n, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = (rng.normal(size=(n, 3)) * (0.1 if n <= 2 else 0.5)).astype(f32)
    return xyzw, rgba, (0.35 if n <= 2 else 0.3 if n <= 257 else 0.08)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4099])
def test_ragged_counts_and_every_op_between_other_selections(pkg, orc, n):
    xyzw, rgba, r = _ragged(orc, n)
    lab = cr.labels(xyzw, r)
    if n <= 4000:
        assert np.array_equal(lab, cr.labels_brute(xyzw, r))
    sz = cr.sizes(lab)
    assert n < 63 or (len(set(sz)) >= 4 and 0 < cr.hits(lab, 5).sum() < cr.hits(lab, 2).sum() < n and cr.hits(lab, 2, 4).any())
    assert n != 2 or list(lab) == [0, 0]
    planes = f32([[1, 0, 0, 0.05]])
    half = pkg.clip_keep(planes, xyzw)
    nb, _ = nr.select(xyzw, r, 2)
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            sel = np.zeros(n, bool)
            for step in (("cl", (1, 0), "replace", False, False), ("planes", "replace"), ("cl", (2, 0), "toggle", True, False),
                         ("nb", "subtract"), ("cl", (5, 0), "add", False, False), ("cl", (1, 0), "intersect", True, False),
                         ("planes", "toggle"), ("cl", (2, 4), "subtract", False, False), ("cl", (2, 0), "replace", False, True),
                         ("nb", "add"), ("cl", (5, 0), "intersect", False, False), ("planes", "add"), ("cl", (2, 4), "toggle", False, True),
                         ("cl", (2, 0), "replace", True, False), ("cl", (1, 0), "toggle", False, False), ("cl", (1, 1), "add", True, True)):
                if step[0] == "planes":
                    sel = sr.combine(step[1], sel, half)
                    assert p.select_points(planes=planes, op=step[1])[0] == int(sel.sum())
                elif step[0] == "nb":
                    sel = sr.combine(step[1], sel, nb)
                    assert p.select_neighbours(r, 2, op=step[1])[0] == int(sel.sum())
                else:
                    _, window, op, outside, seeded = step
                    hit, ref = _want(lab, window, outside, sel if seeded else None)
                    sel = sr.combine(op, sel, hit)
                    st, got = p.select_clusters(r, window[0], window[1], seeded=seeded, op=op, outside=outside, labels=True)
                    _check(pkg, p, n, sel, ref, st, (n, name, step))  # (_sel: no bit at or past n)
                    assert np.array_equal(got, lab), (n, name, step)
                    continue
                assert np.array_equal(_sel(pkg, p, n), sel), (n, name, step)
            # the combining ops on a selection that does not exist yet: it counts as empty; stats=False still waits
            every = np.ones(n, bool)
            for op, want in (("add", every), ("subtract", ~every), ("intersect", ~every), ("toggle", every)):
                p.clear_selection()
                assert p.select_clusters(r, op=op, stats=False) is None
                assert np.array_equal(_sel(pkg, p, n), want), op
        finally:
            p.close()


def test_seeds_grow_to_exactly_the_clusters_they_touch(pkg, clouds):
    scene, r = "room_shell", 0.08
    xyzw, rgba, labs = clouds[scene]
    n, lab = xyzw.shape[0], labs[r]
    planes = f32([[1, 0, 0, -3.2]])  # x >= 3.2: a slab by one wall
    seeds = pkg.clip_keep(planes, xyzw)
    grown, ref = _want(lab, (1, 0), seeds=seeds)
    assert 0 < seeds.sum() < grown.sum() < n // 2 and (grown | ~seeds).all() and 20 < ref[1] < ref[0]
    assert np.array_equal(np.unique(lab[grown]), np.unique(lab[seeds]))  # (exactly the clusters the seeds touch)
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            # seeded with no selection: nothing hits, and an empty selection is created
            st = p.select_clusters(r, seeded=True)
            assert st == (0, ref[0], 0, ref[2]) and p.get_option("selection") == 1 and not _sel(pkg, p, n).any()
            p.clear_selection()
            _check(pkg, p, n, np.ones(n, bool), (ref[0], 0, ref[2]), p.select_clusters(r, seeded=True, outside=True), (name, "no seeds, outside"))
            assert p.select_points(planes=planes)[0] == int(seeds.sum())
            _check(pkg, p, n, grown, ref, p.select_clusters(r, seeded=True), (name, "grow"))
            _check(pkg, p, n, grown, ref, p.select_clusters(r, seeded=True), (name, "grown already: a fixed point"))
            # with a window: the touched clusters of 50 points or more
            p.select_points(planes=planes, stats=False)
            big, ref_big = _want(lab, (50, 0), seeds=seeds)
            assert 0 < big.sum() < grown.sum()
            _check(pkg, p, n, big, ref_big, p.select_clusters(r, 50, seeded=True), (name, "grow, 50"))
            # SUBTRACT and INTERSECT take the selection as it was before the call for seeds
            p.select_points(planes=planes, stats=False)
            sub, ref_sub = _want(lab, (2, 49), seeds=seeds)
            assert 0 < (seeds & sub).sum() < seeds.sum()
            _check(pkg, p, n, seeds & ~sub, ref_sub, p.select_clusters(r, 2, 49, seeded=True, op="subtract"), (name, "subtract"))
            p.select_points(planes=planes, stats=False)
            _check(pkg, p, n, seeds & sub, ref_sub, p.select_clusters(r, 2, 49, seeded=True, op="intersect"), (name, "intersect"))
            # the facade: growSelection
            pc = pkg.ProjectCloud(xyzw, rgba, reorder=sort, point_ids=sort)
            assert pc.projector.select_points(planes=planes)[0] == int(seeds.sum())
            assert pc.growSelection(r) == int(grown.sum()) == pc.selectedCount()
            assert np.array_equal(_sel(pkg, pc.projector, n), grown)
        finally:
            p.close()


def _boustrophedon(rows, length):
    """A chain of rows * (length + 1) points STEP apart: rows of `length` points along x, two steps apart in y, joined at
    alternating ends by one point half way up.  Consecutive points are exactly STEP apart; all others at least
    sqrt(2) STEP.  Returns the chain in chain order."""
    pts = []
    for i in range(rows):
        xs = range(length) if i % 2 == 0 else range(length - 1, -1, -1)
        pts += [(x, 2 * i) for x in xs]
        pts.append((pts[-1][0], 2 * i + 1))
    k = np.array(pts, np.int64)
    return np.stack([k[:, 0] * STEP - f32(2.5), k[:, 1] * STEP - f32(1.25), np.full(len(pts), f32(0.75))], 1).astype(f32)


def _run_chain(pkg, orc, xyz, lab, windows):
    n = xyz.shape[0]
    xyzw, rgba = orc.generate("room_shell", 21, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = xyz
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for window in windows:
                sel, ref = _want(lab, window)
                st, got = p.select_clusters(STEP, window[0], window[1], labels=True)
                _check(pkg, p, n, sel, ref, st, (name, window))
                assert np.array_equal(got, lab), (name, window)
        finally:
            p.close()


def test_a_shuffled_chain_is_one_cluster_and_one_ulp_splits_it(pkg, orc):
    chain = _boustrophedon(50, 99)
    n = chain.shape[0]
    assert n == 5000
    d2 = nr._d2(chain[1:], chain[:-1])
    assert (d2 == nr.r2_of(STEP)).all()
    order = np.random.default_rng(77).permutation(n)  # upload index -> chain index
    xyz = chain[order]
    cnt = nr.counts(xyz, STEP)
    assert (cnt == 2).sum() == n - 2 and (cnt == 1).sum() == 2  # (a chain: nothing else touches)
    lab = cr.labels(xyz, STEP)
    assert (lab == 0).all()
    _run_chain(pkg, orc, xyz, lab, ((1, 0), (5000, 5000), (5001, 0)))
    # one link an ulp of its coordinate longer: chain points 0 .. 1733 and 1734 .. 4999
    cut = 1733
    longer = chain.copy()
    away = np.sign(chain[cut + 1, 0] - chain[cut, 0])
    assert away != 0 and chain[cut + 2, 0] - chain[cut + 1, 0] == chain[cut + 1, 0] - chain[cut, 0]  # (mid-row)
    longer[cut + 1, 0] = np.nextafter(chain[cut + 1, 0], f32(np.inf) * away)
    assert nr._d2(longer[cut + 1], longer[cut]) > nr.r2_of(STEP) >= nr._d2(longer[cut + 2], longer[cut + 1])
    xyz = longer[order]
    lab = cr.labels(xyz, STEP)
    first = np.flatnonzero(order <= cut).min(), np.flatnonzero(order > cut).min()
    assert np.array_equal(lab, np.where(order <= cut, first[0], first[1]).astype(np.uint32))
    assert sorted(np.bincount(lab)[list(first)]) == [cut + 1, n - cut - 1]
    _run_chain(pkg, orc, xyz, lab, ((1, 0), (cut + 2, 0), (1, cut + 1)))


def test_parallel_chains_stay_apart(pkg, orc):
    k, c = np.meshgrid(np.arange(80), np.arange(64))
    xyz = np.stack([k.ravel() * STEP - f32(2), c.ravel() * (3 * STEP) - f32(5), np.full(k.size, f32(-0.5))], 1).astype(f32)
    order = np.random.default_rng(78).permutation(k.size)
    xyz = xyz[order]
    lab = cr.labels(xyz, STEP)
    assert cr.stats(lab, cr.hits(lab)) == (64, 64, 80) and (np.bincount(lab)[np.unique(lab)] == 80).all()
    assert (lab[np.argsort(order)].reshape(64, 80) == lab[np.argsort(order)].reshape(64, 80)[:, :1]).all()
    _run_chain(pkg, orc, xyz, lab, ((1, 0), (80, 80), (81, 0)))


def test_coincident_piles(pkg, orc):
    n = 3000 + 65 + 500
    xyzw, rgba = orc.generate("room_shell", 12, 0, n, n)
    xyzw = xyzw.copy()
    rng = np.random.default_rng(2)
    at = rng.permutation(n)
    big, small, rest = at[:3000], at[3000:3065], at[3065:]
    xyzw[big, :3] = f32([0.7, -0.3, 1.9])
    xyzw[small, :3] = f32([-2.5, 0.25, -0.004])
    xyzw[rest, :3] = (rng.uniform(-1, 1, (500, 3)) * [50, 50, 50] + [100, 0, 0]).astype(f32)  # (far from both, sparse)
    r = 0.01
    lab = cr.labels(xyzw, r)
    assert (lab[big] == big.min()).all() and (lab[small] == small.min()).all() and np.array_equal(lab[rest], rest)
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for window, who in (((1, 0), (True, True, True)), ((2, 0), (True, True, False)), ((66, 0), (True, False, False)),
                                ((3000, 3000), (True, False, False)), ((3001, 0), (False, False, False)),
                                ((2, 65), (False, True, False)), ((65, 2999), (False, True, False)), ((1, 1), (False, False, True))):
                sel, ref = _want(lab, window)
                assert (sel[big].all(), sel[small].all(), sel[rest].all()) == who == (sel[big].any(), sel[small].any(), sel[rest].any())
                assert ref[0] == 502 and ref[2] == 3000
                st, got = p.select_clusters(r, window[0], window[1], labels=True)
                _check(pkg, p, n, sel, ref, st, (name, window))
                assert np.array_equal(got, lab), (name, window)
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
    lab = cr.labels(xyzw, r)
    assert np.array_equal(lab[bad], np.flatnonzero(bad)) and (cr.sizes(lab)[bad] == 1).all()  # singletons, their own label
    for name, options, sort in THREE_FORMS + (("hash", {"auto_reorder": 0, "pack": 2}, False),):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for window in ((1, 0), (2, 0), (3, 0), (1, 1)):
                sel, ref = _want(lab, window)
                assert (window[0] == 1) == bool(sel[bad].all()) == bool(sel[bad].any()) and 0 < sel.sum()  # hit iff min_points == 1
                st, got = p.select_clusters(r, window[0], window[1], labels=True)
                _check(pkg, p, n, sel, ref, st, (axis, name, window))
                assert np.array_equal(got, lab), (axis, name, window)
                _check(pkg, p, n, ~sel, ref, p.select_clusters(r, window[0], window[1], outside=True), (axis, name, window, "outside"))
        finally:
            p.close()
    # a coordinate within 2^20 radius of the origin is inside the span; a finite one beyond the span fails the call
    edge = xyzw.copy()
    edge[at[9], axis], edge[at[10], axis] = f32(2.0 ** 20 * r), f32(-(2.0 ** 20) * r)
    with np.errstate(invalid="ignore"):
        lab_edge = cr.labels_brute(edge, r)
    assert lab_edge[at[9]] == at[9] and lab_edge[at[10]] == at[10]
    p = _new(pkg, {}, edge, rgba)
    try:
        sel, ref = _want(lab_edge, (2, 0))
        st, got = p.select_clusters(r, 2, labels=True)
        _check(pkg, p, n, sel, ref, st, (axis, "edge of the span"))
        assert np.array_equal(got, lab_edge)
    finally:
        p.close()
    far = {"1e30": 1e30, "-1e30": -1e30, "beyond": 2.0 ** 20 * r * 1.0011, "-beyond": -(2.0 ** 20) * r * 1.0011}
    for what, v in far.items():
        moved = xyzw.copy()
        moved[at[11], axis] = f32(v)
        p = _new(pkg, {}, moved, rgba)
        try:
            planes = f32([[0, 1, 0, 0.2]])
            want = pkg.clip_keep(planes, moved)
            p.select_points(planes=planes, stats=False)
            sentinel = np.full(n, 0xABCD1234, np.uint32)
            st = np.full(4, 77, np.uint64)
            rc = p._lib.rtr_select_clusters(p._ctx, r, 1, 0, 0, 0, sentinel.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p))
            assert rc == pkg._lib.RTR_ERR_UNSUPPORTED and "span" in p._lib.rtr_last_error(p._ctx).decode(), what
            assert "rtr_select_clusters" in p._lib.rtr_last_error(p._ctx).decode()
            assert (sentinel == 0xABCD1234).all() and (st == 77).all(), what  # (labels and stats untouched)
            rc, got = _device_labels(p, n, r, (1, 0), fill=0xABCD1234)
            assert rc == pkg._lib.RTR_ERR_UNSUPPORTED and (got == 0xABCD1234).all(), what
            assert np.array_equal(_sel(pkg, p, n), want) and p.get_option("selection") == 1, what  # (intact word for word)
            p.clear_selection()
            with pytest.raises(pkg.RtrError) as e:
                p.select_clusters(r, op="add", seeded=True)
            assert e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED
            assert p.get_option("selection") == 0 and p.selection() is None, what  # (and none is created)
        finally:
            p.close()


def test_same_words_and_labels_in_every_resident_order(pkg, orc):
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
            lab = cr.labels(xyzw, r)
            assert np.array_equal(lab[5000:5100], lab[:100]) and np.array_equal(lab[35_000:35_100], lab[:100])  # (the copies join)
            if r == 1e-4:  # (a radius so small that only the copies have neighbours: clusters of three, labelled by the first)
                assert np.array_equal(lab[:100], np.arange(100)) and cr.hits(lab, 2).sum() == 300 == cr.hits(lab, 3, 3).sum()
            for window in ((1, 0), (2, 0), (3, 3), (4, 0)):
                sel, ref = _want(lab, window)
                labels = []
                for name, p in got.items():
                    st, la = p.select_clusters(r, window[0], window[1], labels=True)
                    _check(pkg, p, n, sel, ref, st, (name, r, window))
                    labels.append(la)
                words = [p.download(pkg._lib.BUF_SELECTION) for p in got.values()]
                assert np.array_equal(words[0], words[1]) and np.array_equal(words[0], words[2])
                assert np.array_equal(labels[0], lab) and np.array_equal(labels[1], lab) and np.array_equal(labels[2], lab)
    finally:
        for p in got.values():
            p.close()


@pytest.mark.parametrize("form", ["default", "sorted"])
def test_remove_small_clusters_cleans_the_cloud(pkg, orc, form):
    options, sort = FORMS[form]
    n, W, H = 120_001, 320, 240
    r, k = 0.04, 5
    xyzw, rgba = orc.generate("room_shell", 52, 0, n, n)
    lab = cr.labels(xyzw, r)
    hit, ref = _want(lab, (k, 0))
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
        # the small clusters' words, complemented on the device, as the keep words of remove_points
        a = _new(pkg, options, xyzw, rgba, W, H, sort=sort)
        try:
            assert a.select_clusters(r, k, outside=True) == (int((~hit).sum()),) + ref
            assert a.select_points(op="toggle")[0] == int(hit.sum())  # (no region: every point is inside)
            a.remove_points(a.selection())
            assert a.num_points == int(hit.sum()) and a.selection() is None
            _same_frames(_frames(pkg, a, Ps), want, (form, "remove"))
        finally:
            a.close()
        # the facade's removeSmallClusters
        pc = pkg.ProjectCloud(xyzw, rgba, reorder=sort, point_ids=sort)
        assert pc.selectClusters(r, k) == int(hit.sum()) == pc.selectedCount()
        assert pc.removeSmallClusters(r, k) == int((~hit).sum()) and pc.projector.num_points == int(hit.sum())
        assert pc.projector.selection() is None and pc.selectedCount() == 0
        pc.projector.set_resolution(W, H)
        _same_frames(_frames(pkg, pc.projector, Ps), want, (form, "removeSmallClusters"))
    finally:
        b.close()


def test_the_call_moves_nothing_else(pkg, orc):
    L = pkg._lib
    n, W, H = 60_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 88, 0, n, n)
    P, P2 = pkg.orbit_projection(40, W, H), pkg.orbit_projection(41, W, H)
    keep = np.arange(n) % 3 != 0
    planes = f32([[0, 0, 1, 100], [1, 0, 0, 50]])
    labs = {r: cr.labels(xyzw, r) for r in (0.05, 0.07)}
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
        for kw in (dict(radius=0.05, min_points=2), dict(radius=0.07, min_points=50, op="add", labels=True),
                   dict(radius=0.05, min_points=2, max_points=49, op="toggle", outside=True, stats=False),
                   dict(radius=0.07, min_points=2, max_points=49, seeded=True, op="intersect")):
            seeds = want if kw.get("seeded") else None
            hit, _ = _want(labs[kw["radius"]], (kw["min_points"] if "min_points" in kw else 1, kw.get("max_points", 0)), seeds=seeds)
            assert 0 < hit.sum() < n
            want = sr.combine(kw.get("op", "replace"), want, hit != kw.get("outside", False)) if want is not None else hit
            p.select_clusters(**kw)
            assert np.array_equal(_sel(pkg, p, n), want), kw  # (the clip planes and the keep mask in force play no part)
        assert same(before, state()) and p.get_option("p2p_open") == 1
        p.p2p_close()
        p.set_clip_planes(None)
        p.set_point_keep(None)
        # issued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.select_clusters(0.07, 2)
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
            fresh.select_clusters(0.25)
        assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        want, _ = _want(cr.labels(xyzw, 0.1), (3, 0))
        assert 0 < want.sum() < n
        p.select_clusters(0.1, 3)
        options = {k: p.get_option(k) for k in ("clusters_keys_us", "clusters_sort_us", "clusters_label_us", "clusters_pair_tests_k",
                                                "selection", "resident_millibytes_per_point")}
        lib, ctx = p._lib, p._ctx
        den = np.array([1], np.uint32).view(f32)[0]
        # (radius, min_points, max_points, flags, op, the argument named)
        bad = [(v, 1, 0, 0, 0, "radius") for v in (0.0, -0.0, -0.25, np.nan, np.inf, -np.inf)]
        bad += [(v, 1, 0, 0, 0, "square of radius") for v in (float(den), 1e-20, 1e-30, 2e19, 3e38)]  # (r2 subnormal, 0 or infinite)
        bad += [(0.1, 0, 0, 0, 0, "min_points"), (0.1, 0, 5, 1, 0, "min_points")]
        bad += [(0.1, lo, hi, 0, 0, "max_points") for lo, hi in ((2, 1), (50, 49), (2 ** 32 - 1, 7))]
        bad += [(0.1, 1, 0, flags, 0, "flags") for flags in (2, 3, 4, -1, 256)]
        bad += [(0.1, 1, 0, 0, op, "op") for op in (-1, 9, 10, 11, 13, 16, 32)]
        for case in bad:
            st = np.full(4, 77, np.uint64)
            lab = np.full(n, 0x5A5A5A5A, np.uint32)
            assert lib.rtr_select_clusters(ctx, case[0], case[1], case[2], case[3], case[4], vp(lab), vp(st)) == L.RTR_ERR_INVALID, case
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_select_clusters" in text and case[5] in text, (case, text)
            assert np.array_equal(_sel(pkg, p, n), want) and (st == 77).all() and (lab == 0x5A5A5A5A).all(), case
            assert {k: p.get_option(k) for k in options} == options, case
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        with pytest.raises(pkg.RtrError) as e:
            p.select_clusters(0.1, 2)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert np.array_equal(_sel(pkg, p, n), want)
        # an error on a context without a selection makes none
        p.clear_selection()
        assert lib.rtr_select_clusters(ctx, 0.1, 0, 0, 0, 0, None, None) == L.RTR_ERR_INVALID and p.selection() is None
        assert p.get_option("selection") == 0
    finally:
        p.close()
