"""Selecting by smooth segment on the GPU (include/rtr_segments.h section 6q): rtr_select_segments' words, labels (into
host and into device memory) and all four statistics compared exactly (np.array_equal) with the numpy float32 reference
of tests/segments_ref.py -- the three pinned cases of segments_cases.py in every form the cloud can take, normals and
curvature from host and from device memory; constant normals against rtr_select_clusters on the same context; ragged
point counts with every op chained between other selections, seeded, oriented and with a curvature limit; the special
clouds (the fold at the threshold, the curvature at the limit, opposite sheets, bad normals, non-finite coordinates);
a long chain whose normals turn link by link; a coincident pile with two normals; the span; every argument error; what
the call must leave alone."""
import ctypes as C

import numpy as np
import pytest

import clusters_cases as cc
import clusters_ref as cr
import neighbours_ref as nr
import normals_ref as nref
import segments_cases as sc
import segments_ref as sg
import select_ref as sr
from test_gpu_clusters import STEP, THREE_FORMS, _boustrophedon
from test_gpu_select import FORMS, _new, _sel

pytestmark = pytest.mark.gpu

f32 = np.float32
DIRS = f32([[0, 0, 1], [0, 0, -1], [0, 1, 0], [1, 0, 0]])  # three classes by |dot|, four by dot


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev(a):
    """a numpy array as a torch tensor in device memory (None stays None)"""
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _want(lab, window, outside=False, seeds=None):
    """(the hits after OUTSIDE, stats[1..3])"""
    hit = sg.hits(lab, window[0], window[1], seeds)
    return hit != outside, sg.stats(lab, hit)


def _check(pkg, p, n, sel, ref_stats, st, what):
    assert st == (int(sel.sum()),) + tuple(ref_stats), (what, st, ref_stats)
    assert np.array_equal(_sel(pkg, p, n), sel), what


def _device_labels(p, n, radius, cos_angle, normals, curvature, max_curvature, window, flags=0, fill=0xDEADBEEF):
    """rtr_select_segments with labels in device memory (a torch tensor); normals / curvature: pointers.  (return code,
    the labels read back)"""
    import torch
    t = torch.full((max(n, 1),), fill - 2 ** 32, dtype=torch.int32, device="cuda:0")
    rc = p._lib.rtr_select_segments(p._ctx, radius, cos_angle, normals, curvature, max_curvature, window[0], window[1], flags, 0,
                                    C.c_void_p(t.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, t.cpu().numpy().view(np.uint32)[:n]


@pytest.fixture(scope="module")
def cases(orc):
    """name -> (xyzw, rgba, normals, curvature, max_curvature, radius, labels): computed once, never changed."""
    out = {}
    for name, (scene, n, radius, _) in sc.CASES.items():
        xyzw, rgba, normals, curvature, max_curvature = sc.make(orc, nref, name)
        out[name] = (xyzw, rgba, normals, curvature, max_curvature, radius, sg.labels(xyzw, radius, sc.COS_ANGLE, normals, curvature, max_curvature))
    return out


@pytest.mark.parametrize("form", sorted(FORMS))
def test_pinned_cases_match_the_reference_in_every_form(pkg, cases, form):
    options, sort = FORMS[form]
    for name, (xyzw, rgba, normals, curvature, max_curvature, r, lab) in cases.items():
        n = xyzw.shape[0]
        opts = dict(options)
        if sc.CASES[name][0] == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            before = (normals.copy(), None if curvature is None else curvature.copy())
            dn, dc = _dev(normals), _dev(curvature)
            pins = sc.PINS[name]
            for k, (window, pinned) in enumerate(zip(sc.WINDOWS, pins[3])):
                for outside in (False, True):
                    sel, ref = _want(lab, window, outside)
                    assert ref[0] == pins[0] and ref[2] == pins[2] and (outside or int(sel.sum()) == pinned)
                    nrm, curv = (normals, curvature) if (k + outside) % 2 == 0 else (dn, dc)  # host and device inputs in turn
                    if window == sc.WINDOWS[1]:  # (labels into host memory)
                        st, got = p.select_segments(r, sc.COS_ANGLE, nrm, curv, max_curvature, *window, outside=outside, labels=True)
                        assert got.dtype == np.uint32 and np.array_equal(got, lab), (form, name)
                        if name in sc.FACES and not outside:  # the six faces of the room, on the GPU
                            assert tuple(sorted(np.bincount(got)[np.unique(got)])[::-1][:6]) == sc.FACES[name]
                    else:
                        st = p.select_segments(r, sc.COS_ANGLE, nrm, curv, max_curvature, *window, outside=outside)
                    _check(pkg, p, n, sel, ref, st, (form, name, window, outside))
            # labels into device memory, from device inputs and from host inputs
            for nptr, cptr in ((C.c_void_p(dn.data_ptr()), None if dc is None else C.c_void_p(dc.data_ptr())), (_vp(normals), _vp(curvature))):
                rc, got = _device_labels(p, n, r, sc.COS_ANGLE, nptr, cptr, max_curvature, sc.WINDOWS[2])
                assert rc == 0 and np.array_equal(got, lab), (form, name, "device labels")
                assert np.array_equal(_sel(pkg, p, n), _want(lab, sc.WINDOWS[2])[0])
            # the caller's arrays are never written, in host or in device memory
            assert nref.same_bits(normals, before[0]) and nref.same_bits(dn.cpu().numpy(), before[0])
            assert curvature is None or (nref.same_bits(curvature, before[1]) and nref.same_bits(dc.cpu().numpy(), before[1]))
        finally:
            p.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_constant_normals_without_curvature_equal_select_clusters(pkg, orc, form):
    options, sort = FORMS[form]
    for scene, (n, radii) in cc.SCENES.items():
        xyzw, rgba = orc.generate(scene, cc.SEED, 0, n, n)
        opts = dict(options)
        if scene == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1
        nrm = np.tile(f32([0.6, 0, -0.8]), (n, 1))
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            for r in radii:
                for window, outside, oriented in ((w, o, k % 2 == 1) for k, w in enumerate(cc.WINDOWS) for o in (False, True)):
                    st_c, lab_c = p.select_clusters(r, *window, outside=outside, labels=True)
                    words_c = p.download(pkg._lib.BUF_SELECTION).copy()
                    p.clear_selection()
                    st_s, lab_s = p.select_segments(r, 0.99, nrm, None, np.inf, *window, oriented=oriented, outside=outside, labels=True)
                    assert st_s == st_c and np.array_equal(lab_s, lab_c), (form, scene, r, window, outside)
                    assert np.array_equal(p.download(pkg._lib.BUF_SELECTION), words_c), (form, scene, r, window, outside)
                assert st_c[1] == cc.PINS[(scene, r)][0] and st_c[3] == cc.PINS[(scene, r)][2]
        finally:
            p.close()


def _ragged(orc, n):
    rng = np.random.default_rng(100 + n)
    xyzw, rgba = orc.generate("room_shell", 100 + n, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = (rng.normal(size=(n, 3)) * (0.1 if n <= 2 else 0.5)).astype(f32)
    normals = DIRS[rng.integers(0, 4, n)]
    curvature = rng.uniform(0, 0.04, n).astype(f32)
    return xyzw, rgba, (0.35 if n <= 2 else 0.3 if n <= 257 else 0.08), np.ascontiguousarray(normals), curvature


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4099])
def test_ragged_counts_and_every_op_between_other_selections(pkg, orc, n):
    xyzw, rgba, r, normals, curvature = _ragged(orc, n)
    near = cr.pairs(xyzw, r)
    lim = f32(0.03)
    # the three relations of the chain: by |dot|, by dot, by |dot| with the curvature limit
    labs = {"abs": sg.labels(xyzw, r, 0.9, normals, near=near), "dot": sg.labels(xyzw, r, 0.9, normals, oriented=True, near=near),
            "smooth": sg.labels(xyzw, r, 0.9, normals, curvature, lim, near=near)}
    if n <= 4000:
        assert np.array_equal(labs["abs"], sg.labels_brute(xyzw, r, 0.9, normals))
        assert np.array_equal(labs["dot"], sg.labels_brute(xyzw, r, 0.9, normals, oriented=True))
        assert np.array_equal(labs["smooth"], sg.labels_brute(xyzw, r, 0.9, normals, curvature, lim))
    if n >= 63:  # (non-trivial: segments of several sizes, three different partitions, none of them plain clustering's)
        plain = cr.labels_of_pairs(n, *near)
        assert all(len(set(sg.sizes(lab))) >= (7 if n >= 255 else 2) and not np.array_equal(lab, plain) for lab in labs.values())
        assert not np.array_equal(labs["abs"], labs["dot"]) and not np.array_equal(labs["abs"], labs["smooth"])
        assert 0 < sg.hits(labs["abs"], 3).sum() < sg.hits(labs["abs"], 2).sum() < n
    planes = f32([[1, 0, 0, 0.05]])
    half = pkg.clip_keep(planes, xyzw)
    nb, _ = nr.select(xyzw, r, 2)
    kinds = {"abs": dict(), "dot": dict(oriented=True), "smooth": dict(curvature=curvature, max_curvature=lim)}
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            dn, dc = _dev(normals), _dev(curvature)
            sel = np.zeros(n, bool)
            for k, step in enumerate((("sg", "abs", (1, 0), "replace", False, False), ("planes", "replace"), ("sg", "dot", (2, 0), "toggle", True, False),
                                      ("nb", "subtract"), ("sg", "smooth", (3, 0), "add", False, False), ("sg", "abs", (1, 0), "intersect", True, False),
                                      ("planes", "toggle"), ("sg", "dot", (2, 4), "subtract", False, False), ("sg", "abs", (2, 0), "replace", False, True),
                                      ("nb", "add"), ("sg", "smooth", (3, 0), "intersect", False, False), ("planes", "add"),
                                      ("sg", "abs", (2, 4), "toggle", False, True), ("sg", "smooth", (2, 0), "replace", True, True),
                                      ("sg", "dot", (1, 0), "toggle", False, False), ("sg", "abs", (1, 1), "add", True, True))):
                if step[0] == "planes":
                    sel = sr.combine(step[1], sel, half)
                    assert p.select_points(planes=planes, op=step[1])[0] == int(sel.sum())
                elif step[0] == "nb":
                    sel = sr.combine(step[1], sel, nb)
                    assert p.select_neighbours(r, 2, op=step[1])[0] == int(sel.sum())
                else:
                    _, kind, window, op, outside, seeded = step
                    lab = labs[kind]
                    hit, ref = _want(lab, window, outside, sel if seeded else None)
                    sel = sr.combine(op, sel, hit)
                    kw = dict(kinds[kind])
                    if k % 2 and "curvature" in kw:
                        kw["curvature"] = dc
                    st, got = p.select_segments(r, 0.9, dn if k % 2 else normals, min_points=window[0], max_points=window[1], seeded=seeded, op=op,
                                                outside=outside, labels=True, **kw)
                    _check(pkg, p, n, sel, ref, st, (n, name, step))  # (_sel: no bit at or past n)
                    assert np.array_equal(got, lab), (n, name, step)
                    continue
                assert np.array_equal(_sel(pkg, p, n), sel), (n, name, step)
            # the combining ops on a selection that does not exist yet: it counts as empty; stats=False still waits
            every = np.ones(n, bool)
            for op, want in (("add", every), ("subtract", ~every), ("intersect", ~every), ("toggle", every)):
                p.clear_selection()
                assert p.select_segments(r, 0.9, normals, op=op, stats=False) is None
                assert np.array_equal(_sel(pkg, p, n), want), op
            # seeded with no selection: nothing hits, and an empty selection is created
            p.clear_selection()
            ref = sg.stats(labs["abs"], np.zeros(n, bool))
            assert p.select_segments(r, 0.9, normals, seeded=True) == (0,) + ref and p.get_option("selection") == 1
        finally:
            p.close()


def _upload(orc, xyz, seed=21):
    n = xyz.shape[0]
    xyzw, rgba = orc.generate("room_shell", seed, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = xyz
    return xyzw, rgba


@pytest.mark.parametrize("name", sorted(sc.special_clouds()))
def test_special_clouds(pkg, orc, name):
    """the fold at the threshold and one ulp below it, the curvature at the limit and the next float, the opposite sheets
    with and without ORIENTED, bad normals and curvatures, non-finite coordinates: the labels written down by hand"""
    case = sc.special_clouds()[name]
    lab, n = case["labels"], case["xyz"].shape[0]
    order = np.random.default_rng(3).permutation(n)  # (and in a shuffled upload order: the labels follow the indices)
    with np.errstate(invalid="ignore"):
        lab_shuffled = sg.labels(case["xyz"][order], sc.R, case["cos_angle"], case["normals"][order],
                                 None if case["curvature"] is None else case["curvature"][order], case["max_curvature"], case["oriented"])
    for perm, want in ((np.arange(n), lab), (order, lab_shuffled)):
        xyzw, rgba = _upload(orc, case["xyz"][perm])
        normals = np.ascontiguousarray(case["normals"][perm])
        curvature = None if case["curvature"] is None else np.ascontiguousarray(case["curvature"][perm])
        for form, options, sort in THREE_FORMS:
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                for dev in (False, True):
                    for window in ((1, 0), (2, 0)):
                        sel, ref = _want(want, window)
                        st, got = p.select_segments(sc.R, case["cos_angle"], _dev(normals) if dev else normals, _dev(curvature) if dev else curvature,
                                                    case["max_curvature"], *window, oriented=case["oriented"], labels=True)
                        assert np.array_equal(got, want), (name, form, dev, got)
                        _check(pkg, p, n, sel, ref, st, (name, form, dev, window))
            finally:
                p.close()


def _turning_chain():
    """A shuffled chain of 5000 points STEP apart whose normals turn by a constant angle per link: normal t is (cos(t a),
    sin(t a), 0) rounded to float32.  The dots of the links, in the contract's arithmetic, differ by rounding in their last
    bits; `a` is the first angle of a short list at which ONE link has the smallest dot.  Returns (xyz, normals, the
    smallest dot, the chain index of the link's lower end, the upload index -> chain index order)."""
    chain = _boustrophedon(50, 99)
    n = chain.shape[0]
    t = np.arange(n, dtype=np.float64)
    for a in np.arange(40, 80) / 256.0:
        nrm = np.stack([np.cos(t * a), np.sin(t * a), np.zeros(n)], 1).astype(f32)
        d = sg.dot(nrm[1:], nrm[:-1])
        at = np.flatnonzero(d == d.min())
        if at.size == 1 and 100 < at[0] < n - 100:
            order = np.random.default_rng(79).permutation(n)
            return chain[order], np.ascontiguousarray(nrm[order]), d.min(), int(at[0]), order
    raise AssertionError("no angle of the list gives a unique weakest link")


def test_a_chain_of_turning_normals_is_one_segment_and_one_ulp_splits_it(pkg, orc):
    xyz, normals, weakest, cut, order = _turning_chain()
    n = xyz.shape[0]
    assert n == 5000 and 0.9 < weakest < 0.99
    assert np.abs(sg.dot(normals[order.argsort()][0], normals)).min() < 0.1  # (along the chain the normals turn to a right angle and on)
    near = cr.pairs(xyz, STEP)
    assert near[0].size == 2 * (n - 1)  # (a chain: nothing else touches)
    one = sg.labels(xyz, STEP, weakest, normals, near=near)
    assert (one == 0).all()
    tight = np.nextafter(weakest, f32(1))
    two = sg.labels(xyz, STEP, tight, normals, near=near)
    first = np.flatnonzero(order <= cut).min(), np.flatnonzero(order > cut).min()
    assert np.array_equal(two, np.where(order <= cut, first[0], first[1]).astype(np.uint32))  # split at that link and nowhere else
    xyzw, rgba = _upload(orc, xyz)
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for cos_angle, lab, windows in ((weakest, one, ((1, 0), (5000, 5000), (5001, 0))), (tight, two, ((1, 0), (cut + 2, 0), (1, cut + 1)))):
                for oriented in (False, True):  # (consecutive normals are 0.2 rad apart: the sign plays no part)
                    for window in windows:
                        sel, ref = _want(lab, window)
                        st, got = p.select_segments(STEP, cos_angle, normals, None, np.inf, *window, oriented=oriented, labels=True)
                        _check(pkg, p, n, sel, ref, st, (name, cos_angle, window))
                        assert np.array_equal(got, lab), (name, cos_angle, window)
        finally:
            p.close()


def test_a_coincident_pile_with_two_normals_is_two_segments(pkg, orc):
    n = 3000 + 500
    rng = np.random.default_rng(2)
    at = rng.permutation(n)
    pile, rest = at[:3000], at[3000:]
    xyz = np.zeros((n, 3), f32)
    xyz[pile] = f32([0.7, -0.3, 1.9])
    xyz[rest] = (rng.uniform(-1, 1, (500, 3)) * [50, 50, 50] + [100, 0, 0]).astype(f32)  # (far from the pile, sparse)
    normals = np.tile(f32([0, 0, 1]), (n, 1))
    tilted = pile[rng.random(3000) < 0.4]
    normals[tilted] = f32([0, 0.6, 0.8])
    flat = np.setdiff1d(pile, tilted)
    assert (tilted.size, flat.size) == (1211, 1789)  # the pinned sizes
    r = 0.01
    lab = sg.labels(xyz, r, sc.COS_ANGLE, normals)
    assert (lab[tilted] == tilted.min()).all() and (lab[flat] == flat.min()).all() and np.array_equal(lab[rest], rest)
    assert (cr.labels(xyz, r)[pile] == pile.min()).all()  # (one cluster without the normals)
    xyzw, rgba = _upload(orc, xyz, 12)
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for window, who in (((1, 0), (True, True, True)), ((2, 0), (True, True, False)), ((1212, 0), (False, True, False)),
                                ((1211, 1211), (True, False, False)), ((1790, 0), (False, False, False)), ((1, 1), (False, False, True))):
                sel, ref = _want(lab, window)
                assert (sel[tilted].all(), sel[flat].all(), sel[rest].all()) == who == (sel[tilted].any(), sel[flat].any(), sel[rest].any())
                assert ref[0] == 502 and ref[2] == 1789
                st, got = p.select_segments(r, sc.COS_ANGLE, normals, None, np.inf, *window, labels=True)
                _check(pkg, p, n, sel, ref, st, (name, window))
                assert np.array_equal(got, lab), (name, window)
        finally:
            p.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_special_coordinates_and_the_span(pkg, orc, axis):
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
    normals = np.ascontiguousarray(DIRS[rng.integers(0, 4, n)])
    lab = sg.labels(xyzw, r, 0.9, normals)
    assert np.array_equal(lab[bad], np.flatnonzero(bad)) and (sg.sizes(lab)[bad] == 1).all()  # singletons, their own label
    assert len(set(sg.sizes(lab))) >= 3
    for name, options, sort in THREE_FORMS + (("hash", {"auto_reorder": 0, "pack": 2}, False),):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for window in ((1, 0), (2, 0), (1, 1)):
                sel, ref = _want(lab, window)
                assert (window[0] == 1) == bool(sel[bad].all()) == bool(sel[bad].any()) and 0 < sel.sum()  # hit iff min_points == 1
                st, got = p.select_segments(r, 0.9, normals, None, np.inf, *window, labels=True)
                _check(pkg, p, n, sel, ref, st, (axis, name, window))
                assert np.array_equal(got, lab), (axis, name, window)
                _check(pkg, p, n, ~sel, ref, p.select_segments(r, 0.9, normals, None, np.inf, *window, outside=True), (axis, name, window, "outside"))
        finally:
            p.close()
    # a coordinate within 2^20 radius of the origin is inside the span; a finite one beyond the span fails the call
    edge = xyzw.copy()
    edge[at[9], axis], edge[at[10], axis] = f32(2.0 ** 20 * r), f32(-(2.0 ** 20) * r)
    with np.errstate(invalid="ignore"):
        lab_edge = sg.labels_brute(edge, r, 0.9, normals)
    assert lab_edge[at[9]] == at[9] and lab_edge[at[10]] == at[10]
    p = _new(pkg, {}, edge, rgba)
    try:
        sel, ref = _want(lab_edge, (2, 0))
        st, got = p.select_segments(r, 0.9, normals, min_points=2, labels=True)
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
            rc = p._lib.rtr_select_segments(p._ctx, r, 0.9, _vp(normals), None, 0.0, 1, 0, 0, 0, _vp(sentinel), _vp(st))
            assert rc == pkg._lib.RTR_ERR_UNSUPPORTED and "span" in p._lib.rtr_last_error(p._ctx).decode(), what
            assert "rtr_select_segments" in p._lib.rtr_last_error(p._ctx).decode()
            assert (sentinel == 0xABCD1234).all() and (st == 77).all(), what  # (labels and stats untouched)
            rc, got = _device_labels(p, n, r, 0.9, _vp(normals), None, 0.0, (1, 0), fill=0xABCD1234)
            assert rc == pkg._lib.RTR_ERR_UNSUPPORTED and (got == 0xABCD1234).all(), what
            assert np.array_equal(_sel(pkg, p, n), want) and p.get_option("selection") == 1, what  # (intact word for word)
            p.clear_selection()
            with pytest.raises(pkg.RtrError) as e:
                p.select_segments(r, 0.9, normals, op="add", seeded=True)
            assert e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED
            assert p.get_option("selection") == 0 and p.selection() is None, what  # (and none is created)
        finally:
            p.close()


def test_the_call_moves_nothing_else(pkg, orc):
    from test_gpu_voxel import _frames  # noqa: F401  (the frame helpers' module must import: the buffers below are its)
    L = pkg._lib
    n, W, H = 60_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 88, 0, n, n)
    P, P2 = pkg.orbit_projection(40, W, H), pkg.orbit_projection(41, W, H)
    keep = np.arange(n) % 3 != 0
    planes = f32([[0, 0, 1, 100], [1, 0, 0, 50]])
    r = 0.09
    est = nref.estimate(xyzw, r, 12)
    normals, curvature = est["normals"], est["curvature"]
    near = cr.pairs(xyzw, r)
    labs = {None: sg.labels(xyzw, r, sc.COS_ANGLE, normals, near=near), 0.02: sg.labels(xyzw, r, sc.COS_ANGLE, normals, curvature, 0.02, near=near)}
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        def state():
            return [p.download(b).copy() for b in (L.BUF_DEPTH, L.BUF_IMAGE, L.BUF_TENSOR, L.BUF_VISIBLE, L.BUF_POINT_ID, L.BUF_POINT_KEEP)] + \
                   [p.clip_planes(), p.frame_stats(), p.get_option("p2p_open"), p.get_option("packed"), p.get_option("reordered"),
                    p.get_option("point_keep"), p.num_points, p.get_option("resident_millibytes_per_point")] + \
                   [p.get_option(k) for k in ("clusters_keys_us", "clusters_sort_us", "clusters_label_us", "clusters_pair_tests_k",
                                              "neighbours_pair_tests_k", "normals_pair_tests_k")]

        def same(a, b):
            return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

        p.set_clip_planes(planes)
        p.set_point_keep(keep)
        p.p2p_open(0, 1, [p.p2p_export()])  # (the one-rank form of test_gpu_p2p.py: a rank maps its own buffers)
        p.p2p_render(P, True)
        p.point_pass(P)
        p.select_points(stats=False)  # (the selection's own words count as resident: they exist before the first call)
        p.select_clusters(r, 2)  # (... and so do the cluster call's option values: the new call has none of its own)
        p.select_points(stats=False)
        before = state()
        host = (normals.copy(), curvature.copy())
        dn, dc = _dev(normals), _dev(curvature)
        want = np.ones(n, bool)
        for kw in (dict(min_points=2), dict(min_points=50, op="intersect", labels=True, curvature=curvature, max_curvature=0.02),
                   dict(min_points=2, max_points=49, op="toggle", outside=True, stats=False, device=True),
                   dict(min_points=2, max_points=49, seeded=True, op="intersect", curvature=curvature, max_curvature=0.02, device=True)):
            kw = dict(kw)
            dev = kw.pop("device", False)
            lab = labs[0.02 if "curvature" in kw else None]
            seeds = want if kw.get("seeded") else None
            hit, _ = _want(lab, (kw["min_points"], kw.get("max_points", 0)), seeds=seeds)
            assert 0 < hit.sum() < n
            want = sr.combine(kw.get("op", "replace"), want, hit != kw.get("outside", False))
            if dev and "curvature" in kw:
                kw["curvature"] = dc
            p.select_segments(r, sc.COS_ANGLE, dn if dev else normals, **kw)
            assert np.array_equal(_sel(pkg, p, n), want), kw  # (the clip planes and the keep mask in force play no part)
        assert 0 < want.sum() < n
        assert same(before, state()) and p.get_option("p2p_open") == 1
        # the caller's arrays are bit-identical afterwards, in host and in device memory
        assert nref.same_bits(normals, host[0]) and nref.same_bits(curvature, host[1])
        assert nref.same_bits(dn.cpu().numpy(), host[0]) and nref.same_bits(dc.cpu().numpy(), host[1])
        p.p2p_close()
        p.set_clip_planes(None)
        p.set_point_keep(None)
        # issued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.select_segments(r, sc.COS_ANGLE, normals, min_points=2)
        p.wait_outputs(0)
        o = orc.project(xyzw, rgba, P2, W, H)
        assert np.array_equal(depth.view(np.uint32), o["depth_bits"]) and np.array_equal(img, o["img"])
    finally:
        p.close()


def test_errors_leave_the_selection_intact(pkg, orc):
    L = pkg._lib
    n = 20_001
    xyzw, rgba = orc.generate("room_shell", 4, 0, n, n)
    normals = np.tile(f32([0, 0, 1]), (n, 1))
    curvature = np.zeros(n, f32)
    fresh = pkg.Projector(0)
    try:
        with pytest.raises(pkg.RtrError) as e:
            fresh.select_segments(0.25, 0.9, np.zeros((0, 3), f32))
        assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        want, _ = _want(cr.labels(xyzw, 0.1), (3, 0))
        assert 0 < want.sum() < n
        p.select_segments(0.1, 0.9, normals, min_points=3)
        assert np.array_equal(_sel(pkg, p, n), want)
        options = {k: p.get_option(k) for k in ("clusters_keys_us", "clusters_sort_us", "clusters_label_us", "clusters_pair_tests_k",
                                                "selection", "resident_millibytes_per_point")}
        lib, ctx = p._lib, p._ctx
        den = np.array([1], np.uint32).view(f32)[0]
        nan, inf = float("nan"), float("inf")
        ok = dict(radius=0.1, cos=0.9, normals=True, curvature=True, max_curvature=0.5, lo=1, hi=0, flags=0, op=0)
        bad = [(dict(radius=v), "radius") for v in (0.0, -0.0, -0.25, nan, inf, -inf)]
        bad += [(dict(radius=v), "square of radius") for v in (float(den), 1e-20, 1e-30, 2e19, 3e38)]  # (r2 subnormal, 0 or infinite)
        bad += [(dict(cos=v), "cos_angle") for v in (0.0, -0.0, -0.5, float(np.nextafter(f32(1), f32(2))), 2.0, nan, inf, -inf)]
        bad += [(dict(normals=False), "normals"), (dict(normals=False, curvature=False), "normals")]
        bad += [(dict(max_curvature=nan), "max_curvature")]
        bad += [(dict(lo=0), "min_points"), (dict(lo=0, hi=5, flags=1), "min_points")]
        bad += [(dict(lo=lo, hi=hi), "max_points") for lo, hi in ((2, 1), (50, 49), (2 ** 32 - 1, 7))]
        bad += [(dict(flags=flags), "flags") for flags in (4, 5, 7, 8, -1, 256)]
        bad += [(dict(op=op), "op") for op in (-1, 9, 10, 11, 13, 16, 32)]
        for change, named in bad:
            a = dict(ok, **change)
            st = np.full(4, 77, np.uint64)
            lab = np.full(n, 0x5A5A5A5A, np.uint32)
            rc = lib.rtr_select_segments(ctx, a["radius"], a["cos"], _vp(normals) if a["normals"] else None, _vp(curvature) if a["curvature"] else None,
                                         a["max_curvature"], a["lo"], a["hi"], a["flags"], a["op"], _vp(lab), _vp(st))
            assert rc == L.RTR_ERR_INVALID, change
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_select_segments" in text and named in text, (change, text)
            assert np.array_equal(_sel(pkg, p, n), want) and (st == 77).all() and (lab == 0x5A5A5A5A).all(), change
            assert {k: p.get_option(k) for k in options} == options, change
        # a NaN max_curvature is not read without a curvature array; cos_angle = 1 and both flags together are legal
        assert lib.rtr_select_segments(ctx, 0.1, 0.9, _vp(normals), None, nan, 3, 0, 0, 0, None, None) == 0
        assert lib.rtr_select_segments(ctx, 0.1, 1.0, _vp(normals), _vp(curvature), inf, 3, 0, 3, 0, None, None) == 0
        assert np.array_equal(_sel(pkg, p, n), want)
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        with pytest.raises(pkg.RtrError) as e:
            p.select_segments(0.1, 0.9, normals, min_points=2)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert np.array_equal(_sel(pkg, p, n), want)
        # an error on a context without a selection makes none
        p.clear_selection()
        assert lib.rtr_select_segments(ctx, 0.1, 0.9, None, None, 0.0, 1, 0, 0, 0, None, None) == L.RTR_ERR_INVALID and p.selection() is None
        assert p.get_option("selection") == 0
    finally:
        p.close()
