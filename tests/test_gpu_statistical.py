"""Selecting by mean neighbour distance on the GPU (include/rtr_statistics.h section 6n): rtr_select_statistical's words,
mean_dist and found compared bit for bit, and its four statistics exactly, with the numpy reference of
tests/statistical_ref.py -- in every form the cloud can take, on the scenes of statistical_cases.py and the dense cloud
whose rows all overflow; the moments against numpy float64 within the bound of a reordered sum and bit-identical across
forms and calls; the rows against rtr_nearest_k_points on the device; ragged point counts with every op chained between
other selection calls; coincident piles, the lattice, subnormal distances, special coordinates; outputs in host and in
device memory; the error paths and what the call must leave alone; removeStatisticalOutliers against an upload of A[hit]
and the oracle."""
import ctypes as C

import numpy as np
import pytest

import neighbours_ref as nr
import select_ref as sr
import statistical_cases as sc
import statistical_ref as sf
import voxel_ref as vr
from test_gpu_select import FORMS, _new, _sel
from test_gpu_voxel import _frames, _same_frames

pytestmark = pytest.mark.gpu

f32 = np.float32
THREE_FORMS = (("packed", {}, False), ("unpacked", {"pack": 0}, False), ("sorted", {"point_ids": 1}, True))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _close(got, want, c):
    tol = sf.moments_tolerance(c)
    return all(abs(g - w) <= tol * abs(w) for g, w in zip(got, want))


def _check(pkg, p, n, xyzw, s, got, outside=False, what=None, want_sel=None):
    """got: select_statistical(..., mean_dist=True, found=True)'s tuple; s: statistical_ref.select's dict."""
    st, mom, md, fd = got
    c = int((s["found"] > 0).sum())
    assert np.array_equal(fd, s["found"]), what
    assert np.array_equal(_bits(md), _bits(s["mean"])), (what, np.flatnonzero(_bits(md) != _bits(s["mean"]))[:5])
    assert _close(mom, s["moments"], c), (what, mom, s["moments"])
    hit = sf.hits(md, fd, mom[2])  # (the words are the hits recomputed from the RETURNED t, exactly)
    assert np.array_equal(hit, s["hit"]), what
    want = (hit != outside) if want_sel is None else want_sel
    assert st == (int(want.sum()),) + s["stats"], (what, st, s["stats"])
    assert np.array_equal(_sel(pkg, p, n), want), what


@pytest.fixture(scope="module")
def clouds(orc):
    """(scene, radius) -> (xyzw, rgba, statistical_ref.rows at the largest k): computed once, never changed."""
    out = {}
    for scene, (n, radii) in sc.SCENES.items():
        xyzw, rgba = orc.generate(scene, sc.SEED, 0, n, n)
        for r in radii:
            out[(scene, r)] = (xyzw, rgba, sf.rows(xyzw, r, max(sc.KS)))
    return out


_shared = {}  # (scene, radius, k, std_mul) -> the moments of the first form that ran: every other form returns the same bits


@pytest.mark.parametrize("form", sorted(FORMS))
def test_everything_matches_the_reference_in_every_form(pkg, clouds, form):
    L = pkg._lib
    options, sort = FORMS[form]
    for scene, (n, radii) in sc.SCENES.items():
        xyzw, rgba, _ = clouds[(scene, radii[0])]
        opts = dict(options)
        if scene == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            if form == "sorted":
                assert p.get_option("reordered") == 1
            for r in radii:
                rf = clouds[(scene, r)][2]
                for k in sc.KS:
                    for mul in sc.STD_MULS:
                        s = sf.select(xyzw, r, k, mul, rows_found=rf)
                        assert s["stats"][0] == sc.pin((scene, r), k, mul)  # (test_statistical_host.py: pinned and spread without a GPU)
                        outside = mul == 1
                        got = p.select_statistical(k, r, mul, outside=outside, mean_dist=True, found=True)
                        _check(pkg, p, n, xyzw, s, got, outside, (form, scene, r, k, mul))
                        again = p.select_statistical(k, r, mul, stats=False)  # (a second call: the same bits)
                        assert again[0] == got[1] == _shared.setdefault((scene, r, k, mul), got[1]), (form, scene, r, k, mul)
                    # the threshold given: t from numpy, everything bit for bit
                    s = sf.select(xyzw, r, k, 1, rows_found=rf)
                    t = s["moments"][2]
                    got = p.select_statistical(k, r, std_mul=np.nan, threshold=t, mean_dist=True, found=True)
                    assert got[1][2] == t and got[1][:2] == _shared[(scene, r, k, 1)][:2]
                    _check(pkg, p, n, xyzw, s, got, False, (form, scene, r, k, "given"))
            assert p.get_option("statistical_us0") > 0 and p.get_option("statistical_us1") > 0 and p.get_option("statistical_us2") > 0
            assert p.get_option("statistical_pair_tests_k") > 0 and p.get_option("statistical_row_updates_k") > 0
        finally:
            p.close()


def test_rows_equal_the_nearest_k_rows_on_the_device(pkg, clouds):
    scene, r = "room_shell", 0.18
    xyzw, rgba, _ = clouds[(scene, r)]
    n = xyzw.shape[0]
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            xyz = p.extract_points(rgb=False)[0]
            assert np.array_equal(_bits(xyz[:, :3]), _bits(xyzw[:, :3]))
            for k in (1, 8, 63):
                idx, d2, found, _ = p.nearest_k_points(xyz, k + 1, r)
                own = idx == np.arange(n, dtype=np.uint32)[:, None]
                assert (own.sum(axis=1) == 1).all()  # (no pile of k + 1 copies in this scene)
                rows = np.where(own, f32(np.inf), d2)
                rows = np.sort(rows.view(np.uint32), axis=1).view(f32)[:, :k]  # (bits order = value order for d2 >= +0 and +inf)
                cnt = np.minimum(found - 1, k).astype(np.uint32)
                _, mom, md, fd = p.select_statistical(k, r, mean_dist=True, found=True)
                assert np.array_equal(fd, cnt), (name, k)
                assert np.array_equal(_bits(md), _bits(sf.means(np.ascontiguousarray(rows), cnt))), (name, k)
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
    rf = sf.rows(xyzw, r, 64)
    ref = {(k, mul): sf.select(xyzw, r, k, mul, rows_found=rf) for k, mul in ((3, 0.0), (8, 1.0), (64, -0.5), (1, 0.5))}
    assert n < 63 or all(0 < s["hit"].sum() < n for s in ref.values())
    assert n != 1 or (ref[(3, 0.0)]["stats"] == (0, 1, 0) and ref[(3, 0.0)]["moments"] == (0.0, 0.0, 0.0))
    assert n != 2 or ref[(3, 0.0)]["hit"].all()  # (c = 2: both means equal, sigma 0, t = mu)
    planes = f32([[1, 0, 0, 0.05]])
    half = pkg.clip_keep(planes, xyzw)
    vox, _ = vr.select(xyzw, 0.25, (0.013, -0.4, 0), 1)
    moments = {}
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            sel = np.zeros(n, bool)
            for step in (("st", 3, 0.0, "replace", False), ("planes", "add"), ("st", 8, 1.0, "toggle", True), ("voxel", "subtract"),
                         ("st", 64, -0.5, "add", False), ("st", 1, 0.5, "intersect", True), ("planes", "toggle"),
                         ("st", 8, 1.0, "subtract", False), ("voxel", "add"), ("st", 64, -0.5, "intersect", False),
                         ("st", 3, 0.0, "replace", True), ("st", 1, 0.5, "toggle", False)):
                if step[0] == "planes":
                    sel = sr.combine(step[1], sel, half)
                    assert p.select_points(planes=planes, op=step[1])[0] == int(sel.sum())
                elif step[0] == "voxel":
                    sel = sr.combine(step[1], sel, vox)
                    assert p.select_voxel_grid(0.25, (0.013, -0.4, 0), op=step[1])[0] == int(sel.sum())
                else:
                    _, k, mul, op, outside = step
                    s = ref[(k, mul)]
                    sel = sr.combine(op, sel, s["hit"] != outside)
                    got = p.select_statistical(k, r, mul, op=op, outside=outside, mean_dist=True, found=True)
                    _check(pkg, p, n, xyzw, s, got, outside, (n, name, step), want_sel=sel)  # (_sel: no bit at or past n)
                    assert moments.setdefault((k, mul), got[1]) == got[1], (n, name, step)
                    continue
                assert np.array_equal(_sel(pkg, p, n), sel), (n, name, step)
            # the combining ops on a selection that does not exist yet: it counts as empty
            hit = ref[(8, 1.0)]["hit"]
            for op, want in (("add", hit), ("subtract", np.zeros(n, bool)), ("intersect", np.zeros(n, bool)), ("toggle", hit)):
                p.clear_selection()
                assert p.select_statistical(8, r, op=op, stats=False) == (moments[(8, 1.0)],)
                assert np.array_equal(_sel(pkg, p, n), want), op
        finally:
            p.close()


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
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for k in (1, 8, 64):
                s = sf.select(xyzw, r, k)
                assert (s["found"][big] == k).all() and (s["found"][small] == min(k, 64)).all() and not s["found"][rest].any()
                assert not _bits(s["mean"])[np.r_[big, small]].any() and s["moments"] == (0.0, 0.0, 0.0) and s["stats"] == (3065, 500, 0)
                got = p.select_statistical(k, r, mean_dist=True, found=True)
                assert got[1] == (0.0, 0.0, 0.0)
                _check(pkg, p, n, xyzw, s, got, False, (name, k))
            assert p.get_option("statistical_pair_tests_k") >= (3000 * 3000 + 65 * 65) // 1000
        finally:
            p.close()


def test_the_dense_cloud_replaces_in_every_row(pkg, orc):
    xyz = sc.dense_cloud()
    n = sc.DENSE_N
    xyzw, rgba = orc.generate("room_shell", 3, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = xyz
    rf = sf.rows(xyz, sc.DENSE_RADIUS, 64)
    moments = {}
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for k in sc.DENSE_KS:
                for mul in sc.STD_MULS:
                    s = sf.select(xyzw, sc.DENSE_RADIUS, k, mul, rows_found=rf)
                    assert s["stats"][0] == sc.DENSE_PINS[(k, mul)]
                    got = p.select_statistical(k, sc.DENSE_RADIUS, mul, mean_dist=True, found=True)
                    _check(pkg, p, n, xyzw, s, got, False, (name, k, mul))
                    assert moments.setdefault((k, mul), got[1]) == got[1]
                # every row filled and then replaced in: more values written than slots
                assert p.get_option("statistical_row_updates_k") * 1000 > n * k
        finally:
            p.close()


def test_the_lattice_has_its_ties_at_the_rows_end(pkg, orc):
    lattice = (np.stack(np.meshgrid(*[np.arange(-7, 8)] * 3), -1).reshape(-1, 3) * 0.1).astype(f32)  # spacing = the radius
    n = lattice.shape[0]
    xyzw, rgba = orc.generate("room_shell", 5, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = lattice
    moments = {}
    for name, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for k in (1, 3, 5, 6, 8):
                s = sf.select(xyzw, 0.1, k)
                st, mom, md, fd = p.select_statistical(k, 0.1, mean_dist=True, found=True)
                assert np.array_equal(fd, s["found"]) and np.array_equal(_bits(md), _bits(s["mean"])), (name, k)
                assert abs(mom[0] - s["moments"][0]) <= sf.moments_tolerance(n) * s["moments"][0]
                hit = sf.hits(md, fd, mom[2])  # (sigma is tiny against mu here: the words are held to the returned t alone)
                assert st == (int(hit.sum()), int(hit.sum()), s["stats"][1], 0) and np.array_equal(_sel(pkg, p, n), hit), (name, k)
                assert moments.setdefault(k, mom) == mom
        finally:
            p.close()


def test_subnormal_distances_and_special_coordinates(pkg, orc):
    n = 4099
    xyzw, rgba = orc.generate("room_shell", 301, 0, n, n)
    xyzw = xyzw.copy()
    rng = np.random.default_rng(8)
    at = rng.choice(np.arange(300, 3500), 24, replace=False)
    xyzw[at[:9], 1] = np.tile(f32([np.nan, np.inf, -np.inf]), 3)
    # pairs 1e-20 apart at coordinates where fp32 can tell (the axis value is 0 or itself tiny), far from everything else
    for j, (a, b) in enumerate(zip(at[9:17:2], at[10:17:2])):
        xyzw[a, :3] = f32([40 + j, 0, 0])
        xyzw[b, :3] = f32([40 + j, 1e-20 * (j + 1), 0])
    xyzw[at[17], :3] = xyzw[at[18], :3] = f32([60, 60, 60])  # (a coincident pair)
    xyzw[at[19], :3] = f32([80, -80, 80])  # (an isolated point)
    r = 0.15
    bad = np.zeros(n, bool)
    bad[at[:9]] = True
    for k in (1, 4):
        s = sf.select(xyzw, r, k)
        tiny = s["mean"][at[9:17]]
        assert (tiny > 0).all() and (tiny < 1e-19).all() and (s["rows"][at[9:17], 0] < np.finfo(f32).tiny).all()
        assert list(_bits(s["mean"][at[17:19]])) == [0, 0] and np.isinf(s["mean"][at[19]]) and np.isinf(s["mean"][bad]).all()
        assert s["stats"][1] >= 1 and s["stats"][2] == 9
        for name, options, sort in THREE_FORMS + (("hash", {"auto_reorder": 0, "pack": 2}, False),):
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                got = p.select_statistical(k, r, mean_dist=True, found=True)
                _check(pkg, p, n, xyzw, s, got, False, (name, k))
                assert not _sel(pkg, p, n)[bad].any() and not _sel(pkg, p, n)[at[19]]
                got = p.select_statistical(k, r, outside=True, mean_dist=True, found=True)
                _check(pkg, p, n, xyzw, s, got, True, (name, k, "outside"))
                assert _sel(pkg, p, n)[bad].all() and _sel(pkg, p, n)[at[19]]
            finally:
                p.close()


def _raw(p, k, r, mul, flags, op, mean, found, mom, st):
    ptr = lambda a: a if (a is None or isinstance(a, C.c_void_p)) else _vp(a)  # noqa: E731
    return p._lib.rtr_select_statistical(p._ctx, k, r, mul, flags, op, ptr(mean), ptr(found), ptr(mom), ptr(st))


def test_outputs_in_host_and_device_memory_and_each_null(pkg, clouds):
    import torch
    L = pkg._lib
    scene, r, k = "uniform_box", 0.12, 8
    xyzw, rgba, rf = clouds[(scene, r)]
    n = xyzw.shape[0]
    s = sf.select(xyzw, r, k, 1, rows_found=rf)
    p = _new(pkg, {"point_ids": 1}, xyzw, rgba)
    try:
        want_mom = None
        for mean_at in ("host", "device", None):
            for found_at in ("host", "device", None):
                for with_mom in (True, False):
                    md = {"host": np.full(n, 7, f32), "device": torch.full((n,), 7.0, dtype=torch.float32, device="cuda"), None: None}[mean_at]
                    fd = {"host": np.full(n, 7, np.uint32), "device": torch.full((n,), 7, dtype=torch.int32, device="cuda"), None: None}[found_at]
                    mom = np.full(3, -1.0) if with_mom else None
                    st = np.full(4, 77, np.uint64)
                    dev = lambda t: None if t is None else (C.c_void_p(t.data_ptr()) if hasattr(t, "data_ptr") else t)  # noqa: E731
                    assert _raw(p, k, r, 1.0, 0, 0, dev(md), dev(fd), mom, st) == L.RTR_OK, (mean_at, found_at, with_mom)
                    assert tuple(int(v) for v in st) == (s["stats"][0],) + s["stats"]
                    if md is not None:
                        got = md if mean_at == "host" else md.cpu().numpy()
                        assert np.array_equal(_bits(got), _bits(s["mean"])), (mean_at, found_at)
                    if fd is not None:
                        got = fd if found_at == "host" else fd.cpu().numpy().view(np.uint32)
                        assert np.array_equal(got, s["found"]), (mean_at, found_at)
                    if with_mom:
                        want_mom = want_mom if want_mom is not None else tuple(mom)
                        assert tuple(mom) == want_mom and _close(mom, s["moments"], n)
        assert _raw(p, k, r, 1.0, 0, 0, None, None, None, None) == L.RTR_OK  # (everything NULL: the selection alone)
        assert np.array_equal(_sel(pkg, p, n), s["hit"])
    finally:
        p.close()


def test_errors_leave_everything_intact(pkg, orc):
    L = pkg._lib
    n = 20_001
    xyzw, rgba = orc.generate("room_shell", 4, 0, n, n)
    fresh = pkg.Projector(0)
    try:
        with pytest.raises(pkg.RtrError) as e:
            fresh.select_statistical(8, 0.25)
        assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        want = sf.select(xyzw, 0.1, 8)["hit"]
        assert 0 < want.sum() < n
        p.select_statistical(8, 0.1)
        lib, ctx = p._lib, p._ctx
        den = float(np.array([1], np.uint32).view(f32)[0])
        G = L.STAT_THRESHOLD_GIVEN
        ok = dict(k=8, r=0.1, mul=1.0, flags=0, op=0, t=0.5)
        bad = [(dict(r=v), "radius") for v in (0.0, -0.0, -0.25, np.nan, np.inf, -np.inf)]
        bad += [(dict(r=v), "square of radius") for v in (den, 1e-20, 1e-30, 2e19, 3e38)]  # (r2 subnormal, 0 or infinite)
        bad += [(dict(k=v), "k outside") for v in (0, 65, 2 ** 32 - 1)]
        bad += [(dict(mul=v), "std_mul") for v in (np.nan, np.inf, -np.inf)]
        bad += [(dict(flags=v), "flags") for v in (2, 3, 4, -1, 1 << 30)]
        bad += [(dict(flags=G, t=np.nan), "moments[2]"), (dict(flags=G, t=None), "moments is NULL")]
        bad += [(dict(op=v), "op") for v in (-1, 9, 10, 11, 13, 16, 32)]
        for change, word in bad:
            a = dict(ok, **change)
            st, md, fd = np.full(4, 77, np.uint64), np.full(n, 7, f32), np.full(n, 7, np.uint32)
            mom = None if a["t"] is None else np.array([-1.0, -2.0, a["t"]])
            before = None if mom is None else mom.tobytes()
            assert _raw(p, a["k"], a["r"], a["mul"], a["flags"], a["op"], md, fd, mom, st) == L.RTR_ERR_INVALID, change
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_select_statistical" in text and word in text, (change, text)
            assert np.array_equal(_sel(pkg, p, n), want) and p.get_option("selection") == 1, change
            assert (st == 77).all() and (md == 7).all() and (fd == 7).all() and (mom is None or mom.tobytes() == before), change
        # std_mul is ignored with the flag, NaN or not; an infinite threshold is legal
        mom = np.array([0.0, 0.0, np.inf])
        assert _raw(p, 8, 0.1, np.nan, G, 0, None, None, mom, None) == L.RTR_OK and mom[2] == np.inf
        c = sf.select(xyzw, 0.1, 8)["found"] > 0
        assert np.array_equal(_sel(pkg, p, n), c)  # (t = +inf: every point with a neighbour)
        mom = np.array([0.0, 0.0, -np.inf])
        assert _raw(p, 8, 0.1, 1.0, G, 0, None, None, mom, None) == L.RTR_OK and not _sel(pkg, p, n).any()
        p.select_statistical(8, 0.1)
        # a finite point beyond the span: found by the key sweep, before anything changes
        moved = xyzw.copy()
        moved[777, 0] = f32(2.0 ** 20 * 0.1 * 1.0011)
        q = _new(pkg, {}, moved, rgba)
        try:
            vox, _ = vr.select(moved, 0.25)
            q.select_voxel_grid(0.25, stats=False)
            st, md, fd, mom = np.full(4, 77, np.uint64), np.full(n, 7, f32), np.full(n, 7, np.uint32), np.full(3, -1.0)
            assert _raw(q, 8, 0.1, 1.0, 0, 0, md, fd, mom, st) == L.RTR_ERR_UNSUPPORTED
            assert "span" in q._lib.rtr_last_error(q._ctx).decode()
            assert np.array_equal(_sel(pkg, q, n), vox) and (st == 77).all() and (md == 7).all() and (fd == 7).all() and (mom == -1).all()
            q.clear_selection()
            with pytest.raises(pkg.RtrError):
                q.select_statistical(8, 0.1, op="add")
            assert q.get_option("selection") == 0 and q.selection() is None
        finally:
            q.close()
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        with pytest.raises(pkg.RtrError) as e:
            p.select_statistical(8, 0.1)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert np.array_equal(_sel(pkg, p, n), want)
        # an error on a context without a selection makes none
        p.clear_selection()
        assert _raw(p, 0, 0.1, 1.0, 0, 0, None, None, None, None) == L.RTR_ERR_INVALID and p.selection() is None
        assert p.get_option("selection") == 0
    finally:
        p.close()


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
        rf = sf.rows(xyzw, 0.12, 16)
        for kw in (dict(k=8, std_mul=1.0), dict(k=16, std_mul=0.5, op="add"), dict(k=4, std_mul=2.0, op="toggle", outside=True, stats=False)):
            hit = sf.select(xyzw, 0.12, kw["k"], kw["std_mul"], rows_found=rf)["hit"]
            assert 0 < hit.sum() < n
            want = sr.combine(kw.get("op", "replace"), want, hit != kw.get("outside", False)) if want is not None else hit
            p.select_statistical(radius=0.12, **kw)
            assert np.array_equal(_sel(pkg, p, n), want), kw  # (the clip planes and the keep mask in force play no part)
        assert same(before, state()) and p.get_option("p2p_open") == 1
        p.p2p_close()
        p.set_clip_planes(None)
        p.set_point_keep(None)
        # issued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.select_statistical(8, 0.12)
        p.wait_outputs(0)
        o = orc.project(xyzw, rgba, P2, W, H)
        assert np.array_equal(depth.view(np.uint32), o["depth_bits"]) and np.array_equal(img, o["img"])
    finally:
        p.close()


@pytest.mark.parametrize("form", ["default", "sorted"])
def test_remove_statistical_outliers_cleans_the_cloud(pkg, orc, form):
    options, sort = FORMS[form]
    n, W, H = 120_001, 320, 240
    r, k, mul = 0.05, 8, 1.0
    xyzw, rgba = orc.generate("room_shell", 52, 0, n, n)
    s = sf.select(xyzw, r, k, mul)
    hit = s["hit"]
    assert n // 4 < hit.sum() < 9 * n // 10
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
        pc = pkg.ProjectCloud(xyzw, rgba, reorder=sort, point_ids=sort)
        assert pc.selectStatistical(k, r, mul) == int(hit.sum()) == pc.selectedCount()
        assert pc.removeStatisticalOutliers(k, r, mul) == int((~hit).sum()) and pc.projector.num_points == int(hit.sum())
        assert pc.projector.selection() is None and pc.selectedCount() == 0
        pc.projector.set_resolution(W, H)
        _same_frames(_frames(pkg, pc.projector, Ps), want, (form, "removeStatisticalOutliers"))
    finally:
        b.close()
