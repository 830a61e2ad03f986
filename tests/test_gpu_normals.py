"""Normals and curvature on the GPU (include/rtr_normals.h section 6o): rtr_estimate_normals' normals, curvature and found
compared bit for bit, and its four statistics exactly, with the numpy reference of tests/normals_ref.py -- in every form
the cloud can take, on the scenes and special clouds of normals_cases.py, with and without a viewpoint; identical across
forms and calls; ragged point counts and every k at which the kernel changes its row capacity; outputs in host memory,
in device memory and NULL; the rows against rtr_nearest_k_points on the device; the error paths; and what the call must
leave alone."""
import ctypes as C

import numpy as np
import pytest

import normals_cases as ncs
import normals_ref as nf
import voxel_ref as vr
from test_gpu_select import FORMS, _new, _sel

pytestmark = pytest.mark.gpu

f32 = np.float32
THREE_FORMS = (("packed", {}, False), ("unpacked", {"pack": 0}, False), ("sorted", {"point_ids": 1}, True))
OTHER_VIEW = (0.5, -0.25, 2.0)  # for the cases that name no viewpoint of their own


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cloud(orc, xyz, seed=7):
    """(xyzw, rgba) with the given coordinates"""
    n = xyz.shape[0]
    xyzw, rgba = orc.generate("room_shell", seed, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = xyz
    return xyzw, rgba


def _check(got, e, what):
    nrm, curv, fd, st = got
    assert np.array_equal(fd, e["found"]), (what, np.flatnonzero(fd != e["found"])[:5])
    bad = np.flatnonzero((nf.bits(nrm) != nf.bits(e["normals"])).any(axis=1))
    assert bad.size == 0, (what, bad[:5], nrm[bad[:3]], e["normals"][bad[:3]])
    assert nf.same_bits(curv, e["curvature"]), (what, np.flatnonzero(nf.bits(curv) != nf.bits(e["curvature"]))[:5])
    assert st == e["stats"], (what, st, e["stats"])


def _views(vp):
    return (None, vp) if vp is not None else (None, OTHER_VIEW)


@pytest.fixture(scope="module")
def scene_refs(orc):
    """(scene, radius) -> (xyzw, rgba, {(k, viewpoint): normals_ref.estimate}): computed once, never changed."""
    out = {}
    for scene, (n, radii) in ncs.SCENES.items():
        xyzw, rgba = orc.generate(scene, ncs.SEED, 0, n, n)
        for r in radii:
            rk = nf.rows(xyzw, r, max(ncs.KS))
            out[(scene, r)] = (xyzw, rgba, {(k, vp): nf.estimate(xyzw, r, k, vp, rows_k=rk) for k in ncs.KS for vp in _views(ncs.SCENE_VIEWPOINT)})
    return out


@pytest.mark.parametrize("form", sorted(FORMS))
def test_everything_matches_the_reference_in_every_form(pkg, scene_refs, form):
    options, sort = FORMS[form]
    for scene, (n, radii) in ncs.SCENES.items():
        xyzw, rgba, _ = scene_refs[(scene, radii[0])]
        opts = dict(options)
        if scene == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            if form == "sorted":
                assert p.get_option("reordered") == 1
            for r in radii:
                for (k, vp), e in scene_refs[(scene, r)][2].items():
                    assert 0 < e["stats"][0] <= n and (vp is None or 0 < e["stats"][3] < e["stats"][0])
                    got = p.estimate_normals(k, r, vp, found=True)
                    _check(got, e, (form, scene, r, k, vp))
                again = p.estimate_normals(k, r, vp, found=True)  # (a second call: the same bits)
                _check(again, e, (form, scene, r, "again"))
            for key in ("normals_us0", "normals_us1", "normals_us2", "normals_pair_tests_k", "normals_row_updates_k"):
                assert p.get_option(key) > 0, key
            assert p.selection() is None and p.get_option("selection") == 0
        finally:
            p.close()


@pytest.mark.parametrize("case", [c[0] for c in ncs.special_cases()])
def test_the_special_clouds(pkg, orc, case):
    name, xyz, r, ks, vp = next(c for c in ncs.special_cases() if c[0] == case)
    xyzw, rgba = _cloud(orc, xyz)
    n = xyz.shape[0]
    rk = nf.rows(xyz, r, max(ks))
    refs = {(k, view): nf.estimate(xyz, r, k, view, rows_k=rk) for k in ks for view in _views(vp)}
    if case in ("lattice", "lattice_from_below"):
        sign = -1.0 if case == "lattice_from_below" else 1.0
        for k in ks:
            e = refs[(k, vp)]
            assert (e["normals"] == f32([0, 0, sign])).all() and e["stats"] == (n, 0, 0, n if sign < 0 else 0)
    if case == "piles":
        _, big, small, rest = ncs.piles()
        assert all((refs[(k, None)]["normals"][np.r_[big, small]] == f32([1, 0, 0])).all() for k in ks)
    if case == "sphere_shell":
        assert all((refs[(k, None)]["curvature"] > 0).all() for k in ks)
    for form, options, sort in THREE_FORMS + (("hash", {"auto_reorder": 0, "pack": 2}, False),):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for (k, view), e in refs.items():
                _check(p.estimate_normals(k, r, view, found=True), e, (case, form, k, view))
        finally:
            p.close()


def test_the_dense_cloud_replaces_in_every_row(pkg, orc):
    xyz = ncs.dense_cloud()
    n, r, k = ncs.DENSE_N, ncs.DENSE_RADIUS, ncs.DENSE_K
    xyzw, rgba = _cloud(orc, xyz, 3)
    rk = nf.rows(xyz, r, k)
    refs = {view: nf.estimate(xyz, r, k, view, rows_k=rk) for view in _views(None)}
    assert (refs[None]["found"] == k).all()
    for form, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for view, e in refs.items():
                _check(p.estimate_normals(k, r, view, found=True), e, (form, view))
            # every row filled and then replaced in: more entries written than slots
            assert p.get_option("normals_row_updates_k") * 1000 > n * k
        finally:
            p.close()


def _ragged(n):
    rng = np.random.default_rng(100 + n)
    return (rng.normal(size=(n, 3)) * (0.05 if n <= 3 else 0.15 if n <= 257 else 0.5)).astype(f32), (0.35 if n <= 257 else 0.3)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 4099])
def test_ragged_counts_and_every_k(pkg, orc, n):
    xyz, r = _ragged(n)
    xyzw, rgba = _cloud(orc, xyz, 100 + n)
    rk = nf.rows(xyz, r, 64)
    refs = {k: nf.estimate(xyz, r, k, OTHER_VIEW if k % 2 else None, rows_k=rk) for k in (1, 2, 7, 8, 9, 63, 64)}
    assert n != 1 or refs[8]["stats"] == (0, 1, 0, 0)
    assert n != 2 or refs[8]["stats"] == (0, 2, 0, 0)
    assert n != 3 or refs[8]["stats"][0] == 3
    assert n < 63 or refs[2]["stats"][0] > n // 2
    assert n < 255 or (refs[64]["found"] == 64).sum() > n // 4  # (rows of every capacity fill and overflow)
    for form, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for k, e in refs.items():
                _check(p.estimate_normals(k, r, OTHER_VIEW if k % 2 else None, found=True), e, (n, form, k))
        finally:
            p.close()


def test_rows_equal_the_nearest_k_rows_on_the_device(pkg, orc):
    """extract_points, then nearest_k_points(k + 1) on the device: the same found, and the same normals when the
    reference's sums and fit run over THOSE rows with the own index dropped."""
    import torch
    n = 4099
    xyz, r = _ragged(n)
    xyzw, rgba = _cloud(orc, xyz, 100 + n)
    for form, options, sort in THREE_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            dev = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            assert p.extract_points(out={"xyz": dev}) == n
            assert nf.same_bits(dev.cpu().numpy()[:, :3], xyz)
            for k in (1, 8, 63):
                idx, d2, found, _ = p.nearest_k_points(dev, k + 1, r)
                idx, d2, found = idx.cpu().numpy().view(np.uint32), d2.cpu().numpy(), found.cpu().numpy().view(np.uint32)
                ridx, rd2, rfound = nf.rows_from_nearest_k(idx, d2, found, k)
                S, Q = nf.sums(xyz, ridx, rfound)
                want_n, want_c, _ = nf.fit(xyz, nf.covariance(S, Q, rfound), rfound)
                nrm, curv, fd, st = p.estimate_normals(k, r, found=True)
                assert np.array_equal(fd, rfound), (form, k)
                assert nf.same_bits(nrm, want_n) and nf.same_bits(curv, want_c), (form, k)
        finally:
            p.close()


def _raw(p, k, r, flags, view, nrm, curv, fd, st):
    ptr = lambda a: a if (a is None or isinstance(a, C.c_void_p)) else _vp(a)  # noqa: E731
    return p._lib.rtr_estimate_normals(p._ctx, k, r, flags, ptr(view), ptr(nrm), ptr(curv), ptr(fd), ptr(st))


def test_outputs_in_host_and_device_memory_and_each_null(pkg, scene_refs):
    import torch
    L = pkg._lib
    scene, r, k = "uniform_box", 0.12, 8
    xyzw, rgba, refs = scene_refs[(scene, r)]
    n = xyzw.shape[0]
    e = refs[(k, None)]
    p = _new(pkg, {"point_ids": 1}, xyzw, rgba)
    try:
        dev = lambda t: None if t is None else (C.c_void_p(t.data_ptr()) if hasattr(t, "data_ptr") else t)  # noqa: E731
        for n_at in ("host", "device", None):
            for c_at in ("host", "device", None):
                for f_at in ("host", "device", None):
                    nrm = {"host": np.full((n, 3), 7, f32), "device": torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda"), None: None}[n_at]
                    curv = {"host": np.full(n, 7, f32), "device": torch.full((n,), 7.0, dtype=torch.float32, device="cuda"), None: None}[c_at]
                    fd = {"host": np.full(n, 7, np.uint32), "device": torch.full((n,), 7, dtype=torch.int32, device="cuda"), None: None}[f_at]
                    st = np.full(4, 77, np.uint64)
                    what = (n_at, c_at, f_at)
                    assert _raw(p, k, r, 0, None, dev(nrm), dev(curv), dev(fd), st) == L.RTR_OK, what
                    assert tuple(int(v) for v in st) == e["stats"], what
                    if nrm is not None:
                        assert nf.same_bits(nrm if n_at == "host" else nrm.cpu().numpy(), e["normals"]), what
                    if curv is not None:
                        assert nf.same_bits(curv if c_at == "host" else curv.cpu().numpy(), e["curvature"]), what
                    if fd is not None:
                        assert np.array_equal(fd if f_at == "host" else fd.cpu().numpy().view(np.uint32), e["found"]), what
        assert _raw(p, k, r, 0, None, None, None, None, None) == L.RTR_OK  # (everything NULL: legal, nothing to see)
        # the facade's device form: torch tensors on the context's device, the same bits
        nrm, curv, fd, st = p.estimate_normals(k, r, found=True, device=True)
        assert nrm.is_cuda and tuple(nrm.shape) == (n, 3) and st == e["stats"]
        assert nf.same_bits(nrm.cpu().numpy(), e["normals"]) and nf.same_bits(curv.cpu().numpy(), e["curvature"])
        assert np.array_equal(fd.cpu().numpy().view(np.uint32), e["found"])
    finally:
        p.close()


def test_errors_leave_everything_intact(pkg, orc):
    L = pkg._lib
    n = 20_001
    xyzw, rgba = orc.generate("room_shell", 4, 0, n, n)
    fresh = pkg.Projector(0)
    try:
        with pytest.raises(pkg.RtrError) as e:
            fresh.estimate_normals(8, 0.25)
        assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        vox, _ = vr.select(xyzw, 0.25)
        p.select_voxel_grid(0.25, stats=False)
        lib, ctx = p._lib, p._ctx
        den = float(np.array([1], np.uint32).view(f32)[0])
        V = L.NORMAL_VIEWPOINT
        ok = dict(k=8, r=0.1, flags=0, view=(0.0, 0.0, 0.0))
        bad = [(dict(r=v), "radius") for v in (0.0, -0.0, -0.25, np.nan, np.inf, -np.inf)]
        bad += [(dict(r=v), "square of radius") for v in (den, 1e-20, 1e-30, 2e19, 3e38)]  # (r2 subnormal, 0 or infinite)
        bad += [(dict(k=v), "k outside") for v in (0, 65, 2 ** 32 - 1)]
        bad += [(dict(flags=v), "flags") for v in (2, 3, 4, -1, 1 << 30)]
        bad += [(dict(flags=V, view=None), "viewpoint is NULL")]
        bad += [(dict(flags=V, view=v), "viewpoint has a non-finite") for v in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf))]
        for change, word in bad:
            a = dict(ok, **change)
            st, nrm, curv, fd = np.full(4, 77, np.uint64), np.full((n, 3), 7, f32), np.full(n, 7, f32), np.full(n, 7, np.uint32)
            view = None if a["view"] is None else f32(a["view"])
            assert _raw(p, a["k"], a["r"], a["flags"], view, nrm, curv, fd, st) == L.RTR_ERR_INVALID, change
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_estimate_normals" in text and word in text, (change, text)
            assert np.array_equal(_sel(pkg, p, n), vox) and p.get_option("selection") == 1, change
            assert (st == 77).all() and (nrm == 7).all() and (curv == 7).all() and (fd == 7).all(), change
        # without the flag the viewpoint is not read: NULL and NaN alike
        assert _raw(p, 8, 0.1, 0, None, None, None, None, None) == L.RTR_OK
        assert _raw(p, 8, 0.1, 0, f32([np.nan, 0, 0]), None, None, None, None) == L.RTR_OK
        # a finite point beyond the span -- +-FLT_MAX among them: found by the key sweep, before anything is written
        for far in (f32(2.0 ** 20 * 0.1 * 1.0011), np.finfo(f32).max, -np.finfo(f32).max):
            moved = xyzw.copy()
            moved[777, 0] = far
            q = _new(pkg, {}, moved, rgba)
            try:
                st, nrm, curv, fd = np.full(4, 77, np.uint64), np.full((n, 3), 7, f32), np.full(n, 7, f32), np.full(n, 7, np.uint32)
                assert _raw(q, 8, 0.1, 0, None, nrm, curv, fd, st) == L.RTR_ERR_UNSUPPORTED, far
                assert "span" in q._lib.rtr_last_error(q._ctx).decode()
                assert (st == 77).all() and (nrm == 7).all() and (curv == 7).all() and (fd == 7).all()
                assert q.get_option("selection") == 0 and q.selection() is None
            finally:
                q.close()
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        with pytest.raises(pkg.RtrError) as e:
            p.estimate_normals(8, 0.1)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert np.array_equal(_sel(pkg, p, n), vox)
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
            return [p.download(b).copy() for b in (L.BUF_DEPTH, L.BUF_IMAGE, L.BUF_TENSOR, L.BUF_VISIBLE, L.BUF_POINT_ID, L.BUF_POINT_KEEP,
                                                   L.BUF_SELECTION)] + \
                   [p.clip_planes(), p.frame_stats(), p.get_option("p2p_open"), p.get_option("packed"), p.get_option("reordered"),
                    p.get_option("point_keep"), p.num_points, p.get_option("resident_millibytes_per_point"), p.get_option("selection")]

        def same(a, b):
            return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

        p.set_clip_planes(planes)
        p.set_point_keep(keep)
        p.p2p_open(0, 1, [p.p2p_export()])  # (the one-rank form of test_gpu_p2p.py: a rank maps its own buffers)
        p.p2p_render(P, True)
        p.point_pass(P)
        p.select_points(planes=f32([[1, 0, 0, 0.05]]), stats=False)
        before = state()
        rk = nf.rows(xyzw, 0.12, 16)
        for k, view in ((8, None), (16, (0.0, 0.0, 1.5))):
            e = nf.estimate(xyzw, 0.12, k, view, rows_k=rk)
            _check(p.estimate_normals(k, 0.12, view, found=True), e, (k, view))  # (the clip planes and the keep mask in force play no part)
            assert same(before, state()) and p.get_option("p2p_open") == 1, k
        p.p2p_close()
        p.set_clip_planes(None)
        p.set_point_keep(None)
        # issued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.estimate_normals(8, 0.12)
        p.wait_outputs(0)
        o = orc.project(xyzw, rgba, P2, W, H)
        assert np.array_equal(depth.view(np.uint32), o["depth_bits"]) and np.array_equal(img, o["img"])
    finally:
        p.close()
