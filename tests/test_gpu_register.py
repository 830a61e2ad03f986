"""Registration on the GPU (include/rtr_register.h section 6p): rtr_register_points' moments and step compared bit for
bit, and its four statistics exactly, with the numpy reference of tests/register_ref.py -- in every form the cloud can take,
on the scenes and special clouds of register_cases.py, in both modes; given points and normals in host and in device
memory; with and without a pose; identical on a second call; every count at an edge of the summation shape; small clouds;
one winner and all-distinct winners; the degenerate cases; the error paths; what the call must leave alone; and
registerPoints through the Python facade against the reference loop."""
import ctypes as C

import numpy as np
import pytest

import nearest_ref as nr
import normals_ref as nf
import register_cases as rc
import register_ref as rr
import voxel_ref as vr
from test_gpu_select import FORMS, _new, _sel

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
IDENT = np.eye(4)[:3].copy()


def _cloud(orc, xyz, seed=7):
    n = xyz.shape[0]
    xyzw, rgba = orc.generate("room_shell", seed, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = xyz
    return xyzw, rgba


def _same(got, want, what):
    mom, step, st = got
    wm, ws, wst = want
    assert st == wst, (what, st, wst)
    bad = np.flatnonzero(rr.bits64(mom) != rr.bits64(wm))
    assert bad.size == 0, (what, "moments", bad[:6], mom[bad[:3]], wm[bad[:3]])
    assert np.array_equal(rr.bits64(step).reshape(-1), rr.bits64(ws).reshape(-1)), (what, "step", step, ws)


def _options(form):
    options, sort = FORMS[form]
    opts = dict(options)
    if form != "hash_unpacked":
        opts["point_ids"] = 1  # (the library may sort a hash-ordered cloud: the call then needs the upload indices)
    return opts, sort


@pytest.fixture(scope="module")
def special_refs():
    """name -> (case, {(plane, posed): register_ref.register}): computed once, never changed."""
    out = {}
    with np.errstate(all="ignore"):
        for name, c in rc.special_cases().items():
            refs = {}
            for plane in (0, 1):
                for pose in (None,) if c["pose"] is None else (None, c["pose"]):
                    refs[(plane, pose is not None)] = rr.register(c["res"], c["scan"], c["radius"], plane, pose, c["normals"] if plane else None)
            out[name] = (c, refs)
    return out


@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_special_clouds_in_every_form(pkg, orc, special_refs, form):
    opts, sort = _options(form)
    for name, (c, refs) in special_refs.items():
        xyzw, rgba = _cloud(orc, c["res"])
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            for (plane, posed), want in refs.items():
                got = p.register_points(c["scan"], c["radius"], bool(plane), c["pose"] if posed else None, c["normals"] if plane else None)
                _same(got, want, (form, name, plane, posed))
            assert p.selection() is None and p.get_option("selection") == 0
        finally:
            p.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_scenes_in_every_form(pkg, orc, form):
    opts, sort = _options(form)
    for scene in ("room_shell", "uniform_box"):
        c = rc.scene_case(orc, scene)
        n = c["res"].shape[0]
        xyzw, rgba = orc.generate(scene, rc.nbc.SEED, 0, n, n)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            if form == "sorted":
                assert p.get_option("reordered") == 1
            for plane in (0, 1):
                want = rr.register(c["res"], c["scan"], c["radius"], plane, rc.GENERAL_POSE, c["normals"] if plane else None, finder=nr.nearest_bucket)
                assert want[2][0] > 1000 and want[2][1] > 100 and want[2][3] == 0  # (pairs, and scan points without one)
                got = p.register_points(c["scan"], c["radius"], bool(plane), rc.GENERAL_POSE, c["normals"] if plane else None)
                _same(got, want, (form, scene, plane))
                _same(p.register_points(c["scan"], c["radius"], bool(plane), rc.GENERAL_POSE, c["normals"] if plane else None), want, "again")
        finally:
            p.close()


def test_host_and_device_inputs_and_the_poses(pkg, orc, special_refs):
    import torch
    c, refs = special_refs["corner"]
    xyzw, rgba = _cloud(orc, c["res"])
    p = _new(pkg, {}, xyzw, rgba)
    try:
        scan4 = np.concatenate([c["scan"], np.full((c["scan"].shape[0], 1), 7, f32)], axis=1)  # (stride 16)
        forms = {"host": (c["scan"], c["normals"]), "host16": (scan4, c["normals"]),
                 "device": (torch.from_numpy(c["scan"]).cuda(), torch.from_numpy(c["normals"]).cuda()),
                 "mixed": (torch.from_numpy(scan4).cuda(), c["normals"])}
        ident = rr.register(c["res"], c["scan"], c["radius"], 0, IDENT, None)
        assert np.array_equal(rr.bits64(ident[0]), rr.bits64(refs[(0, False)][0]))  # (the identity moves no bit)
        for where, (scan, nrm) in forms.items():
            before = scan.clone() if hasattr(scan, "clone") else scan.copy()
            for plane in (0, 1):
                for pose, posed in ((None, False), (IDENT, False), (np.eye(4), False), (c["pose"], True)):
                    got = p.register_points(scan, c["radius"], bool(plane), pose, nrm if plane else None)
                    _same(got, refs[(plane, posed)], (where, plane, posed))
            after = scan.cpu().numpy() if hasattr(scan, "cpu") else scan
            assert np.array_equal(np.asarray(before.cpu() if hasattr(before, "cpu") else before).view(np.uint32), after.view(np.uint32)), where
            if hasattr(nrm, "cpu"):
                assert np.array_equal(nrm.cpu().numpy().view(np.uint32), c["normals"].view(np.uint32))
    finally:
        p.close()


COUNTS = (0, 1, 2, 3, 5, 6, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4099)


def _ragged():
    rng = np.random.default_rng(4099)
    res = (rng.normal(size=(4099, 3)) * 0.5).astype(f32)
    M = rc.rigid(1.0, (2, -1, 1), (0.01, 0.01, -0.005))
    nrm = rc._unit(rng.normal(size=res.shape))
    return res, rc.unmoved(res, M), nrm


def test_every_count_at_an_edge_of_the_summation_shape(pkg, orc):
    res, scan, nrm = _ragged()
    xyzw, rgba = _cloud(orc, res, 11)
    gi = nr.nearest(res, scan, 0.08)[0]
    assert (gi != nr.NONE).mean() > 0.9
    p = _new(pkg, {}, xyzw, rgba)
    q = _new(pkg, {"point_ids": 1}, xyzw, rgba, sort=True)
    try:
        for count in COUNTS:
            for plane in (0, 1):
                want = rr.register(res, scan[:count], 0.08, plane, None, nrm if plane else None)
                if count < (6 if plane else 3):  # (the pair-count thresholds)
                    assert want[2][3] == 1, (count, plane, want[2])
                for ctx in (p, q):
                    _same(ctx.register_points(scan[:count], 0.08, bool(plane), None, nrm if plane else None), want, (count, plane))
    finally:
        p.close()
        q.close()


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_small_clouds(pkg, orc, n):
    rng = np.random.default_rng(n)
    res = (rng.normal(size=(n, 3)) * 0.2).astype(f32)
    scan = (np.repeat(res, 3, axis=0).astype(f64) + rng.normal(size=(3 * n, 3)) * 0.004).astype(f32)
    nrm = rc._unit(rng.normal(size=res.shape))
    xyzw, rgba = _cloud(orc, res, n)
    for options, sort in (({}, False), ({"pack": 0}, False), ({"point_ids": 1}, True)):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for plane in (0, 1):
                want = rr.register(res, scan, 0.05, plane, rc.GENERAL_POSE, nrm if plane else None)
                _same(p.register_points(scan, 0.05, bool(plane), rc.GENERAL_POSE, nrm if plane else None), want, (n, options, plane))
        finally:
            p.close()


def test_one_winner_and_all_distinct_winners(pkg, orc):
    rng = np.random.default_rng(77)
    n = 5000  # (twenty chunks)
    res = np.c_[np.arange(n) % 100, np.arange(n) // 100, np.zeros(n)].astype(f32)  # (a unit lattice: 1 apart)
    nrm = rc._unit(rng.normal(size=res.shape))
    xyzw, rgba = _cloud(orc, res, 5)
    one = (res[2345].astype(f64) + rng.normal(size=(700, 3)) * 0.05).astype(f32)      # every given point -> winner 2345
    spread = (res[::2].astype(f64) + rng.normal(size=(n // 2, 3)) * 0.05).astype(f32)  # 2500 distinct winners over all chunks
    for options, sort in (({}, False), ({"point_ids": 1}, True)):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for scan, winners in ((one, 1), (spread, n // 2)):
                gi = nr.nearest(res, scan, 0.4)[0]
                assert np.unique(gi).size == winners and (gi != nr.NONE).all()
                for plane in (0, 1):
                    want = rr.register(res, scan, 0.4, plane, None, nrm if plane else None)
                    _same(p.register_points(scan, 0.4, bool(plane), None, nrm if plane else None), want, (options, winners, plane))
        finally:
            p.close()


def test_the_degenerate_cases_return_the_identity(pkg, orc, special_refs):
    for name, plane in (("lattice_plane", 1), ("nothing_near", 0), ("nothing_near", 1), ("pairs2", 0), ("pairs5", 1), ("pairs3", 1)):
        c, refs = special_refs[name]
        want = refs[(plane, False)]
        assert want[2][3] == 1 and np.array_equal(want[1].reshape(3, 4), IDENT)
        xyzw, rgba = _cloud(orc, c["res"])
        p = _new(pkg, {}, xyzw, rgba)
        try:
            mom, step, st = p.register_points(c["scan"], c["radius"], bool(plane), None, c["normals"] if plane else None)
            assert st[3] == 1 and np.array_equal(step, IDENT) and mom[0] == want[0][0], name
        finally:
            p.close()
    assert special_refs["pairs3"][1][(0, False)][2][3] == 0 and special_refs["pairs6"][1][(1, False)][2][3] == 0


def _raw(p, xyz, stride, count, r, flags, pose, nrm, mom, step, st):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return p._lib.rtr_register_points(p._ctx, ptr(xyz), stride, count, r, flags, ptr(pose), ptr(nrm), ptr(mom), ptr(step), ptr(st))


def test_errors_leave_everything_intact(pkg, orc, special_refs):
    L = pkg._lib
    c, _ = special_refs["corner"]
    n, m = c["res"].shape[0], c["scan"].shape[0]
    xyzw, rgba = _cloud(orc, c["res"])
    fresh = pkg.Projector(0)
    try:
        with pytest.raises(pkg.RtrError) as e:
            fresh.register_points(c["scan"], 0.1)
        assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        vox, _ = vr.select(xyzw, 0.25)
        p.select_voxel_grid(0.25, stats=False)
        den = float(np.array([1], np.uint32).view(f32)[0])
        pose = np.ascontiguousarray(rc.GENERAL_POSE).reshape(12)
        ok = dict(xyz=c["scan"], stride=12, count=m, r=0.1, flags=0, pose=pose, nrm=None)
        bad = [(dict(r=v), "radius") for v in (0.0, -0.25, np.nan, np.inf)]
        bad += [(dict(r=v), "square of radius") for v in (den, 1e-30, 3e38)]
        bad += [(dict(xyz=None), "xyz is NULL")]
        bad += [(dict(stride=v), "xyz_stride_bytes") for v in (0, 8, 13, 18)]
        bad += [(dict(flags=v), "flags") for v in (2, 3, 4, -1, 1 << 30)]
        bad += [(dict(flags=1), "normals is NULL"), (dict(nrm=c["normals"]), "normals given without")]
        for k, v in ((0, np.nan), (5, np.inf), (11, -np.inf)):
            t = pose.copy()
            t[k] = v
            bad += [(dict(pose=t), "pose has a non-finite")]
        for change, word in bad:
            a = dict(ok, **change)
            mom, step, st = np.full(32, 7.0), np.full(12, 7.0), np.full(4, 77, np.uint64)
            assert _raw(p, a["xyz"], a["stride"], a["count"], a["r"], a["flags"], a["pose"], a["nrm"], mom, step, st) == L.RTR_ERR_INVALID, change
            text = p._lib.rtr_last_error(p._ctx).decode()
            assert "rtr_register_points" in text and word in text, (change, text)
            assert np.array_equal(_sel(pkg, p, n), vox) and p.get_option("selection") == 1, change
            assert (mom == 7).all() and (step == 7).all() and (st == 77).all(), change
        assert _raw(p, None, 12, 0, 0.1, 0, None, None, None, None, None) == L.RTR_OK  # (no points, every output NULL: legal)
        # a finite posed point beyond the span: found by the key sweep, before anything is written
        far = c["scan"].copy()
        far[17, 1] = f32(2.0 ** 20 * 0.1 * 1.0011)
        mom, step, st = np.full(32, 7.0), np.full(12, 7.0), np.full(4, 77, np.uint64)
        assert _raw(p, far, 12, m, 0.1, 0, None, None, mom, step, st) == L.RTR_ERR_UNSUPPORTED
        assert "span" in p._lib.rtr_last_error(p._ctx).decode()
        shift = IDENT.copy().reshape(12)
        shift[3] = 2.0 ** 20 * 0.1 * 1.01  # (the pose carries every point out)
        assert _raw(p, c["scan"], 12, m, 0.1, 0, shift, None, mom, step, st) == L.RTR_ERR_UNSUPPORTED
        assert (mom == 7).all() and (step == 7).all() and (st == 77).all()
        assert np.array_equal(_sel(pkg, p, n), vox)
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        with pytest.raises(pkg.RtrError) as e:
            p.register_points(c["scan"], 0.1)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert np.array_equal(_sel(pkg, p, n), vox)
    finally:
        p.close()


def test_the_call_moves_nothing_else(pkg, orc):
    L = pkg._lib
    n, W, H = 60_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 88, 0, n, n)
    res = np.ascontiguousarray(xyzw[:, :3])
    scan = rc.unmoved(res[::40], rc.MOTION)
    nrm = rc._unit(np.random.default_rng(1).normal(size=res.shape))
    P, P2 = pkg.orbit_projection(40, W, H), pkg.orbit_projection(41, W, H)
    keep = np.arange(n) % 3 != 0
    planes = f32([[0, 0, 1, 100], [1, 0, 0, 50]])
    refs = {plane: rr.register(res, scan, 0.1, plane, None, nrm if plane else None, finder=nr.nearest_bucket) for plane in (0, 1)}
    for with_selection in (True, False):
        p = _new(pkg, {}, xyzw, rgba, W, H)
        try:
            def state():
                return [p.download(b).copy() for b in (L.BUF_DEPTH, L.BUF_IMAGE, L.BUF_TENSOR, L.BUF_VISIBLE, L.BUF_POINT_ID, L.BUF_POINT_KEEP)] + \
                       [p.download(L.BUF_SELECTION).copy() if with_selection else None] + \
                       [p.clip_planes(), p.frame_stats(), p.get_option("p2p_open"), p.get_option("packed"), p.get_option("reordered"),
                        p.get_option("point_keep"), p.num_points, p.get_option("resident_millibytes_per_point"), p.get_option("selection")]

            def same(a, b):
                return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

            p.set_clip_planes(planes)
            p.set_point_keep(keep)
            p.p2p_open(0, 1, [p.p2p_export()])
            p.p2p_render(P, True)
            p.point_pass(P)
            if with_selection:
                p.select_points(planes=f32([[1, 0, 0, 0.05]]), stats=False)
            before = state()
            for plane in (0, 1):
                _same(p.register_points(scan, 0.1, bool(plane), None, nrm if plane else None), refs[plane], plane)
                assert same(before, state()) and p.get_option("p2p_open") == 1 and p.get_option("selection") == int(with_selection)
            p.p2p_close()
            p.set_clip_planes(None)
            p.set_point_keep(None)
            img, depth = p.host_output_buffers(0)
            p.project_async(P2, 0, filtered=False)
            p.register_points(scan, 0.1)
            p.wait_outputs(0)
            o = orc.project(xyzw, rgba, P2, W, H)
            assert np.array_equal(depth.view(np.uint32), o["depth_bits"]) and np.array_equal(img, o["img"])
        finally:
            p.close()


def test_register_points_loops_as_the_reference_does(pkg, orc):
    """ProjectCloud.registerPoints against register_ref.loop, bit for bit: the pose, the rms list and so the iteration
    count; in plane mode the facade estimates the normals itself (section 6o: the same bits as normals_ref)."""
    import torch
    c = rc.scene_case(orc, "room_shell", rc.LOOP_N, rc.LOOP_STRIDE)
    n = rc.LOOP_N
    xyzw, rgba = orc.generate("room_shell", rc.nbc.SEED, 0, n, n)
    nrm = nf.estimate(xyzw, c["radius"], 16)["normals"]
    cloud = pkg.ProjectCloud.__new__(pkg.ProjectCloud)
    p = _new(pkg, {"point_ids": 1}, xyzw, rgba)
    cloud._p = p
    try:
        dev = torch.from_numpy(c["scan"]).cuda()
        for plane in (False, True):
            with np.errstate(all="ignore"):
                want = rr.loop(c["res"], c["scan"], c["radius"], 20, plane, nrm if plane else None)
            assert 3 <= len(want[1]) < 20 and want[1][-1] < want[1][0] * 1e-2
            for scan in (c["scan"], dev):
                pose, rms, st = cloud.registerPoints(scan, c["radius"], point_to_plane=plane)
                assert np.array_equal(rr.bits64(pose), rr.bits64(want[0])), (plane, pose, want[0])
                assert np.array_equal(rr.bits64(rms), rr.bits64(want[1])) and st == want[2], (plane, rms, want[1])
            assert np.array_equal(dev.cpu().numpy().view(np.uint32), c["scan"].view(np.uint32))
        # a start pose and a fixed number of iterations
        with np.errstate(all="ignore"):
            want = rr.loop(c["res"], c["scan"], c["radius"], 2, False, None, rc.GENERAL_POSE)
        pose, rms, st = cloud.registerPoints(dev, c["radius"], iterations=2, pose=rc.GENERAL_POSE)
        assert len(rms) == 2 and np.array_equal(rr.bits64(pose), rr.bits64(want[0])) and np.array_equal(rr.bits64(rms), rr.bits64(want[1]))
    finally:
        p.close()
