"""-m gpu: every entry point that takes a projection matrix, under the matrices of tests/camera_cases.py -- off-axis,
rolled, anisotropic, skewed, mirrored, left-handed, rescaled by 2^+-40 and 2^-104, general rows, clouds kilometres from
the origin.  Between the cloud and the exact arithmetic stand five conservative rejections (box test, per-view box
test, lane test, quad test, rectangle test); if one of them let a point go that the exact test keeps, a pixel would be
missing.  So everything here is np.array_equal against the oracle, in every configuration that switches a rejection on
or off."""
import numpy as np
import pytest

import camera_cases as cc
import select_ref as sr
from test_gpu_point_pass import _check as _check_point_pass
from test_gpu_views import _check_batch

pytestmark = pytest.mark.gpu

W, H = cc.W0, cc.H0
CASES = [(name, pose, cname) for name in cc.NAMES for pose in range(len(cc.POSES)) for cname in cc.CLOUDS]
# (options, sort the cloud with rtr_reorder_points, frames in a row)
CONFIGS = {"default": ({}, False, 1),
           "pack2": ({"pack": 2, "auto_reorder": 0}, False, 1),
           "pack0": ({"pack": 0}, False, 1),
           "pack0_cull_sorted": ({"pack": 0, "cull": 1}, True, 1),
           "packed_cull": ({"pack": 2, "cull": 1}, False, 1),
           "chunk_test0": ({"chunk_test": 0}, False, 1),
           "lane_test0": ({"lane_test": 0}, False, 1),
           "mode0": ({"mode": 0}, False, 1),
           "overlap3": ({"overlap": 1}, False, 3)}
OPTIONS = ("pack", "auto_reorder", "cull", "chunk_test", "lane_test", "mode", "overlap", "point_ids")
_refs = {}


@pytest.fixture
def cam(projector):
    """The shared context; every option this file touches is put back as it was, planes and mask cleared."""
    saved = {k: projector.get_option(k) for k in OPTIONS}
    yield projector
    projector.set_clip_planes(None)
    projector.set_point_keep(None)
    for k in OPTIONS:
        projector.set_option(k, saved[k])


def _frame(orc, xyzw, rgba, P, Wf, Hf):
    """The oracle's answers for one cloud and matrix: the frame, the filtered frame, the kept points and the chunks of
    the upload order that hold one."""
    r = orc.project(xyzw, rgba, P, Wf, Hf)
    f = orc.filter(r["depth_bits"], r["img"])
    kept = sr.pixels(orc, xyzw, P, Wf, Hf) >= 0
    return {"depth_bits": r["depth_bits"], "img": r["img"], "f": f, "kept": int(kept.sum()),
            "chunks": int(np.unique(np.nonzero(kept)[0] // 256).size)}


def _ref(pkg, orc, name, pose, cname, Wf=W, Hf=H):
    """Computed once per (matrix, pose, cloud, shape) and shared by the configurations; never written to."""
    key = (name, pose, cname, Wf, Hf)
    if key not in _refs:
        cl = cc.clouds(pkg, orc, name, pose, Wf, Hf)[cname]
        _refs[key] = _frame(orc, cl["xyzw"], cl["rgba"], cc.matrices(pkg, Wf, Hf)[name][pose], Wf, Hf)
    return _refs[key]


def _same_frame(pkg, p, P, e, what, frames=1, stats=True, unfiltered=True):
    L = pkg._lib
    Hf, Wf = e["img"].shape[:2]
    if unfiltered:
        img, depth = p.project(P)
        assert np.array_equal(depth.view(np.uint32), e["depth_bits"]), ("depth", what, int((depth.view(np.uint32) != e["depth_bits"]).sum()))
        assert np.array_equal(img, e["img"]), ("image", what)
    for _ in range(frames):
        p.render(P, True)
    f = e["f"]
    assert np.array_equal(p.download(L.BUF_DEPTH), f["depth"].view(np.uint32)), ("filtered depth", what)
    assert np.array_equal(p.download(L.BUF_IMAGE), f["img"]), ("filtered image", what)
    assert np.array_equal(p.download(L.BUF_MASK), f["mask"]), ("mask", what)
    assert np.array_equal(p.download(L.BUF_MINMAX), f["minmax"]), ("min / max", what)
    assert np.array_equal(p.download(L.BUF_TENSOR).reshape(5, Hf, Wf), f["tensor"]), ("tensor", what)
    if stats:
        st = p.frame_stats()
        assert st["entries"] == e["kept"] and st["errors"] == 0, ("in-frustum entries", what, st, e["kept"])
        if p.get_option("reordered") == 0:
            assert st["colour_chunks"] == e["chunks"], ("chunks with an in-frustum point", what, st, e["chunks"])


@pytest.mark.parametrize("config", list(CONFIGS))
def test_frames_equal_the_oracle(pkg, orc, cam, config):
    options, sort, frames = CONFIGS[config]
    for k, v in options.items():
        cam.set_option(k, v)
    cam.set_resolution(W, H)
    failed = []
    for name, pose, cname in CASES:
        cl = cc.clouds(pkg, orc, name, pose)[cname]
        cam.upload_points(cl["xyzw"], cl["rgba"])
        if sort or (config == "default" and cname == "scene" and pose == 1):
            cam.reorder_points()
            assert cam.get_option("reordered") == 1
        if "pack" in options and "cull" not in options:
            assert cam.get_option("packed") == (1 if options["pack"] else 0)
        try:
            _same_frame(pkg, cam, cc.matrices(pkg)[name][pose], _ref(pkg, orc, name, pose, cname), (config, name, pose, cname),
                        frames=frames, stats=config != "mode0")
        except AssertionError as e:  # (go on: the message names every case that differs, not the first)
            failed.append(e.args[0] if e.args else (name, pose, cname))
    assert not failed, (len(failed), failed[:12])


BATCHES = (("centre", "offaxis_near", "roll_pitch", "aniso", "skew", "wide", "mirror_x", "rows_general"),
           ("offaxis_far", "tele", "mirror_xy", "lefthanded", "scale_up", "scale_down", "scale_tiny", "grid_km"),
           ("grid_far", "scale_guard", "grid_km", "centre", "offaxis_near", "tele", "roll_pitch", "mirror_xy"))


@pytest.mark.parametrize("batch", [0, 1, 2])
@pytest.mark.parametrize("config", ["default", "pack0", "sorted"])
def test_views_mix_the_matrices(pkg, orc, cam, batch, config):
    """Eight different matrices in one batch: each view has its own constants in the view table.  The cloud is what the
    eight aim at, one after the other, and the room."""
    names = BATCHES[batch]
    parts = [cc.clouds(pkg, orc, n, 0)["straddle" if i % 2 == 0 else "lanes"] for i, n in enumerate(names)]
    parts.append(cc.clouds(pkg, orc, names[0], 0)["scene"])  # (the room where the batch's first matrix looks)
    xyzw = np.concatenate([c["xyzw"] for c in parts])
    rgba = np.concatenate([c["rgba"] for c in parts])
    Ps = np.stack([cc.matrices(pkg)[n][0].reshape(4, 4) for n in names])
    if config == "pack0":
        cam.set_option("pack", 0)
    cam.set_resolution(W, H)
    cam.upload_points(xyzw, rgba)
    if config == "sorted":
        cam.reorder_points()
    cache = {}
    for filtered in (False, True):
        _check_batch(pkg, orc, cam, xyzw, rgba, Ps, W, H, filtered, cache, (batch, config, filtered))


@pytest.mark.parametrize("sort", [False, True])
def test_point_pass(pkg, orc, cam, sort):
    for i, name in enumerate(cc.NAMES):
        cl = cc.clouds(pkg, orc, name, 0)["straddle"]
        cam.upload_points(cl["xyzw"], cl["rgba"], point_ids=sort)
        if sort:
            cam.reorder_points()
            assert cam.get_option("reordered") == 1
        _check_point_pass(pkg, orc, cam, cl["xyzw"], cl["rgba"], cc.matrices(pkg)[name][0], W, H, i % 2 == 1, (name, sort))


def _planes_through(xyz, rng):
    """Two half-spaces through the middle of the cloud."""
    mid = np.median(xyz.astype(np.float64), axis=0)
    out = []
    for _ in range(2):
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        out.append([*nrm, -float(nrm @ mid)])
    return np.float32(out)


@pytest.mark.parametrize("form", ["packed", "pack0", "sorted"])
def test_selection(pkg, orc, cam, form):
    rng = np.random.default_rng(71)
    cam.set_option("pack", 0 if form == "pack0" else 2)
    cam.set_option("auto_reorder", 0)
    cam.set_resolution(W, H)
    for name in cc.NAMES:
        cl = cc.clouds(pkg, orc, name, 1)["straddle"]
        xyzw, P = cl["xyzw"], cc.matrices(pkg)[name][1]
        n, chunks = len(xyzw), (len(xyzw) + 255) // 256
        cam.upload_points(xyzw, cl["rgba"], point_ids=form == "sorted")
        if form == "sorted":
            cam.reorder_points()
        planes = _planes_through(xyzw[:, :3], rng)
        for rect in ((0, 0, W, H), (0, 0, 1, H), (W - 1, 0, W, H), (W // 4, H // 3, W // 4 + 37, H // 3 + 1), (3, 5, W - 7, H - 2)):
            for pl in (None, planes):
                st = cam.select_points(planes=pl, P=P, rect=rect)
                want = sr.inside(pkg, orc, xyzw, pl, P, rect, W, H)
                assert np.array_equal(cam.download(pkg._lib.BUF_SELECTION), sr.words(want)), (form, name, rect, pl is not None)
                assert st[0] == want.sum() and st[1] + st[2] + st[3] == chunks, (form, name, rect, st, n)


@pytest.mark.parametrize("form", ["default", "pack0"])
def test_clip_planes_and_keep_mask(pkg, orc, cam, form):
    rng = np.random.default_rng(72)
    if form == "pack0":
        cam.set_option("pack", 0)
    cam.set_resolution(W, H)
    for name in cc.NAMES:
        cl = cc.clouds(pkg, orc, name, 0)["straddle"]
        xyzw, rgba, P = cl["xyzw"], cl["rgba"], cc.matrices(pkg)[name][0]
        cam.upload_points(xyzw, rgba, point_ids=True)
        planes = _planes_through(xyzw[:, :3], rng)
        keep = rng.random(len(xyzw)) < 0.7
        keep[256 * 3:256 * 9] = False  # (whole chunks hidden, and whole chunks kept)
        keep[256 * 20:256 * 30] = True
        cam.set_clip_planes(planes)
        cam.set_point_keep(keep)
        left = keep & pkg.clip_keep(planes, xyzw)
        assert 0 < left.sum() < len(xyzw)
        e = _frame(orc, np.ascontiguousarray(xyzw[left]), np.ascontiguousarray(rgba[left]), P, W, H)
        _same_frame(pkg, cam, P, e, (form, name), stats=False)
        assert cam.frame_stats()["entries"] == e["kept"], (form, name)
        cam.set_clip_planes(None)
        cam.set_point_keep(None)


def _shifted(xyzw, d):
    """What rtr_transform_points computes for [I | d]: ((1 x + 0 y) + 0 z) + d per coordinate, in fp32."""
    out = xyzw.copy()
    out[:, :3] = (xyzw[:, :3] + np.float32(0)) + np.float32(d)
    return out


@pytest.mark.parametrize("form", ["default", "pack0"])
def test_absmax_follows_the_edits(pkg, orc, cam, form):
    """grid_km: a cloud at the origin is moved out to the grid, grows there and comes back.  The lane test's zsafe and
    zfront come from the cloud's largest coordinates, which every edit has to carry along -- upwards above all."""
    if form == "pack0":
        cam.set_option("pack", 0)
    cam.set_option("auto_reorder", 0)
    cam.set_resolution(W, H)
    shift = np.asarray(cc.SHIFTS["grid_km"], np.float64)
    M = np.eye(4)
    for pose in (0, 1):
        P0, Pk = cc.matrices(pkg)["centre"][pose], cc.matrices(pkg)["grid_km"][pose]
        near, far = cc.clouds(pkg, orc, "centre", pose), cc.clouds(pkg, orc, "grid_km", pose)
        xyzw = np.concatenate([near["scene"]["xyzw"], near["lanes"]["xyzw"]])
        rgba = np.concatenate([near["scene"]["rgba"], near["lanes"]["rgba"]])
        cam.upload_points(xyzw, rgba)
        _same_frame(pkg, cam, P0, _frame(orc, xyzw, rgba, P0, W, H), (form, pose, "at the origin"))
        M[:3, 3] = shift
        cam.transform_points(M)
        xyzw = _shifted(xyzw, shift)
        _same_frame(pkg, cam, Pk, _frame(orc, xyzw, rgba, Pk, W, H), (form, pose, "moved out"))
        for cname in ("lanes", "straddle"):
            cam.append_points(far[cname]["xyzw"], far[cname]["rgba"])
            xyzw, rgba = np.concatenate([xyzw, far[cname]["xyzw"]]), np.concatenate([rgba, far[cname]["rgba"]])
            _same_frame(pkg, cam, Pk, _frame(orc, xyzw, rgba, Pk, W, H), (form, pose, "appended", cname))
        M[:3, 3] = -shift
        cam.transform_points(M)
        xyzw = _shifted(xyzw, -shift)
        _same_frame(pkg, cam, P0, _frame(orc, xyzw, rgba, P0, W, H), (form, pose, "moved back"))


@pytest.mark.parametrize("name", ["offaxis_far", "tele", "wide"])
def test_large_frame(pkg, orc, cam, name):
    """4112 x 1047: 64-wide tiles and a large hiW in the margins, ragged in both directions."""
    Wl, Hl = 4112, 1047
    cam.set_resolution(Wl, Hl)
    P = cc.matrices(pkg, Wl, Hl)[name][0]
    for cname in cc.CLOUDS:
        cl = cc.clouds(pkg, orc, name, 0, Wl, Hl)[cname]
        cam.upload_points(cl["xyzw"], cl["rgba"])
        e = _frame(orc, cl["xyzw"], cl["rgba"], P, Wl, Hl)
        assert e["kept"] >= 100, (name, cname, e["kept"])
        _same_frame(pkg, cam, P, e, (name, cname, "4112x1047"))
