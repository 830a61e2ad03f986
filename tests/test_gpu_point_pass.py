"""rtr_point_pass on the GPU (include/rtr.h section 6b): per-pixel point IDs and per-point visibility, bit for bit
against the reference answer (tests/point_pass_ref.py: the oracle's frame + the definitions), in every form the
frame and the resident cloud can take."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import point_pass_ref as ppr

pytestmark = pytest.mark.gpu

CONFIGS = {"pack0": {"pack": 0}, "pack2": {"pack": 2}, "default": {}, "mode0": {"mode": 0}}
REMOVED = int(np.float32(-1.0).view(np.uint32))


def _expected(orc, xyzw, rgba, P, W, H, filtered):
    ref = orc.project(xyzw, rgba, P, W, H)
    depth = ref["depth_bits"]
    if filtered:
        depth = orc.filter(depth, ref["img"])["depth"].view(np.uint32)
    ids, vis = ppr.point_pass(orc, xyzw, P, W, H, depth)
    return depth, ids, vis


def _check(pkg, orc, p, xyzw, rgba, P, W, H, filtered, what=""):
    L = pkg._lib
    p.set_resolution(W, H)
    p.render(P, filtered)
    p.point_pass(P)
    ids, vis, depth = p.download(L.BUF_POINT_ID), p.download(L.BUF_VISIBLE), p.download(L.BUF_DEPTH)
    e_depth, e_ids, e_vis = _expected(orc, xyzw, rgba, P, W, H, filtered)
    assert np.array_equal(depth, e_depth), ("frame", what)
    assert vis.shape == ((len(xyzw) + 31) // 32,) and ids.shape == (H, W)
    assert np.array_equal(ids, e_ids), ("ids", what, int((ids != e_ids).sum()))
    assert np.array_equal(vis, e_vis), ("visible", what)
    if filtered:
        removed = e_depth == REMOVED
        assert (ids[removed] == L.NO_POINT).all()
    return ids, vis


def _clouds(pkg, orc):
    W, H = 320, 240
    for n in (0, 1, 3, 4, 5, 31, 32, 33, 255, 256, 257, 1000, 4099):
        xyzw, rgba = orc.generate("room_shell", 100 + n, 0, n, n)
        yield "ragged%d" % n, xyzw, rgba, pkg.orbit_projection(n * 13, W, H), W, H
    xyzw, rgba, _ = ppr.hot_cloud(orc, 21)
    yield "hot", xyzw, rgba, pkg.orbit_projection(21, W, H), W, H
    xyzw, rgba = ppr.edge_cloud(22)
    yield "edge", xyzw, rgba, ppr.EDGE_P, W, H
    for scene in ("room_shell", "uniform_box"):
        n = 300_000
        xyzw, rgba = orc.generate(scene, 23, 0, n, n)
        for W2, H2 in ((320, 240), (1920, 1080)):
            yield "%s_%dx%d" % (scene, W2, H2), xyzw, rgba, pkg.orbit_projection(77, W2, H2), W2, H2


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_point_pass_exact(pkg, orc, config):
    p = pkg.Projector(0)
    try:
        for k, v in CONFIGS[config].items():
            p.set_option(k, v)
        for name, xyzw, rgba, P, W, H in _clouds(pkg, orc):
            p.upload_points(xyzw, rgba, point_ids=True)  # (the uniform box is hash-ordered: the default policy sorts it)
            for filtered in (False, True):
                _check(pkg, orc, p, xyzw, rgba, P, W, H, filtered, (config, name, filtered))
    finally:
        p.close()


def test_hot_pixel_tie_goes_to_the_smallest_upload_index(pkg, orc):
    """5000 copies of one point in front of everything else on their pixel (alone in the cloud)."""
    rng = np.random.default_rng(5)
    xyzw = np.zeros((6000, 4), np.float32)
    xyzw[:, 3] = 1
    xyzw[:, :3] = rng.uniform(-0.5, 0.5, (6000, 3)).astype(np.float32) + np.float32([0, 0, 3])
    hot = rng.permutation(6000)[:5000]
    xyzw[hot, :3] = np.float32([0.01, 0.02, 1.5])
    rgba = rng.integers(0, 256, (6000, 4), dtype=np.uint8)
    for config in sorted(CONFIGS):
        p = pkg.Projector(0)
        try:
            for k, v in CONFIGS[config].items():
                p.set_option(k, v)
            p.upload_points(xyzw, rgba)
            ids, vis = _check(pkg, orc, p, xyzw, rgba, ppr.EDGE_P, 320, 240, False, config)
            pix = orc.project_point(ppr.EDGE_P, 0.01, 0.02, 1.5, 320, 240)[0]
            assert pix >= 0 and ids.reshape(-1)[pix] == hot.min()
            assert ppr.unpack(vis, 6000)[hot].all()
        finally:
            p.close()


def test_reordered_cloud_keeps_upload_order(pkg, orc):
    n, W, H = 200_000, 640, 480
    xyzw, rgba = orc.generate("room_shell", 31, 0, n, n)
    perm = np.random.default_rng(31).permutation(n)  # hash order: the sort is worth it
    xyzw, rgba = np.ascontiguousarray(xyzw[perm]), np.ascontiguousarray(rgba[perm])
    L = pkg._lib
    ctx = {}
    for name, reorder, pids in (("sorted_ids", 1, 1), ("sorted", 1, 0), ("plain_ids", 0, 1), ("plain", 0, 0)):
        p = pkg.Projector(0)
        p.set_option("auto_reorder", reorder)
        p.upload_points(xyzw, rgba, point_ids=bool(pids))
        p.set_resolution(W, H)
        assert p.get_option("reordered") == reorder and p.get_option("point_ids") == pids
        ctx[name] = (p, p.get_option("resident_millibytes_per_point"))
    try:
        # +4 B per point only where a sorted cloud keeps its permutation; nothing otherwise
        assert ctx["sorted_ids"][1] == ctx["sorted"][1] + 4000
        assert ctx["plain_ids"][1] == ctx["plain"][1]
        with pytest.raises(pkg.RtrError) as e:
            ctx["sorted"][0].point_pass(pkg.orbit_projection(3, W, H))
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        for k in (3, 400):
            P = pkg.orbit_projection(k, W, H)
            for filtered in (False, True):
                got = [_check(pkg, orc, ctx[c][0], xyzw, rgba, P, W, H, filtered, (c, k)) for c in ("sorted_ids", "plain")]
                assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
        p = ctx["sorted_ids"][0]  # sorted again: the permutation is composed, not restarted
        p.reorder_points()
        _check(pkg, orc, p, xyzw, rgba, pkg.orbit_projection(5, W, H), W, H, False, "sorted twice")
    finally:
        for p, _ in ctx.values():
            p.close()


def _overview():
    K = np.array([[100.0, 0, 320], [0, 100.0, 240], [0, 0, 1]])  # the whole room in ~60 x 30 pixels
    E = np.eye(4)
    E[2, 3] = 20.0
    return K, E


def test_adaptive_pool_overflow_repeats_the_point_pass(pkg, orc):
    """First frame after the upload sees the whole cloud: the adaptive extent pool (n / 2 entries) overflows, the
    download's synchronisation renders the frame again -- and the point pass queued behind it."""
    n, W, H = 2_000_000, 640, 480
    xyzw, rgba = orc.generate("room_shell", 41, 0, n, n)
    K, E = _overview()
    P = orc.compose_projection(K, E)
    assert orc.envelope_points(xyzw, P, W, H, 0, 0)["accepted"] == n
    _, e_ids, e_vis = _expected(orc, xyzw, rgba, P, W, H, False)
    L = pkg._lib
    p = pkg.Projector(0)
    try:
        p.upload_points(xyzw, rgba)
        assert p.get_option("reordered") == 0 and p.get_option("pool_worst_case") == 0
        p.set_resolution(W, H)
        p.render(P, False)
        p.point_pass(P)
        ids = p.download(L.BUF_POINT_ID)
        assert p.get_option("resident_millibytes_per_point") >= 16_000  # (the pool was grown to the worst case)
        assert np.array_equal(ids, e_ids)
        assert np.array_equal(p.download(L.BUF_VISIBLE), e_vis)
    finally:
        p.close()
    cal = pkg.CameraCalibration.pinhole(K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H)
    pc = pkg.ProjectCloud(xyzw, rgba)
    try:
        got = pc.computePointIds(cal, E)
        assert pc.projector.get_option("resident_millibytes_per_point") >= 16_000
        want = e_ids.astype(np.int64)
        want[e_ids == L.NO_POINT] = -1
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert np.array_equal(pc.visible_points(cal, E), ppr.unpack(e_vis, n))
    finally:
        pc.projector.close()


def test_room_1e7_at_1080p(pkg, orc):
    n, W, H = 10_000_000, 1920, 1080
    xyzw, rgba = orc.generate("room_shell", 0xC0FFEE03, 0, n, n)
    p = pkg.Projector(0)
    try:
        p.upload_points(xyzw, rgba)
        for k in (0, 333, 666):
            _check(pkg, orc, p, xyzw, rgba, pkg.orbit_projection(k, W, H), W, H, False, k)
    finally:
        p.close()


def test_cpp_facade_point_ids_match_python(tmp_path, pkg, orc):
    n, W, H = 30_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 51, 0, n, n)
    cal, E = pkg.benchmark_calibration(W, H), pkg.orbit_pose(222)
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "cam.bin", "wb") as f:
        f.write(np.ascontiguousarray(cal.getIntrinsicsMatrix(), np.float64).tobytes())
        f.write(np.ascontiguousarray(E, np.float64).tobytes())
    exe = str(tmp_path / "point_ids_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "point_ids_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH)])
    out = str(tmp_path / "out")
    subprocess.run([exe, str(tmp_path / "cloud.bin"), str(W), str(H), str(tmp_path / "cam.bin"), out], check=True, timeout=300)
    pc = pkg.ProjectCloud(xyzw, rgba, point_ids=True)
    try:
        ids = pc.computePointIds(cal, E)
        vis = pc.visible_points(cal, E)
    finally:
        pc.projector.close()
    assert (ids >= 0).any()
    assert np.array_equal(np.fromfile(out + ".ids", np.int64).reshape(H, W), ids)
    assert np.array_equal(np.fromfile(out + ".vis", np.uint8).astype(bool), vis)
