"""rtr_render_views on the GPU (include/rtr.h section 6c): every view of every batch bit for bit against the oracle's
frame AND against rtr_render of the same pose on the same context -- depth bits, image, and (filtered) the fp16 tensor
and min / max -- in every form the cloud and the frame can take; the single frame left alone; one point-kernel launch
per binned batch; pool overflows repaired; argument errors."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import pool_overflow_scenes as sc

pytestmark = pytest.mark.gpu

CONFIGS = {"pack0": {"pack": 0}, "pack2": {"pack": 2}, "default": {}, "mode0": {"mode": 0}, "sorted": {},
           "chunk_test0": {"chunk_test": 0}, "lane_test0": {"lane_test": 0}, "overlap": {"overlap": 1}}
NOTHING = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, -1], [0, 0, 0, 1]], np.float32)  # r.z = -1 for every point


def _ref(orc, xyzw, rgba, P, W, H, filtered, cache):
    key = (np.asarray(P, np.float32).tobytes(), W, H, filtered)
    if key not in cache:
        r = orc.project(xyzw, rgba, P, W, H)
        if filtered:
            f = orc.filter(r["depth_bits"], r["img"])
            r = {"depth_bits": f["depth"].view(np.uint32), "img": f["img"], "tensor": f["tensor"], "minmax": f["minmax"]}
        cache[key] = r
    return cache[key]


def _stereo(pkg, k, W, H):
    cal = pkg.benchmark_calibration(W, H)
    E = pkg.orbit_pose(k)
    E2 = E.copy()
    E2[0, 3] -= 0.064
    return [pkg.compose_projection(cal.getIntrinsicsMatrix(), e) for e in (E, E2)]


def _poses(pkg, orc, W, H, K, seed):
    rng = np.random.default_rng(seed)
    Ps = _stereo(pkg, int(rng.integers(1000)), W, H)
    Ps += [pkg.orbit_projection(int(k), W, H) for k in rng.integers(0, 1000, 4)]
    Ps += [NOTHING, sc.p_one(orc, cx=W / 3)[0]]
    Ps.append(Ps[2])  # two identical poses
    out = np.stack([np.asarray(P, np.float32).reshape(4, 4) for P in Ps])
    return out[rng.permutation(len(out))][:K] if K < len(out) else out


def _check_batch(pkg, orc, p, xyzw, rgba, Ps, W, H, filtered, cache, what=""):
    L = pkg._lib
    p.render_views(Ps, filtered)
    K = len(Ps)
    assert p.get_option("views") == K
    got = {"depth_bits": p.download(L.BUF_VIEW_DEPTH), "img": p.download(L.BUF_VIEW_IMAGE)}
    assert got["depth_bits"].shape == (K, H, W) and got["img"].shape == (K, H, W, 3)
    if filtered:
        got["tensor"], got["minmax"] = p.download(L.BUF_VIEW_TENSOR), p.download(L.BUF_VIEW_MINMAX)
        assert got["tensor"].shape == (K, 5, H, W) and got["minmax"].shape == (K, 2)
    for v in range(K):
        e = _ref(orc, xyzw, rgba, Ps[v], W, H, filtered, cache)
        assert np.array_equal(got["depth_bits"][v], e["depth_bits"]), ("depth", what, v)
        assert np.array_equal(got["img"][v], e["img"]), ("image", what, v)
        if filtered:
            assert np.array_equal(got["tensor"][v], e["tensor"].view(np.uint16)), ("tensor", what, v)
            assert np.array_equal(got["minmax"][v], np.asarray(e["minmax"]).view(np.uint32).reshape(2)), ("minmax", what, v)
    for v in range(K):  # the same pose through rtr_render on the same context
        p.render(Ps[v], filtered)
        assert np.array_equal(p.download(L.BUF_DEPTH), got["depth_bits"][v]), ("render depth", what, v)
        assert np.array_equal(p.download(L.BUF_IMAGE), got["img"][v]), ("render image", what, v)
        if filtered:
            assert np.array_equal(p.download(L.BUF_TENSOR), got["tensor"][v][None]), ("render tensor", what, v)
            assert np.array_equal(p.download(L.BUF_MINMAX), got["minmax"][v]), ("render minmax", what, v)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_views_exact(pkg, orc, config):
    p = pkg.Projector(0)
    try:
        for k, v in CONFIGS[config].items():
            p.set_option(k, v)
        clouds = [("room_shell", 200_000), ("uniform_box", 100_000)]
        for ci, (scene, n) in enumerate(clouds):
            xyzw, rgba = orc.generate(scene, 31 + ci, 0, n, n)
            p.upload_points(xyzw, rgba)
            if config == "sorted":
                p.reorder_points()
                assert p.get_option("reordered") == 1
            cache = {}
            for W, H in ((64, 48), (1000, 562), (1920, 1080)):
                p.set_resolution(W, H)
                for K in (1, 2, 3, 8):
                    for filtered in ((False, True) if W % 16 == 0 else (False,)):
                        if W == 1920 and K == 3:
                            continue
                        Ps = _poses(pkg, orc, W, H, K, seed=K * 7 + W + ci)
                        _check_batch(pkg, orc, p, xyzw, rgba, Ps, W, H, filtered, cache, (config, scene, W, K, filtered))
    finally:
        p.close()


def test_views_stereo_and_inside(pkg, orc):
    """A stereo pair, and views from inside a volume cloud (the orbit camera sits inside the uniform box)."""
    p = pkg.Projector(0)
    try:
        n, W, H = 300_000, 320, 240
        xyzw, rgba = orc.generate("uniform_box", 5, 0, n, n)
        p.upload_points(xyzw, rgba)
        p.set_resolution(W, H)
        cache = {}
        Ps = np.stack([np.asarray(P, np.float32) for P in _stereo(pkg, 40, W, H)])
        for filtered in (False, True):
            _check_batch(pkg, orc, p, xyzw, rgba, Ps, W, H, filtered, cache, ("stereo", filtered))
        inside = np.stack([np.asarray(pkg.orbit_projection(k, W, H), np.float32) for k in (0, 250, 500, 750)])
        _check_batch(pkg, orc, p, xyzw, rgba, inside, W, H, True, cache, "inside")
    finally:
        p.close()


def test_views_leave_single_frame(pkg, orc):
    L = pkg._lib
    p = pkg.Projector(0)
    try:
        n, W, H = 200_000, 320, 240
        xyzw, rgba = orc.generate("room_shell", 9, 0, n, n)
        p.upload_points(xyzw, rgba)
        p.set_resolution(W, H)
        P = pkg.orbit_projection(3, W, H)
        p.render(P, True)
        before = {b: p.download(b) for b in (L.BUF_DEPTH, L.BUF_IMAGE, L.BUF_TENSOR, L.BUF_MINMAX, L.BUF_MASK)}
        Ps = np.stack([np.asarray(pkg.orbit_projection(k, W, H), np.float32) for k in (100, 400, 700)])
        p.render_views(Ps, True)
        p.synchronize()
        for b, a in before.items():
            assert np.array_equal(p.download(b), a), b
        e = _ref(orc, xyzw, rgba, P, W, H, True, {})
        assert np.array_equal(p.download(L.BUF_DEPTH), e["depth_bits"])
    finally:
        p.close()


@pytest.mark.parametrize("packed", (True, False))
def test_views_one_point_kernel_launch(pkg, orc, packed):
    """A binned K-view batch adds exactly ONE point-kernel launch (RTR_K_MIN_DEPTH): the cloud is streamed once."""
    p = pkg.Projector(0)
    try:
        if not packed:
            p.set_option("pack", 0)
        n, W, H = 300_000, 640, 480
        xyzw, rgba = orc.generate("room_shell", 11, 0, n, n)
        p.upload_points(xyzw, rgba)
        p.set_resolution(W, H)
        for K in (2, 5, 8):
            Ps = np.stack([np.asarray(pkg.orbit_projection(10 * k, W, H), np.float32) for k in range(K)])
            p.render_views(Ps, True)  # (allocation, first use)
            p.synchronize()
            p.timing_enable(True)
            p.timing_reset()
            p.render_views(Ps, True)
            t = p.timing()
            p.timing_enable(False)
            assert t["min_depth"][1] == 1, (K, t)
            assert t["tile"][1] == K, (K, t)
    finally:
        p.close()


@pytest.mark.parametrize("config", ("default", "pack0"))
def test_views_first_frame_overflow(pkg, orc, config):
    """The cloud's first work is a batch whose first view holds the whole cloud in one tile: it overflows the adaptive
    pool, and the synchronising download renders the batch again -- exact."""
    L = pkg._lib
    xyzw, rgba = sc.cloud(orc)
    W, H = sc.W, sc.H
    p = pkg.Projector(0)
    try:
        if config == "pack0":
            p.set_option("pack", 0)
        before = sc.prepare(pkg, orc, p, xyzw, rgba, "first")
        Ps = np.stack([np.asarray(sc.p_one(orc)[0], np.float32), np.asarray(pkg.orbit_projection(0, W, H), np.float32)])
        p.render_views(Ps, False)
        depth = p.download(L.BUF_VIEW_DEPTH)
        img = p.download(L.BUF_VIEW_IMAGE)
        # (the views' pools grew to the worst case, 16 B per point each)
        assert p.get_option("resident_millibytes_per_point") - before >= 2 * sc.WORST_MB - 4_000, before
        for v in range(2):
            e = orc.project(xyzw, rgba, Ps[v], W, H)
            assert np.array_equal(depth[v], e["depth_bits"]) and np.array_equal(img[v], e["img"]), v
        p.render_views(Ps, True)  # (and again through rtr_synchronize, filtered, on worst-case pools)
        p.synchronize()
        f = orc.filter(orc.project(xyzw, rgba, Ps[0], W, H)["depth_bits"], orc.project(xyzw, rgba, Ps[0], W, H)["img"])
        assert np.array_equal(p.download(L.BUF_VIEW_DEPTH)[0], f["depth"].view(np.uint32))
    finally:
        p.close()


def test_views_errors_change_nothing(pkg, orc):
    import ctypes as C
    L = pkg._lib
    p = pkg.Projector(0)
    try:
        P4 = np.zeros((4, 16), np.float32)
        assert p._lib.rtr_render_views(p._ctx, 2, P4.ctypes.data_as(C.c_void_p), 0) == L.RTR_ERR_INVALID  # no cloud
        n, W, H = 50_000, 128, 96
        xyzw, rgba = orc.generate("room_shell", 13, 0, n, n)
        p.upload_points(xyzw, rgba)
        assert p._lib.rtr_render_views(p._ctx, 2, P4.ctypes.data_as(C.c_void_p), 0) == L.RTR_ERR_INVALID  # no resolution
        p.set_resolution(W, H)
        Ps = np.stack([np.asarray(pkg.orbit_projection(k, W, H), np.float32) for k in (1, 2)])
        p.render_views(Ps, True)
        keep = {b: p.download(b) for b in (L.BUF_VIEW_DEPTH, L.BUF_VIEW_IMAGE, L.BUF_VIEW_TENSOR, L.BUF_VIEW_MINMAX)}
        P9 = np.zeros((9, 16), np.float32)
        for count, ptr in ((0, P9), (-1, P9), (9, P9), (2, None)):
            arg = None if ptr is None else ptr.ctypes.data_as(C.c_void_p)
            assert p._lib.rtr_render_views(p._ctx, count, arg, 1) == L.RTR_ERR_INVALID, count
        assert p.get_option("views") == 2
        for b, a in keep.items():
            assert np.array_equal(p.download(b), a), b
    finally:
        p.close()


def test_compute_full_views(pkg, orc):
    """computeFullViews with a stand-in model equals K computeFull calls."""
    import torch
    n, W, H = 60_000, 160, 128
    xyzw, rgba = orc.generate("room_shell", 17, 0, n, n)
    pc = pkg.ProjectCloud(xyzw[:, :3], rgba[:, :3], device=0)
    pc.set_model(lambda x: x[:, 0:3] * 0.5 + x[:, 3:4] * 0.25)
    cal = pkg.benchmark_calibration(W, H)
    Es = [pkg.orbit_pose(k) for k in (5, 200, 600)]
    colors = [np.zeros((H, W, 3), np.uint8), None, np.zeros((H, W, 3), np.uint8)]
    depths = [np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), None]
    assert pc.computeFullViews(cal, Es, colors, depths) == 1
    for v, E in enumerate(Es):
        c1, d1 = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.float32)
        assert pc.computeFull(cal, E, c1, d1) == 1
        if colors[v] is not None:
            assert np.array_equal(colors[v], c1), v
        if depths[v] is not None:
            assert np.array_equal(depths[v].view(np.uint32), d1.view(np.uint32)), v
    torch.cuda.synchronize()
