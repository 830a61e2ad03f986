"""Clip planes on the GPU (include/rtr.h section 6d): every frame bit for bit against the oracle run on the subset of the
cloud that the numpy float32 test (camera.clip_keep) keeps -- depth bits, image, and (filtered) the fp16 tensor and
min / max -- in every form the cloud and the frame can take; the point pass, several views, the phase calls, the
peer-to-peer frame, the async slots and the repair journal with planes that change under them."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import point_pass_ref as ppr
import pool_overflow_scenes as sc

pytestmark = pytest.mark.gpu

EMPTY = 0x7F7FFFFF


def _planes(pkg, name):
    f = np.float32
    box = pkg.clip_box_planes([-2.0, -1.5, -2.0], [2.0, 1.5, 2.0])
    return {
        "none_set": np.zeros((0, 4), f),
        "half": f([[1, 0, 0, 0]]),                        # x >= 0
        "ceiling": f([[0, -1, 0, 1.0]]),                  # y <= 1
        "box": box,
        "oblique": f([[0.3, -0.2, 0.9, 0.35], [-0.7, 0.1, 0.2, 1.3]]),
        "wall": f([[-1, 0, 0, -4]]),                      # x <= -4: only the wall at x = -4, every value exactly 0
        "keep_all": f([[0, 0, 1, 100]]),
        "keep_none": f([[0, 0, 1, -100]]),
        "eight": np.concatenate([box, f([[1, 1, 0, 2], [0.3, -0.2, 0.9, 1.1]])]),
    }[name]


def _ref(pkg, orc, xyzw, rgba, planes, P, W, H, filtered):
    keep = pkg.clip_keep(planes, xyzw)
    r = orc.project(xyzw[keep], rgba[keep], P, W, H)
    out = {"depth_bits": r["depth_bits"], "img": r["img"], "keep": keep}
    if filtered:
        f = orc.filter(r["depth_bits"], r["img"])
        out.update(depth_bits=f["depth"].view(np.uint32), img=f["img"], tensor=f["tensor"], minmax=f["minmax"])
    return out


def _check_frame(pkg, orc, p, xyzw, rgba, planes, P, W, H, filtered, what):
    L = pkg._lib
    filtered = filtered and W % 16 == 0 and H >= 16
    img, depth = p.project(P, filtered=filtered)
    r = _ref(pkg, orc, xyzw, rgba, planes, P, W, H, filtered)
    assert np.array_equal(depth.view(np.uint32), r["depth_bits"]), ("depth", what)
    assert np.array_equal(img, r["img"]), ("image", what)
    if filtered:
        assert np.array_equal(p.download(L.BUF_TENSOR).reshape(5, H, W), r["tensor"]), ("tensor", what)
        assert np.array_equal(p.download(L.BUF_MINMAX), np.asarray(r["minmax"]).view(np.uint32).reshape(2)), ("minmax", what)
    return r


def _new(pkg, options, xyzw, rgba, W, H, sort=False):
    p = pkg.Projector(0)
    for k, v in options.items():
        p.set_option(k, v)
    if sort:
        p.set_option("point_ids", 1)
    p.upload_points(xyzw, rgba)
    if sort:
        p.reorder_points()
    p.set_resolution(W, H)
    return p


CONFIGS = {"default": {}, "pack0": {"pack": 0}, "pack2": {"pack": 2}, "mode0": {"mode": 0}, "cull": {"cull": 1},
           "cull_pack0": {"cull": 1, "pack": 0}, "chunk_test0": {"chunk_test": 0}, "lane_test0": {"lane_test": 0},
           "lane_test0_pack0": {"lane_test": 0, "pack": 0}, "overlap": {"overlap": 1}, "sorted": {}}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_clip_frames_match_subset_oracle(pkg, orc, config):
    sort = config == "sorted"
    for scene, n, (W, H) in (("room_shell", 200_000, (640, 480)), ("uniform_box", 150_000, (64, 48)),
                             ("room_shell", 4099, (64, 48))):
        xyzw, rgba = orc.generate(scene, 31, 0, n, n)
        p = _new(pkg, CONFIGS[config], xyzw, rgba, W, H, sort)
        try:
            for k, name in enumerate(("half", "box", "ceiling", "oblique", "wall", "eight", "keep_none")):
                planes = _planes(pkg, name)
                p.set_clip_planes(planes)
                assert np.array_equal(p.clip_planes(), planes)
                P = pkg.orbit_projection(97 * k + 5, W, H)
                r = _check_frame(pkg, orc, p, xyzw, rgba, planes, P, W, H, k % 2 == 1, (config, scene, n, name))
                if name == "wall" and scene == "room_shell" and n > 100_000:
                    assert 0 < r["keep"].sum() < n // 4  # points with a plane value of exactly 0 are there, and kept
            # a plane that keeps everything: byte for byte the frame without planes
            P = pkg.orbit_projection(11, W, H)
            p.set_clip_planes(None)
            img0, depth0 = p.project(P)
            p.set_clip_planes(_planes(pkg, "keep_all"))
            img1, depth1 = p.project(P)
            assert np.array_equal(depth0.view(np.uint32), depth1.view(np.uint32)) and np.array_equal(img0, img1)
        finally:
            p.close()


def test_clip_ragged_counts_and_resolutions(pkg, orc):
    for n in (0, 1, 2, 3, 5, 37, 255, 256, 257, 1023, 4099):
        xyzw, rgba = orc.generate("room_shell", 100 + n, 0, n, n) if n else (np.zeros((0, 4), np.float32), np.zeros((0, 4), np.uint8))
        for options in ({}, {"mode": 0}, {"pack": 2}):
            p = _new(pkg, options, xyzw, rgba, 64, 48)
            try:
                for name in ("half", "eight", "keep_none"):
                    planes = _planes(pkg, name)
                    p.set_clip_planes(planes)
                    _check_frame(pkg, orc, p, xyzw, rgba, planes, pkg.orbit_projection(n, 64, 48), 64, 48, True, (n, options, name))
            finally:
                p.close()
    n, W, H = 1_000_000, 1920, 1080
    xyzw, rgba = orc.generate("room_shell", 5, 0, n, n)
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        for name in ("box", "ceiling"):
            planes = _planes(pkg, name)
            p.set_clip_planes(planes)
            _check_frame(pkg, orc, p, xyzw, rgba, planes, pkg.orbit_projection(333, W, H), W, H, True, ("1080p", name))
    finally:
        p.close()


def test_clip_errors_change_nothing(pkg, orc):
    L = pkg._lib
    xyzw, rgba = orc.generate("room_shell", 1, 0, 1000, 1000)
    p = _new(pkg, {}, xyzw, rgba, 64, 48)
    try:
        good = _planes(pkg, "oblique")
        p.set_clip_planes(good)
        bad = [np.zeros((9, 4), np.float32) + [1, 0, 0, 0], np.float32([[0, 0, 0, 1]]), np.float32([[np.nan, 0, 1, 0]]),
               np.float32([[1, 0, 0, np.inf]])]
        for b in bad:
            with pytest.raises(L.RtrError) as e:
                p.set_clip_planes(b)
            assert e.value.code == L.RTR_ERR_INVALID
            assert np.array_equal(p.clip_planes(), good)
        lib = L.lib()
        assert lib.rtr_set_clip_planes(p._ctx, 1, None) == L.RTR_ERR_INVALID
        assert lib.rtr_set_clip_planes(p._ctx, -1, None) == L.RTR_ERR_INVALID
        assert np.array_equal(p.clip_planes(), good)
        p.set_clip_planes(np.zeros((0, 4), np.float32))
        assert p.clip_planes().shape == (0, 4)
    finally:
        p.close()


@pytest.mark.parametrize("config", ["default", "pack0", "mode0", "lane_test0"])
def test_clip_render_views(pkg, orc, config):
    L = pkg._lib
    n, W, H = 150_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 8, 0, n, n)
    p = _new(pkg, CONFIGS[config], xyzw, rgba, W, H)
    try:
        Ps = np.stack([pkg.orbit_projection(k, W, H).reshape(4, 4) for k in (3, 170, 400, 650, 900)])
        for name in ("box", "eight", "half"):
            planes = _planes(pkg, name)
            p.set_clip_planes(planes)
            p.render_views(Ps, True)
            depth = p.download(L.BUF_VIEW_DEPTH).reshape(len(Ps), H, W)
            img = p.download(L.BUF_VIEW_IMAGE).reshape(len(Ps), H, W, 3)
            tensor = p.download(L.BUF_VIEW_TENSOR).reshape(len(Ps), 5, H, W)
            for v, P in enumerate(Ps):
                r = _ref(pkg, orc, xyzw, rgba, planes, P.reshape(16), W, H, True)
                assert np.array_equal(depth[v], r["depth_bits"]), (config, name, v)
                assert np.array_equal(img[v], r["img"]), (config, name, v)
                assert np.array_equal(tensor[v], r["tensor"]), (config, name, v)
    finally:
        p.close()


@pytest.mark.parametrize("config", ["default", "pack0", "mode0", "sorted"])
def test_clip_point_pass(pkg, orc, config):
    L = pkg._lib
    n, W, H = 60_000, 160, 120
    xyzw, rgba = orc.generate("room_shell", 12, 0, n, n)
    p = _new(pkg, {k: v for k, v in CONFIGS[config].items()}, xyzw, rgba, W, H, sort=config == "sorted")
    try:
        for k, name in enumerate(("box", "half", "keep_none")):
            planes = _planes(pkg, name)
            p.set_clip_planes(planes)
            P = pkg.orbit_projection(50 + 200 * k, W, H)
            p.render(P, False)
            p.point_pass(P)
            ids, vis = p.download(L.BUF_POINT_ID), p.download(L.BUF_VISIBLE)
            keep = pkg.clip_keep(planes, xyzw)
            sub = np.flatnonzero(keep)
            r = orc.project(xyzw[keep], rgba[keep], P, W, H)
            assert np.array_equal(p.download(L.BUF_DEPTH), r["depth_bits"])
            e_ids, e_vis = ppr.point_pass(orc, xyzw[keep], P, W, H, r["depth_bits"])
            full_ids = np.where(e_ids == L.NO_POINT, L.NO_POINT, sub[np.minimum(e_ids, max(len(sub) - 1, 0))] if len(sub) else L.NO_POINT)
            assert np.array_equal(ids, full_ids.astype(np.uint32)), (config, name)
            named = ids[ids != L.NO_POINT]
            assert keep[named].all()
            bits = ppr.unpack(vis, n)
            e_bits = np.zeros(n, bool)
            e_bits[sub] = ppr.unpack(e_vis, len(sub))
            assert np.array_equal(bits, e_bits), (config, name)
            assert not bits[~keep].any()
    finally:
        p.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_clip_phase_calls_two_contexts(pkg, orc, mode):
    import torch
    n, W, H = 120_000, 640, 480
    xyzw, rgba = orc.generate("room_shell", 21, 0, n, n)
    P = pkg.orbit_projection(300, W, H)
    planes = _planes(pkg, "oblique")
    keep = pkg.clip_keep(planes, xyzw)
    ref = orc.project(xyzw[keep], rgba[keep], P, W, H)
    reff = orc.filter(ref["depth_bits"], ref["img"])
    locs = []
    for r in range(2):
        lo, hi = pkg.shard_range(n, r, 2)
        p = pkg.Projector(0)
        p.set_option("mode", mode)
        p.upload_points(xyzw[lo:hi], rgba[lo:hi])
        p.set_resolution(W, H)
        p.set_clip_planes(planes)
        loc = pkg.sharded.HipLocal(p)
        loc.bind_stream()
        locs.append(loc)
    try:
        for loc in locs:
            loc.clear()
            loc.min_depth_pass(P)
        d = torch.minimum(locs[0].depth_tensor(), locs[1].depth_tensor())
        for loc in locs:
            loc.depth_tensor().copy_(d)
            loc.accumulate_pass(P)
        a = locs[0].accum_tensor() + locs[1].accum_tensor()
        for loc in locs:
            loc.accum_tensor().copy_(a)
            loc.resolve()
            loc.filter()
        torch.cuda.synchronize()
        for loc in locs:
            assert np.array_equal(loc.p.download(pkg._lib.BUF_ACCUM), ref["acc"])
            assert np.array_equal(loc.p.download(pkg._lib.BUF_IMAGE), reff["img"])
            assert np.array_equal(loc.p.download(pkg._lib.BUF_DEPTH), reff["depth"].view(np.uint32))
            assert np.array_equal(loc.p.download(pkg._lib.BUF_TENSOR).reshape(5, H, W), reff["tensor"])
    finally:
        for loc in locs:
            loc.p.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("form", ["p2p", "owned"])
def test_clip_p2p_render_two_ranks(form):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "clip_p2p_worker.py"), form]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("[")][-1])
    assert len(out) == 2 and all(r["ok"] for r in out), out


def test_clip_async_slots_keep_their_planes(pkg, orc):
    n, W, H = 200_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 44, 0, n, n)
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        outs = [p.host_output_buffers(s) for s in range(2)]
        Ps = [pkg.orbit_projection(k, W, H) for k in (10, 510)]
        names = ("box", "half")
        for s in range(2):
            p.set_clip_planes(_planes(pkg, names[s]))
            p.project_async(Ps[s], s, filtered=False)
        p.set_clip_planes(_planes(pkg, "ceiling"))  # changed between queueing and rtr_wait
        p.wait_outputs(-1)
        for s in range(2):
            r = _ref(pkg, orc, xyzw, rgba, _planes(pkg, names[s]), Ps[s], W, H, False)
            img, depth = outs[s]
            assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(img, r["img"]), s
    finally:
        p.close()


def test_clip_overflow_repaired_with_the_planes_it_was_issued_with(pkg, orc):
    """A fresh 2 M-point cloud whose first frame (P_ONE: the whole cloud in one tile) overflows the adaptive extent pool
    while it keeps ~63 % of the cloud; the planes change before the synchronising call, which renders the frame again --
    with the planes it was issued with.  The same for an async slot that rtr_wait repeats."""
    L = pkg._lib
    xyzw, rgba = sc.cloud(orc)
    W, H = sc.W, sc.H
    P = sc.p_one(orc)[0]
    issued, later = np.float32([[1, 0, 0, 1.5]]), np.float32([[-1, 0, 0, 0]])  # x >= -1.5, then x <= 0
    r = _ref(pkg, orc, xyzw, rgba, issued, P, W, H, False)
    assert r["keep"].sum() > 1_100_000  # (a fresh pool holds max(n / 2, 2^20) entries)
    for form in ("render", "async"):
        p = _new(pkg, {}, xyzw, rgba, W, H)
        try:
            before = sc.footprint(p)
            p.set_clip_planes(issued)
            if form == "render":
                p.render(P, False)
                p.set_clip_planes(later)
                p.synchronize()
                img, depth = p.download(L.BUF_IMAGE), p.download(L.BUF_DEPTH)
            else:
                img, depth = p.host_output_buffers(0)
                p.project_async(P, 0, filtered=False)
                p.set_clip_planes(later)
                p.wait_outputs(0)
                depth = depth.view(np.uint32)
            assert sc.footprint(p) > before  # the pool grew: the frame did overflow and was rendered again
            assert np.array_equal(np.asarray(depth).view(np.uint32).reshape(H, W), r["depth_bits"]), form
            assert np.array_equal(np.asarray(img).reshape(H, W, 3), r["img"]), form
            assert np.array_equal(p.clip_planes(), later)
        finally:
            p.close()


def test_clip_cleared_after_clipped_frames(pkg, orc):
    """Clipped frames size the adaptive pool for few entries; with the planes cleared the whole cloud jumps past it --
    a normal overflow, repaired by the synchronising call."""
    L = pkg._lib
    xyzw, rgba = sc.cloud(orc)
    W, H = sc.W, sc.H
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        crop = pkg.clip_box_planes([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5])
        p.set_clip_planes(crop)
        for k in sc.ORDINARY:
            _check_frame(pkg, orc, p, xyzw, rgba, crop, pkg.orbit_projection(k, W, H), W, H, False, k)
        _check_frame(pkg, orc, p, xyzw, rgba, crop, sc.p_one(orc)[0], W, H, False, "p_one clipped")
        p.set_clip_planes(None)
        P = sc.p_one(orc)[0]
        p.render(P, True)
        p.synchronize()
        r = _ref(pkg, orc, xyzw, rgba, np.zeros((0, 4), np.float32), P, W, H, True)
        assert np.array_equal(p.download(L.BUF_DEPTH), r["depth_bits"])
        assert np.array_equal(p.download(L.BUF_IMAGE), r["img"])
        assert np.array_equal(p.download(L.BUF_TENSOR).reshape(5, H, W), r["tensor"])
    finally:
        p.close()


def test_clip_c3_crop_box_full_size(pkg, orc):
    N, W, H = 100_000_000, 1920, 1080
    p = pkg.Projector(0)
    try:
        p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
        p.set_resolution(W, H)
        crop = pkg.clip_box_planes([-2.0, -1.5, 0.0], [2.0, 0.0, 4.0])
        p.set_clip_planes(crop)
        P = pkg.orbit_projection(17, W, H)
        img, depth = p.project(P, filtered=True)
        xyzw, rgba = p.download_points()
        keep = pkg.clip_keep(crop, xyzw)
        assert 0 < keep.sum() < N // 4
        xs, rs = xyzw[keep], rgba[keep]
        del xyzw, rgba
        try:
            threads = max(1, min(16, len(os.sched_getaffinity(0))))
        except AttributeError:
            threads = 8
        ref = orc.MTProjector(W, H, threads).project(xs, rs, P)
        rf = orc.filter(ref["depth_bits"], ref["img"])
        assert np.array_equal(depth.view(np.uint32), rf["depth"].view(np.uint32))
        assert np.array_equal(img, rf["img"])
        assert np.array_equal(p.download(pkg._lib.BUF_TENSOR).reshape(5, H, W), rf["tensor"])
    finally:
        p.close()
