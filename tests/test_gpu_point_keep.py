"""The keep mask on the GPU (include/rtr.h section 6e): every frame bit for bit against the oracle run on the subset of
the cloud the mask keeps -- depth bits, image, and (filtered) the fp16 tensor and min / max -- in every form the cloud
and the frame can take; the point pass, several views, the phase calls, the peer-to-peer frame, clip planes together
with the mask, a point pass's visibility fed back, the async slots and the repair journal across a change of mask."""
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

CONFIGS = {"default": {}, "pack0": {"pack": 0}, "pack2": {"pack": 2}, "mode0": {"mode": 0}, "cull": {"cull": 1},
           "cull_pack0": {"cull": 1, "pack": 0}, "chunk_test0": {"chunk_test": 0}, "lane_test0": {"lane_test": 0},
           "lane_test0_pack0": {"lane_test": 0, "pack": 0}, "overlap": {"overlap": 1}, "sorted": {}}
MASKS = ("none_set", "all", "none", "hide10", "hide90", "lane_first", "lane_rest", "one_per_chunk", "half")


def _mask(name, n, seed=0):
    """bool[n] over upload indices, or None (no mask)."""
    i = np.arange(n)
    rng = np.random.default_rng(1000 + seed)
    return {
        "none_set": None,
        "all": np.ones(n, bool),
        "none": np.zeros(n, bool),
        "hide10": rng.random(n) >= 0.10,
        "hide90": rng.random(n) >= 0.90,
        "lane_first": i % 4 != 0,      # point 4 l of every lane hidden: the lane test's probe point
        "lane_rest": i % 4 == 0,       # only 4 l + 1 .. 4 l + 3 hidden
        "one_per_chunk": i % 256 == 77,
        "half": i >= n // 2,           # a contiguous upload-order half hidden
    }[name]


def _words(keep):
    n = keep.size
    pad = np.zeros(32 * ((n + 31) // 32), bool)
    pad[:n] = keep
    return np.packbits(pad, bitorder="little").view("<u4").copy()


def _ref(orc, xyzw, rgba, keep, P, W, H, filtered):
    keep = np.ones(len(xyzw), bool) if keep is None else keep
    r = orc.project(xyzw[keep], rgba[keep], P, W, H)
    out = {"depth_bits": r["depth_bits"], "img": r["img"], "acc": r["acc"]}
    if filtered:
        f = orc.filter(r["depth_bits"], r["img"])
        out.update(depth_bits=f["depth"].view(np.uint32), img=f["img"], tensor=f["tensor"], minmax=f["minmax"])
    return out


def _check_frame(pkg, orc, p, xyzw, rgba, keep, P, W, H, filtered, what):
    L = pkg._lib
    filtered = filtered and W % 16 == 0 and H >= 16
    img, depth = p.project(P, filtered=filtered)
    r = _ref(orc, xyzw, rgba, keep, P, W, H, filtered)
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
    p.set_option("point_ids", 1)  # (the mask is in upload order: an unordered cloud is sorted at upload)
    p.upload_points(xyzw, rgba)
    if sort:
        p.reorder_points()
    p.set_resolution(W, H)
    return p


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_keep_frames_match_subset_oracle(pkg, orc, config):
    sort = config == "sorted"
    for scene, n, (W, H) in (("room_shell", 200_000, (640, 480)), ("uniform_box", 150_000, (64, 48)),
                             ("room_shell", 4099, (64, 48))):
        xyzw, rgba = orc.generate(scene, 37, 0, n, n)
        p = _new(pkg, CONFIGS[config], xyzw, rgba, W, H, sort)
        try:
            for k, name in enumerate(MASKS):
                keep = _mask(name, n, k)
                p.set_point_keep(keep)
                got = p.point_keep()
                assert (got is None) if keep is None else np.array_equal(got, keep), name
                P = pkg.orbit_projection(89 * k + 3, W, H)
                _check_frame(pkg, orc, p, xyzw, rgba, keep, P, W, H, k % 2 == 1, (config, scene, n, name))
            # an all-kept mask: byte for byte the frame without one
            P = pkg.orbit_projection(11, W, H)
            p.set_point_keep(None)
            img0, depth0 = p.project(P, filtered=W % 16 == 0)
            p.set_point_keep(np.ones(n, bool))
            img1, depth1 = p.project(P, filtered=W % 16 == 0)
            assert np.array_equal(depth0.view(np.uint32), depth1.view(np.uint32)) and np.array_equal(img0, img1)
        finally:
            p.close()


def test_keep_ragged_counts(pkg, orc):
    for n in (1, 3, 5, 37, 255, 256, 257, 1023, 4099):
        xyzw, rgba = orc.generate("room_shell", 200 + n, 0, n, n)
        for options in ({}, {"mode": 0}, {"pack": 2}):
            p = _new(pkg, options, xyzw, rgba, 64, 48)
            try:
                for k, name in enumerate(("hide10", "lane_first", "none", "half")):
                    keep = _mask(name, n, k)
                    p.set_point_keep(_words(keep))
                    _check_frame(pkg, orc, p, xyzw, rgba, keep, pkg.orbit_projection(n + k, 64, 48), 64, 48, True,
                                 (n, options, name))
            finally:
                p.close()


def test_keep_given_in_upload_order_follows_a_sort(pkg, orc):
    L = pkg._lib
    n, W, H = 150_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 9, 0, n, n)
    keep = _mask("hide10", n, 3) & (np.arange(n) % 7 != 0)
    p = pkg.Projector(0)
    try:
        p.set_option("auto_reorder", 0)
        p.set_option("point_ids", 1)
        p.upload_points(xyzw, rgba)
        p.set_resolution(W, H)
        p.set_point_keep(keep)
        _check_frame(pkg, orc, p, xyzw, rgba, keep, pkg.orbit_projection(40, W, H), W, H, True, "before the sort")
        p.reorder_points()
        assert p.get_option("reordered") == 1
        assert np.array_equal(p.point_keep(), keep)  # (still in upload order)
        _check_frame(pkg, orc, p, xyzw, rgba, keep, pkg.orbit_projection(40, W, H), W, H, True, "after the sort")
        p.reorder_points()  # (a second sort: through the permutation again)
        _check_frame(pkg, orc, p, xyzw, rgba, keep, pkg.orbit_projection(500, W, H), W, H, False, "sorted twice")
    finally:
        p.close()
    # a sorted cloud without point_ids: no upload order to map, nothing changes
    p = pkg.Projector(0)
    try:
        p.set_option("auto_reorder", 0)
        p.upload_points(xyzw, rgba)
        p.set_resolution(W, H)
        p.reorder_points()
        with pytest.raises(L.RtrError) as e:
            p.set_point_keep(keep)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        assert p.point_keep() is None
        p.set_point_keep(None)  # (clearing is always fine)
    finally:
        p.close()
    # a masked cloud is not sorted without point_ids
    p = pkg.Projector(0)
    try:
        p.set_option("auto_reorder", 0)
        p.upload_points(xyzw, rgba)
        p.set_resolution(W, H)
        p.set_point_keep(keep)
        with pytest.raises(L.RtrError) as e:
            p.reorder_points()
        assert e.value.code == L.RTR_ERR_INVALID
        assert p.get_option("reordered") == 0
        _check_frame(pkg, orc, p, xyzw, rgba, keep, pkg.orbit_projection(40, W, H), W, H, False, "sort refused")
    finally:
        p.close()


@pytest.mark.parametrize("config", ["default", "pack0", "mode0", "sorted"])
def test_keep_point_pass(pkg, orc, config):
    L = pkg._lib
    n, W, H = 60_000, 160, 120
    xyzw, rgba = orc.generate("room_shell", 12, 0, n, n)
    p = _new(pkg, CONFIGS[config], xyzw, rgba, W, H, sort=config == "sorted")
    try:
        for k, name in enumerate(("hide10", "half", "lane_first", "none", "all")):
            keep = _mask(name, n, k)
            p.set_point_keep(keep)
            P = pkg.orbit_projection(50 + 200 * k, W, H)
            p.render(P, False)
            p.point_pass(P)
            ids, vis = p.download(L.BUF_POINT_ID), p.download(L.BUF_VISIBLE)
            sub = np.flatnonzero(keep)
            r = orc.project(xyzw[keep], rgba[keep], P, W, H)
            assert np.array_equal(p.download(L.BUF_DEPTH), r["depth_bits"])
            e_ids, e_vis = ppr.point_pass(orc, xyzw[keep], P, W, H, r["depth_bits"])
            full_ids = np.where(e_ids == L.NO_POINT, L.NO_POINT,
                                sub[np.minimum(e_ids, max(len(sub) - 1, 0))] if len(sub) else L.NO_POINT)
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


@pytest.mark.parametrize("config", ["default", "pack0", "mode0", "lane_test0"])
def test_keep_render_views(pkg, orc, config):
    L = pkg._lib
    n, W, H = 150_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 8, 0, n, n)
    p = _new(pkg, CONFIGS[config], xyzw, rgba, W, H)
    try:
        poses = (3, 170, 400, 650, 900, 40, 555, 777)
        for K, name in ((1, "hide10"), (3, "half"), (8, "lane_first"), (3, "hide90")):
            keep = _mask(name, n, K)
            p.set_point_keep(keep)
            Ps = np.stack([pkg.orbit_projection(k, W, H).reshape(4, 4) for k in poses[:K]])
            p.render_views(Ps, True)
            depth = p.download(L.BUF_VIEW_DEPTH).reshape(K, H, W)
            img = p.download(L.BUF_VIEW_IMAGE).reshape(K, H, W, 3)
            tensor = p.download(L.BUF_VIEW_TENSOR).reshape(K, 5, H, W)
            for v, P in enumerate(Ps):
                r = _ref(orc, xyzw, rgba, keep, P.reshape(16), W, H, True)
                assert np.array_equal(depth[v], r["depth_bits"]), (config, name, K, v)
                assert np.array_equal(img[v], r["img"]), (config, name, K, v)
                assert np.array_equal(tensor[v], r["tensor"]), (config, name, K, v)
    finally:
        p.close()


@pytest.mark.parametrize("config", ["default", "pack0", "mode0", "sorted"])
def test_keep_with_clip_planes(pkg, orc, config):
    n, W, H = 150_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 14, 0, n, n)
    p = _new(pkg, CONFIGS[config], xyzw, rgba, W, H, sort=config == "sorted")
    try:
        for k, (planes, name) in enumerate(((pkg.clip_box_planes([-2.0, -1.5, -2.0], [2.0, 1.5, 2.0]), "hide10"),
                                            (np.float32([[1, 0, 0, 0]]), "half"),
                                            (np.float32([[0, -1, 0, 1.0]]), "lane_rest"))):
            mask = _mask(name, n, k)
            p.set_clip_planes(planes)
            p.set_point_keep(mask)
            keep = pkg.clip_keep(planes, xyzw) & mask
            _check_frame(pkg, orc, p, xyzw, rgba, keep, pkg.orbit_projection(60 + 150 * k, W, H), W, H, k != 1, (config, k))
        p.set_clip_planes(None)
        _check_frame(pkg, orc, p, xyzw, rgba, mask, pkg.orbit_projection(20, W, H), W, H, False, (config, "mask only"))
    finally:
        p.close()


def test_keep_fed_back_from_the_visibility_device_buffer(pkg, orc):
    L = pkg._lib
    n, W, H = 200_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 15, 0, n, n)
    for sort in (False, True):
        p = _new(pkg, {}, xyzw, rgba, W, H, sort=sort)
        try:
            PA, PB = pkg.orbit_projection(100, W, H), pkg.orbit_projection(180, W, H)
            p.render(PA, False)
            p.point_pass(PA, ids=False, visible=True)
            vis = ppr.unpack(p.download(L.BUF_VISIBLE), n)
            assert 0 < vis.sum() < n
            p.set_point_keep(p.device_buffer(L.BUF_VISIBLE))  # device memory, straight back
            assert np.array_equal(p.point_keep(), vis)
            _check_frame(pkg, orc, p, xyzw, rgba, vis, PB, W, H, True, ("feedback", sort))
            # a torch tensor holding the words works the same
            import torch
            words = torch.as_tensor(_words(~vis).view(np.int32), device="cuda")
            p.set_point_keep(words)
            _check_frame(pkg, orc, p, xyzw, rgba, ~vis, PB, W, H, False, ("torch", sort))
        finally:
            p.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_keep_phase_calls_two_contexts(pkg, orc, mode):
    import torch
    n, W, H = 120_000, 640, 480
    xyzw, rgba = orc.generate("room_shell", 21, 0, n, n)
    P = pkg.orbit_projection(300, W, H)
    keep = _mask("hide10", n, 5) & (np.arange(n) % 3 != 1)
    ref = orc.project(xyzw[keep], rgba[keep], P, W, H)
    reff = orc.filter(ref["depth_bits"], ref["img"])
    locs = []
    for r in range(2):
        lo, hi = pkg.shard_range(n, r, 2)
        p = pkg.Projector(0)
        p.set_option("mode", mode)
        p.upload_points(xyzw[lo:hi], rgba[lo:hi])
        p.set_resolution(W, H)
        p.set_point_keep(keep[lo:hi])  # (each context its own mask, in its own indices)
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
def test_keep_p2p_render_two_ranks(form):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "keep_p2p_worker.py"), form]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("[")][-1])
    assert len(out) == 2 and all(r["ok"] for r in out), out


def test_keep_lifetime_readback_and_errors(pkg, orc):
    L = pkg._lib
    lib = L.lib()
    n, W, H = 1000, 64, 48
    xyzw, rgba = orc.generate("room_shell", 1, 0, n, n)
    p = pkg.Projector(0)
    try:
        assert lib.rtr_set_point_keep(p._ctx, None, 1) == L.RTR_ERR_INVALID  # no cloud (and NULL words)
        w0 = np.ones(1, np.uint32)
        assert lib.rtr_set_point_keep(p._ctx, w0.ctypes.data_as(np.ctypeslib.ctypes.c_void_p), 1) == L.RTR_ERR_INVALID
        p.upload_points(xyzw, rgba)
        p.set_resolution(W, H)
        assert p.point_keep() is None and p.get_option("point_keep") == 0
        keep = _mask("hide10", n, 2)
        words = _words(keep)
        words[-1] |= ~np.uint32((1 << (n % 32)) - 1)  # bits past n set on input: ignored, read back as 0
        p.set_point_keep(words)
        back = p.download(L.BUF_POINT_KEEP)
        assert np.array_equal(back, _words(keep)) and back[-1] >> (n % 32) == 0
        for bad_words, bad_n in ((np.ones(len(words) + 1, np.uint32), len(words) + 1),
                                 (np.ones(len(words) - 1, np.uint32), len(words) - 1)):
            assert lib.rtr_set_point_keep(p._ctx, bad_words.ctypes.data_as(np.ctypeslib.ctypes.c_void_p), bad_n) == L.RTR_ERR_INVALID
        assert lib.rtr_set_point_keep(p._ctx, None, len(words)) == L.RTR_ERR_INVALID
        with pytest.raises(ValueError):
            p.set_point_keep(np.ones(n + 1, bool))
        assert np.array_equal(p.point_keep(), keep)  # nothing changed
        _check_frame(pkg, orc, p, xyzw, rgba, keep, pkg.orbit_projection(5, W, H), W, H, True, "after the errors")
        # a new cloud clears the mask
        p.upload_points(xyzw, rgba)
        assert p.point_keep() is None
        _check_frame(pkg, orc, p, xyzw, rgba, None, pkg.orbit_projection(5, W, H), W, H, True, "new upload")
        p.set_point_keep(keep)
        p.generate_synthetic("room_shell", 1, 0, n, n)
        assert p.point_keep() is None
        # a download returns every point, masked or not
        p.set_point_keep(keep)
        got, _ = p.download_points()
        assert len(got) == n
    finally:
        p.close()


def test_keep_project_cloud_methods(pkg, orc):
    n, W, H = 50_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 31, 0, n, n)
    rng = np.random.default_rng(3)
    order = rng.permutation(n)  # an unordered cloud: the library sorts it, point_ids keeps the indices
    xyzw, rgba = xyzw[order], rgba[order]
    pc = pkg.ProjectCloud(xyzw, rgba, point_ids=True)
    try:
        cal, E = pkg.benchmark_calibration(W, H), pkg.orbit_pose(123)
        P = orc.compose_projection(cal.getIntrinsicsMatrix(), E)
        hide1, hide2 = rng.choice(n, 5000, replace=False), rng.choice(n, 9000, replace=False)
        pc.hidePoints(hide1)
        pc.hidePoints(hide2)
        keep = np.ones(n, bool)
        keep[hide1] = keep[hide2] = False
        color, depth = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.float32)
        assert pc.computeRGBD(cal, E, color, depth) == 1
        r = orc.project(xyzw[keep], rgba[keep], P, W, H)
        assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(color, r["img"])
        ids = pc.computePointIds(cal, E)
        assert keep[ids[ids >= 0]].all()
        vis = pc.visible_points(cal, E)
        assert not vis[~keep].any()
        pc.setPointKeep(vis)  # what one pose shows, for the next
        assert pc.computeRGBD(cal, E, color, depth) == 1
        r2 = orc.project(xyzw[vis], rgba[vis], P, W, H)
        assert np.array_equal(depth.view(np.uint32), r2["depth_bits"]) and np.array_equal(color, r2["img"])
        pc.clearPointKeep()
        assert pc.computeRGBD(cal, E, color, depth) == 1
        r3 = orc.project(xyzw, rgba, P, W, H)
        assert np.array_equal(depth.view(np.uint32), r3["depth_bits"])
    finally:
        pc.projector.close()


def test_keep_overflow_repaired_with_the_mask_it_was_issued_with(pkg, orc):
    """A fresh 2 M-point cloud whose first frame (P_ONE: the whole cloud in one tile) overflows the adaptive extent pool
    under mask A; rtr_set_point_keep(B) completes it first -- rendered again with A -- and the next frame is B's.  The
    same for an async slot (rtr_wait after the change) and a batch of views."""
    L = pkg._lib
    xyzw, rgba = sc.cloud(orc)
    n, W, H = len(xyzw), sc.W, sc.H
    P = sc.p_one(orc)[0]
    rng = np.random.default_rng(77)
    A, B = rng.random(n) >= 0.3, rng.random(n) >= 0.6
    assert A.sum() > 1_100_000  # (a fresh pool holds max(n / 2, 2^20) entries)
    ra, rb = _ref(orc, xyzw, rgba, A, P, W, H, False), _ref(orc, xyzw, rgba, B, P, W, H, False)
    for form in ("render", "async", "views"):
        p = _new(pkg, {}, xyzw, rgba, W, H)
        try:
            before = sc.footprint(p)
            p.set_point_keep(A)
            if form == "render":
                p.render(P, False)
                p.set_point_keep(B)
                img, depth = p.download(L.BUF_IMAGE), p.download(L.BUF_DEPTH)
                assert sc.footprint(p) > before  # the pool grew: the frame did overflow and was rendered again
            elif form == "async":
                img, depth = p.host_output_buffers(0)
                p.project_async(P, 0, filtered=False)
                p.set_point_keep(B)
                p.wait_outputs(0)
                assert sc.footprint(p) > before
            else:
                p.render_views(np.stack([P.reshape(4, 4), pkg.orbit_projection(7, W, H).reshape(4, 4)]), False)
                p.set_point_keep(B)
                depth = p.download(L.BUF_VIEW_DEPTH).reshape(2, H, W)[0]
                img = p.download(L.BUF_VIEW_IMAGE).reshape(2, H, W, 3)[0]
            assert np.array_equal(np.asarray(depth).view(np.uint32).reshape(H, W), ra["depth_bits"]), form
            assert np.array_equal(np.asarray(img).reshape(H, W, 3), ra["img"]), form
            assert np.array_equal(p.point_keep(), B)
            img2, depth2 = p.project(P)
            assert np.array_equal(depth2.view(np.uint32), rb["depth_bits"]) and np.array_equal(img2, rb["img"]), form
        finally:
            p.close()


def test_keep_c3_random_half_full_size(pkg, orc):
    N, W, H = 100_000_000, 1920, 1080
    p = pkg.Projector(0)
    try:
        p.set_option("auto_reorder", 0)  # (resident order = upload order: download_points gives the indices)
        p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
        p.set_resolution(W, H)
        keep = np.random.default_rng(50).random(N) < 0.5
        p.set_point_keep(keep)
        P = pkg.orbit_projection(17, W, H)
        img, depth = p.project(P, filtered=True)
        xyzw, rgba = p.download_points()
        xs, rs = xyzw[keep], rgba[keep]
        del xyzw, rgba, keep
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
