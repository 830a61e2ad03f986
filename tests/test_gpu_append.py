"""Appending points to the resident cloud on the GPU (include/rtr.h section 2b): a cloud built by rtr_upload_points(A)
and rtr_append_points(B1) .. (Bk) renders bit for bit what one upload of A ++ B1 ++ .. ++ Bk renders -- compared with a
second context that uploads the concatenation AND with the oracle on it -- in every form the cloud and the frame can
take; the point pass, the keep mask, clip planes, views, the phase calls, the async slots, an overflowing extent pool,
the error paths, downloads, the peer-to-peer exchange and the memory the grown arrays hold."""
import ctypes as C

import numpy as np
import pytest

import pool_overflow_scenes as sc

pytestmark = pytest.mark.gpu

CONFIGS = {"default": {}, "pack0": {"pack": 0}, "pack2": {"pack": 2}, "mode0": {"mode": 0}, "cull": {"cull": 1},
           "chunk_test0": {"chunk_test": 0}, "lane_test0": {"lane_test": 0}, "overlap": {"overlap": 1},
           "auto_reorder1": {"auto_reorder": 1}, "keep_soa1": {"keep_soa": 1}, "point_ids1": {"point_ids": 1}}


def _new(pkg, options, W, H):
    p = pkg.Projector(0)
    for k, v in options.items():
        p.set_option(k, v)
    p.set_resolution(W, H)
    return p


def _build(pkg, options, xyzw, rgba, cuts, W, H):
    """(appended, one-shot): the first cloud uploads xyzw[:cuts[0]] and appends the pieces between the cuts."""
    a = _new(pkg, options, W, H)
    a.upload_points(xyzw[:cuts[0]], rgba[:cuts[0]])
    for lo, hi in zip(cuts, list(cuts[1:]) + [len(xyzw)]):
        a.append_points(xyzw[lo:hi], rgba[lo:hi])
    assert a.num_points == len(xyzw)
    b = _new(pkg, options, W, H)
    b.upload_points(xyzw, rgba)
    return a, b


def _ref(orc, xyzw, rgba, P, W, H, filtered):
    r = orc.project(xyzw, rgba, P, W, H)
    out = {"depth_bits": r["depth_bits"], "img": r["img"]}
    if filtered:
        f = orc.filter(r["depth_bits"], r["img"])
        out.update(depth_bits=f["depth"].view(np.uint32), img=f["img"], tensor=f["tensor"], minmax=f["minmax"])
    return out


def _frame(pkg, p, P, filtered):
    L = pkg._lib
    img, depth = p.project(P, filtered=filtered)
    out = {"depth_bits": depth.view(np.uint32).copy(), "img": img.copy()}
    if filtered:
        out["tensor"] = p.download(L.BUF_TENSOR).reshape(5, p.H, p.W)
        out["minmax"] = p.download(L.BUF_MINMAX)
    return out


def _check(pkg, orc, a, b, xyzw, rgba, P, filtered, what, keep=None):
    """a's frame == b's frame == the oracle's on the (kept) concatenation."""
    filtered = filtered and a.W % 16 == 0 and a.H >= 16
    fa, fb = _frame(pkg, a, P, filtered), _frame(pkg, b, P, filtered) if b is not None else None
    sel = np.ones(len(xyzw), bool) if keep is None else keep
    r = _ref(orc, xyzw[sel], rgba[sel], P, a.W, a.H, filtered)
    for k in ("depth_bits", "img") + (("tensor", "minmax") if filtered else ()):
        ref = r[k] if k != "minmax" else np.asarray(r[k]).view(np.uint32).reshape(2)
        assert np.array_equal(fa[k], ref), (k, what)
        if fb is not None:
            assert np.array_equal(fa[k], fb[k]), (k, "one-shot", what)


SCENES = (("room_shell", 150_000, (60_001, 130_000)),   # blocks of a coherent scan: never sorted
          ("uniform_box", 160_000, (30_001, 100_000)))  # hash order: the 70 000-point block is sorted on its own


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_append_configs_match_one_shot_and_oracle(pkg, orc, config):
    W, H = 320, 240
    for scene, n, cuts in SCENES:
        xyzw, rgba = orc.generate(scene, 71, 0, n, n)
        a, b = _build(pkg, CONFIGS[config], xyzw, rgba, cuts, W, H)
        try:
            if scene == "uniform_box" and config != "auto_reorder1":
                assert a.get_option("reordered") == 1  # (the 70 000-point block took the block sort)
            for k in range(4):
                _check(pkg, orc, a, b, xyzw, rgba, pkg.orbit_projection(37 * k + 5, W, H), k % 2 == 1, (config, scene, k))
        finally:
            a.close(); b.close()


SPLITS = ((0, 1000), (1, 1), (255, 1), (256, 256), (1000, 3), (4099, 70_001), ((1 << 20) + 13, (1 << 16) + 5))


@pytest.mark.parametrize("options", ({}, {"pack": 2, "point_ids": 1}, {"pack": 0}), ids=("default", "pack2", "pack0"))
def test_append_split_shapes(pkg, orc, options):
    W, H = 160, 128
    for scene in ("room_shell", "uniform_box"):
        for nA, m in SPLITS:
            n = nA + m
            xyzw, rgba = orc.generate(scene, 900 + nA, 0, n, n)
            a = _new(pkg, options, W, H)
            if nA:
                a.upload_points(xyzw[:nA], rgba[:nA])
            a.append_points(xyzw[nA:], rgba[nA:])
            try:
                assert a.num_points == n
                for k, filt in enumerate((False, True)):
                    _check(pkg, orc, a, None, xyzw, rgba, pkg.orbit_projection(3 * nA + k, W, H), filt, (scene, nA, m))
            finally:
                a.close()
    # ten successive appends of uneven sizes
    sizes = (5000, 1, 255, 257, 70_001, 3, 40_000, 66_000, 17, 100_000)
    n = 20_000 + sum(sizes)
    for scene in ("room_shell", "uniform_box"):
        xyzw, rgba = orc.generate(scene, 4242, 0, n, n)
        cuts = [20_000] + list(20_000 + np.cumsum(sizes[:-1]))
        a, b = _build(pkg, options, xyzw, rgba, cuts, W, H)
        try:
            for k, filt in enumerate((False, True, False)):
                _check(pkg, orc, a, b, xyzw, rgba, pkg.orbit_projection(100 + k, W, H), filt, (scene, "ten"))
        finally:
            a.close(); b.close()


def test_append_point_pass(pkg, orc):
    L = pkg._lib
    W, H = 320, 240
    n, cuts = 160_000, (30_001, 100_000)
    xyzw, rgba = orc.generate("uniform_box", 17, 0, n, n)
    a, b = _build(pkg, {"point_ids": 1}, xyzw, rgba, cuts, W, H)
    try:
        assert a.get_option("reordered") == 1
        for k in range(3):
            P = pkg.orbit_projection(11 * k + 2, W, H)
            for p in (a, b):
                p.render(P)
                p.point_pass(P)
            ids_a, ids_b = a.download(L.BUF_POINT_ID), b.download(L.BUF_POINT_ID)
            assert np.array_equal(ids_a, ids_b)
            assert np.array_equal(a.download(L.BUF_VISIBLE), b.download(L.BUF_VISIBLE))
            assert (ids_a[ids_a != 0xFFFFFFFF] >= cuts[0]).any()  # (appended points are named n_A + j)
    finally:
        a.close(); b.close()
    # point_ids = 0 on a cloud the block sort reordered: the point pass is refused
    p = _new(pkg, {}, W, H)
    try:
        p.upload_points(xyzw[:30_001], rgba[:30_001])
        assert p.get_option("reordered") == 0
        p.append_points(xyzw[30_001:], rgba[30_001:])
        assert p.get_option("reordered") == 1
        P = pkg.orbit_projection(2, W, H)
        p.render(P)
        with pytest.raises(pkg.RtrError) as e:
            p.point_pass(P)
        assert e.value.code == L.RTR_ERR_INVALID
    finally:
        p.close()


def test_append_keep_mask(pkg, orc):
    W, H = 320, 240
    for scene, ids in (("room_shell", 1), ("uniform_box", 1), ("uniform_box", 0)):
        n, nA = 130_000, 30_000
        xyzw, rgba = orc.generate(scene, 23, 0, n, n)
        p = _new(pkg, {"point_ids": ids}, W, H)
        try:
            p.upload_points(xyzw[:nA], rgba[:nA])
            keepA = np.random.default_rng(5).random(nA) >= 0.3
            p.set_point_keep(keepA)
            p.append_points(xyzw[nA:], rgba[nA:])
            keep = np.concatenate([keepA, np.ones(n - nA, bool)])
            assert np.array_equal(p.point_keep(), keep)
            assert p.download(pkg._lib.BUF_POINT_KEEP).size == (n + 31) // 32
            if ids == 0:  # masked, in upload order, point_ids 0: the 100 000-point block stays unsorted
                assert p.get_option("reordered") == 0
            for k in range(2):
                _check(pkg, orc, p, None, xyzw, rgba, pkg.orbit_projection(7 * k + 1, W, H), k == 1, (scene, ids), keep)
        finally:
            p.close()


def test_append_clip_views_phases(pkg, orc):
    L = pkg._lib
    W, H = 320, 240
    n, cuts = 150_000, (60_001, 130_000)
    xyzw, rgba = orc.generate("room_shell", 29, 0, n, n)
    a, b = _build(pkg, {}, xyzw, rgba, cuts, W, H)
    try:
        planes = np.array([[1.0, 0.0, 0.0, 0.5], [0.0, -1.0, 0.2, 1.0]], np.float32)
        for p in (a, b):
            p.set_clip_planes(planes)
        x, y, z = (xyzw[:, k].astype(np.float32) for k in range(3))
        inside = np.ones(n, bool)
        for a_, b_, c_, d_ in planes:  # (float32, in the header's order)
            inside &= ((a_ * x + b_ * y) + c_ * z) + d_ >= np.float32(0)
        _check(pkg, orc, a, b, xyzw, rgba, pkg.orbit_projection(44, W, H), True, "clip", inside)
        for p in (a, b):
            p.set_clip_planes(None)
        Ps = np.stack([pkg.orbit_projection(9 * k, W, H) for k in range(3)])
        for p in (a, b):
            p.render_views(Ps, with_filter=True)
        for which in (L.BUF_VIEW_DEPTH, L.BUF_VIEW_IMAGE, L.BUF_VIEW_TENSOR, L.BUF_VIEW_MINMAX):
            assert np.array_equal(a.download(which), b.download(which)), which
        r = orc.project(xyzw, rgba, Ps[1], W, H)
        rf = orc.filter(r["depth_bits"], r["img"])
        assert np.array_equal(a.download(L.BUF_VIEW_DEPTH)[1], rf["depth"].view(np.uint32))
        P = pkg.orbit_projection(61, W, H)
        for p in (a, b):
            p.clear(); p.min_depth_pass(P); p.accumulate_pass(P); p.resolve()
        r = orc.project(xyzw, rgba, P, W, H)
        for which in (L.BUF_DEPTH, L.BUF_ACCUM, L.BUF_IMAGE):
            assert np.array_equal(a.download(which), b.download(which)), which
        assert np.array_equal(a.download(L.BUF_DEPTH), r["depth_bits"])
        for p in (a, b):
            p.project(P)
        sa, sb = a.frame_stats(), b.frame_stats()
        assert (sa["entries"], sa["heaviest_tile"]) == (sb["entries"], sb["heaviest_tile"])
    finally:
        a.close(); b.close()


def test_append_async_slot_keeps_old_frame(pkg, orc):
    W, H = 320, 240
    n, nA = 150_000, 60_000
    xyzw, rgba = orc.generate("room_shell", 31, 0, n, n)
    p = _new(pkg, {}, W, H)
    try:
        p.upload_points(xyzw[:nA], rgba[:nA])
        P = pkg.orbit_projection(12, W, H)
        p.project_async(P, 0)
        p.append_points(xyzw[nA:], rgba[nA:])
        p.wait_outputs(0)
        img, depth = p.host_output_buffers(0)
        r = orc.project(xyzw[:nA], rgba[:nA], P, W, H)
        assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(img, r["img"])
        _check(pkg, orc, p, None, xyzw, rgba, P, False, "after")
    finally:
        p.close()


def test_append_overflows_adaptive_pool_and_repairs(pkg, orc):
    xyzw, rgba = sc.cloud(orc)
    nA = 100_000
    P = sc.p_one(orc)[0]
    p = _new(pkg, {}, sc.W, sc.H)
    try:
        p.upload_points(xyzw[:nA], rgba[:nA])
        p.project(P)  # (a frame that sees the small cloud whole: no overflow)
        p.append_points(xyzw[nA:], rgba[nA:])
        mb0 = p.get_option("resident_millibytes_per_point")
        p.render(P)  # (~2 n entries into a pool of max(n / 2, 2^20): it overflows)
        p.synchronize()  # (repairs the frame: the pool grows to 2 n entries, 16 B per point)
        assert p.get_option("resident_millibytes_per_point") - mb0 >= sc.JUMP_MB
        r = orc.project(xyzw, rgba, P, sc.W, sc.H)
        assert np.array_equal(p.download(pkg._lib.BUF_DEPTH), r["depth_bits"])
        assert np.array_equal(p.download(pkg._lib.BUF_IMAGE), r["img"])
    finally:
        p.close()


def test_append_errors_change_nothing(pkg, orc):
    L = pkg._lib
    W, H = 160, 128
    n = 50_000
    xyzw, rgba = orc.generate("room_shell", 37, 0, n, n)
    p = _new(pkg, {"point_ids": 1}, W, H)
    try:
        p.upload_points(xyzw, rgba)
        p.set_point_keep(np.arange(n) % 3 != 0)
        P = pkg.orbit_projection(8, W, H)
        img0, depth0 = p.project(P)
        keep0 = p.download(L.BUF_POINT_KEEP)
        x = np.ascontiguousarray(xyzw[:10])
        c = np.ascontiguousarray(rgba[:10])
        vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        lib = p._lib
        bad = ((vp(x), 8, vp(c), 4, 10), (vp(x), 18, vp(c), 4, 10), (vp(x), 16, vp(c), 2, 10), (None, 16, vp(c), 4, 10),
               (vp(x), 16, None, 4, 10), (vp(x), 16, vp(c), 4, (1 << 32) - n), (vp(x), 16, vp(c), 4, 1 << 40))
        for args in bad:
            assert lib.rtr_append_points(p._ctx, *args) == L.RTR_ERR_INVALID, args
            assert p.num_points == n
        assert lib.rtr_append_points(p._ctx, vp(x), 16, vp(c), 4, 0) == L.RTR_OK  # (m = 0: nothing)
        assert p.num_points == n
        img1, depth1 = p.project(P)
        assert np.array_equal(depth0.view(np.uint32), depth1.view(np.uint32)) and np.array_equal(img0, img1)
        assert np.array_equal(p.download(L.BUF_POINT_KEEP), keep0)
    finally:
        p.close()


def test_append_downloads(pkg, orc):
    n, nA = 140_000, 60_000
    xyzw, rgba = orc.generate("uniform_box", 41, 0, n, n)
    for options in ({"auto_reorder": 0}, {}):
        p = _new(pkg, options, 64, 48)
        try:
            p.upload_points(xyzw[:nA], rgba[:nA])
            p.append_points(xyzw[nA:100_000], rgba[nA:100_000])
            p.append_points(xyzw[100_000:], rgba[100_000:])
            gx, gc = p.download_points()
            want = np.concatenate([xyzw[:, :3].view(np.uint32), rgba.view(np.uint32)], axis=1)
            got = np.concatenate([gx[:, :3].view(np.uint32), gc.view(np.uint32)], axis=1)
            if options:
                assert np.array_equal(got, want)  # exactly A then B
            else:
                key = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
                assert np.array_equal(key(got), key(want))
        finally:
            p.close()


def test_append_closes_p2p(pkg, orc):
    n = 60_000
    xyzw, rgba = orc.generate("room_shell", 43, 0, n, n)
    p = _new(pkg, {}, 160, 128)
    try:
        p.upload_points(xyzw[:40_000], rgba[:40_000])
        p.p2p_open(0, 1, [p.p2p_export()])
        assert p.get_option("p2p_open") == 1
        p.append_points(xyzw[40_000:], rgba[40_000:])
        assert p.get_option("p2p_open") == 0
        p.p2p_open(0, 1, [p.p2p_export()])  # (every rank exports and opens again)
        assert p.get_option("p2p_open") == 1
    finally:
        p.close()


def test_append_memory_bound(pkg, orc):
    n, W, H = 10_000_000, 640, 480
    xyzw, rgba = orc.generate("room_shell", 47, 0, n, n)
    a = _new(pkg, {}, W, H)
    for lo in range(0, n, 1_000_000):  # (ten contiguous appends, the first one onto an empty context)
        a.append_points(xyzw[lo:lo + 1_000_000], rgba[lo:lo + 1_000_000])
    b = _new(pkg, {}, W, H)
    b.upload_points(xyzw, rgba)
    try:
        assert a.num_points == n
        P = pkg.orbit_projection(3, W, H)
        a.project(P)
        b.project(P)
        ma, mb = a.get_option("resident_millibytes_per_point"), b.get_option("resident_millibytes_per_point")
        assert ma <= 1.25 * mb, (ma, mb)
    finally:
        a.close(); b.close()
