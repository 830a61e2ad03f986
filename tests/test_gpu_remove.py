"""Removing points from the resident cloud on the GPU (include/rtr.h section 2c): rtr_upload_points(A) then
rtr_remove_points(keep) renders bit for bit what one upload of A[keep] renders -- compared with a second context that
uploads A[keep] AND with the oracle on it -- in every form the cloud and the frame can take; the renumbered point pass,
the keep mask in force, sequences with appends, clip planes, views, the phase calls, the async slots, an overflowing
extent pool, the error paths, downloads, the peer-to-peer exchange and the memory the compacted arrays hold."""
import ctypes as C
import os

import numpy as np
import pytest

import pool_overflow_scenes as sc

pytestmark = pytest.mark.gpu

CONFIGS = {"default": {}, "pack0": {"pack": 0}, "pack2": {"pack": 2}, "mode0": {"mode": 0}, "cull": {"cull": 1},
           "chunk_test0": {"chunk_test": 0}, "lane_test0": {"lane_test": 0}, "overlap": {"overlap": 1},
           "auto_reorder1": {"auto_reorder": 1}, "keep_soa1": {"keep_soa": 1}, "point_ids1": {"point_ids": 1}}
SCENES = (("room_shell", 150_001), ("uniform_box", 160_003))  # (a coherent scan, never sorted; hash order: sorted)


def _new(pkg, options, W, H):
    p = pkg.Projector(0)
    for k, v in options.items():
        p.set_option(k, v)
    p.set_resolution(W, H)
    return p


def _options(config, scene):
    o = dict(CONFIGS[config])
    if scene == "uniform_box" or config == "auto_reorder1":  # (the library sorts these clouds)
        o["point_ids"] = 1
    return o


def _shapes(n, seed):
    """Removal shapes as keep masks over the upload indices."""
    idx = np.arange(n)
    rng = np.random.default_rng(seed)
    last = n - n % 256 if n % 256 else n - 256
    return {"random": rng.random(n) >= 0.3,
            "middle": (idx < n // 3) | (idx >= n // 2),
            "tail": idx < n - n // 5,
            "last_partial_chunk": idx < last,
            "one_chunk": (idx < 256 * 5) | (idx >= 256 * 6),
            "every_other_chunk": (idx // 256) % 2 == 0}


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


def _check(pkg, orc, a, b, xyzw, rgba, P, filtered, what):
    """a's frame == b's frame == the oracle's on (xyzw, rgba)."""
    filtered = filtered and a.W % 16 == 0 and a.H >= 16
    fa = _frame(pkg, a, P, filtered)
    fb = _frame(pkg, b, P, filtered) if b is not None else None
    r = _ref(orc, xyzw, rgba, P, a.W, a.H, filtered)
    for k in ("depth_bits", "img") + (("tensor", "minmax") if filtered else ()):
        ref = r[k] if k != "minmax" else np.asarray(r[k]).view(np.uint32).reshape(2)
        assert np.array_equal(fa[k], ref), (k, what)
        if fb is not None:
            assert np.array_equal(fa[k], fb[k]), (k, "one-shot", what)


def _words(keep):
    n = keep.size
    return np.packbits(np.concatenate([keep, np.zeros(-n % 32, bool)]), bitorder="little").view("<u4").copy()


def _pair(pkg, options, xyzw, rgba, keep, W, H):
    """(removed, one-shot): the first context uploads everything and removes ~keep, the second uploads the survivors."""
    a = _new(pkg, options, W, H)
    a.upload_points(xyzw, rgba)
    a.remove_points(keep)
    b = _new(pkg, options, W, H)
    b.upload_points(xyzw[keep], rgba[keep])
    assert a.num_points == b.num_points == int(keep.sum())
    return a, b


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_remove_configs_match_one_shot_and_oracle(pkg, orc, config):
    W, H = 320, 240
    for scene, n in SCENES:
        options = _options(config, scene)
        xyzw, rgba = orc.generate(scene, 73, 0, n, n)
        a, b = _new(pkg, options, W, H), _new(pkg, options, W, H)
        try:
            for j, (shape, keep) in enumerate(_shapes(n, 5).items()):
                a.upload_points(xyzw, rgba)
                if scene == "uniform_box":
                    assert a.get_option("reordered") == 1
                a.remove_points(keep)
                b.upload_points(xyzw[keep], rgba[keep])
                assert a.num_points == int(keep.sum())
                if config == "pack2" or (config == "default" and scene == "room_shell"):
                    assert a.get_option("packed") == 1  # (a packed cloud stays packed)
                for k, filt in enumerate((False, True)):
                    P = pkg.orbit_projection(37 * j + 11 * k + 5, W, H)
                    _check(pkg, orc, a, b, xyzw[keep], rgba[keep], P, filt, (config, scene, shape, filt))
        finally:
            a.close(); b.close()


def test_remove_ragged_sizes(pkg, orc):
    W, H = 160, 128
    for scene in ("room_shell", "uniform_box"):
        for n in (1, 255, 256, 257, 4099, 70_000):
            xyzw, rgba = orc.generate(scene, 200 + n, 0, n, n)
            idx = np.arange(n)
            shapes = [idx != 0, idx != n - 1, (idx < 255) | (idx >= 257), idx >= 256, idx < 256, idx % 256 != 255,
                      (idx // 256) % 3 != 1]
            for s, keep in enumerate(shapes):
                if keep.all() or not keep.any():
                    continue
                a, b = _pair(pkg, {"point_ids": 1}, xyzw, rgba, keep, W, H)
                try:
                    for k, filt in enumerate((False, True)):
                        _check(pkg, orc, a, b, xyzw[keep], rgba[keep], pkg.orbit_projection(3 * n + 7 * s + k, W, H),
                               filt, (scene, n, s))
                finally:
                    a.close(); b.close()


def test_remove_all_and_keep_all(pkg, orc):
    L = pkg._lib
    W, H = 160, 128
    for n in (1, 257, 70_000):
        xyzw, rgba = orc.generate("room_shell", 300 + n, 0, n, n)
        p = _new(pkg, {"point_ids": 1}, W, H)
        try:
            p.upload_points(xyzw, rgba)
            p.set_point_keep(np.arange(n) % 2 == 0)
            P = pkg.orbit_projection(n % 97, W, H)
            img0, depth0 = p.project(P)
            # keep-all: a no-op (frames, mask, p2p unchanged)
            p.p2p_open(0, 1, [p.p2p_export()])
            assert p.get_option("p2p_open") == 1
            p.remove_points(np.ones(n, bool))
            assert p.num_points == n and p.get_option("p2p_open") == 1
            img1, depth1 = p.project(P)
            assert np.array_equal(depth0.view(np.uint32), depth1.view(np.uint32)) and np.array_equal(img0, img1)
            assert np.array_equal(p.point_keep(), np.arange(n) % 2 == 0)
            # remove-all: the context of an upload of 0 points, no mask
            p.remove_points(np.zeros(n, bool))
            assert p.num_points == 0 and p.point_keep() is None
            assert p.get_option("p2p_open") == 0
            e = orc.project(xyzw[:0], rgba[:0], P, W, H)
            for filt in (False, True):
                img, depth = p.project(P, filtered=filt)
                if not filt:
                    assert np.array_equal(depth.view(np.uint32), e["depth_bits"]) and np.array_equal(img, e["img"])
                else:
                    f = orc.filter(e["depth_bits"], e["img"])
                    assert np.array_equal(depth.view(np.uint32), f["depth"].view(np.uint32))
                    assert np.array_equal(img, f["img"])
            with pytest.raises(pkg.RtrError) as err:  # (no cloud now)
                p.remove_points(np.zeros(0, bool))
            assert err.value.code == L.RTR_ERR_INVALID
            p.append_points(xyzw, rgba)  # (an empty context takes an append as an upload)
            _check(pkg, orc, p, None, xyzw, rgba, P, False, ("after remove-all", n))
        finally:
            p.close()


def test_remove_point_pass_renumbered(pkg, orc):
    L = pkg._lib
    W, H = 320, 240
    n = 160_000
    xyzw, rgba = orc.generate("uniform_box", 17, 0, n, n)
    keep = np.random.default_rng(9).random(n) >= 0.4
    a, b = _pair(pkg, {"point_ids": 1}, xyzw, rgba, keep, W, H)
    try:
        assert a.get_option("reordered") == 1
        for k in range(3):
            P = pkg.orbit_projection(11 * k + 2, W, H)
            for p in (a, b):
                p.render(P)
                p.point_pass(P)
            ids_a = a.download(L.BUF_POINT_ID)
            assert np.array_equal(ids_a, b.download(L.BUF_POINT_ID))
            assert np.array_equal(a.download(L.BUF_VISIBLE), b.download(L.BUF_VISIBLE))
            assert ids_a[ids_a != 0xFFFFFFFF].max() < keep.sum()  # (the new indices)
    finally:
        a.close(); b.close()


def test_remove_with_keep_mask_in_force(pkg, orc):
    L = pkg._lib
    W, H = 320, 240
    for scene, ids in (("room_shell", 0), ("room_shell", 1), ("uniform_box", 1)):
        n = 130_001
        xyzw, rgba = orc.generate(scene, 23, 0, n, n)
        rng = np.random.default_rng(ids + 7)
        mask, keep = rng.random(n) >= 0.3, rng.random(n) >= 0.25
        keep[40_000:60_000] = False
        p = _new(pkg, {"point_ids": ids}, W, H)
        b = _new(pkg, {"point_ids": ids}, W, H)
        try:
            p.upload_points(xyzw, rgba)
            p.set_point_keep(mask)
            p.remove_points(keep)
            assert np.array_equal(p.point_keep(), mask[keep])
            assert p.download(L.BUF_POINT_KEEP).size == (int(keep.sum()) + 31) // 32
            b.upload_points(xyzw[keep], rgba[keep])
            b.set_point_keep(mask[keep])
            both = keep & mask
            for k in range(2):
                _check(pkg, orc, p, b, xyzw[both], rgba[both], pkg.orbit_projection(7 * k + 1, W, H), k == 1,
                       (scene, ids))
        finally:
            p.close(); b.close()


def test_remove_commit_point_keep_and_remove_points_methods(pkg, orc):
    n, W, H = 50_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 31, 0, n, n)
    rng = np.random.default_rng(3)
    order = rng.permutation(n)  # an unordered cloud: the library sorts it, point_ids keeps the indices
    xyzw, rgba = xyzw[order], rgba[order]
    pc = pkg.ProjectCloud(xyzw, rgba, point_ids=True)
    try:
        cal, E = pkg.benchmark_calibration(W, H), pkg.orbit_pose(123)
        P = orc.compose_projection(cal.getIntrinsicsMatrix(), E)
        color, depth = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.float32)
        hide = rng.choice(n, 9000, replace=False)
        pc.hidePoints(hide)
        keep = np.ones(n, bool)
        keep[hide] = False
        pc.commitPointKeep()
        assert pc.projector.num_points == int(keep.sum()) and pc.projector.point_keep() is None
        assert pc.computeRGBD(cal, E, color, depth) == 1
        r = orc.project(xyzw[keep], rgba[keep], P, W, H)
        assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(color, r["img"])
        pc.commitPointKeep()  # (no mask: nothing)
        assert pc.projector.num_points == int(keep.sum())
        xs, cs = xyzw[keep], rgba[keep]
        gone = rng.choice(xs.shape[0], 4000, replace=False)  # (the new indices)
        pc.removePoints(gone)
        k2 = np.ones(xs.shape[0], bool)
        k2[gone] = False
        assert pc.computeRGBD(cal, E, color, depth) == 1
        r = orc.project(xs[k2], cs[k2], P, W, H)
        assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(color, r["img"])
        ids = pc.computePointIds(cal, E)
        assert ids.max() < k2.sum()
    finally:
        pc.projector.close()


def test_remove_whole_chunk_tail_of_packed_cloud_sizes(pkg, orc):
    """Only whole trailing chunks removed (undoing an append onto a multiple of 256 points, the last partial chunk of a
    ragged cloud): nothing is rebuilt, and the packed form holds exactly the one-shot's units -- then keeps working for
    a later append."""
    W, H = 320, 240
    for nA, m, config in ((256 * 3907, 100_000, {}), (256 * 400, 50_001, {"pack": 2}), (256 * 401, 300, {"keep_soa": 1})):
        n = nA + m
        xyzw, rgba = orc.generate("room_shell", 0x7A11 + m, 0, n, n)
        a, b = _new(pkg, config, W, H), _new(pkg, config, W, H)
        try:
            a.upload_points(xyzw[:nA], rgba[:nA])
            a.append_points(xyzw[nA:], rgba[nA:])
            a.remove_points(np.arange(n) < nA)  # (the last append, undone)
            b.upload_points(xyzw[:nA], rgba[:nA])
            assert a.get_option("packed") == b.get_option("packed") == 1
            assert a.get_option("packed_millibytes_per_point") == b.get_option("packed_millibytes_per_point")
            P = pkg.orbit_projection(nA % 113, W, H)
            _check(pkg, orc, a, b, xyzw[:nA], rgba[:nA], P, True, ("tail", nA, m))
            ma, mb = a.get_option("resident_millibytes_per_point"), b.get_option("resident_millibytes_per_point")
            assert ma <= 1.25 * mb, (ma, mb)
            # the last partial chunk of a ragged cloud, then an append behind what is left
            k2 = np.arange(nA) < nA - 100
            a.remove_points(k2)
            assert a.num_points == nA - 100
            a.append_points(xyzw[nA:], rgba[nA:])
            sel = np.concatenate([k2, np.ones(m, bool)])
            b.upload_points(xyzw[sel], rgba[sel])
            assert a.get_option("packed_millibytes_per_point") == b.get_option("packed_millibytes_per_point")
            _check(pkg, orc, a, b, xyzw[sel], rgba[sel], P, True, ("tail + append", nA, m))
        finally:
            a.close(); b.close()


def test_remove_fed_back_from_visibility_device_buffer(pkg, orc):
    L = pkg._lib
    n, W, H = 200_000, 320, 240
    xyzw, rgba = orc.generate("uniform_box", 15, 0, n, n)
    p = _new(pkg, {"point_ids": 1}, W, H)
    try:
        p.upload_points(xyzw, rgba)
        PA, PB = pkg.orbit_projection(100, W, H), pkg.orbit_projection(180, W, H)
        p.render(PA)
        p.point_pass(PA, ids=False, visible=True)
        words = p.download(L.BUF_VISIBLE)
        vis = np.unpackbits(words.astype("<u4").view(np.uint8), bitorder="little")[:n].astype(bool)
        assert 0 < vis.sum() < n
        p.remove_points(p.device_buffer(L.BUF_VISIBLE))  # device memory, straight back
        assert p.num_points == int(vis.sum())
        _check(pkg, orc, p, None, xyzw[vis], rgba[vis], PB, True, "feedback")
        _check(pkg, orc, p, None, xyzw[vis], rgba[vis], PA, False, "feedback, same pose")
        import torch  # a torch tensor holding the words works the same
        k2 = np.arange(p.num_points) % 5 != 0
        p.remove_points(torch.as_tensor(_words(k2).view(np.int32), device="cuda"))
        _check(pkg, orc, p, None, xyzw[vis][k2], rgba[vis][k2], PB, False, "torch")
    finally:
        p.close()


def test_remove_sequences(pkg, orc):
    W, H = 320, 240
    for scene in ("room_shell", "uniform_box"):
        n, nA = 180_000, 110_000
        xyzw, rgba = orc.generate(scene, 61, 0, n, n)
        rng = np.random.default_rng(61)
        k1 = rng.random(nA) >= 0.2
        k1[nA - 3000:] = False  # (and a tail)
        p = _new(pkg, {"point_ids": 1}, W, H)
        try:
            p.upload_points(xyzw[:nA], rgba[:nA])
            p.remove_points(k1)
            p.append_points(xyzw[nA:], rgba[nA:])
            cx = np.concatenate([xyzw[:nA][k1], xyzw[nA:]])
            cc = np.concatenate([rgba[:nA][k1], rgba[nA:]])
            k2 = rng.random(cx.shape[0]) >= 0.5
            k2[-20_000:] = False  # (part of the appended block as well)
            p.remove_points(k2)
            b = _new(pkg, {"point_ids": 1}, W, H)
            b.upload_points(cx[k2], cc[k2])
            try:
                for k, filt in enumerate((False, True)):
                    _check(pkg, orc, p, b, cx[k2], cc[k2], pkg.orbit_projection(5 + 40 * k, W, H), filt, (scene, "seq"))
                P = pkg.orbit_projection(77, W, H)
                for q in (p, b):
                    q.render(P)
                    q.point_pass(P)
                assert np.array_equal(p.download(pkg._lib.BUF_POINT_ID), b.download(pkg._lib.BUF_POINT_ID))
            finally:
                b.close()
        finally:
            p.close()
    # after rtr_generate_synthetic
    n = 300_000
    xyzw, rgba = orc.generate("room_shell", 0x5EED, 0, n, n)
    keep = np.random.default_rng(1).random(n) >= 0.1
    p = _new(pkg, {}, W, H)
    try:
        p.generate_synthetic("room_shell", 0x5EED, 0, n, n)
        p.remove_points(keep)
        _check(pkg, orc, p, None, xyzw[keep], rgba[keep], pkg.orbit_projection(19, W, H), True, "synthetic")
    finally:
        p.close()


def test_remove_clip_views_phases(pkg, orc):
    L = pkg._lib
    W, H = 320, 240
    n = 150_000
    xyzw, rgba = orc.generate("room_shell", 29, 0, n, n)
    keep = np.random.default_rng(29).random(n) >= 0.35
    a, b = _pair(pkg, {}, xyzw, rgba, keep, W, H)
    xs, cs = xyzw[keep], rgba[keep]
    try:
        planes = np.array([[1.0, 0.0, 0.0, 0.5], [0.0, -1.0, 0.2, 1.0]], np.float32)
        for p in (a, b):
            p.set_clip_planes(planes)
        x, y, z = (xs[:, k].astype(np.float32) for k in range(3))
        inside = np.ones(xs.shape[0], bool)
        for a_, b_, c_, d_ in planes:  # (float32, in the header's order)
            inside &= ((a_ * x + b_ * y) + c_ * z) + d_ >= np.float32(0)
        _check(pkg, orc, a, b, xs[inside], cs[inside], pkg.orbit_projection(44, W, H), True, "clip")
        for p in (a, b):
            p.set_clip_planes(None)
        Ps = np.stack([pkg.orbit_projection(9 * k, W, H) for k in range(3)])
        for p in (a, b):
            p.render_views(Ps, with_filter=True)
        for which in (L.BUF_VIEW_DEPTH, L.BUF_VIEW_IMAGE, L.BUF_VIEW_TENSOR, L.BUF_VIEW_MINMAX):
            assert np.array_equal(a.download(which), b.download(which)), which
        r = orc.project(xs, cs, Ps[1], W, H)
        rf = orc.filter(r["depth_bits"], r["img"])
        assert np.array_equal(a.download(L.BUF_VIEW_DEPTH)[1], rf["depth"].view(np.uint32))
        P = pkg.orbit_projection(61, W, H)
        for p in (a, b):
            p.clear(); p.min_depth_pass(P); p.accumulate_pass(P); p.resolve()
        r = orc.project(xs, cs, P, W, H)
        for which in (L.BUF_DEPTH, L.BUF_ACCUM, L.BUF_IMAGE):
            assert np.array_equal(a.download(which), b.download(which)), which
        assert np.array_equal(a.download(L.BUF_DEPTH), r["depth_bits"])
        for p in (a, b):
            p.project(P)
        sa, sb = a.frame_stats(), b.frame_stats()
        assert (sa["entries"], sa["heaviest_tile"]) == (sb["entries"], sb["heaviest_tile"])
    finally:
        a.close(); b.close()


def test_remove_async_slot_keeps_old_frame(pkg, orc):
    W, H = 320, 240
    n = 150_000
    xyzw, rgba = orc.generate("room_shell", 31, 0, n, n)
    keep = np.arange(n) < 60_000
    p = _new(pkg, {}, W, H)
    try:
        p.upload_points(xyzw, rgba)
        P = pkg.orbit_projection(12, W, H)
        p.project_async(P, 0)
        p.remove_points(keep)
        p.wait_outputs(0)
        img, depth = p.host_output_buffers(0)
        r = orc.project(xyzw, rgba, P, W, H)
        assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(img, r["img"])
        _check(pkg, orc, p, None, xyzw[keep], rgba[keep], P, False, "after")
    finally:
        p.close()


def test_remove_first_frame_overflows_adaptive_pool_and_repairs(pkg, orc):
    xyzw, rgba = sc.cloud(orc)
    junk, jc = orc.generate("uniform_box", 5, 0, sc.N, sc.N)
    ax, ac = np.concatenate([xyzw, junk]), np.concatenate([rgba, jc])
    keep = np.arange(ax.shape[0]) < sc.N
    P = sc.p_one(orc)[0]
    p = _new(pkg, {"auto_reorder": 0}, sc.W, sc.H)
    try:
        p.upload_points(ax, ac)
        p.project(pkg.orbit_projection(0, sc.W, sc.H))  # (an ordinary frame sizes the pool for the big cloud)
        p.remove_points(keep)
        mb0 = p.get_option("resident_millibytes_per_point")
        p.render(P)  # (~2 n entries into a pool of max(n / 2, 2^20) sized afresh for the survivors: it overflows)
        p.synchronize()
        assert p.get_option("resident_millibytes_per_point") - mb0 >= sc.JUMP_MB
        r = orc.project(xyzw, rgba, P, sc.W, sc.H)
        assert np.array_equal(p.download(pkg._lib.BUF_DEPTH), r["depth_bits"])
        assert np.array_equal(p.download(pkg._lib.BUF_IMAGE), r["img"])
    finally:
        p.close()


def test_remove_errors_change_nothing(pkg, orc):
    L = pkg._lib
    W, H = 160, 128
    n = 50_000
    xyzw, rgba = orc.generate("room_shell", 37, 0, n, n)
    e = pkg.Projector(0)
    try:  # no cloud
        w = np.ones(1, np.uint32)
        assert e._lib.rtr_remove_points(e._ctx, C.c_void_p(w.ctypes.data), 1) == L.RTR_ERR_INVALID
        assert e._lib.rtr_remove_points(e._ctx, C.c_void_p(w.ctypes.data), 0) == L.RTR_ERR_INVALID
    finally:
        e.close()
    p = _new(pkg, {"point_ids": 1}, W, H)
    try:
        p.upload_points(xyzw, rgba)
        p.set_point_keep(np.arange(n) % 3 != 0)
        P = pkg.orbit_projection(8, W, H)
        img0, depth0 = p.project(P)
        keep0 = p.download(L.BUF_POINT_KEEP)
        words = _words(np.arange(n) % 2 == 0)
        vp = C.c_void_p(words.ctypes.data)
        lib = p._lib
        for args in ((vp, words.size - 1), (vp, words.size + 1), (vp, 0), (None, words.size)):
            assert lib.rtr_remove_points(p._ctx, *args) == L.RTR_ERR_INVALID, args
            assert p.num_points == n
        with pytest.raises(ValueError):
            p.remove_points(None)
        img1, depth1 = p.project(P)
        assert np.array_equal(depth0.view(np.uint32), depth1.view(np.uint32)) and np.array_equal(img0, img1)
        assert np.array_equal(p.download(L.BUF_POINT_KEEP), keep0)
    finally:
        p.close()
    # a cloud the library sorted without point_ids: upload indices cannot be mapped
    xu, cu = orc.generate("uniform_box", 37, 0, 70_000, 70_000)
    p = _new(pkg, {}, W, H)
    try:
        p.upload_points(xu, cu)
        assert p.get_option("reordered") == 1
        img0, depth0 = p.project(P)
        with pytest.raises(pkg.RtrError) as err:
            p.remove_points(np.arange(70_000) % 2 == 0)
        assert err.value.code == L.RTR_ERR_INVALID and "point_ids" in str(err.value)
        assert p.num_points == 70_000
        img1, depth1 = p.project(P)
        assert np.array_equal(depth0.view(np.uint32), depth1.view(np.uint32)) and np.array_equal(img0, img1)
    finally:
        p.close()


def test_remove_downloads(pkg, orc):
    n = 140_000
    xyzw, rgba = orc.generate("uniform_box", 41, 0, n, n)
    keep = np.random.default_rng(41).random(n) >= 0.3
    for options in ({"auto_reorder": 0}, {"point_ids": 1}):
        p = _new(pkg, options, 64, 48)
        try:
            p.upload_points(xyzw, rgba)
            p.remove_points(keep)
            gx, gc = p.download_points()
            want = np.concatenate([xyzw[keep][:, :3].view(np.uint32), rgba[keep].view(np.uint32)], axis=1)
            got = np.concatenate([gx[:, :3].view(np.uint32), gc.view(np.uint32)], axis=1)
            if "auto_reorder" in options:
                assert np.array_equal(got, want)  # exactly A[keep]
            else:
                key = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
                assert np.array_equal(key(got), key(want))
        finally:
            p.close()


def test_remove_closes_p2p(pkg, orc):
    n = 60_000
    xyzw, rgba = orc.generate("room_shell", 43, 0, n, n)
    p = _new(pkg, {}, 160, 128)
    try:
        p.upload_points(xyzw, rgba)
        p.p2p_open(0, 1, [p.p2p_export()])
        assert p.get_option("p2p_open") == 1
        p.remove_points(np.arange(n) < 40_000)
        assert p.get_option("p2p_open") == 0
        p.p2p_open(0, 1, [p.p2p_export()])  # (every rank exports and opens again)
        assert p.get_option("p2p_open") == 1
    finally:
        p.close()


def test_remove_memory_bound(pkg, orc):
    n, W, H = 10_000_000, 640, 480
    xyzw, rgba = orc.generate("room_shell", 47, 0, n, n)
    keep = np.random.default_rng(47).random(n) >= 0.5
    a, b = _pair(pkg, {}, xyzw, rgba, keep, W, H)
    try:
        P = pkg.orbit_projection(3, W, H)
        a.project(P)
        b.project(P)
        ma, mb = a.get_option("resident_millibytes_per_point"), b.get_option("resident_millibytes_per_point")
        assert ma <= 1.25 * mb, (ma, mb)
    finally:
        a.close(); b.close()


def test_remove_c3_random_tenth_full_size(pkg, orc):
    N, W, H = 100_000_000, 1920, 1080
    p = pkg.Projector(0)
    try:
        p.set_option("auto_reorder", 0)  # (resident order = upload order: download_points gives the indices)
        p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
        p.set_resolution(W, H)
        keep = np.random.default_rng(51).random(N) >= 0.1
        p.remove_points(keep)
        assert p.num_points == int(keep.sum())
        P = pkg.orbit_projection(17, W, H)
        img, depth = p.project(P, filtered=True)
        xs, rs = p.download_points()
        xyzw, rgba = orc.generate("room_shell", 0xC0FFEE03, 0, N, N)
        assert np.array_equal(xs.view(np.uint32), xyzw[keep].view(np.uint32)) and np.array_equal(rs, rgba[keep])
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
