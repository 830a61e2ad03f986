"""Reading resident points back out on the GPU (include/rtr.h section 2e): rtr_extract_points against numpy --
xyzw[sel][first:first + count], rgba[sel][...], flatnonzero(sel)[...] -- compared with np.array_equal on the uint32 views
of the floats, in every form the cloud can take; ragged counts and special bit patterns; the multi-window path; device
selections into device tensors; the cloud after appends, removals and moves; what an extraction must leave alone; the
sorted cloud without point_ids; the error paths."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_select import FORMS, M_RIGID, _moved, _new, _octant, _specials

pytestmark = pytest.mark.gpu

CLOUDS = (("room_shell", 70_001), ("uniform_box", 70_003))  # just above the 65536 at which the library sorts by itself


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _words(sel, garbage=False):
    n = sel.size
    nwords = (n + 31) // 32
    w = np.packbits(np.concatenate([sel, np.zeros(32 * nwords - n, bool)]), bitorder="little").view("<u4").copy()
    if garbage and n % 32:
        w[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    return w


def _selections(pkg, xyzw, seed):
    n = xyzw.shape[0]
    lo, hi = _octant(xyzw)
    return {"random30": np.random.default_rng(seed).random(n) < 0.3,
            "octant": pkg.clip_keep(pkg.clip_box_planes(lo, hi), xyzw),
            "empty": np.zeros(n, bool), "full": np.ones(n, bool), "none": None}


def _check_streams(p, select, xyzw, rgba, want, what, first=0, count=None):
    """All three streams at strides 16 / 4, 12 / 3 and 32 / 8 (pre-filled: the bytes behind a record stay)."""
    idx = np.flatnonzero(want)[first:None if count is None else first + count]
    k = idx.size
    x, c, i = p.extract_points(select, first, count, indices=True)
    assert x.shape == (k, 4) and c.shape == (k, 4) and i.shape == (k,), what
    assert np.array_equal(i, idx.astype(np.uint32)), what
    assert np.array_equal(_bits(x[:, :3]), _bits(xyzw[idx, :3])) and np.array_equal(c[:, :3], rgba[idx, :3]), what
    assert np.array_equal(_bits(x[:, 3]), _bits(np.ones(k, np.float32))) and (c[:, 3] == 255).all(), what
    out = {"xyz": np.full((k, 3), 7.0, np.float32), "rgb": np.full((k, 3), 7, np.uint8), "indices": np.full(k, 7, np.uint32)}
    assert p.extract_points(select, first, count, out=out) == k, what
    assert np.array_equal(_bits(out["xyz"]), _bits(xyzw[idx, :3])) and np.array_equal(out["rgb"], rgba[idx, :3]), what
    assert np.array_equal(out["indices"], idx.astype(np.uint32)), what
    wide = {"xyz": np.full((k, 8), 7.0, np.float32), "rgb": np.full((k, 8), 7, np.uint8)}
    assert p.extract_points(select, first, count, out=wide) == k, what
    assert np.array_equal(_bits(wide["xyz"][:, :3]), _bits(xyzw[idx, :3])) and (wide["xyz"][:, 3:] == 7.0).all(), what
    assert np.array_equal(wide["rgb"][:, :3], rgba[idx, :3]) and (wide["rgb"][:, 3:] == 7).all(), what


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_form_matches_numpy(pkg, orc, form):
    options, sort = FORMS[form]
    for scene, n in CLOUDS:
        xyzw, rgba = orc.generate(scene, 41, 0, n, n)
        opts = dict(options)
        if scene == "uniform_box" and form != "hash_unpacked":
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            if form == "hash_unpacked" and scene == "uniform_box":
                assert p.get_option("reordered") == 0 and p.get_option("packed") == 0
            if form == "sorted" or (scene == "uniform_box" and form != "hash_unpacked"):
                assert p.get_option("reordered") == 1
            packed, mb = p.get_option("packed"), p.get_option("resident_millibytes_per_point")
            for name, sel in _selections(pkg, xyzw, 5).items():
                want = np.ones(n, bool) if sel is None else sel
                _check_streams(p, sel, xyzw, rgba, want, (form, scene, name))
                assert p.count_selected(sel) == int(want.sum())
            assert (p.get_option("packed"), p.get_option("resident_millibytes_per_point")) == (packed, mb)
        finally:
            p.close()


def test_small_and_edge_counts_with_special_bit_patterns(pkg):
    rng = np.random.default_rng(3)
    sp = _specials()
    for n in (1, 3, 4, 255, 256, 257, 1025):
        xyzw = np.concatenate([rng.choice(sp, (n, 3)), np.ones((n, 1), np.float32)], axis=1).astype(np.float32)
        nanbits = rng.integers(0x7F800001, 0x7FFFFFFF, n // 3 + 1, dtype=np.uint32)  # (NaN payloads round-trip too)
        xyzw[::3, 0] = nanbits.view(np.float32)[:xyzw[::3].shape[0]]
        rgba = rng.integers(0, 256, (n, 4), dtype=np.uint8)
        rgba[:, 3] = 255
        last = np.zeros(n, bool)
        last[-1] = True
        rnd = rng.random(n) < 0.5
        for options, sort in (({"auto_reorder": 0}, False), ({"auto_reorder": 0, "pack": 2}, False),
                              ({"auto_reorder": 0, "pack": 0}, False), ({"point_ids": 1}, True)):
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                for name, sel, arg in (("last", last, last), ("garbage", rnd, _words(rnd, garbage=True)),
                                       ("garbage_last", last, _words(last, garbage=True)), ("full", np.ones(n, bool), np.ones(n, bool)),
                                       ("none", np.ones(n, bool), None)):
                    _check_streams(p, arg, xyzw, rgba, sel, (n, options, name))
            finally:
                p.close()


@pytest.mark.parametrize("form", ["default", "pack0", "sorted"])
def test_windows(pkg, orc, form):
    options, sort = FORMS[form]
    for scene, n in CLOUDS:
        xyzw, rgba = orc.generate(scene, 43, 0, n, n)
        opts = dict(options)
        if scene == "uniform_box":
            opts["point_ids"] = 1
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            sels = _selections(pkg, xyzw, 9)
            one = {name: p.extract_points(sels[name], indices=True) for name in ("random30", "none")}
            p.set_option("debug_extract_window", 4096)
            assert p.get_option("debug_extract_window") == 4096
            for name in ("random30", "none"):
                sel = sels[name]
                want = np.ones(n, bool) if sel is None else sel
                k = int(want.sum())
                many = p.extract_points(sel, indices=True)  # (five to eighteen windows)
                for a, b in zip(one[name], many):
                    assert np.array_equal(_bits(a), _bits(b)), (form, scene, name)
                _check_streams(p, sel, xyzw, rgba, want, (form, scene, name, "windows"))
                for first, count in ((0, 4096), (4096, 4096), (4095, 2), (4000, 200), (32, 32), (31, 2), (256, 256), (255, 258),
                                     (8192 - 256, 512), (1, 3 * 4096 + 1), (k - 1, 1), (k - 5, 100), (12_288, None)):
                    _check_streams(p, sel, xyzw, rgba, want, (form, scene, name, first, count), first, count)
                # count = 0 gives only the total; first >= k writes nothing
                assert p.count_selected(sel) == k
                for first, count in ((0, 0), (k, 10), (k + 7, None)):
                    out = {"xyz": np.full((4, 4), 7.0, np.float32), "rgb": np.full((4, 4), 7, np.uint8), "indices": np.full(4, 7, np.uint32)}
                    assert p.extract_points(sel, first, count, out=out) == 0
                    assert (out["xyz"] == 7.0).all() and (out["rgb"] == 7).all() and (out["indices"] == 7).all()
                    tot = C.c_uint64(99)
                    words = None if sel is None else _words(sel)
                    rc = p._lib.rtr_extract_points(p._ctx, None if sel is None else words.ctypes.data_as(C.c_void_p), 0 if sel is None else words.size,
                                                   first, (1 << 40) if count is None else count, out["xyz"].ctypes.data_as(C.c_void_p), 16,
                                                   out["rgb"].ctypes.data_as(C.c_void_p), 4, out["indices"].ctypes.data_as(C.c_void_p), C.byref(tot))
                    assert rc == 0 and tot.value == k
                    assert (out["xyz"] == 7.0).all() and (out["rgb"] == 7).all() and (out["indices"] == 7).all()
            p.set_option("debug_extract_window", -1)
        finally:
            p.close()


@pytest.mark.parametrize("form", ["default", "sorted"])
def test_device_selection_into_device_tensors(pkg, orc, form):
    import torch
    L = pkg._lib
    options, sort = FORMS[form]
    n = 70_001
    xyzw, rgba = orc.generate("room_shell", 47, 0, n, n)
    lo, hi = _octant(xyzw)
    planes = pkg.clip_box_planes(lo, hi)
    want = pkg.clip_keep(planes, xyzw)
    k = int(want.sum())
    p = _new(pkg, options, xyzw, rgba, sort=sort)
    try:
        assert p.select_points(planes=planes)[0] == k
        before = p.download(L.BUF_SELECTION).copy()
        host = p.extract_points(p.selection(), indices=True)
        dev = {"xyz": torch.zeros((k, 4), dtype=torch.float32, device="cuda"), "rgb": torch.zeros((k, 4), dtype=torch.uint8, device="cuda"),
               "indices": torch.zeros(k, dtype=torch.int32, device="cuda")}
        torch.cuda.synchronize()
        for window in (-1, 4096):
            p.set_option("debug_extract_window", window)
            assert p.extract_points(p.selection(), out=dev) == k
            got = [dev["xyz"].cpu().numpy(), dev["rgb"].cpu().numpy(), dev["indices"].cpu().numpy().view(np.uint32)]
            for a, b in zip(host, got):
                assert np.array_equal(_bits(a), _bits(b)), (form, window)
            for t in dev.values():
                t.zero_()
            torch.cuda.synchronize()
        p.set_option("debug_extract_window", -1)
        # tight device records, host indices: every stream goes its own way
        mixed = {"xyz": torch.zeros((k, 3), dtype=torch.float32, device="cuda"), "rgb": np.zeros((k, 3), np.uint8),
                 "indices": torch.zeros(k, dtype=torch.int32, device="cuda")}
        torch.cuda.synchronize()
        assert p.extract_points(p.selection(), out=mixed) == k
        assert np.array_equal(_bits(mixed["xyz"].cpu().numpy()), _bits(xyzw[want, :3])) and np.array_equal(mixed["rgb"], rgba[want, :3])
        assert np.array_equal(mixed["indices"].cpu().numpy().view(np.uint32), np.flatnonzero(want).astype(np.uint32))
        assert np.array_equal(host[2], np.flatnonzero(want).astype(np.uint32))
        assert p.get_option("selection") == 1 and np.array_equal(p.download(L.BUF_SELECTION), before)
    finally:
        p.close()


@pytest.mark.parametrize("form", ["default", "pack0", "sorted"])
def test_after_edits_the_cloud_comes_back_and_renders_the_same(pkg, orc, form):
    options, sort = FORMS[form]
    na, nb, W, H = 70_001, 5_003, 64, 48
    A = orc.generate("room_shell", 51, 0, na, na)
    B = orc.generate("uniform_box", 52, 0, nb, nb)
    rng = np.random.default_rng(8)
    pc = pkg.ProjectCloud(A[0], A[1], reorder=sort, point_ids=True)
    p = pc.projector
    for key, v in options.items():
        if key != "point_ids":
            p.set_option(key, v)
    if sort:
        p.reorder_points()
    pc.appendPoints(B[0], B[1])
    x = np.concatenate([A[0], B[0]])
    c = np.concatenate([A[1], B[1]])
    keep = rng.random(x.shape[0]) < 0.8
    keep[300:900] = False
    p.remove_points(keep)
    x, c = x[keep], c[keep]
    sel = rng.random(x.shape[0]) < 0.4
    p.transform_points(M_RIGID, sel)
    x = _moved(x, M_RIGID, sel)
    vx, vc = pc.extractAll()
    assert np.array_equal(_bits(vx), _bits(x)) and np.array_equal(vc[:, :3], c[:, :3])
    assert np.array_equal(p.extract_points(xyz=False, rgb=False, indices=True)[0], np.arange(x.shape[0], dtype=np.uint32))
    some = np.sort(rng.choice(x.shape[0], 500, replace=False))
    sx, sc = pc.extractPoints(some)
    assert np.array_equal(_bits(sx), _bits(x[some])) and np.array_equal(sc[:, :3], c[some, :3])
    cal = pkg.benchmark_calibration(W, H)
    fresh = pkg.ProjectCloud(vx, vc)
    for k in (5, 300):
        frames = []
        for cloud in (pc, fresh):
            color, depth = np.empty((H, W, 3), np.uint8), np.empty((H, W), np.float32)
            assert cloud.computeFilteredRGBD(cal, pkg.orbit_pose(k), color, depth) == 1
            frames.append((color, depth.view(np.uint32)))
        assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1]), (form, k)


def test_save_ply_round_trips(pkg, orc, tmp_path):
    n = 3_001
    xyzw, rgba = orc.generate("room_shell", 53, 0, n, n)
    pc = pkg.ProjectCloud(xyzw, rgba)
    lo, hi = _octant(xyzw)
    k = pc.selectBox(lo, hi)
    assert pc.savePly(str(tmp_path / "all.ply")) == n and pc.savePly(str(tmp_path / "sel.ply"), selected=True) == k
    xyz, bgr = pkg.formats.read_ply(str(tmp_path / "all.ply"))
    assert np.array_equal(_bits(xyz), _bits(xyzw[:, :3])) and np.array_equal(bgr, rgba[:, :3])
    xyz, bgr = pkg.formats.read_ply(str(tmp_path / "sel.ply"))
    box = pkg.clip_keep(pkg.clip_box_planes(lo, hi), xyzw)
    assert np.array_equal(_bits(xyz), _bits(xyzw[box, :3])) and np.array_equal(bgr, rgba[box, :3])
    vx, vc, vi = pc.extractSelected(indices=True)
    assert np.array_equal(vi, np.flatnonzero(box).astype(np.uint32)) and np.array_equal(_bits(vx), _bits(xyzw[box]))


def test_an_extraction_moves_nothing_else(pkg, orc):
    L = pkg._lib
    n, W, H = 70_001, 64, 48
    xyzw, rgba = orc.generate("room_shell", 57, 0, n, n)
    P = pkg.orbit_projection(40, W, H)
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        assert p.get_option("packed") == 1
        hidden = np.arange(n) % 3 == 0
        planes = np.float32([[1, 0, 0, 0.5]])
        p.set_point_keep(~hidden)
        p.set_clip_planes(planes)
        clipped = ~pkg.clip_keep(planes, xyzw)
        assert clipped.any() and not clipped.all()

        def state():
            p.project(P, filtered=True)
            return [p.download(b).copy() for b in (L.BUF_DEPTH, L.BUF_IMAGE)] + \
                   [p.frame_stats(), p.point_keep(), p.clip_planes(), p.get_option("packed"), p.get_option("resident_millibytes_per_point")]

        def same(a, b):
            return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

        before = state()
        sel = hidden | clipped  # (points the mask or the planes hide are extracted like the others)
        _check_streams(p, sel, xyzw, rgba, sel, "hidden and clipped")
        _check_streams(p, None, xyzw, rgba, np.ones(n, bool), "everything")
        mid = [p.download(b).copy() for b in (L.BUF_DEPTH, L.BUF_IMAGE)] + [p.frame_stats()]
        assert same(before[:3], mid)  # (the frame, its buffers and its statistics words as they were)
        after = state()  # (... and the next render gives the same frame under the same mask and planes)
        assert same(before[:2] + before[3:], after[:2] + after[3:])
    finally:
        p.close()


def test_sorted_without_point_ids(pkg, orc):
    L = pkg._lib
    n = 70_001
    xyzw, rgba = orc.generate("room_shell", 59, 0, n, n)
    p = _new(pkg, {}, xyzw, rgba, sort=True)
    try:
        assert p.get_option("reordered") == 1 and p.get_option("point_ids") == 0
        with pytest.raises(pkg.RtrError) as e:
            p.extract_points(np.arange(n) % 2 == 0)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        with pytest.raises(pkg.RtrError) as e:
            p.extract_points(indices=True)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
        dx, dc = p.download_points()
        for window in (-1, 4096):
            p.set_option("debug_extract_window", window)
            x, c = p.extract_points()
            assert np.array_equal(_bits(x), _bits(dx)) and np.array_equal(c, dc)
            x, c = p.extract_points(first=1000, count=5000)
            assert np.array_equal(_bits(x), _bits(dx[1000:6000])) and np.array_equal(c, dc[1000:6000])
        assert not np.array_equal(_bits(dx), _bits(xyzw))  # (the resident order is not the upload order)
    finally:
        p.close()


def test_errors_write_nothing(pkg, orc):
    L = pkg._lib
    n = 5_001
    xyzw, rgba = orc.generate("room_shell", 61, 0, n, n)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    x, c, i = np.full((n, 4), 7.0, np.float32), np.full((n, 4), 7, np.uint8), np.full(n, 7, np.uint32)
    tot = C.c_uint64(99)
    words = _words(np.arange(n) % 2 == 0)

    def untouched():
        return (x == 7.0).all() and (c == 7).all() and (i == 7).all() and tot.value == 99

    fresh = pkg.Projector(0)
    try:  # no cloud
        assert fresh._lib.rtr_extract_points(fresh._ctx, None, 0, 0, n, vp(x), 16, vp(c), 4, vp(i), C.byref(tot)) == L.RTR_ERR_INVALID
        assert untouched()
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        lib, ctx = p._lib, p._ctx
        bad = [(vp(words), words.size - 1, vp(x), 16, vp(c), 4, vp(i), C.byref(tot)),   # nwords != (n + 31) / 32
               (vp(words), words.size + 1, vp(x), 16, vp(c), 4, vp(i), C.byref(tot)),
               (vp(words), 0, vp(x), 16, vp(c), 4, vp(i), C.byref(tot)),
               (None, words.size, vp(x), 16, vp(c), 4, vp(i), C.byref(tot)),            # select_words NULL with nwords > 0
               (vp(words), words.size, vp(x), 8, vp(c), 4, vp(i), C.byref(tot)),        # bad strides
               (vp(words), words.size, vp(x), 14, vp(c), 4, vp(i), C.byref(tot)),
               (vp(words), words.size, vp(x), 16, vp(c), 2, vp(i), C.byref(tot)),
               (None, 0, vp(x), 0, None, 0, None, C.byref(tot)),
               (None, 0, None, 0, vp(c), 0, None, C.byref(tot)),
               (None, 0, None, 0, None, 0, None, None)]                                 # nothing to produce
        for case in bad:
            assert lib.rtr_extract_points(ctx, case[0], case[1], 0, n, *case[2:]) == L.RTR_ERR_INVALID, case
            assert untouched(), case
        # a bad stride of a stream that is NULL does not matter
        assert lib.rtr_extract_points(ctx, vp(words), words.size, 0, n, None, 1, None, 0, vp(i), C.byref(tot)) == 0
        assert tot.value == (n + 1) // 2 and np.array_equal(i[:tot.value], np.arange(0, n, 2, dtype=np.uint32)) and (i[tot.value:] == 7).all()
    finally:
        p.close()
