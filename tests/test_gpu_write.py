"""Writing points back on the GPU (include/rtr.h section 2f): rtr_upload_points(A) then rtr_write_points(sel, first,
count, X, C) leaves, bit for bit, the cloud the host statement write_ref.written gives, in every form the cloud can
take.  After each write: (i) the extraction of every point with indices equals the statement (coordinates as uint32,
colours), (ii) the unfiltered and the filtered frame and the point pass equal a second context that uploads the written
cloud once AND the oracle, (iii) the point count, the keep words, the selection words and the `packed` read-back are what
they were.  Everything at 160 x 128 on clouds of 1 .. 8229 points (the chunk edges); the clouds, writes and poses are
write_cases.py's, which test_write_host.py walks without a GPU."""
import ctypes as C

import numpy as np
import pytest

import edit_model as em
import helpers
import point_pass_ref as ppr
import pool_overflow_scenes as sc
import write_cases as wc
import write_model as wm
import write_ref
from test_gpu_transform import CONFIGS
from transform_ref import TRANSFORMS

pytestmark = pytest.mark.gpu

W, H = wc.W, wc.H
XCOLS, CCOLS = (3, 4, 7), (3, 4, 7)  # row widths: strides 12 / 16 / 28 and 3 / 4 / 7


def _options(config):
    o = dict(CONFIGS[config])
    if config == "auto_reorder1":  # (small clouds are sorted only on request; indices then need the permutation)
        o["point_ids"] = 1
    return o


def _new(pkg, options):
    p = pkg.Projector(0)
    for k, v in options.items():
        p.set_option(k, v)
    p.set_resolution(W, H)
    return p


def _rows(arr, cols, device):
    """The caller's array of a stream: rows of `cols` columns (the first three are the record), host or device."""
    if arr is None or arr.ndim == 1:
        return arr
    wide = np.full((arr.shape[0], cols), 77, arr.dtype)
    wide[:, :3] = arr
    if not device:
        return wide
    import torch
    return torch.from_numpy(wide).to(torch.device("cuda", 0))


class Pair:
    """Context `a` takes the writes, context `b` one upload of the model's cloud; `model` is the host statement."""

    def __init__(self, pkg, orc, options, b_options=None):
        self.pkg, self.orc, self.L = pkg, orc, pkg._lib
        self.a = _new(pkg, options)
        self.b = _new(pkg, options if b_options is None else b_options)
        self.model = wm.Model("pack2_ids")
        self.writes = 0

    def close(self):
        self.a.close(); self.b.close()

    def upload(self, xyz, rgb):
        self.a.upload_points(*helpers.cloud(xyz, rgb))
        self.model.upload(xyz, rgb)

    def _state(self):
        a, L = self.a, self.L
        return (a.num_points, a.get_option("packed"), a.get_option("reordered"),
                a.download(L.BUF_POINT_KEEP).tobytes() if a.get_option("point_keep") else None,
                a.download(L.BUF_SELECTION).tobytes() if a.get_option("selection") else None)

    def write(self, st, what, form=None, device=None, select=None):
        """One write of a write_cases step; the argument form, the sources and the strides rotate with the writes."""
        j = self.writes
        self.writes += 1
        sel = st["sel"]
        k = self.model.n if sel is None else int(sel.sum())
        arg = select if select is not None else (None if sel is None else (sel if (form or ("bool", "words")[j % 2]) == "bool" else em.words_of(sel)))
        dev_x, dev_c = ((j // 2) % 2 == 1, (j // 3) % 2 == 1) if device is None else device
        X, Cc = _rows(st["X"], XCOLS[j % 3], dev_x), _rows(st["C"], CCOLS[(j + 1) % 3], dev_c)
        before, mb0 = self._state(), self.a.get_option("packed_millibytes_per_point")
        one = st["C"] is not None and st["C"].ndim == 1
        got = self.a.write_points(X, Cc, arg, st["first"], broadcast=one)
        idx = self.model.write(sel, st["first"], st["X"], st["C"])
        assert got == idx.size, ("points written", got, idx.size, what)
        assert idx.size <= max(0, k - st["first"])
        assert self._state() == before, ("count / packed / keep / selection changed", what)  # (iii)
        if st["X"] is None:  # (a colour-only write touches no packed block)
            assert self.a.get_option("packed_millibytes_per_point") == mb0, ("packed size after colours", what)
        return idx

    def check_points(self, what):
        """(i)"""
        m = self.model
        xyz, rgb, idx = self.a.extract_points(indices=True)
        assert np.array_equal(idx, np.arange(m.n, dtype=np.uint32)), ("indices", what)
        assert np.array_equal(xyz[:, :3].view(np.uint32), m.xyz.view(np.uint32)), ("coordinates", what)
        assert np.array_equal(rgb[:, :3], m.rgb) and (rgb[:, 3] == 255).all(), ("colours", what)

    def check_frames(self, k, what, b_current=False):
        """(ii) at write_cases.pose(model, k)"""
        pkg, orc, L, m = self.pkg, self.orc, self.L, self.model
        if not b_current:
            self.b.upload_points(*helpers.cloud(m.xyz, m.rgb))
            if m.keep is not None:
                self.b.set_point_keep(m.keep)
        P = wc.pose(m, k)
        d = m.drawable()
        xyzw, rgba = helpers.cloud(m.xyz[d], m.rgb[d])
        r = orc.project(xyzw, rgba, P, W, H)
        f = orc.filter(r["depth_bits"], r["img"])
        for p, who in ((self.a, "written"), (self.b, "one upload")):
            img, depth = p.project(P)
            assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(img, r["img"]), ("frame", who, what)
            img, depth = p.project(P, filtered=True)
            assert np.array_equal(depth.view(np.uint32), f["depth"].view(np.uint32)), ("filtered depth", who, what)
            assert np.array_equal(img, f["img"]), ("filtered image", who, what)
            assert np.array_equal(p.download(L.BUF_TENSOR).reshape(5, H, W), f["tensor"]), ("tensor", who, what)
            assert np.array_equal(p.download(L.BUF_MINMAX), np.asarray(f["minmax"]).view(np.uint32).reshape(2)), ("minmax", who, what)
            p.point_pass(P)
            ids, vis = p.download(L.BUF_POINT_ID), p.download(L.BUF_VISIBLE)
            e_ids, e_vis = ppr.point_pass(orc, xyzw, P, W, H, f["depth"].view(np.uint32))
            none = e_ids == ppr.NO_POINT
            want = np.where(none, ppr.NO_POINT, d[np.where(none, 0, e_ids)] if d.size else ppr.NO_POINT)
            assert np.array_equal(ids, want.astype(np.uint32)), ("point ids", who, what)
            seen = np.zeros(m.n, bool)
            seen[d] = ppr.unpack(e_vis, d.size)
            assert np.array_equal(vis, em.words_of(seen)), ("visible", who, what)
            assert p.get_option("mode") == 0 or p.frame_stats()["errors"] == 0, ("frame_stats", who, what)


def _run_scenario(pr, name, n, what, frames="ends"):
    xyz, rgb, steps = wc.scenario(name, n)
    pr.upload(xyz, rgb)
    for j, st in enumerate(steps):
        pr.write(st, (what, name, j))
        pr.check_points((what, name, j))
        if frames == "all" or j in (0, 1, len(steps) - 1):
            pr.check_frames(j, (what, name, j))


@pytest.mark.parametrize("n", wc.COUNTS)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_write_selection_forms_windows_and_streams(pkg, orc, config, n):
    """Every selection shape x the six windows, the streams, strides, argument forms and host / device sources in turn;
    the special bit patterns; a selection written in three pieces; one broadcast colour."""
    pr = Pair(pkg, orc, _options(config))
    try:
        for name in wc.names(n):
            if name != "packed":
                _run_scenario(pr, name, n, (config, n))
        if config == "auto_reorder1" and n >= 2:
            assert pr.a.get_option("reordered") == 1
        if config == "pack2":
            assert pr.a.get_option("packed") == 1
    finally:
        pr.close()


@pytest.mark.parametrize("n", wc.BIG)
@pytest.mark.parametrize("config", ["default", "pack2", "pack0", "keep_soa1", "auto_reorder1", "cull", "overlap"])
def test_write_values_that_move_the_packed_form(pkg, orc, config, n):
    """Collapsed points (widths 0: the tail's blocks move down), wide mixed-sign values into the whole cloud (32-bit chunks
    with box words: the planes outgrow their capacity), collapsed again (they shrink by more than 1/8: reallocated),
    then a part 1000 x farther out (the lane test's absmax follows: a third context runs with lane_test = 0).  Where the
    resident order is the upload order the packed sizes equal those of one upload of the written cloud."""
    o = _options(config)
    if config not in ("default", "pack0"):
        o["pack"] = 2  # (always packed, and every rebuilt chunk decoded and compared)
    pr = Pair(pkg, orc, o)
    c = _new(pkg, dict(o, lane_test=0))
    L = pkg._lib
    try:
        xyz, rgb, steps = wc.scenario("packed", n)
        pr.upload(xyz, rgb)
        sizes = [pr.a.get_option("packed_millibytes_per_point")]
        for j, st in enumerate(steps):
            pr.write(st, (config, n, "packed", j))
            pr.check_points((config, n, "packed", j))
            pr.check_frames(j, (config, n, "packed", j))
            if o.get("pack") == 2 and not pr.a.get_option("reordered"):
                for key in ("packed", "packed_millibytes_per_point", "wide_chunks", "wide_chunks_boxed"):
                    assert pr.a.get_option(key) == pr.b.get_option(key), (config, n, j, key)
            sizes.append(pr.a.get_option("packed_millibytes_per_point"))
        if o.get("pack") == 2 and not pr.a.get_option("reordered"):  # (down, up again, down by more than 1/8)
            assert sizes[1] < sizes[0] and sizes[2] > sizes[1] and 8 * sizes[3] < 7 * sizes[2], sizes
        assert pr.a.get_option("lane_test") == 1 and c.get_option("lane_test") == 0
        m = pr.model
        c.upload_points(*helpers.cloud(m.xyz, m.rgb))
        P = wc.pose(m, len(steps) - 1)
        for filt in (False, True):
            ia, da = pr.a.project(P, filtered=filt)
            ic, dc = c.project(P, filtered=filt)
            assert np.array_equal(da.view(np.uint32), dc.view(np.uint32)) and np.array_equal(ia, ic), (config, n, "lane_test 0", filt)
    finally:
        pr.close(); c.close()


def test_write_takes_the_contexts_own_selection_and_keeps_it(pkg, orc):
    """The selection as the context's own RTR_BUF_SELECTION device pointer, as a torch tensor of words and as host
    words; the selection survives every write and names the same points."""
    import torch
    for options in ({"point_ids": 1}, {"auto_reorder": 1, "point_ids": 1}, {"pack": 0}):
        for n in (257, 4099):
            pr = Pair(pkg, orc, options)
            try:
                xyz, rgb = wc.cloud(n)
                pr.upload(xyz, rgb)
                planes = np.float32([[1, 0, 0, 0.5], [0, 0, -1, 2.0]])
                pr.a.select_points(planes=planes)
                pr.model.select(planes, "replace", False)
                sel = pr.model.selection.copy()
                k = int(sel.sum())
                assert 0 < k < n
                words = torch.from_numpy(em.words_of(sel).view(np.int32)).to(torch.device("cuda", 0))
                for j, (select, (first, count)) in enumerate(zip((pr.a.selection(), words, pr.a.selection(), em.words_of(sel)),
                                                                 ((0, k), (k // 3, k // 2), (1, 2), (0, k)))):
                    st = wc._step(sel, first, count, "box", ("both", "rgb", "xyz", "colour")[j], 40 + j)
                    pr.write(st, (options, n, j), select=select if j < 3 else None, form="words")
                    pr.check_points((options, n, j))
                    pr.check_frames(j, (options, n, j))
                    assert np.array_equal(pr.a.download(pkg._lib.BUF_SELECTION), em.words_of(sel))
            finally:
                pr.close()


def test_write_round_trips(pkg, orc):
    """extract(sel) then write(sel) of the same arrays changes nothing -- frames and packed sizes identical; and points
    extracted from context A into device buffers, written into context B that holds the same indices, make B's frames
    A's.  Also on a cloud the library sorted WITHOUT point_ids: extract-all, edit, write-all addresses the resident order."""
    import torch
    L = pkg._lib
    n = 8229
    xyz, rgb = wc.cloud(n)
    sel = wc.selection("random", n)
    for options in ({"pack": 2, "point_ids": 1}, {"pack": 0}, {"auto_reorder": 1, "point_ids": 1}, {"keep_soa": 1}):
        pr = Pair(pkg, orc, options)
        try:
            pr.upload(xyz, rgb)
            pr.a.transform_points(TRANSFORMS["rigid"], np.arange(n) % 5 == 0)
            pr.model.transform(TRANSFORMS["rigid"], np.arange(n) % 5 == 0)
            mb = pr.a.get_option("packed_millibytes_per_point")
            P = wc.pose(pr.model, 3)
            f0 = [x.copy() for x in pr.a.project(P, filtered=True)]
            gx, gc = pr.a.extract_points(sel)
            assert pr.a.write_points(gx, gc, sel) == int(sel.sum())
            assert pr.a.get_option("packed_millibytes_per_point") == mb
            f1 = pr.a.project(P, filtered=True)
            assert np.array_equal(f0[0], f1[0]) and np.array_equal(f0[1].view(np.uint32), f1[1].view(np.uint32)), options
            pr.check_points(options)
            # A -> device buffers -> B (b holds the start cloud: the same indices)
            k = int(sel.sum())
            dx = torch.empty((k, 4), dtype=torch.float32, device="cuda:0")
            dc = torch.empty((k, 4), dtype=torch.uint8, device="cuda:0")
            assert pr.a.extract_points(sel, out={"xyz": dx, "rgb": dc}) == k
            torch.cuda.synchronize()
            pr.b.upload_points(*helpers.cloud(xyz, rgb))
            rest = ~sel
            pr.b.write_points(dx, dc, sel)
            gx, gc = pr.a.extract_points(rest)
            pr.b.write_points(gx, gc, rest)
            pr.check_frames(5, (options, "A to B"), b_current=True)
        finally:
            pr.close()
    # sorted without point_ids: a selection is refused, "every point" is the resident order
    p = _new(pkg, {"auto_reorder": 1, "point_ids": 0})
    try:
        p.upload_points(*helpers.cloud(xyz, rgb))
        assert p.get_option("reordered") == 1 and p.get_option("packed_millibytes_per_point") >= 0
        with pytest.raises(pkg.RtrError) as err:
            p.write_points(xyz[:5], None, np.arange(n) < 5)
        assert err.value.code == L.RTR_ERR_INVALID and "point_ids" in str(err.value)
        gx, gc = p.extract_points()
        edited = gx[:, :3] + np.float32([0.5, 0.0, -0.25])
        assert p.write_points(edited, 255 - gc[:, :3]) == n
        hx, hc = p.extract_points()
        assert np.array_equal(hx[:, :3].view(np.uint32), edited.view(np.uint32)) and np.array_equal(hc[:, :3], 255 - gc[:, :3])
        m = wm.Model("pack2_ids")
        m.upload(edited, 255 - gc[:, :3])
        P = wc.pose(m, 1)
        r = orc.project(*helpers.cloud(m.xyz, m.rgb), P, W, H)
        img, depth = p.project(P)
        assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(img, r["img"])
        # a window of the resident order
        assert p.write_points(edited[100:400] * np.float32(0.5), None, None, first=100) == 300
        hx2, _ = p.extract_points()
        want = edited.copy()
        want[100:400] *= np.float32(0.5)
        assert np.array_equal(hx2[:, :3].view(np.uint32), want.view(np.uint32))
    finally:
        p.close()


def test_write_under_a_keep_mask_and_clip_planes(pkg, orc):
    """A hidden point that is written stays hidden and shows its new values once un-hidden; clip planes are world-space
    and act on the written coordinates."""
    n = 4099
    xyz, rgb = wc.cloud(n)
    for options in ({"point_ids": 1}, {"pack": 0}, {"auto_reorder": 1, "point_ids": 1}):
        pr = Pair(pkg, orc, options)
        try:
            pr.upload(xyz, rgb)
            keep = np.random.default_rng(8).random(n) >= 0.4
            pr.a.set_point_keep(keep)
            pr.model.set_keep(keep)
            sel = wc.selection("every_other_chunk", n)
            st = wc._step(sel, 0, int(sel.sum()), "box", "both", 21)
            idx = pr.write(st, (options, "masked"))
            assert (~keep[idx]).any() and keep[idx].any()  # (hidden and shown points were written)
            pr.check_points((options, "masked"))
            pr.check_frames(0, (options, "masked"))
            pr.a.set_point_keep(None)
            pr.model.clear_keep()
            pr.check_frames(1, (options, "un-hidden"))
            planes = np.float32([[1, 0, 0, -3.0], [0, -1, 0, 1.5]])  # (x >= 3: inside the written box, outside the start cloud's)
            for p in (pr.a, pr.b):
                p.set_clip_planes(planes)
            inside = np.ones(n, bool)
            m = pr.model
            for a_, b_, c_, d_ in planes:
                inside &= ((a_ * m.xyz[:, 0] + b_ * m.xyz[:, 1]) + c_ * m.xyz[:, 2]) + d_ >= np.float32(0)
            assert inside.any() and not inside.all()
            P = wc.pose(m, 2)
            r = orc.project(*helpers.cloud(m.xyz[inside], m.rgb[inside]), P, W, H)
            for p in (pr.a, pr.b):
                img, depth = p.project(P)
                assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(img, r["img"]), options
        finally:
            pr.close()


def test_write_between_appends_removals_and_moves(pkg, orc):
    """write -> append -> remove -> transform -> write, checked after each step; then render_views and the phase calls."""
    L = pkg._lib
    n = 4099
    for options in ({"pack": 2, "point_ids": 1}, {"pack": 0}, {"auto_reorder": 1, "point_ids": 1}, {"keep_soa": 1}):
        pr = Pair(pkg, orc, options)
        try:
            xyz, rgb = wc.cloud(n)
            pr.upload(xyz, rgb)
            m = pr.model
            sel = wc.selection("random", n)
            pr.write(wc._step(sel, 0, int(sel.sum()), "box", "both", 31), (options, 0))
            pr.check_points((options, 0)); pr.check_frames(0, (options, 0))
            ax, ac = wc.records("wide", 700, 32)
            pr.a.append_points(*helpers.cloud(ax, ac)); m.append(ax, ac)
            pr.check_points((options, 1)); pr.check_frames(1, (options, 1))
            bits = np.arange(m.n) % 9 != 4
            pr.a.remove_points(bits); m.remove(bits)
            pr.check_points((options, 2)); pr.check_frames(2, (options, 2))
            part = np.arange(m.n) < 1500
            pr.a.transform_points(TRANSFORMS["rigid"], part); m.transform(TRANSFORMS["rigid"], part)
            pr.check_points((options, 3)); pr.check_frames(3, (options, 3))
            tail = np.arange(m.n) >= m.n - 900
            pr.write(wc._step(tail, 100, 600, "collapse", "both", 33), (options, 4))
            pr.check_points((options, 4)); pr.check_frames(4, (options, 4))
            # views and phase calls on the written cloud (b holds one upload of it)
            Ps = np.stack([wc.pose(m, k) for k in (5, 6)])
            xyzw, rgba = helpers.cloud(m.xyz, m.rgb)
            for p in (pr.a, pr.b):
                p.render_views(Ps, with_filter=True)
            for which in (L.BUF_VIEW_DEPTH, L.BUF_VIEW_IMAGE, L.BUF_VIEW_TENSOR, L.BUF_VIEW_MINMAX):
                assert np.array_equal(pr.a.download(which), pr.b.download(which)), (options, which)
            r = orc.project(xyzw, rgba, Ps[1], W, H)
            rf = orc.filter(r["depth_bits"], r["img"])
            assert np.array_equal(pr.a.download(L.BUF_VIEW_DEPTH)[1], rf["depth"].view(np.uint32)), options
            assert np.array_equal(pr.a.download(L.BUF_VIEW_IMAGE)[1], rf["img"]), options
            P = Ps[0]
            for p in (pr.a, pr.b):
                p.clear(); p.min_depth_pass(P); p.accumulate_pass(P); p.resolve()
            r = orc.project(xyzw, rgba, P, W, H)
            for which in (L.BUF_DEPTH, L.BUF_ACCUM, L.BUF_IMAGE):
                assert np.array_equal(pr.a.download(which), pr.b.download(which)), (options, which)
            assert np.array_equal(pr.a.download(L.BUF_DEPTH), r["depth_bits"]) and np.array_equal(pr.a.download(L.BUF_IMAGE), r["img"])
        finally:
            pr.close()


def test_write_ordering_async_slot_comes_out_with_the_old_cloud(pkg, orc):
    n = 8229
    xyz, rgb = wc.cloud(n)
    for options in ({}, {"pack": 0}, {"overlap": 1}):
        pr = Pair(pkg, orc, options)
        try:
            pr.upload(xyz, rgb)
            old = pr.model.copy()
            P = wc.pose(old, 0)
            pr.a.project_async(P, 0)
            st = wc._step(None, 0, n, "box", "both", 51)
            pr.write(st, (options, "behind a slot"))
            pr.a.wait_outputs(0)
            img, depth = pr.a.host_output_buffers(0)
            r = orc.project(*helpers.cloud(old.xyz, old.rgb), P, W, H)  # (the slot comes out with the old cloud)
            assert np.array_equal(depth.view(np.uint32), r["depth_bits"]) and np.array_equal(img, r["img"]), options
            r1 = orc.project(*helpers.cloud(pr.model.xyz, pr.model.rgb), P, W, H)
            assert not np.array_equal(r1["depth_bits"], r["depth_bits"])
            pr.check_points(options)
            pr.check_frames(1, (options, "after"))
        finally:
            pr.close()


@pytest.mark.parametrize("streams", ["both", "rgb"])
def test_write_behind_a_frame_that_overflowed_the_pool(pkg, orc, streams):
    """A frame that overflows the adaptive extent pool (pool_overflow_scenes.py), then a write: the synchronising replay
    shows the OLD cloud, the next frame the new one."""
    L = pkg._lib
    xyzw, rgba = sc.cloud(orc)
    P = sc.p_one(orc)[0]
    p = pkg.Projector(0)
    try:
        before = sc.prepare(pkg, orc, p, xyzw, rgba, "first", {"auto_reorder": 0})
        p.render(P)  # (the first frame after the upload overflows; nothing has synchronised yet)
        sel = np.arange(sc.N) % 4 == 1
        k = int(sel.sum())
        # the frame is one pixel, the mean colour of the nearest points: a quarter of the cloud comes 3 m nearer (the
        # depth changes), or turns red (the mean changes)
        X = np.ascontiguousarray(xyzw[sel, :3]) + np.float32([0.0, 0.0, -3.0]) if streams == "both" else None
        Cc = 255 - rgba[sel, :3] if streams == "both" else np.uint8([255, 0, 0])
        assert p.write_points(X, Cc, sel, broadcast=streams == "rgb") == k
        sc.assert_overflowed(p, before, streams)
        old = orc.project(xyzw, rgba, P, sc.W, sc.H)  # (the replay the call waited for: the old cloud)
        assert np.array_equal(p.download(L.BUF_DEPTH), old["depth_bits"]) and np.array_equal(p.download(L.BUF_IMAGE), old["img"])
        x1, c1, _ = write_ref.written(xyzw, rgba, sel, 0, X, Cc)
        new = orc.project(x1, c1, P, sc.W, sc.H)
        assert not (np.array_equal(new["img"], old["img"]) and np.array_equal(new["depth_bits"], old["depth_bits"]))
        img, depth = p.project(P)
        assert np.array_equal(depth.view(np.uint32), new["depth_bits"]) and np.array_equal(img, new["img"])
        sc.no_errors(p)
    finally:
        p.close()


def test_write_errors_change_nothing(pkg, orc):
    """Every error of section 2f returns RTR_ERR_INVALID with a message naming the argument; the extraction of every
    point is identical before and after."""
    L = pkg._lib
    n = 4099
    xyz, rgb = wc.cloud(n)
    X, Cc = wc.records("box", n, 1)
    vx, vc = C.c_void_p(X.ctypes.data), C.c_void_p(Cc.ctypes.data)
    tot = C.c_uint64(123)
    e = pkg.Projector(0)
    try:  # no cloud
        assert e._lib.rtr_write_points(e._ctx, None, 0, 0, 5, vx, 12, vc, 3, None) == L.RTR_ERR_INVALID
        assert "no cloud" in e._lib.rtr_last_error(e._ctx).decode()
    finally:
        e.close()
    p = _new(pkg, {"point_ids": 1})
    try:
        p.upload_points(*helpers.cloud(xyz, rgb))
        p.set_point_keep(np.arange(n) % 3 != 0)
        p.select_points(planes=np.float32([[1, 0, 0, 0]]))
        before = [x.copy() for x in p.extract_points(indices=True)]
        keep0, sel0 = p.download(L.BUF_POINT_KEEP), p.download(L.BUF_SELECTION)
        words = em.words_of(np.arange(n) % 2 == 0)
        vw, nw = C.c_void_p(words.ctypes.data), words.size
        lib = p._lib
        cases = [((None, 0, 0, 5, None, 12, None, 3), "xyz and rgb"),
                 ((None, 0, 0, 5, vx, 0, None, 3), "xyz_stride_bytes"), ((None, 0, 0, 5, vx, 8, None, 3), "xyz_stride_bytes"),
                 ((None, 0, 0, 5, vx, 14, None, 3), "xyz_stride_bytes"), ((None, 0, 0, 5, None, 12, vc, 2), "rgb_stride_bytes"),
                 ((None, 0, 0, 5, vx, 12, vc, 1), "rgb_stride_bytes"),
                 ((vw, nw - 1, 0, 5, vx, 12, vc, 3), "nwords"), ((vw, nw + 1, 0, 5, vx, 12, vc, 3), "nwords"),
                 ((vw, 0, 0, 5, vx, 12, vc, 3), "nwords"), ((None, nw, 0, 5, vx, 12, vc, 3), "select_words")]
        for args, name in cases:
            assert lib.rtr_write_points(p._ctx, *args, C.byref(tot)) == L.RTR_ERR_INVALID, args
            assert name in lib.rtr_last_error(p._ctx).decode(), (name, lib.rtr_last_error(p._ctx))
        assert tot.value == 123
        # the windows that change nothing return RTR_OK and the total
        k = int((np.arange(n) % 2 == 0).sum())
        for first, count in ((k, 3), (k + 7, 1), (0, 0), (5, 0)):
            assert lib.rtr_write_points(p._ctx, vw, nw, first, count, vx, 12, vc, 3, C.byref(tot)) == 0 and tot.value == k
        assert lib.rtr_write_points(p._ctx, None, 0, n, 1, vx, 12, None, 0, C.byref(tot)) == 0 and tot.value == n
        after = p.extract_points(indices=True)
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert np.array_equal(p.download(L.BUF_POINT_KEEP), keep0) and np.array_equal(p.download(L.BUF_SELECTION), sel0)
    finally:
        p.close()
