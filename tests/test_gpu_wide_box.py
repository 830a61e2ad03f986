"""-m gpu: the box word of wide packed chunks (hdr[2 c + 1].w, csrc/rtr_chunk_box.h).  Chunks that straddle one, two and
three coordinate planes -- a chunk holding a NaN and a partial last chunk among them -- under cameras that see all, some
and none of them and cameras sitting on a coordinate plane: every frame bit for bit the oracle's, with chunk_test 0 / 1
and pack 0 / 1 / 2, with clip planes, a keep mask and through rtr_render_views; the point pass and the selection against
their references; the same after append, remove and transform (a chunk moved across a coordinate plane included), where
the options wide_chunks / wide_chunks_boxed must equal those of a fresh upload of the edited cloud."""
import numpy as np
import pytest

from helpers import cloud
import point_pass_ref as ppr
import select_ref as sr

pytestmark = pytest.mark.gpu

W, H = 320, 240
EMPTY = 0x7F7FFFFF  # depth bits of a pixel no point landed on


def _new(pkg, xyzw, rgba, **options):
    p = pkg.Projector(0)
    p.set_option("auto_reorder", 0)  # the chunks as built here
    for k, v in options.items():
        p.set_option(k, v)
    p.upload_points(xyzw, rgba)
    p.set_resolution(W, H)
    return p


def _chunk(rng, centre, size):
    return (np.asarray(centre, np.float32) + rng.uniform(-size, size, size=(256, 3))).astype(np.float32)


def _wide_cloud(seed, nan_chunk=True, tail=37):
    """Chunks of 256 points in a room around the origin.  -> (xyzw, rgba, kinds): kinds[c] = the coordinate planes chunk
    c straddles (0 .. 3), -1 for the chunk with the NaN."""
    rng = np.random.default_rng(seed)
    chunks, kinds = [], []
    for rep in range(3):
        for axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2), ()):
            for size in (0.02, 0.3):
                c = rng.uniform(0.6, 3.5, 3) * rng.choice([-1.0, 1.0], 3)
                c[1] *= 0.4
                for a in axes:
                    c[a] = rng.uniform(-0.5, 0.5) * size
                pts = _chunk(rng, c, size)
                for a in axes:  # (both signs for certain)
                    pts[0, a], pts[1, a] = -abs(pts[0, a]) - 1e-6, abs(pts[1, a]) + 1e-6
                chunks.append(pts)
                kinds.append(len(axes))
    # +-0 and denormals on an axis; a wall lying IN a coordinate plane (every x exactly +0: not wide)
    pts = _chunk(rng, (1.0, 0.2, 2.0), 0.1)
    pts[:, 0] = np.where(rng.random(256) < 0.5, np.float32(0.0), np.float32(-0.0))
    chunks.append(pts), kinds.append(1)
    pts = _chunk(rng, (1.0, 0.2, -2.0), 0.1)
    pts[:, 1] = (rng.integers(1, 1 << 22, 256).astype(np.uint32) | (rng.integers(0, 2, 256).astype(np.uint32) << 31)).view(np.float32)
    chunks.append(pts), kinds.append(1)
    pts = _chunk(rng, (0.0, 0.2, 1.5), 0.2)
    pts[:, 0] = np.float32(0.0)
    chunks.append(pts), kinds.append(0)
    if nan_chunk:
        pts = _chunk(rng, (0.0, 0.1, 2.5), 0.2)
        pts[0, 0], pts[1, 0] = -0.1, 0.1
        pts[77, 1] = np.float32(np.nan)
        chunks.append(pts), kinds.append(-1)
    if tail:  # a partial last chunk on the plane z = 0 (its last quad ends in NaN padding when tail % 4 != 0)
        pts = _chunk(rng, (-1.5, 0.3, 0.0), 0.1)[:tail]
        pts[0, 2], pts[-1, 2] = -0.05, 0.05
        chunks.append(pts), kinds.append(1)
    xyz = np.concatenate(chunks)
    xyzw, rgba = cloud(xyz, rng.integers(0, 256, size=(len(xyz), 3), dtype=np.uint8))
    return xyzw, rgba, np.array(kinds)


def _wide_count(xyzw):
    """The packer's width rule on the host: chunks with an axis whose 256 patterns differ in more than 25 bits; the cloud
    is padded to whole quads with NaN and the lanes past its end repeat the last quad."""
    x = np.asarray(xyzw, np.float32)[:, :3]
    n = len(x)
    n4 = (n + 3) // 4
    x = np.concatenate([x, np.full((4 * n4 - n, 3), np.nan, np.float32)])
    nch = (n4 + 63) // 64
    x = np.concatenate([x] + [x[-4:]] * (64 * nch - n4)).view(np.uint32).reshape(nch, 256, 3)
    diff = np.bitwise_or.reduce(x ^ x[:, :1, :], axis=1)
    return int(((diff >> 25) != 0).any(axis=1).sum())


def _look(orc, eye, yaw, pitch=0.0, f=0.8):
    """A camera at `eye` turned by yaw about y and pitch about x."""
    K = np.array([[f * W, 0, W / 2], [0, f * W, H / 2], [0, 0, 1.0]])
    cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    R = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ np.asarray(eye, np.float64)
    return orc.compose_projection(K, E)


def _cameras(pkg, orc):
    cams = [pkg.orbit_projection(k, W, H) for k in (0, 17, 250, 600)]  # some of the wide chunks
    cams.append(_look(orc, (0.0, 0.0, -30.0), 0.0, f=1.5))    # all of them, far away, on the planes x = 0 and y = 0
    cams.append(_look(orc, (0.0, 0.0, -30.0), np.pi, f=1.5))  # none: the cloud behind the camera
    cams.append(_look(orc, (40.0, 30.0, 40.0), 0.3))          # none: looking past the room
    cams.append(_look(orc, (0.0, 0.0, 0.0), 0.7, 0.2))        # at the origin, inside the chunk on all three planes
    cams.append(_look(orc, (0.0, 0.4, -2.0), 0.0))            # on x = 0, looking along it
    cams.append(_look(orc, (1.0, 0.0, 1.0), 2.0))             # on y = 0
    cams.append(_look(orc, (-2.0, 0.5, 0.0), 1.2, -0.1))      # on z = 0
    return cams


def _assert_frame(orc, p, xyzw, rgba, P, what):
    ref = orc.project(xyzw, rgba, P, W, H)
    img, depth = p.project(P)
    assert np.array_equal(depth.view(np.uint32), ref["depth_bits"]), what
    assert np.array_equal(img, ref["img"]), what
    return ref


def _counts(p):
    return p.get_option("wide_chunks"), p.get_option("wide_chunks_boxed")


@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("pack", [0, 1, 2])
def test_frames_equal_the_oracle(pkg, orc, pack, grid):
    """grid 1: one workgroup, so every wave tests batches that mix wide chunks and others, lane by lane."""
    xyzw, rgba, kinds = _wide_cloud(61)
    p = _new(pkg, xyzw, rgba, pack=pack, **({"point_grid": 1} if grid else {}))
    try:
        if pack == 2:
            assert p.get_option("packed") == 1
            wide, boxed = _counts(p)
            assert wide == _wide_count(xyzw) and wide >= int((kinds != 0).sum())
            assert boxed == wide - 1  # (the chunk with the NaN; the partial chunk's NaN padding is no point)
        elif not p.get_option("packed"):
            assert _counts(p) == (0, 0)
        seen = []
        for k, P in enumerate(_cameras(pkg, orc)):
            for ct in (1, 0):
                p.set_option("chunk_test", ct)
                ref = _assert_frame(orc, p, xyzw, rgba, P, (pack, grid, k, ct))
            seen.append(int((ref["depth_bits"] != EMPTY).sum()))
        assert seen[4] > 0 and seen[5] == 0 and seen[6] == 0  # (all / none of the cloud in view)
    finally:
        p.close()


def test_room_cloud_counts_and_frames(pkg, orc):
    n = 300_001
    xyzw, rgba = orc.generate("room_shell", 62, 0, n, n)
    p = _new(pkg, xyzw, rgba, pack=2)
    try:
        wide, boxed = _counts(p)
        assert wide == _wide_count(xyzw) and wide > 10 and boxed == wide  # a finite cloud: every wide chunk has its box
        for k in (5, 333, 777):
            for ct in (1, 0):
                p.set_option("chunk_test", ct)
                _assert_frame(orc, p, xyzw, rgba, pkg.orbit_projection(k, W, H), (k, ct))
    finally:
        p.close()


def test_clip_planes_keep_mask_and_views(pkg, orc):
    L = pkg._lib
    xyzw, rgba, kinds = _wide_cloud(63)
    n = len(xyzw)
    rng = np.random.default_rng(64)
    keep = rng.random(n) < 0.7
    keep[256 * 3:256 * 5] = False  # two wide chunks hidden entirely
    keep[256 * 8:256 * 9] = True
    cams = _cameras(pkg, orc)
    f = np.float32
    plane_sets = [f([[1, 0, 0, 0]]), f([[0, -1, 0, 0.0]]), f([[0.3, -0.2, 0.9, 0.05], [-0.7, 0.1, 0.2, 1.3]]), f([[1, 0, 0, -0.01], [0, 0, -1, 0.015]])]
    for grid in (0, 1):
        p = _new(pkg, xyzw, rgba, pack=2, **({"point_grid": 1} if grid else {}))
        try:
            for ct in (1, 0):
                p.set_option("chunk_test", ct)
                for j, planes in enumerate(plane_sets):
                    p.set_clip_planes(planes)
                    for use_keep in (False, True):
                        p.set_point_keep(keep if use_keep else None)
                        sub = pkg.clip_keep(planes, xyzw) & (keep if use_keep else True)
                        for k in (0, 4, 7, 8, 10):
                            ref = orc.project(xyzw[sub], rgba[sub], cams[k], W, H)
                            img, depth = p.project(cams[k])
                            assert np.array_equal(depth.view(np.uint32), ref["depth_bits"]), (grid, ct, j, use_keep, k)
                            assert np.array_equal(img, ref["img"]), (grid, ct, j, use_keep, k)
                        if ct == 1:  # several views in one pass (their chunk test has its own form)
                            for lo in (0, 6):
                                Ps = np.stack([np.asarray(c, np.float32).reshape(4, 4) for c in cams[lo:lo + 5]])
                                p.render_views(Ps, False)
                                depth = p.download(L.BUF_VIEW_DEPTH).reshape(len(Ps), H, W)
                                img = p.download(L.BUF_VIEW_IMAGE).reshape(len(Ps), H, W, 3)
                                for v in range(len(Ps)):
                                    ref = orc.project(xyzw[sub], rgba[sub], Ps[v].reshape(16), W, H)
                                    assert np.array_equal(depth[v].view(np.uint32), ref["depth_bits"]), (grid, j, use_keep, lo, v)
                                    assert np.array_equal(img[v], ref["img"]), (grid, j, use_keep, lo, v)
            p.set_clip_planes(None)
            p.set_point_keep(None)
            Ps = np.stack([np.asarray(c, np.float32).reshape(4, 4) for c in cams[3:11]])  # eight views, no filter
            p.render_views(Ps, False)
            depth = p.download(L.BUF_VIEW_DEPTH).reshape(len(Ps), H, W)
            for v in range(len(Ps)):
                ref = orc.project(xyzw, rgba, Ps[v].reshape(16), W, H)
                assert np.array_equal(depth[v].view(np.uint32), ref["depth_bits"]), (grid, v)
        finally:
            p.close()


def test_point_pass_and_selection(pkg, orc):
    L = pkg._lib
    xyzw, rgba, kinds = _wide_cloud(65)
    n = len(xyzw)
    cams = _cameras(pkg, orc)
    f = np.float32
    p = _new(pkg, xyzw, rgba, pack=2)
    try:
        for k in (0, 4, 5, 7, 8, 9, 10):
            P = cams[k]
            p.render(P, False)
            p.point_pass(P)
            ids, vis, depth = p.download(L.BUF_POINT_ID), p.download(L.BUF_VISIBLE), p.download(L.BUF_DEPTH)
            ref = orc.project(xyzw, rgba, P, W, H)
            assert np.array_equal(depth.reshape(-1).view(np.uint32), ref["depth_bits"].reshape(-1)), k
            e_ids, e_vis = ppr.point_pass(orc, xyzw, P, W, H, ref["depth_bits"])
            assert np.array_equal(ids.reshape(-1), e_ids.reshape(-1)), k
            assert np.array_equal(ppr.unpack(vis, n), ppr.unpack(e_vis, n)), k
        boxes = [f([[1, 0, 0, 0]]), f([[-1, 0, 0, 0.0], [0, 1, 0, 0]]), f([[0, 0, 1, 0.01]]), f([[0.3, -0.2, 0.9, 0.05]]),
                 pkg.clip_box_planes([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]), pkg.clip_box_planes([-10, -10, -10], [10, 10, 10]),
                 pkg.clip_box_planes([0.0, -10, -10], [10, 10, 10])]
        for j, planes in enumerate(boxes):
            for outside in (False, True):
                stats = p.select_points(planes=planes, outside=outside)
                want = sr.inside(pkg, orc, xyzw, planes) != outside
                assert stats[0] == int(want.sum()), (j, outside)
                assert np.array_equal(p.download(L.BUF_SELECTION), sr.words(want)), (j, outside)
        decided = 0
        for k in (0, 4, 5, 7, 8, 10):
            for rect in ((0, 0, W, H), (W // 4, H // 4, 3 * W // 4, 3 * H // 4), (0, 0, 1, 1)):
                stats = p.select_points(P=cams[k], rect=rect)
                want = sr.inside(pkg, orc, xyzw, None, cams[k], rect, W, H)
                assert stats[0] == int(want.sum()), (k, rect)
                assert np.array_equal(p.download(L.BUF_SELECTION), sr.words(want)), (k, rect)
                decided += stats[1]
        assert decided > 0
        p.clear_selection()
    finally:
        p.close()


def _moved(xyzw, M, sel):
    m = np.asarray(M, np.float32)[:3]
    out = xyzw.copy()
    x, y, z = xyzw[sel, 0], xyzw[sel, 1], xyzw[sel, 2]
    for r in range(3):
        out[sel, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    return out


def _check_edited(pkg, orc, p, xyzw, rgba, nan_chunks, what):
    """Frames of the edited context against the oracle on the host-edited cloud, and its counts against a fresh upload."""
    assert p.num_points == len(xyzw), what
    q = _new(pkg, xyzw, rgba, pack=2)
    try:
        fresh = _counts(q)
    finally:
        q.close()
    assert _counts(p) == fresh, what
    assert fresh[0] == _wide_count(xyzw) and fresh[1] == fresh[0] - nan_chunks, what
    cams = _cameras(pkg, orc)
    for k in (0, 4, 7, 8, 10):
        for ct in (1, 0):
            p.set_option("chunk_test", ct)
            _assert_frame(orc, p, xyzw, rgba, cams[k], (what, k, ct))
    p.set_option("chunk_test", 1)


@pytest.mark.parametrize("nan_chunk", [False, True])
def test_append_remove_transform(pkg, orc, nan_chunk):
    L = pkg._lib
    xyzw, rgba, kinds = _wide_cloud(66, nan_chunk=nan_chunk, tail=37)
    more, more_rgba, _ = _wide_cloud(67, nan_chunk=False, tail=101)
    nan_chunks = 1 if nan_chunk else 0
    p = _new(pkg, xyzw, rgba, pack=2)
    try:
        # append: the partial chunk is completed by points on the other side of its plane, then whole wide chunks follow
        p.append_points(more, more_rgba)
        xyzw, rgba = np.concatenate([xyzw, more]), np.concatenate([rgba, more_rgba])
        _check_edited(pkg, orc, p, xyzw, rgba, nan_chunks, "append")
        # remove: points out of wide chunks, a whole wide chunk, and every negative-x point of another (no longer wide)
        rng = np.random.default_rng(68)
        keep = rng.random(len(xyzw)) < 0.9
        keep[256 * 2:256 * 3] = False
        s = slice(256 * 12, 256 * 13)
        keep[s] &= ~(xyzw[s, 0] < 0)
        keep |= np.isnan(xyzw[:, :3]).any(axis=1)  # (the NaN stays: one chunk without a box)
        p.remove_points(keep)
        xyzw, rgba = xyzw[keep], rgba[keep]
        _check_edited(pkg, orc, p, xyzw, rgba, nan_chunks, "remove")
        # transform: a chunk off every plane moved ACROSS x = 0, and a chunk on a plane moved off it
        n = len(xyzw)
        chunk_lo = xyzw[:n // 256 * 256, :3].reshape(-1, 256, 3).min(axis=1)
        chunk_hi = xyzw[:n // 256 * 256, :3].reshape(-1, 256, 3).max(axis=1)
        finite = np.isfinite(chunk_lo).all(axis=1) & np.isfinite(chunk_hi).all(axis=1)
        off = [int(np.argmax(np.where(finite, chunk_lo[:, 0], -np.inf)))]  # the chunk furthest on the positive side of x = 0
        on = np.flatnonzero((chunk_lo[:, 0] < 0) & (chunk_hi[:, 0] > 0) & finite)
        assert chunk_lo[off[0], 0] > 0 and len(on) > 1
        c = off[0]
        sel = np.zeros(n, bool)
        sel[256 * c:256 * c + 256] = True
        M = np.eye(4)
        M[0, 3] = -(chunk_lo[c, 0] + chunk_hi[c, 0]) / 2
        p.transform_points(M, sel)
        xyzw = _moved(xyzw, M, sel)
        assert xyzw[sel, 0].min() < 0 < xyzw[sel, 0].max()
        _check_edited(pkg, orc, p, xyzw, rgba, nan_chunks, "transform across")
        c = on[0] if on[0] != off[0] else on[1]
        sel = np.zeros(n, bool)
        sel[256 * c:256 * c + 256] = True
        M = np.eye(4)
        M[0, 3] = 2.0
        p.transform_points(M, sel)
        xyzw = _moved(xyzw, M, sel)
        _check_edited(pkg, orc, p, xyzw, rgba, nan_chunks, "transform off")
        # every point: a rotation about y by a little, the planes cut other chunks now
        cs, sn = np.cos(0.05), np.sin(0.05)
        M = np.array([[cs, 0, sn, 0.01], [0, 1, 0, -0.02], [-sn, 0, cs, 0.03], [0, 0, 0, 1]])
        p.transform_points(M)
        xyzw = _moved(xyzw, M, np.ones(n, bool))
        _check_edited(pkg, orc, p, xyzw, rgba, nan_chunks, "transform all")
        assert np.array_equal(p.download_points()[0][:, :3].view(np.uint32), xyzw[:, :3].view(np.uint32))
    finally:
        p.close()
