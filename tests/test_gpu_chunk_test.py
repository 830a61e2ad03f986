"""-m gpu: option "chunk_test" (the packed point kernel tests its chunks on their header boxes before it streams them).
Every frame must equal the oracle's, bit for bit, with the test on (1) and off (0, the round-4 loop): chunks straddling
each frustum plane within a few ulps, the camera centre inside a chunk's box and on cloud points 4l, 4l+1, 4l+3, tight
lane spreads, wide-flag chunks, a partial last chunk, several header batches per wave, phase groups and lean frames."""
import numpy as np
import pytest

from helpers import cloud

pytestmark = pytest.mark.gpu

W, H = 640, 480


@pytest.fixture
def packed(projector):
    """The packed form whatever the cloud (pack = 2), the chunks in the order given (auto_reorder = 0); every option
    this file touches is put back as it was."""
    keys = ("chunk_test", "pack", "auto_reorder", "point_grid", "phases", "lean")
    saved = {k: projector.get_option(k) for k in keys}
    projector.set_option("auto_reorder", 0)
    projector.set_option("pack", 2)
    projector.saved_options = saved
    yield projector
    for k in keys:
        projector.set_option(k, saved[k])


def _frames_equal(pkg, orc, p, xyzw, rgba, P, lean=False):
    p.upload_points(xyzw, rgba)
    p.set_resolution(W, H)
    assert p.get_option("packed") == 1
    ref = orc.project(xyzw, rgba, P, W, H)
    rf = orc.filter(ref["depth_bits"], ref["img"])
    for ct in (1, 0):
        p.set_option("chunk_test", ct)
        img, depth = p.project(P)
        assert np.array_equal(depth.view(np.uint32), ref["depth_bits"]), ct
        assert np.array_equal(img, ref["img"]), ct
        if lean:  # a whole frame through rtr_render (lean frames skip T1's epilogue)
            p.render(P, True)
            assert np.array_equal(p.download(pkg._lib.BUF_TENSOR).reshape(5, H, W), rf["tensor"]), ct
    return ref


def _camera(P):
    P = np.asarray(P, np.float64).reshape(4, 4)
    M, t = P[:3, :3], P[:3, 3]
    return -np.linalg.solve(M, t), np.linalg.inv(M)


def _ulps(x, rng, k):
    """x moved by -k .. k ulps per coordinate (bit patterns of the same sign)."""
    b = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    d = rng.integers(-k, k + 1, size=b.shape)
    b = np.where(b == 0, np.abs(d), b + d * np.where(b < 0, -1, 1))  # (from 0: denormals, never a sign change)
    return b.astype(np.int32).view(np.float32)


def _chunks(centres, rng, spread, ulps=0):
    """256 points per centre: offsets of at most `spread`, then a few ulps."""
    pts = np.repeat(np.asarray(centres, np.float32), 256, axis=0)
    pts = (pts + rng.uniform(-spread, spread, size=pts.shape)).astype(np.float32)
    return _ulps(pts, rng, ulps) if ulps else pts


def _colours(n, rng):
    return rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def test_chunks_straddling_every_plane(pkg, orc, packed):
    rng = np.random.default_rng(51)
    P = pkg.orbit_projection(17, W, H)
    c, Minv = _camera(P)
    centres = []
    for d in (0.05, 0.7, 3.0, 40.0):
        for u, v in [(-0.5, 100.0), (W - 0.5, 200.0), (300.0, -0.5), (100.0, H - 0.5), (-0.5, -0.5), (W - 0.5, H - 0.5),
                     (-1.0, 50.0), (W, 50.0), (50.0, -1.0), (50.0, H)]:
            for _ in range(3):
                centres.append(c + d * (Minv @ np.array([u, v, 1.0])))
    for _ in range(8):  # on the camera plane r.z = 0, beside and around the centre
        centres.append(c + Minv @ np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 0.0]))
    for spread, ulps in ((1e-4, 0), (1e-6, 0), (0.0, 4), (0.02, 2)):
        pts = _chunks(centres, rng, spread, ulps)
        xyzw, rgba = cloud(pts, _colours(len(pts), rng))
        _frames_equal(pkg, orc, packed, xyzw, rgba, P)


def test_camera_centre_inside_a_chunk_and_on_its_points(pkg, orc, packed):
    rng = np.random.default_rng(52)
    P = pkg.orbit_projection(123, W, H)
    c, Minv = _camera(P)
    ahead = c + 2.0 * (Minv @ np.array([W / 2, H / 2, 1.0]))
    for spread in (1e-4, 0.01, 0.5):
        pts = _chunks([c, c, ahead, c], rng, spread)
        for base in (0, 256 * 3):  # lane l's points 4l, 4l+1, 4l+3 of a chunk on the centre, +-1..4 ulps
            for lane in range(0, 64, 5):
                for k in (0, 1, 3):
                    pts[base + 4 * lane + k] = _ulps(np.asarray(c, np.float32)[None], rng, 1 + lane % 4)[0]
        xyzw, rgba = cloud(pts, _colours(len(pts), rng))
        _frames_equal(pkg, orc, packed, xyzw, rgba, P)


def test_wide_flag_chunks(pkg, orc, packed):
    rng = np.random.default_rng(53)
    P = pkg.orbit_projection(0, W, H)
    c, Minv = _camera(P)
    ahead = [c + d * (Minv @ np.array([rng.uniform(0, W), rng.uniform(0, H), 1.0])) for d in (0.5, 2.0, 5.0, 9.0)]
    pts = _chunks(ahead * 6, rng, 0.05)
    n_ch = len(pts) // 256
    for ch in range(n_ch):
        s = slice(256 * ch, 256 * ch + 256)
        kind = ch % 6
        if kind == 0:    # mixed signs on one axis
            pts[s, 0] = rng.uniform(-1e-3, 1e-3, 256).astype(np.float32)
        elif kind == 1:  # a NaN
            pts[256 * ch + 77, 1] = np.float32(np.nan)
        elif kind == 2:  # -0 next to +0
            pts[s, 2] = np.where(rng.random(256) < 0.5, np.float32(0.0), np.float32(-0.0))
        elif kind == 3:  # values near FLT_MAX (the box's top end reaches exponent 0xFF)
            pts[256 * ch + 5, 0] = np.float32(3.4e38)
        elif kind == 4:  # denormals
            pts[s, 1] = (rng.integers(1, 1 << 20, 256).astype(np.uint32)).view(np.float32)
    xyzw, rgba = cloud(pts, _colours(len(pts), rng))
    for k in (0, 1, 2):
        Pk = P if k == 0 else pkg.orbit_projection(250 * k, W, H)
        _frames_equal(pkg, orc, packed, xyzw, rgba, Pk)


@pytest.mark.parametrize("n", [256 * 40 + 37, 256 * 1000 + 255, 299_999])
def test_partial_last_chunk_and_many_batches(pkg, orc, packed, n):
    """point_grid = 1: four waves, so each holds several batches of 64 chunks (the header prefetch, the batch switch)."""
    xyzw, rgba = orc.generate("room_shell", 54, 0, n, n)
    for grid in (1, 7, packed.saved_options["point_grid"]):  # (the last: the context's own grid)
        packed.set_option("point_grid", grid)
        for k in (3, 500):
            _frames_equal(pkg, orc, packed, xyzw, rgba, pkg.orbit_projection(k, W, H))


def test_phase_groups_lean_frames_and_overview(pkg, orc, packed):
    n = 400_000
    xyzw, rgba = orc.generate("room_shell", 55, 0, n, n)
    packed.set_option("point_grid", 3)
    for phases in (0, 5, 16):
        packed.set_option("phases", phases)
        _frames_equal(pkg, orc, packed, xyzw, rgba, pkg.orbit_projection(40, W, H))
    packed.set_option("phases", packed.saved_options["phases"])
    packed.set_option("lean", 1)
    _frames_equal(pkg, orc, packed, xyzw, rgba, pkg.orbit_projection(41, W, H), lean=True)
    # the whole cloud inside a few pixels (a distant overview: the 16-group case picked from the previous frame)
    K = np.array([[8.0, 0, 320], [0, 8.0, 240], [0, 0, 1]])
    E = np.eye(4)
    E[2, 3] = 60.0
    Pov = orc.compose_projection(K, E)
    _frames_equal(pkg, orc, packed, xyzw, rgba, Pov)
    _frames_equal(pkg, orc, packed, xyzw, rgba, Pov)
