"""The C++ facade's selection calls (include/rtr_project_cloud.hpp, rtr.h section 6f) built with plain g++ against
librtr_hip.so.  GPU: a box, a half-space and a screen rectangle combined into one selection give the counts and words
of the references (camera.clip_keep, the oracle's projection); hiding, moving and removing the selection render what
the oracle renders on the numpy-edited vertices, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import select_ref as sr


def _build(tmp_path, pkg):
    exe = str(tmp_path / "select_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "select_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_select_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


@pytest.mark.gpu
def test_cpp_select_matches_references(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n, W, H = 90_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 15, 0, n, n)
    cal, E = pkg.benchmark_calibration(W, H), pkg.orbit_pose(33)
    c, s = np.cos(0.07), np.sin(0.07)
    M1 = np.array([[c, -s, 0, 0.25], [s, c, 0, -0.4], [0, 0, 1, 0.05], [0, 0, 0, 1]], np.float64)
    lo = xyzw[:, :3].min(axis=0) - 1
    hi = (xyzw[:, :3].min(axis=0) + xyzw[:, :3].max(axis=0)) / 2 + np.float32(0.013)
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "cam.bin", "wb") as f:
        f.write(np.ascontiguousarray(cal.getIntrinsicsMatrix(), np.float64).tobytes())
        f.write(np.ascontiguousarray(E, np.float64).tobytes())
    M1.tofile(tmp_path / "m1.bin")
    np.concatenate([lo, hi]).astype(np.float32).tofile(tmp_path / "box.bin")
    out = str(tmp_path / "out")
    subprocess.check_call([exe, str(tmp_path / "cloud.bin"), str(W), str(H), str(tmp_path / "cam.bin"),
                           str(tmp_path / "m1.bin"), str(tmp_path / "box.bin"), out], timeout=300)
    rd = lambda ext, dt: np.fromfile(out + ext, dtype=dt)  # noqa: E731
    P = orc.compose_projection(cal.getIntrinsicsMatrix(), E)
    box = sr.inside(pkg, orc, xyzw, pkg.clip_box_planes(lo, hi))
    half = sr.inside(pkg, orc, xyzw, np.float32([[1, 0, 0, 0]]))
    rect = sr.inside(pkg, orc, xyzw, None, P, (W // 8, H // 8, 5 * W // 8, 7 * H // 8), W, H)
    sel = (box & half) | rect
    assert 0 < sel.sum() < n
    assert list(rd(".counts", np.uint64)) == [box.sum(), (box & half).sum(), sel.sum(), sel.sum()]
    assert np.array_equal(rd(".words", np.uint32), sr.words(sel))
    # the Python facade's path gives the same words
    pc = pkg.ProjectCloud(xyzw, rgba, point_ids=True)
    pc.selectBox(lo, hi)
    pc.selectPlanes(np.float32([[1, 0, 0, 0]]), op="intersect")
    pc.selectRect(cal, E, W // 8, H // 8, 5 * W // 8, 7 * H // 8, op="add")
    assert np.array_equal(pc.projector.download(pkg._lib.BUF_SELECTION), rd(".words", np.uint32))
    ref = orc.project(xyzw[~sel], rgba[~sel], P, W, H)  # hidden
    assert np.array_equal(rd(".hrgb", np.uint8), ref["img"].reshape(-1))
    assert np.array_equal(rd(".hdepth", np.uint32), ref["depth_bits"].reshape(-1))
    m = M1[:3].astype(np.float32)  # moved
    xs = xyzw.copy()
    x, y, z = xyzw[sel, 0], xyzw[sel, 1], xyzw[sel, 2]
    for r in range(3):
        xs[sel, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    ref = orc.project(xs, rgba, P, W, H)
    rf = orc.filter(ref["depth_bits"], ref["img"])
    assert np.array_equal(rd(".trgb", np.uint8), rf["img"].reshape(-1))
    assert np.array_equal(rd(".tdepth", np.uint32), rf["depth"].view(np.uint32).reshape(-1))
    assert int(rd(".n", np.uint64)[0]) == int((~sel).sum())  # removed
    ref = orc.project(xs[~sel], rgba[~sel], P, W, H)
    assert np.array_equal(rd(".rrgb", np.uint8), ref["img"].reshape(-1))
    assert np.array_equal(rd(".rdepth", np.uint32), ref["depth_bits"].reshape(-1))
