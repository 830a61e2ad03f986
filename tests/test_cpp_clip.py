"""The C++ facade's clip methods (include/rtr_project_cloud.hpp: setClipPlanes / setClipBox / clearClip, rtr.h section
6d) built with plain g++ against librtr_hip.so.  CPU: it compiles and links.  GPU: every frame equals the oracle run
on the subset of the cloud that the numpy float32 test keeps."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path, pkg):
    exe = str(tmp_path / "clip_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "clip_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_clip_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


@pytest.mark.gpu
def test_clip_facade_matches_subset_oracle(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n, W, H = 40_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 5, 0, n, n)
    cal, E = pkg.benchmark_calibration(W, H), pkg.orbit_pose(222)
    lo, hi = np.float32([-2.0, -1.0, -1.5]), np.float32([1.0, 0.5, 2.5])
    a = np.deg2rad(20.0)
    M = np.eye(4)
    M[0, :2], M[1, :2] = [np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]
    M[:3, 3] = [0.3, 0.1, -0.2]
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "cam.bin", "wb") as f:
        f.write(np.ascontiguousarray(cal.getIntrinsicsMatrix(), np.float64).tobytes())
        f.write(np.ascontiguousarray(E, np.float64).tobytes())
    np.concatenate([lo, hi]).astype(np.float32).tofile(str(tmp_path / "box.bin"))
    M.astype(np.float64).tofile(str(tmp_path / "m.bin"))
    out = str(tmp_path / "out")
    subprocess.check_call([exe, str(tmp_path / "cloud.bin"), str(W), str(H), str(tmp_path / "cam.bin"),
                           str(tmp_path / "box.bin"), str(tmp_path / "m.bin"), out], timeout=300)
    P = orc.compose_projection(cal.getIntrinsicsMatrix(), E)
    rd = lambda ext, dt: np.fromfile(out + ext, dtype=dt)  # noqa: E731
    box = pkg.clip_box_planes(lo, hi)
    assert np.array_equal(rd(".planes", np.float32).reshape(6, 4), box)
    obox = pkg.clip_box_planes(lo, hi, M)
    assert np.array_equal(rd(".oplanes", np.float32).reshape(6, 4), obox)
    for tag, planes in (("box", box), ("obox", obox), ("clear", np.zeros((0, 4), np.float32))):
        keep = pkg.clip_keep(planes, xyzw)
        assert 0 < keep.sum() <= n
        ref = orc.project(xyzw[keep], rgba[keep], P, W, H)
        assert np.array_equal(rd("." + tag + ".rgb", np.uint8), ref["img"].reshape(-1)), tag
        assert np.array_equal(rd("." + tag + ".depth", np.uint32), ref["depth_bits"].reshape(-1)), tag
    keep = pkg.clip_keep(np.float32([[0, 1, 0, 0]]), xyzw)
    ref = orc.project(xyzw[keep], rgba[keep], P, W, H)
    rf = orc.filter(ref["depth_bits"], ref["img"])
    assert np.array_equal(rd(".plane.frgb", np.uint8), rf["img"].reshape(-1))
    assert np.array_equal(rd(".plane.fdepth", np.uint32), rf["depth"].view(np.uint32).reshape(-1))
    assert np.array_equal(rd(".plane.tensor", np.uint16), rf["tensor"].reshape(-1))
