"""The C++ facade's removePoints / commitPointKeep (include/rtr_project_cloud.hpp, rtr.h section 2c) built with plain
g++ against librtr_hip.so.  GPU: a grid, then removePoints of every third vertex and commitPointKeep of a mask that hides
every fifth survivor, renders what the oracle renders on the points left, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path, pkg):
    exe = str(tmp_path / "remove_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "remove_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_remove_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


@pytest.mark.gpu
def test_cpp_remove_matches_oracle(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n, W, H = 90_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 15, 0, n, n)
    cal, E = pkg.benchmark_calibration(W, H), pkg.orbit_pose(33)
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "cam.bin", "wb") as f:
        f.write(np.ascontiguousarray(cal.getIntrinsicsMatrix(), np.float64).tobytes())
        f.write(np.ascontiguousarray(E, np.float64).tobytes())
    out = str(tmp_path / "out")
    subprocess.check_call([exe, str(tmp_path / "cloud.bin"), str(W), str(H), str(tmp_path / "cam.bin"), out], timeout=300)
    rd = lambda ext, dt: np.fromfile(out + ext, dtype=dt)  # noqa: E731
    keep = np.arange(n) % 3 != 0
    k2 = np.arange(int(keep.sum())) % 5 != 0
    xs, cs = xyzw[keep][k2], rgba[keep][k2]
    assert int(rd(".n", np.uint64)[0]) == xs.shape[0]
    P = orc.compose_projection(cal.getIntrinsicsMatrix(), E)
    ref = orc.project(xs, cs, P, W, H)
    assert np.array_equal(rd(".rgb", np.uint8), ref["img"].reshape(-1))
    assert np.array_equal(rd(".depth", np.uint32), ref["depth_bits"].reshape(-1))
    rf = orc.filter(ref["depth_bits"], ref["img"])
    assert np.array_equal(rd(".frgb", np.uint8), rf["img"].reshape(-1))
    assert np.array_equal(rd(".fdepth", np.uint32), rf["depth"].view(np.uint32).reshape(-1))
