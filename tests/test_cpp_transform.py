"""The C++ facade's transformPoints (include/rtr_project_cloud.hpp, rtr.h section 2d) built with plain g++ against
librtr_hip.so.  GPU: a grid of two blocks, the second one moved by a rigid transform (one re-registered scan) and a
range of the first moved too, renders what the oracle renders on the moved vertices, bit for bit; a projective bottom
row and a range past the vertex count are refused."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path, pkg):
    exe = str(tmp_path / "transform_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "transform_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_transform_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


def _apply(xyz, M, sel):
    m = M[:3].astype(np.float32)
    out = xyz.copy()
    x, y, z = xyz[sel, 0], xyz[sel, 1], xyz[sel, 2]
    for r in range(3):
        out[sel, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    return out


@pytest.mark.gpu
def test_cpp_transform_matches_oracle(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n, W, H = 90_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 15, 0, n, n)
    cal, E = pkg.benchmark_calibration(W, H), pkg.orbit_pose(33)
    c, s = np.cos(0.07), np.sin(0.07)
    M1 = np.array([[c, -s, 0, 0.25], [s, c, 0, -0.4], [0, 0, 1, 0.05], [0, 0, 0, 1]], np.float64)
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "cam.bin", "wb") as f:
        f.write(np.ascontiguousarray(cal.getIntrinsicsMatrix(), np.float64).tobytes())
        f.write(np.ascontiguousarray(E, np.float64).tobytes())
    M1.tofile(tmp_path / "m1.bin")
    out = str(tmp_path / "out")
    subprocess.check_call([exe, str(tmp_path / "cloud.bin"), str(W), str(H), str(tmp_path / "cam.bin"),
                           str(tmp_path / "m1.bin"), out], timeout=300)
    idx = np.arange(n)
    xs = _apply(xyzw[:, :3].copy(), M1, idx >= n // 2)
    xs = _apply(xs, M1, (idx >= 1000) & (idx < 6000))
    xs = np.concatenate([xs, np.ones((n, 1), np.float32)], axis=1)
    rd = lambda ext, dt: np.fromfile(out + ext, dtype=dt)  # noqa: E731
    P = orc.compose_projection(cal.getIntrinsicsMatrix(), E)
    ref = orc.project(xs, rgba, P, W, H)
    assert np.array_equal(rd(".rgb", np.uint8), ref["img"].reshape(-1))
    assert np.array_equal(rd(".depth", np.uint32), ref["depth_bits"].reshape(-1))
    rf = orc.filter(ref["depth_bits"], ref["img"])
    assert np.array_equal(rd(".frgb", np.uint8), rf["img"].reshape(-1))
    assert np.array_equal(rd(".fdepth", np.uint32), rf["depth"].view(np.uint32).reshape(-1))
