"""The C++ facade's several-views methods (include/rtr_project_cloud.hpp: computeRGBDViews /
computeFilteredRGBDViews) compiled with plain g++ against librtr_hip.so.  CPU: it compiles and links.  GPU: two views
match the oracle bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path, pkg):
    exe = str(tmp_path / "views_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "views_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_views_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


@pytest.mark.gpu
def test_cpp_views_match_oracle(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n, W, H = 80_000, 160, 128
    xyzw, rgba = orc.generate("room_shell", 7, 0, n, n)
    cal = pkg.benchmark_calibration(W, H)
    Es = [pkg.orbit_pose(30), pkg.orbit_pose(420)]
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "cam.bin", "wb") as f:
        f.write(np.ascontiguousarray(cal.getIntrinsicsMatrix(), np.float64).tobytes())
        for E in Es:
            f.write(np.ascontiguousarray(E, np.float64).tobytes())
    out = str(tmp_path / "out")
    res = subprocess.run([exe, str(tmp_path / "cloud.bin"), str(W), str(H), str(tmp_path / "cam.bin"), out],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    rgb = np.fromfile(out + ".rgb", np.uint8).reshape(2, H, W, 3)
    depth = np.fromfile(out + ".depth", np.uint32).reshape(2, H, W)
    frgb = np.fromfile(out + ".frgb", np.uint8).reshape(2, H, W, 3)
    fdepth = np.fromfile(out + ".fdepth", np.uint32).reshape(2, H, W)
    for v, E in enumerate(Es):
        ref = orc.project(xyzw, rgba, orc.compose_projection(cal.getIntrinsicsMatrix(), E), W, H)
        assert np.array_equal(depth[v], ref["depth_bits"]) and np.array_equal(rgb[v], ref["img"]), v
        rf = orc.filter(ref["depth_bits"], ref["img"])
        assert np.array_equal(fdepth[v], rf["depth"].view(np.uint32)) and np.array_equal(frgb[v], rf["img"]), v
