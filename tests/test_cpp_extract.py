"""The C++ facade's extraction calls (include/rtr_project_cloud.hpp, rtr.h section 2e) built with plain g++ against
librtr_hip.so.  GPU: a box selection extracted with indices equals the numpy gather of the uploaded vertices, and a
second cloud built from the extracted vectors renders what the oracle renders on those vertices, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path, pkg):
    exe = str(tmp_path / "extract_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "extract_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_extract_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


@pytest.mark.gpu
def test_cpp_extract_matches_numpy_and_the_oracle(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n, W, H = 90_001, 320, 240
    xyzw, rgba = orc.generate("room_shell", 15, 0, n, n)
    cal, E = pkg.benchmark_calibration(W, H), pkg.orbit_pose(33)
    lo = xyzw[:, :3].min(axis=0) - 1
    hi = (xyzw[:, :3].min(axis=0) + xyzw[:, :3].max(axis=0)) / 2 + np.float32(0.013)
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "cam.bin", "wb") as f:
        f.write(np.ascontiguousarray(cal.getIntrinsicsMatrix(), np.float64).tobytes())
        f.write(np.ascontiguousarray(E, np.float64).tobytes())
    np.concatenate([lo, hi]).astype(np.float32).tofile(tmp_path / "box.bin")
    out = str(tmp_path / "out")
    subprocess.check_call([exe, str(tmp_path / "cloud.bin"), str(W), str(H), str(tmp_path / "cam.bin"),
                           str(tmp_path / "box.bin"), out], timeout=300)
    rd = lambda ext, dt: np.fromfile(out + ext, dtype=dt)  # noqa: E731
    box = pkg.clip_keep(pkg.clip_box_planes(lo, hi), xyzw)
    k = int(box.sum())
    assert 0 < k < n
    assert list(rd(".counts", np.uint64)) == [k, k, n]
    assert np.array_equal(rd(".idx", np.uint32), np.flatnonzero(box).astype(np.uint32))
    assert np.array_equal(rd(".xyz", np.uint32).reshape(-1, 3), np.ascontiguousarray(xyzw[box, :3]).view(np.uint32))
    assert np.array_equal(rd(".rgb", np.uint8).reshape(-1, 3), rgba[box, :3])
    P = orc.compose_projection(cal.getIntrinsicsMatrix(), E)
    ref = orc.project(xyzw[box], rgba[box], P, W, H)
    assert np.array_equal(rd(".rgbimg", np.uint8), ref["img"].reshape(-1))
    assert np.array_equal(rd(".depth", np.uint32), ref["depth_bits"].reshape(-1))
