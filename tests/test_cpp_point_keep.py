"""The C++ facade's keep-mask methods (include/rtr_project_cloud.hpp: setPointKeep / hidePoints / clearPointKeep, rtr.h
section 6e) built with plain g++ against librtr_hip.so.  CPU: it compiles and links.  GPU: every frame equals the oracle
run on the subset of the cloud the mask keeps, and hidePoints accumulates on the mask in force."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build(tmp_path, pkg):
    exe = str(tmp_path / "keep_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "keep_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_keep_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


@pytest.mark.gpu
def test_keep_facade_matches_subset_oracle(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n, W, H = 40_000, 320, 240
    xyzw, rgba = orc.generate("room_shell", 6, 0, n, n)
    order = np.random.default_rng(8).permutation(n)  # (unordered: the library sorts it)
    xyzw, rgba = xyzw[order], rgba[order]
    cal, E = pkg.benchmark_calibration(W, H), pkg.orbit_pose(222)
    rng = np.random.default_rng(9)
    keep = rng.random(n) >= 0.2
    hide = rng.choice(n, 4000, replace=False).astype(np.uint64)
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "cam.bin", "wb") as f:
        f.write(np.ascontiguousarray(cal.getIntrinsicsMatrix(), np.float64).tobytes())
        f.write(np.ascontiguousarray(E, np.float64).tobytes())
    keep.astype(np.uint8).tofile(str(tmp_path / "keep.bin"))
    with open(tmp_path / "hide.bin", "wb") as f:
        f.write(np.uint64(len(hide)).tobytes())
        f.write(hide.tobytes())
    out = str(tmp_path / "out")
    subprocess.check_call([exe, str(tmp_path / "cloud.bin"), str(W), str(H), str(tmp_path / "cam.bin"),
                           str(tmp_path / "keep.bin"), str(tmp_path / "hide.bin"), out], timeout=300)
    P = orc.compose_projection(cal.getIntrinsicsMatrix(), E)
    rd = lambda ext, dt: np.fromfile(out + ext, dtype=dt)  # noqa: E731
    ref = orc.project(xyzw[keep], rgba[keep], P, W, H)
    assert np.array_equal(rd(".set.rgb", np.uint8), ref["img"].reshape(-1))
    assert np.array_equal(rd(".set.depth", np.uint32), ref["depth_bits"].reshape(-1))
    keep2 = keep.copy()
    keep2[hide.astype(np.int64)] = False
    words = rd(".mask", np.uint32)
    assert np.array_equal(np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool), keep2)
    ref2 = orc.project(xyzw[keep2], rgba[keep2], P, W, H)
    rf = orc.filter(ref2["depth_bits"], ref2["img"])
    assert np.array_equal(rd(".hide.frgb", np.uint8), rf["img"].reshape(-1))
    assert np.array_equal(rd(".hide.fdepth", np.uint32), rf["depth"].view(np.uint32).reshape(-1))
    ref3 = orc.project(xyzw, rgba, P, W, H)
    assert np.array_equal(rd(".clear.rgb", np.uint8), ref3["img"].reshape(-1))
    assert np.array_equal(rd(".clear.depth", np.uint32), ref3["depth_bits"].reshape(-1))
