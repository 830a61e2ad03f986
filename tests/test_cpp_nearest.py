"""rtr_nearest_points in C++ (include/rtr.h section 6l).  CPU: the facade's calls of include/rtr_project_cloud.hpp
compiled and linked against librtr_hip.so (tests/cpp/nearest_facade_check.cpp).  GPU: nearestPoints and matchPoints give
the files the reference wrote -- indices, distances as bits, the matched coordinates and colours --, as does the Python
facade."""
import os
import subprocess

import numpy as np
import pytest

import nearest_ref as nf
from conftest import ROOT
from test_cpp_near import _cloud_file


def _build(tmp_path, pkg):
    exe = str(tmp_path / "nearest_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "nearest_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_nearest_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


@pytest.mark.gpu
def test_cpp_nearest_matches_the_reference(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n, m = 30_001, 4_003
    xyzw, rgba = orc.generate("room_shell", 15, 0, n, n)
    g2, c2 = orc.generate("room_shell", 16, 0, n, n)
    gx, gc = np.ascontiguousarray(g2[:m]), np.ascontiguousarray(c2[:m])
    gx[50:60] = xyzw[7:17]  # (coincident with resident points: d2 = +0)
    r = np.float32(0.05)
    _cloud_file(tmp_path / "cloud.bin", xyzw, rgba)
    _cloud_file(tmp_path / "given.bin", gx, gc)
    with open(tmp_path / "params.bin", "wb") as f:
        f.write(np.float32([r]).tobytes())
    gi, gd, _, _, st = nf.nearest_bucket(xyzw, gx, r)
    has = gi != nf.NONE
    assert 0.05 * m < st[0] < 0.95 * m and list(gi[50:60]) == list(range(7, 17)) and not nf.bits(gd)[50:60].any()
    gi.tofile(tmp_path / "want.index")
    nf.bits(gd).tofile(tmp_path / "want.dist2")
    want_xyz, want_rgb = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.uint8)
    want_xyz[has], want_rgb[has] = xyzw[gi[has], :3], rgba[gi[has], :3]
    out = str(tmp_path / "out")
    subprocess.check_call([exe, str(tmp_path / "cloud.bin"), str(tmp_path / "given.bin"), str(tmp_path / "params.bin"),
                           str(tmp_path / "want"), out], timeout=300)
    assert list(np.fromfile(out + ".counts", np.uint64)) == [st[0]]
    assert np.array_equal(np.fromfile(out + ".xyz", np.uint32).reshape(-1, 3), want_xyz.view(np.uint32))
    assert np.array_equal(np.fromfile(out + ".rgb", np.uint8).reshape(-1, 3), want_rgb)
    # the Python facade gives the same
    for sort in (False, True):
        pc = pkg.ProjectCloud(xyzw, rgba, reorder=sort, point_ids=True)
        index, dist2 = pc.nearestPoints(gx, r)
        assert nf.same((index, dist2), (gi, gd))
        index, dist2, xyz, rgb = pc.matchPoints(gx[:, :3], r)
        assert nf.same((index, dist2), (gi, gd))
        assert xyz.dtype == np.float32 and np.array_equal(xyz.view(np.uint32), want_xyz.view(np.uint32)) and np.array_equal(rgb, want_rgb)
        none = pc.matchPoints(gx[:5] + np.float32(100), r)  # (nothing within radius: rows of zeros, no extract)
        assert (none[0] == nf.NONE).all() and np.isinf(none[1]).all() and not none[2].any() and not none[3].any()
