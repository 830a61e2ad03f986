"""rtr_select_clusters in C++ (include/rtr.h section 6i).  CPU: the facade's calls of include/rtr_project_cloud.hpp
compiled and linked against librtr_hip.so.  GPU: selectClusters, growSelection and removeSmallClusters give the
reference's words, labels, counts and cloud (the program compares the words with files the reference wrote), and the
Python facade gives the same."""
import os
import subprocess

import numpy as np
import pytest

import clusters_ref as cr
from conftest import ROOT


def _build(tmp_path, pkg):
    exe = str(tmp_path / "clusters_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "clusters_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_clusters_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


@pytest.mark.gpu
def test_cpp_clusters_match_the_reference(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n = 30_001
    xyzw, rgba = orc.generate("room_shell", 15, 0, n, n)
    r0, r1, k0, k1, m1 = np.float32(0.07), np.float32(0.09), 2, 2, 49
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "params.bin", "wb") as f:
        f.write(np.float32([r0, r1]).tobytes())
        f.write(np.uint32([k0, k1, m1]).tobytes())
    lab0, lab1 = cr.labels(xyzw, r0), cr.labels(xyzw, r1)
    hit0, hit1 = cr.hits(lab0, k0), cr.hits(lab1, k1, m1)
    assert 0.05 * n < hit0.sum() < 0.95 * n and 0.05 * n < hit1.sum() < 0.95 * n
    planes = np.float32([[1, 0, 0, -3.2]])
    seeds = pkg.clip_keep(planes, xyzw)
    grown = cr.hits(lab1, seeds=seeds)
    assert 0 < seeds.sum() < grown.sum() < n // 2
    steps = [hit0, hit0 | ~hit1, grown, grown & cr.hits(lab0, k0, seeds=grown)]
    assert 0 < steps[3].sum() < grown.sum()
    for k, want in enumerate(steps):
        cr.words(want).tofile(tmp_path / ("want.words%d" % k))
    lab0.tofile(tmp_path / "want.labels")
    out = str(tmp_path / "out")
    subprocess.check_call([exe, str(tmp_path / "cloud.bin"), str(tmp_path / "params.bin"), str(tmp_path / "want"), out], timeout=300)
    counts = np.fromfile(out + ".counts", np.uint64)
    assert list(counts) == [s.sum() for s in steps] + [steps[3].sum(), (~hit0).sum(), hit0.sum()]
    left = np.fromfile(out + ".xyz", np.float32).reshape(-1, 3)
    assert np.array_equal(left.view(np.uint32), np.ascontiguousarray(xyzw[hit0, :3]).view(np.uint32))  # the cloud left == A[hit]
    # the Python facade gives the same
    pc = pkg.ProjectCloud(xyzw, rgba, point_ids=True)
    assert pc.selectClusters(r0, k0) == int(hit0.sum()) == pc.selectedCount()
    assert np.array_equal(pc.projector.download(pkg._lib.BUF_SELECTION), cr.words(hit0))
    assert pc.selectClusters(r1, k1, m1, op="add", outside=True) == int(steps[1].sum())
    assert pc.projector.select_points(planes=planes)[0] == int(seeds.sum())
    assert pc.growSelection(r1) == int(grown.sum())
    assert pc.selectClusters(r0, k0, seeded=True, op="intersect") == int(steps[3].sum())
    assert np.array_equal(pc.projector.download(pkg._lib.BUF_SELECTION), cr.words(steps[3]))
    assert pc.removeSmallClusters(r0, k0) == int((~hit0).sum()) and pc.projector.num_points == int(hit0.sum())
    assert pc.projector.selection() is None
    got = pc.projector.extract_points()
    assert np.array_equal(np.ascontiguousarray(got[0][:, :3]).view(np.uint32), np.ascontiguousarray(xyzw[hit0, :3]).view(np.uint32))
