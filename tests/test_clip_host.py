"""Clip planes (include/rtr.h section 6d) on the host: the C ABI surface, the Python and C++ surfaces, and the numpy
float32 reference the GPU tests compare with -- camera.clip_box_planes keeps exactly lo <= p <= hi."""
import os
import re
import subprocess

import numpy as np

from conftest import ROOT


def test_header_declares_the_clip_planes(pkg, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    assert re.search(r"#define RTR_MAX_CLIP_PLANES 8\b", hdr)
    assert re.search(r"int rtr_set_clip_planes\(rtr_ctx \*ctx, int count, const float \*planes\);", hdr)
    assert re.search(r"int rtr_get_clip_planes\(rtr_ctx \*ctx, int \*count, float \*planes\);", hdr)
    assert re.search(r"#define RTR_ABI_VERSION 2\b", hdr)
    L = pkg._lib
    for name in ("rtr_set_clip_planes", "rtr_get_clip_planes"):
        assert name in L.SYMBOLS and hasattr(L.lib(), name)
    assert L.MAX_CLIP_PLANES == 8
    src = tmp_path / "clip_abi.c"
    src.write_text('#include "rtr.h"\n#include <stdio.h>\n'
                   'int main(void) { float pl[RTR_MAX_CLIP_PLANES * 4] = {1, 0, 0, 0}; int n = 0;\n'
                   '  int (*set)(rtr_ctx *, int, const float *) = rtr_set_clip_planes;\n'
                   '  int (*get)(rtr_ctx *, int *, float *) = rtr_get_clip_planes;\n'
                   '  printf("%d %d %d\\n", RTR_MAX_CLIP_PLANES, set(NULL, 1, pl), get(NULL, &n, pl)); return 0; }\n')
    exe = tmp_path / "clip_abi"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + lib_dir, "-lrtr_hip", "-Wl,-rpath," + lib_dir])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert out == ["8", str(L.RTR_ERR_INVALID), str(L.RTR_ERR_INVALID)]  # (a NULL context is refused without a GPU)


def test_python_and_cpp_surfaces_exist(pkg):
    for name in ("set_clip_planes", "clip_planes"):
        assert callable(getattr(pkg.Projector, name))
    for name in ("setClipPlanes", "setClipBox", "clearClip"):
        assert callable(getattr(pkg.ProjectCloud, name))
    assert callable(pkg.clip_box_planes) and callable(pkg.clip_keep)
    hpp = open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read()
    for sig in (r"void setClipPlanes\(const float\* planes, int count\)",
                r"void setClipBox\(const float lo\[3\], const float hi\[3\], const double\* M = nullptr\)",
                r"void clearClip\(\)"):
        assert re.search(sig, hpp), sig


def _specials():
    f = np.float32
    den = np.array([1, 0x80000001, 0x007FFFFF, 0x807FFFFF], np.uint32).view(np.float32)
    return np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 0.5, -2.0, 1e30, -1e30, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan,
                                     np.nextafter(f(1), f(2)), np.nextafter(f(1), f(0)), np.nextafter(f(-1), f(0))],
                                    np.float32), den])


def test_clip_box_planes_keep_exactly_the_box(pkg):
    rng = np.random.default_rng(7)
    sp = _specials()
    finite = sp[np.isfinite(sp)]
    for trial in range(300):
        lo = rng.choice(finite, 3)
        hi = rng.choice(finite, 3)
        lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
        planes = pkg.clip_box_planes(lo, hi)
        assert planes.dtype == np.float32 and planes.shape == (6, 4)
        n = 400
        p = rng.choice(sp, (n, 3))
        faces = rng.integers(0, 3, (n, 3))  # a third of the coordinates exactly on a face
        p = np.where(faces == 1, lo[None, :], np.where(faces == 2, hi[None, :], p)).astype(np.float32)
        want = np.all((lo[None, :] <= p) & (p <= hi[None, :]), axis=1)
        got = pkg.clip_keep(planes, p)
        assert np.array_equal(got, want), (trial, lo, hi)
    # random boxes and points at ordinary magnitudes, faces included
    lo = np.array([-1.5, 0.25, -3.0], np.float32)
    hi = np.array([2.0, 0.75, -1.0], np.float32)
    p = rng.uniform(-4, 4, (100000, 3)).astype(np.float32)
    p[:3000, 0] = lo[0]
    p[3000:6000, 2] = hi[2]
    want = np.all((lo <= p) & (p <= hi), axis=1)
    assert np.array_equal(pkg.clip_keep(pkg.clip_box_planes(lo, hi), p), want)


def test_clip_box_planes_oriented(pkg):
    # a world->box matrix: rotation about z by 30 degrees and a shift; the planes are the box's rows rounded once
    a = np.deg2rad(30.0)
    M = np.eye(4)
    M[:2, :2] = [[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]]
    M[:3, 3] = [0.5, -0.25, 1.0]
    lo, hi = np.array([-1.0, -0.5, 0.0]), np.array([1.0, 0.5, 2.0])
    planes = pkg.clip_box_planes(lo, hi, M)
    assert planes.dtype == np.float32 and planes.shape == (6, 4)
    assert np.array_equal(planes[0], np.float32([M[0, 0], M[0, 1], M[0, 2], M[0, 3] - lo[0]]))
    assert np.array_equal(planes[1], np.float32([-M[0, 0], -M[0, 1], -M[0, 2], hi[0] - M[0, 3]]))
    rng = np.random.default_rng(3)
    p = rng.uniform(-3, 3, (200000, 3))
    q = p @ M[:3, :3].T + M[:3, 3]
    inside = np.all((lo + 1e-4 <= q) & (q <= hi - 1e-4), axis=1)
    outside = np.any((q < lo - 1e-4) | (q > hi + 1e-4), axis=1)
    keep = pkg.clip_keep(planes, p.astype(np.float32))
    assert keep[inside].all() and not keep[outside].any()
    assert inside.sum() > 1000 and outside.sum() > 1000
