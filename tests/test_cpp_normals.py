"""rtr_estimate_normals in C++ (include/rtr_normals.h section 6o).  CPU: csrc/rtr_normal_fit.h -- the lines the rows kernel
runs per lane -- built with g++ as a stand-alone program (tests/cpp/normal_fit_check.cpp), plainly and again with
-fsanitize=address,undefined: the row against a sort by (d2, index) in every order of arrival, and normal_fit on the rows
and coordinates of every case of normals_cases.py, dumped by the numpy reference and compared with it bit for bit;
sqrt_rn must equal the host's sqrt on every argument seen.  The facade's call of include/rtr_project_cloud.hpp compiled
and linked against librtr_hip.so (tests/cpp/normals_facade_check.cpp).  GPU: estimateNormals through both facades gives
the reference's bits."""
import os
import subprocess

import numpy as np
import pytest

import normals_cases as ncs
import normals_ref as nf
from conftest import ROOT

CSRC = os.path.join(ROOT, "real-time-neural-rendering-of-lidar-point-clouds_amd", "csrc")
f32 = np.float32
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _build_fit(tmp_path, flags):
    exe = str(tmp_path / "normal_fit_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", *flags, "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "normal_fit_check.cpp"), "-o", exe])
    return exe


def _run(exe, args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    return out.stdout


def dump_case(path, xyz, idx, found, viewpoint):
    """The input of normal_fit_check: the coordinates and the reference's rows."""
    n, k = idx.shape
    with open(path, "wb") as f:
        f.write(np.uint64(n).tobytes() + np.uint32([k, viewpoint is not None]).tobytes())
        f.write(f32(viewpoint if viewpoint is not None else (0, 0, 0)).tobytes())
        f.write(np.ascontiguousarray(xyz[:, :3], f32).tobytes() + np.ascontiguousarray(found, np.uint32).tobytes())
        f.write(np.ascontiguousarray(idx, np.uint32).tobytes())


@pytest.mark.parametrize("flags", [(), SANITIZE], ids=["plain", "asan_ubsan"])
def test_the_row_equals_a_sort_by_distance_and_index(tmp_path, flags):
    out = _run(_build_fit(tmp_path, flags), ["40"])
    assert "40 trials per k" in out and int(out.split()[0]) >= 6 * (9 * 40 + 72)


@pytest.mark.parametrize("flags", [(), SANITIZE], ids=["plain", "asan_ubsan"])
def test_normal_fit_equals_the_numpy_reference_bit_for_bit(tmp_path, orc, flags):
    exe = _build_fit(tmp_path, flags)
    cases = [(name, xyz, r, ks, vp) for name, xyz, r, ks, vp in ncs.special_cases()]
    cases.append(("dense", ncs.dense_cloud(), ncs.DENSE_RADIUS, (ncs.DENSE_K,), None))
    if not flags:  # (the scenes once: the sanitizer's build runs the special clouds and the dense one)
        for scene, (n, radii) in ncs.SCENES.items():
            xyz = np.ascontiguousarray(orc.generate(scene, ncs.SEED, 0, n, n)[0][:, :3])
            cases += [("%s@%g" % (scene, r), xyz, r, ncs.KS, ncs.SCENE_VIEWPOINT) for r in radii]
    roots = 0
    for name, xyz, r, ks, vp in cases:
        rk = nf.rows(xyz, r, max(ks))
        for k in ks:
            for view in (vp, None) if vp is not None else (None, (0.5, -0.25, 2.0)):
                e = nf.estimate(xyz, r, k, view, rows_k=rk)
                dump_case(tmp_path / "in.bin", xyz, e["index"], e["found"], view)
                out = _run(exe, ["1", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
                roots += int(out.split()[-3])
                n = xyz.shape[0]
                raw = open(tmp_path / "out.bin", "rb").read()
                assert len(raw) == 17 * n
                got_n = np.frombuffer(raw[:12 * n], f32).reshape(n, 3)
                got_c = np.frombuffer(raw[12 * n:16 * n], f32)
                got_f = np.frombuffer(raw[16 * n:], np.uint8) != 0
                what = (name, k, view)
                assert nf.same_bits(got_n, e["normals"]), (what, np.flatnonzero((nf.bits(got_n) != nf.bits(e["normals"])).any(axis=1))[:5])
                assert nf.same_bits(got_c, e["curvature"]), what
                assert np.array_equal(got_f, e["flipped"]), what
    assert roots > 100_000  # (sqrt_rn returned the host's sqrt for every one of them, or the program had failed)


def test_fit_header_is_plain_cpp_and_the_kernel_uses_it():
    src = open(os.path.join(CSRC, "rtr_normal_fit.h")).read()
    for name in ("bool normal_row_insert(Row &row, uint32_t k, NormalRowState &st, const IndexOf &index_of, float d2, uint32_t pos, uint32_t u)",
                 "void normal_row_sort(Row &row, uint32_t count, const IndexOf &index_of)", "double sqrt_rn(double x)",
                 "bool normal_fit(const double S[3], const double Q[6], uint32_t m, const float p[3], bool towards, const float view[3], float normal[3],",
                 "fma(-y0, yu, x) > 0.0", "fma(-y0, yd, x) <= 0.0", "kNormalFitSweeps = 8"):
        assert name in src, name
    assert "__global__" not in src and "#include <hip" not in src and "__shared__" not in src
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert code.count("fma(") == 2  # (sqrt_rn's two residuals: nothing else is fused)
    assert "sqrt(" in code and code.count(" sqrt(") == 1  # (the builtin is called in sqrt_rn alone)
    kern = open(os.path.join(CSRC, "rtr_normals.hip")).read()
    for use in ('#include "rtr_normal_fit.h"', "normal_row_insert(row, k, st, index_of, d2, c0 + (uint32_t)j, cu)", "normal_row_sort(row, st.count, index_of)",
                "normal_fit(S, Q, st.count + 1u, p, with_view != 0, view, nrm, &curv)", "pair_dist2(x, y, z, cx, cy, cz)",
                "f_sub(x, c.x)", "k_nb_normal_rows"):
        assert use in kern, use
    assert "atomicAdd(float" not in kern and "atomicAdd(double" not in kern and "unsafeAtomicAdd" not in kern and "atomicAdd((float" not in kern
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("rtr_normals.hip") >= 3 and "rtr_normal_fit.h" in mk and "resource_usage_normals.txt" in mk


def _build(tmp_path, pkg):
    exe = str(tmp_path / "normals_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "normals_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_normals_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


@pytest.mark.gpu
def test_estimate_normals_through_both_facades_matches_the_reference(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n = 30_001
    xyzw, rgba = orc.generate("room_shell", 15, 0, n, n)
    r, k, view = f32(0.12), 8, f32([0.5, -0.25, 1.0])
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "params.bin", "wb") as f:
        f.write(f32([r]).tobytes() + np.uint32([k]).tobytes() + view.tobytes())
    rk = nf.rows(xyzw, r, k)
    e, e2 = nf.estimate(xyzw, r, k, None, rows_k=rk), nf.estimate(xyzw, r, k, view, rows_k=rk)
    assert 0 < (e["found"] < k).sum() < n and e["stats"][0] > n // 2 and 0 < e2["stats"][3] < e2["stats"][0]
    out = str(tmp_path / "out")
    subprocess.check_call([exe, str(tmp_path / "cloud.bin"), str(tmp_path / "params.bin"), out], timeout=300)
    assert list(np.fromfile(out + ".counts", np.uint64)) == [e["stats"][0], e2["stats"][0], 0, 0]
    assert nf.same_bits(np.fromfile(out + ".normals", f32).reshape(n, 3), e["normals"])
    assert nf.same_bits(np.fromfile(out + ".curvature", f32), e["curvature"])
    assert np.array_equal(np.fromfile(out + ".found", np.uint32), e["found"])
    assert nf.same_bits(np.fromfile(out + ".normals2", f32).reshape(n, 3), e2["normals"])
    assert nf.same_bits(np.fromfile(out + ".curvature2", f32), e2["curvature"])
    pc = pkg.ProjectCloud(xyzw, rgba, point_ids=True)
    nrm, curv = pc.estimateNormals(k, r)
    assert nf.same_bits(nrm, e["normals"]) and nf.same_bits(curv, e["curvature"])
    nrm, curv = pc.estimateNormals(k, r, viewpoint=view)
    assert nf.same_bits(nrm, e2["normals"]) and nf.same_bits(curv, e2["curvature"])
    assert pc.projector.selection() is None and pc.selectedCount() == 0
