"""The point pass (include/rtr.h section 6b) on the host: its C ABI surface, and the reference answer the GPU tests
compare with -- the C helper (tests/cpp/point_pass_ref.c) against the definitions written as a Python loop, and
against what the oracle's own frame says (visible points per pixel = its count accumulator, their colours = its
colour sums, an ID's point lands on its pixel with the pixel's depth bits)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import point_pass_ref as ppr


def test_header_declares_the_point_pass(pkg, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    assert re.search(r"int rtr_point_pass\(rtr_ctx \*ctx, const float P\[16\], int what\);", hdr)
    assert re.search(r"RTR_BUF_POINT_ID = 6\b", hdr) and re.search(r"RTR_BUF_VISIBLE = 7\b", hdr)
    assert re.search(r"#define RTR_POINTS_IDS 1\b", hdr) and re.search(r"#define RTR_POINTS_VISIBLE 2\b", hdr)
    L = pkg._lib
    assert "rtr_point_pass" in L.SYMBOLS and hasattr(L.lib(), "rtr_point_pass")
    assert (L.BUF_POINT_ID, L.BUF_VISIBLE, L.POINTS_IDS, L.POINTS_VISIBLE, L.NO_POINT) == (6, 7, 1, 2, 0xFFFFFFFF)
    src = tmp_path / "pp_abi.c"
    src.write_text('#include "rtr.h"\n#include <stdio.h>\n'
                   'int main(void) { int (*fn)(rtr_ctx *, const float *, int) = rtr_point_pass; rtr_buffer b = RTR_BUF_VISIBLE;\n'
                   '  printf("%d %d %d %d %d\\n", (int)RTR_BUF_POINT_ID, (int)b, RTR_POINTS_IDS, RTR_POINTS_VISIBLE,\n'
                   '         fn(NULL, NULL, RTR_POINTS_IDS)); return 0; }\n')
    exe = tmp_path / "pp_abi"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + lib_dir, "-lrtr_hip", "-Wl,-rpath," + lib_dir])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert out == ["6", "7", "1", "2", str(L.RTR_ERR_INVALID)]  # (a NULL context is refused without a GPU)


def _frames(orc, xyzw, rgba, P, W, H):
    ref = orc.project(xyzw, rgba, P, W, H)
    out = [("unfiltered", ref["depth_bits"], ref)]
    if W % 16 == 0 and H >= 16:
        out.append(("filtered", orc.filter(ref["depth_bits"], ref["img"])["depth"].view(np.uint32), None))
    return out


def _clouds(orc, pkg):
    W, H = 64, 48
    for seed, n in ((1, 1), (2, 37), (3, 1500), (4, 4099)):
        xyzw, rgba = orc.generate("room_shell", seed, 0, n, n)
        yield "room%d" % n, xyzw, rgba, pkg.orbit_projection(seed * 97, W, H), W, H
    xyzw, rgba = orc.generate("uniform_box", 9, 0, 3000, 3000)
    yield "box", xyzw, rgba, pkg.orbit_projection(5, W, H), W, H
    xyzw, rgba, _ = ppr.hot_cloud(orc, 11, n_base=800, copies=1200)
    yield "hot", xyzw, rgba, pkg.orbit_projection(11, W, H), W, H
    xyzw, rgba = ppr.edge_cloud(12)
    yield "edge", xyzw, rgba, ppr.EDGE_P, 320, 240


def test_reference_helper_equals_the_definition(pkg, orc):
    for name, xyzw, rgba, P, W, H in _clouds(orc, pkg):
        for kind, depth, _ in _frames(orc, xyzw, rgba, P, W, H):
            ids, vis = ppr.point_pass(orc, xyzw, P, W, H, depth)
            ids_py, vis_py = ppr.point_pass_py(orc, xyzw, P, W, H, depth)
            assert np.array_equal(ids, ids_py), (name, kind)
            assert np.array_equal(vis, vis_py), (name, kind)
            n = len(xyzw)
            assert not (vis[-1] >> np.uint32(n % 32)).any() if n % 32 else True  # (no bit past n)


def test_reference_helper_agrees_with_the_oracle_frame(pkg, orc):
    seen_tie = seen_edge = False
    for name, xyzw, rgba, P, W, H in _clouds(orc, pkg):
        for kind, depth, ref in _frames(orc, xyzw, rgba, P, W, H):
            ids, vis = ppr.point_pass(orc, xyzw, P, W, H, depth)
            v = ppr.unpack(vis, len(xyzw))
            pix = np.array([orc.project_point(P, *map(float, xyzw[i, :3]), W, H)[0] for i in np.nonzero(v)[0]], np.int64)
            assert (pix >= 0).all()
            if ref is not None:  # unfiltered: the visible points are exactly what the accumulate pass counted
                cnt = np.bincount(pix, minlength=W * H)
                assert np.array_equal(cnt, ref["acc"][..., 3].reshape(-1)), name
                for ch in range(3):
                    s = np.bincount(pix, weights=rgba[np.nonzero(v)[0], ch].astype(np.float64), minlength=W * H)
                    assert np.array_equal(s.astype(np.uint64), ref["acc"][..., ch].reshape(-1).astype(np.uint64)), name
            else:  # filtered: removed pixels show no point and hold no visible one
                removed = depth.reshape(-1) == np.float32(-1.0).view(np.uint32)
                assert (ids.reshape(-1)[removed] == ppr.NO_POINT).all() and not removed[pix].any()
            lit = np.nonzero(ids.reshape(-1) != ppr.NO_POINT)[0]
            for p in lit:
                i = int(ids.reshape(-1)[p])
                q, bits = orc.project_point(P, *map(float, xyzw[i, :3]), W, H)
                assert q == p and bits == depth.reshape(-1)[p]
            d = depth.reshape(-1)
            assert ((d[lit] != 0x7F7FFFFF) & (d[lit] != np.float32(-1.0).view(np.uint32))).all()
            if name == "hot":
                seen_tie = True
            if name == "edge" and ref is not None:
                # the stacks: z0 visible, z0 + window visible (twice), the float above not
                assert v.sum() == 4 * len(xyzw) // 5
                seen_edge = True
    assert seen_tie and seen_edge


def _build_facade_check(tmp_path, pkg):
    exe = str(tmp_path / "point_ids_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "point_ids_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH)])
    return exe


def test_facade_point_ids_compile_and_link(tmp_path, pkg):
    assert os.path.exists(_build_facade_check(tmp_path, pkg))
