"""Appending points to the resident cloud (include/rtr.h section 2b), the parts a CPU can check: the exported symbol,
the header declaration (a new entry point, no struct change: ABI version 2), the Python methods, and the C++ facade's
appendPoints compiled and linked with plain g++ (tests/cpp/append_facade_check.cpp)."""
import os
import re
import subprocess

from conftest import ROOT


def test_append_symbol_exported(pkg):
    L = pkg._lib
    assert "rtr_append_points" in L.SYMBOLS
    getattr(L.lib(), "rtr_append_points")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert re.search(r"\bT rtr_append_points$", nm, re.M)


def test_append_header_declaration():
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    assert re.search(r"int rtr_append_points\(rtr_ctx \*ctx, const float \*xyz, size_t xyz_stride_bytes, const uint8_t \*rgb,"
                     r"\s+size_t rgb_stride_bytes, size_t m\);", hdr)
    assert "#define RTR_ABI_VERSION 2" in hdr
    assert "2b. appending points" in hdr


def test_append_python_methods(pkg):
    assert callable(pkg.Projector.append_points)
    for name in ("appendPoints", "appendGrid"):
        assert callable(getattr(pkg.ProjectCloud, name))


def test_append_facade_compiles_and_links(tmp_path, pkg):
    exe = str(tmp_path / "append_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "append_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    assert os.path.exists(exe)
