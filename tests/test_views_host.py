"""rtr_render_views on the host side (include/rtr.h section 6c): declared, exported, argument checks that need no GPU,
and the Python / C++ surfaces that sit on it."""
import ctypes as C
import os
import re

from conftest import ROOT


def test_views_declared_in_header():
    h = open(os.path.join(ROOT, "include", "rtr.h")).read()
    assert re.search(r"#define RTR_MAX_VIEWS 8\b", h)
    assert re.search(r"int rtr_render_views\(rtr_ctx \*ctx, int count, const float \*P, int with_filter\);", h)
    for name, value in (("RTR_BUF_VIEW_DEPTH", 8), ("RTR_BUF_VIEW_IMAGE", 9), ("RTR_BUF_VIEW_TENSOR", 10),
                        ("RTR_BUF_VIEW_MINMAX", 11)):
        assert re.search(r"\b%s = %d\b" % (name, value), h), name
    assert re.search(r"#define RTR_ABI_VERSION 2\b", h)


def test_views_exported(pkg):
    L = pkg._lib
    assert "rtr_render_views" in L.SYMBOLS
    lib = C.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "rtr_render_views")
    assert (L.BUF_VIEW_DEPTH, L.BUF_VIEW_IMAGE, L.BUF_VIEW_TENSOR, L.BUF_VIEW_MINMAX) == (8, 9, 10, 11)
    assert L.MAX_VIEWS == 8


def test_views_null_context(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    lib.rtr_render_views.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    P = (C.c_float * 32)()
    assert lib.rtr_render_views(None, 2, P, 0) == pkg._lib.RTR_ERR_INVALID
    assert lib.rtr_render_views(None, 0, None, 1) == pkg._lib.RTR_ERR_INVALID


def test_views_python_surface(pkg):
    assert callable(getattr(pkg.Projector, "render_views", None))
    assert callable(getattr(pkg.ProjectCloud, "computeFullViews", None))


def test_views_cpp_facade_declares_methods():
    h = open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read()
    assert "int computeRGBDViews(" in h and "int computeFilteredRGBDViews(" in h
