"""Reference answers of rtr_select_points (include/rtr.h section 6f): the planes from camera.clip_keep (numpy float32),
the rectangle from the oracle's projection, point by point (tests/cpp/select_ref.c, built once per session against the
oracle's shared library)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def _helper(orc):
    global _lib
    if _lib is None:
        orc_so = orc.build()
        out = os.path.join(tempfile.mkdtemp(prefix="select_ref_"), "libselect_ref.so")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                               "-shared", os.path.join(ROOT, "tests", "cpp", "select_ref.c"), "-o", out, orc_so,
                               "-Wl,-rpath," + os.path.dirname(orc_so)])
        L = C.CDLL(out)
        L.sref_pixels.restype = None
        L.sref_pixels.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib = L
    return _lib


def pixels(orc, xyz, P, W, H):
    """int64 [n]: the pixel id the oracle's projection gives each point, -1 for none."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(16)
    pix = np.empty(xyz.shape[0], np.int64)
    _helper(orc).sref_pixels(xyz.ctypes.data_as(C.c_void_p), xyz.strides[0], xyz.shape[0], P.ctypes.data_as(C.c_void_p),
                             W, H, pix.ctypes.data_as(C.c_void_p))
    return pix


def inside(pkg, orc, xyz, planes=None, P=None, rect=None, W=0, H=0):
    """bool [n]: the predicate of section 6f."""
    n = xyz.shape[0]
    out = np.ones(n, bool)
    if planes is not None and len(planes):
        out &= pkg.clip_keep(planes, xyz)
    if P is not None:
        pix = pixels(orc, xyz, P, W, H)
        px, py = pix % W, pix // W
        x0, y0, x1, y1 = rect
        out &= (pix >= 0) & (px >= x0) & (px < x1) & (py >= y0) & (py < y1)
    return out


def words(sel):
    n = sel.size
    return np.packbits(np.concatenate([sel, np.zeros(-n % 32, bool)]), bitorder="little").view("<u4").copy()


def unpack(w, n):
    return np.unpackbits(np.ascontiguousarray(w, "<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


def combine(op, sel, hit):
    return {"replace": hit, "add": sel | hit, "subtract": sel & ~hit, "intersect": sel & hit, "toggle": sel ^ hit}[op]
