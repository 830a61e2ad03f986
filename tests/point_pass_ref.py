"""Reference answers of the point pass (include/rtr.h section 6b) from the oracle's projection.

`point_pass` runs tests/cpp/point_pass_ref.c (built once per session with the system C compiler against the oracle's
shared library); `point_pass_py` is the same definition as a Python loop over orc.project_point, for small clouds --
the cross-check of the C helper."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_POINT = 0xFFFFFFFF
_lib = None


def _helper(orc):
    global _lib
    if _lib is None:
        orc_so = orc.build()
        out = os.path.join(tempfile.mkdtemp(prefix="point_pass_ref_"), "libpoint_pass_ref.so")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                               "-shared", os.path.join(ROOT, "tests", "cpp", "point_pass_ref.c"), "-o", out, orc_so,
                               "-Wl,-rpath," + os.path.dirname(orc_so)])
        L = C.CDLL(out)
        L.ppr_point_pass.restype = None
        L.ppr_point_pass.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                     C.c_float, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def point_pass(orc, xyz, P, W, H, depth_bits, window=0.02):
    """-> (ids uint32 [H, W], vis uint32 [(n + 31) // 32]) for the frame `depth_bits` (uint32 [H, W])."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(16)
    depth = np.ascontiguousarray(depth_bits, dtype=np.uint32).reshape(-1)
    n = xyz.shape[0]
    ids = np.empty(W * H, np.uint32)
    vis = np.empty(max((n + 31) // 32, 1), np.uint32)
    _helper(orc).ppr_point_pass(_p(xyz), xyz.strides[0], n, _p(P), W, H, _p(depth), C.c_float(window), _p(ids), _p(vis))
    return ids.reshape(H, W), vis[:(n + 31) // 32]


def point_pass_py(orc, xyz, P, W, H, depth_bits, window=0.02):
    """The definition, point by point (slow: a few thousand points)."""
    depth = np.asarray(depth_bits, np.uint32).reshape(-1)
    n = xyz.shape[0]
    ids = np.full(W * H, NO_POINT, np.uint32)
    vis = np.zeros((n + 31) // 32, np.uint32)
    w = np.float32(window)
    for i in range(n):
        pix, bits = orc.project_point(P, float(xyz[i, 0]), float(xyz[i, 1]), float(xyz[i, 2]), W, H)
        if pix < 0:
            continue
        m = depth[pix]
        if bits == m and i < ids[pix]:
            ids[pix] = i
        d = np.uint32(bits).view(np.float32)
        lim = np.float32(np.uint32(m).view(np.float32) + w)
        if not (d > lim):
            vis[i // 32] |= np.uint32(1 << (i % 32))
    return ids.reshape(H, W), vis


def unpack(vis, n):
    """bool [n] from the mask words."""
    return np.unpackbits(np.ascontiguousarray(vis, "<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


# ---- clouds with the cases the definitions single out -----------------------------------------------------------
EDGE_P = np.array([[100, 0, 160, 0], [0, 100, 120, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)  # r.z = z exactly


def edge_cloud(seed, window=0.02):
    """Stacks of points on the pixels of EDGE_P (320 x 240): a front point at z0 and points at exactly
    z0 + window (visible: the test is d > depth + window), the next float above it (not visible) and the one below.
    -> (xyzw float32 [n, 4], rgba uint8 [n, 4])"""
    rng = np.random.default_rng(seed)
    w = np.float32(window)
    pts = []
    for a in range(-60, 61, 7):
        for b in range(-50, 51, 9):
            z0 = np.float32(rng.uniform(1.0, 4.0))
            edge = np.float32(z0 + w)
            for z in (z0, edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(0)), edge):
                pts.append((np.float32(np.float32(a / 100.0) * z), np.float32(np.float32(b / 100.0) * z), z))
    xyzw = np.ones((len(pts), 4), np.float32)
    xyzw[:, :3] = np.array(pts, np.float32)
    perm = rng.permutation(len(pts))
    xyzw = xyzw[perm]
    rgba = rng.integers(0, 256, (len(pts), 4), dtype=np.uint8)
    rgba[:, 3] = 255
    return xyzw, rgba


def hot_cloud(orc, seed, n_base=3000, copies=5000):
    """n_base room points plus `copies` copies of one of them, shuffled: the copies tie on their pixel and the ID
    must be the smallest upload index among them.  -> (xyzw, rgba, indices of the copies)"""
    xyzw, rgba = orc.generate("room_shell", seed, 0, n_base, n_base)
    rng = np.random.default_rng(seed)
    hot = rng.integers(0, n_base)
    xyzw = np.concatenate([xyzw, np.repeat(xyzw[hot:hot + 1], copies, 0)])
    rgba = np.concatenate([rgba, np.repeat(rgba[hot:hot + 1], copies, 0)])
    perm = rng.permutation(len(xyzw))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    copies_at = np.sort(np.concatenate([[inv[hot]], inv[n_base:]]))
    return np.ascontiguousarray(xyzw[perm]), np.ascontiguousarray(rgba[perm]), copies_at
