"""ctypes/numpy wrapper around the CPU oracle (oracle/rtr_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and the
cpu_baseline leg of bench.py.  The product package never imports this module.
The reference has no fixtures; `ref(variant)` loads its own kernels compiled for the host
(oracle/ref_build.py -> oracle/_ref/), which is what pins the oracle.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "librtr_oracle.so")
EMPTY_DEPTH = 0x7F7FFFFF
SCENES = {"uniform_box": 0, "room_shell": 1}


class Params(C.Structure):
    _fields_ = [("depth_window", C.c_float), ("filter_strength", C.c_float),
                ("gradient_threshold", C.c_float), ("levels", C.c_int)]


def build(force=False):
    src = os.path.join(_HERE, "rtr_oracle.c")
    if force or not os.path.exists(_LIB_PATH) or os.path.getmtime(_LIB_PATH) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", _HERE, "-s", "-B"])
    return _LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            build()
        L = C.CDLL(_LIB_PATH)
        L.orc_selftest.restype = C.c_int
        L.orc_project_point.restype = C.c_int64
        L.orc_project_point.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p]
        L.orc_f32_to_f16.restype = C.c_uint16
        L.orc_f32_to_f16.argtypes = [C.c_float]
        L.orc_f16_to_f32.restype = C.c_float
        L.orc_f16_to_f32.argtypes = [C.c_uint16]
        L.orc_generate.restype = C.c_int
        L.orc_generate.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
        L.orc_filter.restype = C.c_int
        L.orc_project_mt.restype = C.c_int
        L.orc_envelope_points.restype = C.c_int
        L.orc_project_variant.restype = C.c_int
        _lib = L
        assert L.orc_selftest() == 1, "oracle build violates the arithmetic contract"
    return _lib


def default_params():
    p = Params()
    lib().orc_default_params(C.byref(p))
    return p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _P(P):
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(16)
    return P


def compose_projection(K, E):
    K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    E = np.ascontiguousarray(E, dtype=np.float64).reshape(16)
    P = np.empty(16, np.float32)
    lib().orc_compose_projection(_ptr(K), _ptr(E), _ptr(P))
    return P


def project_point(P, x, y, z, W, H):
    """-> (pixel id or -1, depth bits)"""
    P = _P(P)
    bits = C.c_uint32(0)
    pix = lib().orc_project_point(_ptr(P), x, y, z, W, H, C.addressof(bits))
    return int(pix), int(bits.value)


def generate(scene, seed, first, count, total):
    """-> (xyzw float32 [count,4], rgba uint8 [count,4])"""
    sc = SCENES[scene] if isinstance(scene, str) else int(scene)
    xyzw = np.empty((count, 4), np.float32)
    rgba = np.empty((count, 4), np.uint8)
    rc = lib().orc_generate(sc, seed, first, count, total, _ptr(xyzw), _ptr(rgba))
    if rc != 0:
        raise ValueError("orc_generate failed")
    return xyzw, rgba


def _cloud(xyz, rgb):
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 2 and xyz.shape[1] in (3, 4)
    xyz = np.ascontiguousarray(xyz)
    if rgb is not None:
        rgb = np.asarray(rgb)
        assert rgb.dtype == np.uint8 and rgb.ndim == 2 and rgb.shape[1] in (3, 4) and rgb.shape[0] == xyz.shape[0]
        rgb = np.ascontiguousarray(rgb)
    return xyz, rgb


def clear(W, H):
    depth = np.full(W * H, EMPTY_DEPTH, np.uint32)
    acc = np.zeros(W * H * 4, np.uint32)
    return depth, acc


def min_depth_pass(xyz, P, W, H, depth):
    xyz, _ = _cloud(xyz, None)
    P = _P(P)
    lib().orc_min_depth_pass(_ptr(xyz), C.c_size_t(xyz.strides[0]), C.c_size_t(xyz.shape[0]), _ptr(P),
                             W, H, _ptr(depth))
    return depth


def accumulate_pass(xyz, rgb, P, W, H, depth, acc, window=None):
    xyz, rgb = _cloud(xyz, rgb)
    P = _P(P)
    w = default_params().depth_window if window is None else window
    lib().orc_accumulate_pass(_ptr(xyz), C.c_size_t(xyz.strides[0]), _ptr(rgb), C.c_size_t(rgb.strides[0]),
                              C.c_size_t(xyz.shape[0]), _ptr(P), W, H, _ptr(depth), _ptr(acc), C.c_float(w))
    return acc


def resolve(acc, W, H):
    img = np.empty(W * H * 3, np.uint8)
    lib().orc_resolve(_ptr(acc), C.c_size_t(W * H), _ptr(img))
    return img.reshape(H, W, 3)


def project(xyz, rgb, P, W, H, params=None):
    """Naive single-thread host loop (project_cloud.cu:314-329).
    -> dict(depth_bits uint32 [H,W], acc uint32 [H,W,4], img uint8 [H,W,3])"""
    xyz, rgb = _cloud(xyz, rgb)
    P = _P(P)
    prm = params or default_params()
    depth = np.empty(W * H, np.uint32)
    acc = np.empty(W * H * 4, np.uint32)
    img = np.empty(W * H * 3, np.uint8)
    lib().orc_project(_ptr(xyz), C.c_size_t(xyz.strides[0]), _ptr(rgb), C.c_size_t(rgb.strides[0]),
                      C.c_size_t(xyz.shape[0]), _ptr(P), W, H, C.byref(prm), _ptr(depth), _ptr(acc), _ptr(img))
    return {"depth_bits": depth.reshape(H, W), "acc": acc.reshape(H, W, 4), "img": img.reshape(H, W, 3)}


class MTProjector:
    """Multi-thread CPU projector (the timed CPU baseline); scratch is reused."""

    def __init__(self, W, H, nthreads):
        self.W, self.H, self.nthreads = W, H, nthreads
        self.scratch = np.empty(nthreads * W * H * 4, np.uint32)
        self.depth = np.empty(W * H, np.uint32)
        self.acc = np.empty(W * H * 4, np.uint32)
        self.img = np.empty(W * H * 3, np.uint8)

    def project(self, xyz, rgb, P, params=None):
        xyz, rgb = _cloud(xyz, rgb)
        P = _P(P)
        prm = params or default_params()
        rc = lib().orc_project_mt(_ptr(xyz), C.c_size_t(xyz.strides[0]), _ptr(rgb), C.c_size_t(rgb.strides[0]),
                                  C.c_size_t(xyz.shape[0]), _ptr(P), self.W, self.H, C.byref(prm),
                                  self.nthreads, _ptr(self.scratch), _ptr(self.depth), _ptr(self.acc),
                                  _ptr(self.img))
        assert rc == 0
        return {"depth_bits": self.depth.reshape(self.H, self.W), "acc": self.acc.reshape(self.H, self.W, 4),
                "img": self.img.reshape(self.H, self.W, 3)}


MM_VARIANTS = {0: "contract (right products fused, left to right)", 1: "first add fused with the left product",
               2: "nothing contracted (-fmad=false)", 3: "re-associated: all fused, right to left",
               4: "re-associated: m3 folded into the first fma"}


def mm_rows(mx, my, mz):
    """The `mm` of project_variant() for a matmul whose rows x, y, z take forms mx, my, mz of MM_VARIANTS each."""
    assert all(0 <= m <= 4 for m in (mx, my, mz))
    return 8 + mx + 5 * my + 25 * mz


DV_VARIANTS = {0: "contract: x * RN(1/z)", 1: "IEEE x / z", 2: "x * (RN(1/z) - 2 ulp)", 3: "x * (RN(1/z) - 1 ulp)",
               4: "x * (RN(1/z) + 1 ulp)", 5: "x * (RN(1/z) + 2 ulp)"}


def envelope_points(xyz, P, W, H, mm, dv, nthreads=8):
    """Per-point comparison of arithmetic variant (mm, dv) with the contract (rtr_oracle.c, "ENVELOPE").
    -> dict(accepted, either, flips, max_depth_ulp)"""
    xyz, _ = _cloud(xyz, None)
    P = _P(P)
    out = np.zeros(4, np.uint64)
    rc = lib().orc_envelope_points(_ptr(xyz), C.c_size_t(xyz.strides[0]), C.c_size_t(xyz.shape[0]), _ptr(P), W, H,
                                   int(mm), int(dv), int(nthreads), _ptr(out))
    assert rc == 0
    return {"accepted": int(out[0]), "either": int(out[1]), "flips": int(out[2]), "max_depth_ulp": int(out[3])}


def project_variant(xyz, rgb, P, W, H, mm, dv, params=None):
    """A whole frame under arithmetic variant (mm, dv): same outputs as project().  mm 0..4 or mm_rows(mx, my, mz)."""
    xyz, rgb = _cloud(xyz, rgb)
    P = _P(P)
    prm = params or default_params()
    depth = np.empty(W * H, np.uint32)
    acc = np.empty(W * H * 4, np.uint32)
    img = np.empty(W * H * 3, np.uint8)
    rc = lib().orc_project_variant(_ptr(xyz), C.c_size_t(xyz.strides[0]), _ptr(rgb), C.c_size_t(rgb.strides[0]),
                                   C.c_size_t(xyz.shape[0]), _ptr(P), W, H, C.byref(prm), int(mm), int(dv),
                                   _ptr(depth), _ptr(acc), _ptr(img))
    assert rc == 0
    return {"depth_bits": depth.reshape(H, W), "acc": acc.reshape(H, W, 4), "img": img.reshape(H, W, 3)}


def filter(depth_bits, img, params=None, want_tensor=True):
    """applyDepthFilter (project_cloud.cu:331-392) on copies of the inputs.
    -> dict(depth float32 [H,W], img uint8 [H,W,3], mask uint8 [H,W],
            tensor uint16 (fp16 bits) [5,H,W], minmax uint32[2])"""
    H, W = depth_bits.shape
    prm = params or default_params()
    d = np.ascontiguousarray(depth_bits, dtype=np.uint32).copy()
    im = np.ascontiguousarray(img, dtype=np.uint8).copy()
    mask = np.empty(W * H, np.uint8)
    tensor = np.empty(5 * W * H, np.uint16) if want_tensor else None
    mm = np.empty(2, np.uint32)
    rc = lib().orc_filter(_ptr(d), _ptr(im), W, H, C.byref(prm), _ptr(mask), _ptr(tensor), _ptr(mm))
    if rc != 0:
        raise ValueError("orc_filter: unsupported dimensions (need W %% 2^levels == 0): %dx%d" % (W, H))
    return {"depth": d.view(np.float32).reshape(H, W), "img": im.reshape(H, W, 3), "mask": mask.reshape(H, W),
            "tensor": None if tensor is None else tensor.reshape(5, H, W), "minmax": mm}


REF_VARIANTS = ("off_recip", "off_ieee", "fast_recip", "fast_ieee")
REF_POISON = 0xA5
_refs = {}


class RefLib:
    """One of oracle/_ref/libref_<variant>.so: the REFERENCE's kernels compiled for the host (oracle/ref_build.py),
    run thread by thread by oracle/ref_host/ref_driver.cpp.  Elements that no kernel of the reference writes come back
    holding the `poison` byte; `block_size` stands for project_cloud.cu:216 (it must not change any result)."""

    def __init__(self, variant, path):
        self.variant = variant
        L = C.CDLL(path)
        L.ref_abi.restype = C.c_int
        L.ref_build_traits.restype = C.c_int
        L.ref_config.argtypes = [C.c_int, C.c_int, C.c_int]
        L.ref_config.restype = None
        pv = C.c_void_p
        L.ref_project.restype = C.c_int
        L.ref_project.argtypes = [pv, pv, C.c_size_t, pv, C.c_int, C.c_int, pv, pv, pv]
        L.ref_filter.restype = C.c_int
        L.ref_filter.argtypes = [pv, pv, C.c_int, C.c_int, pv, pv, pv, pv]
        L.ref_resize.restype = C.c_int
        L.ref_resize.argtypes = [pv, pv, pv, C.c_int, C.c_int]
        L.ref_frame.restype = C.c_int
        L.ref_frame.argtypes = [pv, pv, C.c_size_t, pv, C.c_int, C.c_int, pv, pv, pv, pv, pv, pv, pv, pv, pv]
        assert L.ref_abi() == 1
        self.L = L
        self.contracted = bool(L.ref_build_traits() & 1)
        self.ieee_quotient = bool(L.ref_build_traits() & 2)

    @staticmethod
    def _cloud4(xyzw, rgba):
        xyzw = np.ascontiguousarray(xyzw, dtype=np.float32)
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        assert xyzw.ndim == 2 and xyzw.shape[1] == 4 and rgba.shape == (xyzw.shape[0], 4)
        return xyzw, rgba

    def _filtered(self, W, H, d, im, mask, dims, mm, tensor):
        mw, mh = int(dims[0]), int(dims[1])
        return {"depth": d.view(np.float32).reshape(H, W), "img": im.reshape(H, W, 3),
                "mask": mask[:mw * mh].reshape(mh, mw).copy(), "minmax": mm, "tensor_raw": tensor,
                "tensor": tensor[:5 * mw * mh].reshape(5, mh, mw).copy()}

    def project(self, xyzw, rgba, P, W, H, block_size=1024, poison=REF_POISON, slack=1):
        """computeRGBD (project_cloud.cu:268-329) -> dict(depth_bits [H,W], acc [H,W,4], img [H,W,3])"""
        xyzw, rgba = self._cloud4(xyzw, rgba)
        P = _P(P)
        depth, acc, img = np.empty(W * H, np.uint32), np.empty(W * H * 4, np.uint32), np.empty(W * H * 3, np.uint8)
        self.L.ref_config(block_size, slack, poison)
        rc = self.L.ref_project(_ptr(xyzw), _ptr(rgba), xyzw.shape[0], _ptr(P), W, H, _ptr(depth), _ptr(acc), _ptr(img))
        assert rc == 0
        return {"depth_bits": depth.reshape(H, W), "acc": acc.reshape(H, W, 4), "img": img.reshape(H, W, 3)}

    def filter(self, depth_bits, img, block_size=1024, poison=REF_POISON, slack=1):
        """applyDepthFilter (project_cloud.cu:331-392) on copies of a given unfiltered frame.
        -> dict(depth f32 [H,W], img [H,W,3], mask [H_eff,W_eff], minmax u32[2], tensor fp16 bits [5,H_eff,W_eff] -- the
        reference's own layout, plane stride W_eff*H_eff --, tensor_raw [5*W*H]: the whole buffer, poison behind)"""
        H, W = depth_bits.shape
        d = np.ascontiguousarray(depth_bits, dtype=np.uint32).copy().reshape(-1)
        im = np.ascontiguousarray(img, dtype=np.uint8).copy().reshape(-1)
        mask, dims, mm = np.zeros(W * H, np.uint8), np.zeros(2, np.int32), np.zeros(2, np.uint32)
        tensor = np.empty(5 * W * H, np.uint16)
        self.L.ref_config(block_size, slack, poison)
        rc = self.L.ref_filter(_ptr(d), _ptr(im), W, H, _ptr(mask), _ptr(dims), _ptr(mm), _ptr(tensor))
        if rc != 0:
            raise ValueError("ref_filter: unsupported dimensions %dx%d" % (W, H))
        return self._filtered(W, H, d, im, mask, dims, mm, tensor)

    def resize(self, lo, hi, mask, block_size=1024):
        """One launch of resizeKernel (project_cloud.cu:128-161, launched as at :385): lo f32 [h,w], hi f32 [2h(+1),2w(+1)],
        mask u8 like hi -> the new hi (blended where mask == 0)."""
        oh, ow = hi.shape
        assert lo.shape == (oh // 2, ow // 2) and mask.shape == hi.shape
        lo = np.ascontiguousarray(lo, dtype=np.float32)
        out = np.ascontiguousarray(hi, dtype=np.float32).copy()
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        self.L.ref_config(block_size, 1, REF_POISON)
        rc = self.L.ref_resize(_ptr(lo), _ptr(out), _ptr(mask), ow, oh)
        assert rc == 0
        return out

    def frame(self, xyzw, rgba, P, W, H, block_size=1024, poison=REF_POISON, slack=1):
        """computeFilteredRGBD (project_cloud.cu:394-434) -> (project()'s dict, filter()'s dict)"""
        xyzw, rgba = self._cloud4(xyzw, rgba)
        P = _P(P)
        du, acc, iu = np.empty(W * H, np.uint32), np.empty(W * H * 4, np.uint32), np.empty(W * H * 3, np.uint8)
        d, im = np.empty(W * H, np.uint32), np.empty(W * H * 3, np.uint8)
        mask, dims, mm = np.zeros(W * H, np.uint8), np.zeros(2, np.int32), np.zeros(2, np.uint32)
        tensor = np.empty(5 * W * H, np.uint16)
        self.L.ref_config(block_size, slack, poison)
        rc = self.L.ref_frame(_ptr(xyzw), _ptr(rgba), xyzw.shape[0], _ptr(P), W, H, _ptr(du), _ptr(acc), _ptr(iu),
                              _ptr(d), _ptr(im), _ptr(mask), _ptr(dims), _ptr(mm), _ptr(tensor))
        assert rc == 0
        return ({"depth_bits": du.reshape(H, W), "acc": acc.reshape(H, W, 4), "img": iu.reshape(H, W, 3)},
                self._filtered(W, H, d, im, mask, dims, mm, tensor))


def ref_builder():
    """oracle/ref_build.py as a module (the recipe that makes oracle/_ref from the reference tree)."""
    import importlib.util
    import sys
    if "rtr_ref_build" not in sys.modules:
        spec = importlib.util.spec_from_file_location("rtr_ref_build", os.path.join(_HERE, "ref_build.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["rtr_ref_build"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["rtr_ref_build"]


def ref_available():
    """True when the reference tree is there (oracle/_ref can be built) or a built oracle/_ref is."""
    rb = ref_builder()
    return rb.have_reference() or rb.built()


def ref(variant):
    """-> RefLib for "off_recip" | "off_ieee" | "fast_recip" | "fast_ieee"; builds oracle/_ref when the reference tree
    is there, otherwise loads what is already built.  Raises when neither is possible."""
    assert variant in REF_VARIANTS, variant
    if variant not in _refs:
        rb = ref_builder()
        if not rb.build():
            raise RuntimeError("oracle/_ref is not built and there is no reference tree under %s" % rb.reference_dir())
        _refs[variant] = RefLib(variant, rb.lib_path(variant))
    return _refs[variant]


def f32_to_f16(x):
    return int(lib().orc_f32_to_f16(C.c_float(x)))


def f16_to_f32(h):
    return float(lib().orc_f16_to_f32(C.c_uint16(h)))
