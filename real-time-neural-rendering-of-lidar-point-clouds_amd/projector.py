"""Host-side mirror of the reference's ProjectCloud on top of the C ABI.

`Projector` is a 1:1 wrapper of include/rtr.h.  `ProjectCloud` keeps the reference's
public interface (reference: src/RTRenderer/include/project_cloud.h:11-19 and
src/project_cloud.cu:268-434): same method names, argument meaning (calibration,
world->camera extrinsics, optional caller-allocated colour / depth outputs) and return
codes (1 ok, -1 when both outputs are None).
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .camera import clip_box_planes, compose_projection


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _affine_rows(M):
    """The 12 float32 coefficients rtr_transform_points takes (row-major 3 x 4) from a (3, 4) or (4, 4) array whose
    bottom row is exactly 0 0 0 1; every element is rounded to float32 once."""
    m = np.asarray(M)
    if m.dtype.kind not in "fiu" or m.shape not in ((3, 4), (4, 4)):
        raise ValueError("M must be a real (3, 4) or (4, 4) array, got %s %s" % (m.dtype, m.shape))
    if m.shape == (4, 4):
        if not (m[3, 0] == 0 and m[3, 1] == 0 and m[3, 2] == 0 and m[3, 3] == 1):
            raise ValueError("the bottom row of a 4 x 4 M must be exactly (0, 0, 0, 1): only affine transforms")
        m = m[:3]
    return np.ascontiguousarray(m.astype(np.float32)).reshape(12)


class DeviceBuffer:
    """A context-owned device buffer exposed through __cuda_array_interface__ so that
    torch.as_tensor(buf, device='cuda') aliases it (zero copy) for RCCL collectives."""

    def __init__(self, ptr, shape, typestr):
        self.ptr, self.shape, self.typestr = ptr, tuple(shape), typestr
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": typestr, "data": (ptr, False),
                                         "version": 2, "strides": None}


class Projector:
    """Thin object wrapper over the rtr_* C ABI (one context = one GPU)."""

    def __init__(self, device=0):
        self._lib = L.lib()
        self._ctx = C.c_void_p()
        rc = self._lib.rtr_create(C.byref(self._ctx), int(device))
        if rc != 0:
            raise L.RtrError(rc, (self._lib.rtr_last_error(None) or b"").decode())
        self.device = int(device)
        self.W = self.H = 0

    # -- plumbing
    def _chk(self, rc):
        if rc != 0:
            raise L.RtrError(rc, (self._lib.rtr_last_error(self._ctx) or b"").decode())

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.rtr_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._chk(self._lib.rtr_synchronize(self._ctx))

    def set_stream(self, hip_stream_ptr):
        """Run on the given hipStream_t handle (0 / None = HIP's default stream)."""
        self._chk(self._lib.rtr_set_stream(self._ctx, C.c_void_p(hip_stream_ptr or 0)))

    def reset_stream(self):
        self._chk(self._lib.rtr_reset_stream(self._ctx))

    @property
    def params(self):
        p = L.RtrParams()
        self._chk(self._lib.rtr_get_params(self._ctx, C.byref(p)))
        return p

    def set_params(self, **kw):
        p = self.params
        for k, v in kw.items():
            setattr(p, k, v)
        self._chk(self._lib.rtr_set_params(self._ctx, C.byref(p)))

    def set_option(self, key, value):
        self._chk(self._lib.rtr_set_option(self._ctx, key.encode(), int(value)))

    def get_option(self, key):
        """Current value of an option; also "reordered" (the resident cloud was sorted by the library) and
        "order_ratio_ppm" (mean 256-point-chunk diagonal / cloud diagonal as uploaded, in 1e-6)."""
        v = C.c_int()
        self._chk(self._lib.rtr_get_option(self._ctx, key.encode(), C.byref(v)))
        return v.value

    def stream_probe(self, P):
        P = self._P(P)
        self._chk(self._lib.rtr_stream_probe(self._ctx, _vp(P)))

    # -- cloud
    def upload_points(self, xyz, rgb, point_ids=None):
        """xyz: float32 [n,3|4] (the reference's float4 (x,y,z,1) or tight xyz);
        rgb: uint8 [n,3|4] (uchar4 (c0,c1,c2,255) or tight triples).
        point_ids: True / False sets option "point_ids" first (a sorted cloud keeps its upload order for
        point_pass, +4 B per point); None leaves it as it is."""
        if point_ids is not None:
            self.set_option("point_ids", 1 if point_ids else 0)
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if xyz.ndim != 2 or xyz.shape[1] not in (3, 4) or rgb.ndim != 2 or rgb.shape[1] not in (3, 4) \
                or rgb.shape[0] != xyz.shape[0]:
            raise ValueError("xyz must be [n,3|4] float32 and rgb [n,3|4] uint8 with equal n")
        self._chk(self._lib.rtr_upload_points(self._ctx, _vp(xyz), xyz.shape[1] * 4, _vp(rgb), rgb.shape[1],
                                              xyz.shape[0]))

    def append_points(self, xyz, rgb):
        """Adds points behind the resident cloud without uploading it again (include/rtr.h section 2b): the shapes and
        dtypes of upload_points; the new points get upload indices n .. n + m - 1.  Frames equal, bit for bit, those of
        one upload of everything appended so far."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if xyz.ndim != 2 or xyz.shape[1] not in (3, 4) or rgb.ndim != 2 or rgb.shape[1] not in (3, 4) \
                or rgb.shape[0] != xyz.shape[0]:
            raise ValueError("xyz must be [n,3|4] float32 and rgb [n,3|4] uint8 with equal n")
        self._chk(self._lib.rtr_append_points(self._ctx, _vp(xyz), xyz.shape[1] * 4, _vp(rgb), rgb.shape[1],
                                              xyz.shape[0]))

    def remove_points(self, keep):
        """Takes the points whose keep bit is clear out of the resident cloud and gives their memory back
        (include/rtr.h section 2c).  keep: the forms of set_point_keep except None -- a bool array of length n, uint32
        words, a torch tensor, an object with __cuda_array_interface__ (device_buffer(BUF_VISIBLE) included) or a device
        pointer.  The survivors keep their order and are renumbered 0 .. n' - 1; frames equal, bit for bit, those of
        one upload of the survivors."""
        if keep is None:
            raise ValueError("remove_points needs a keep mask (None keeps every point: nothing to remove)")
        ptr, nwords, _hold = self._keep_words(keep)
        self._chk(self._lib.rtr_remove_points(self._ctx, ptr, nwords))

    def transform_points(self, M, select=None):
        """Moves resident points by the affine transform M where they lie (include/rtr.h section 2d): indices, order,
        colours and the keep mask stay.  M: (3, 4) or (4, 4) (bottom row exactly 0 0 0 1), rounded to float32 once; a
        selected point p becomes ((M00 x + M01 y) + M02 z) + M03, ... in fp32.  select: None moves every point, else the
        forms of set_point_keep -- a bool array of length n, uint32 words, device memory -- naming the points that move.
        Frames equal, bit for bit, those of one upload of the moved cloud."""
        m = _affine_rows(M)
        if select is None:
            self._chk(self._lib.rtr_transform_points(self._ctx, _vp(m), None, 0))
            return
        ptr, nwords, _hold = self._keep_words(select)
        self._chk(self._lib.rtr_transform_points(self._ctx, _vp(m), ptr, nwords))

    def generate_synthetic(self, scene, seed, first, count, total):
        sc = L.SCENES[scene] if isinstance(scene, str) else int(scene)
        self._chk(self._lib.rtr_generate_synthetic(self._ctx, sc, seed, first, count, total))

    def reorder_points(self):
        """One-off Morton sort of the resident cloud (never changes a frame)."""
        self._chk(self._lib.rtr_reorder_points(self._ctx))

    @property
    def num_points(self):
        n = C.c_uint64()
        self._chk(self._lib.rtr_num_points(self._ctx, C.byref(n)))
        return n.value

    def download_points(self, first=0, count=None):
        count = self.num_points - first if count is None else count
        xyzw = np.empty((count, 4), np.float32)
        rgba = np.empty((count, 4), np.uint8)
        self._chk(self._lib.rtr_download_points(self._ctx, _vp(xyzw), _vp(rgba), first, count))
        return xyzw, rgba

    # -- frames
    def set_resolution(self, W, H):
        self._chk(self._lib.rtr_set_resolution(self._ctx, int(W), int(H)))
        self.W, self.H = int(W), int(H)

    @staticmethod
    def _P(P):
        P = np.ascontiguousarray(P, dtype=np.float32).reshape(16)
        return P

    def project(self, P, want_img=True, want_depth=True, filtered=False):
        """-> (img uint8 [H,W,3] | None, depth float32 [H,W] | None)"""
        P = self._P(P)
        img = np.empty((self.H, self.W, 3), np.uint8) if want_img else None
        depth = np.empty((self.H, self.W), np.float32) if want_depth else None
        fn = self._lib.rtr_project_filtered if filtered else self._lib.rtr_project
        self._chk(fn(self._ctx, _vp(P), _vp(img), _vp(depth)))
        return img, depth

    def project_into(self, P, img, depth, filtered=False):
        """The reference's call shape: fills caller-allocated arrays (either may be None), synchronous."""
        P = self._P(P)
        fn = self._lib.rtr_project_filtered if filtered else self._lib.rtr_project
        self._chk(fn(self._ctx, _vp(P), _vp(img), _vp(depth)))

    # -- asynchronous host outputs (rtr.h section 4b)
    def host_output_buffers(self, slot):
        """-> (img uint8 [H,W,3], depth float32 [H,W]): numpy views of the library's pinned buffers of `slot`
        (valid until the next set_resolution; filled by project_async, complete after wait_outputs)."""
        pi, pd = C.c_void_p(), C.c_void_p()
        self._chk(self._lib.rtr_host_output_buffers(self._ctx, int(slot), C.byref(pi), C.byref(pd)))
        img = np.ctypeslib.as_array(C.cast(pi, C.POINTER(C.c_uint8)), shape=(self.H, self.W, 3))
        depth = np.ctypeslib.as_array(C.cast(pd, C.POINTER(C.c_float)), shape=(self.H, self.W))
        return img, depth

    def project_async(self, P, slot, filtered=False):
        """Renders a frame and queues the copies of depth + image into the pinned buffers of `slot`; does not wait."""
        P = self._P(P)
        self._chk(self._lib.rtr_project_async(self._ctx, _vp(P), int(slot), 1 if filtered else 0))

    def wait_outputs(self, slot=-1):
        self._chk(self._lib.rtr_wait(self._ctx, int(slot)))

    def render(self, P, with_filter=False):
        P = self._P(P)
        self._chk(self._lib.rtr_render(self._ctx, _vp(P), 1 if with_filter else 0))

    # -- several views (rtr.h section 6c)
    def render_views(self, Ps, with_filter=False):
        """Renders K <= MAX_VIEWS poses (Ps: [K,4,4] or [K,16]) in one pass over the cloud into the BUF_VIEW_*
        buffers ([K, ...] shapes); view v equals render(Ps[v], with_filter).  Asynchronous like render."""
        Ps = np.ascontiguousarray(Ps, dtype=np.float32)
        if Ps.ndim not in (2, 3) or Ps.reshape(Ps.shape[0], -1).shape[1] != 16:
            raise ValueError("Ps must have shape [K,4,4] or [K,16]")
        Ps = Ps.reshape(-1, 16)
        self._chk(self._lib.rtr_render_views(self._ctx, Ps.shape[0], _vp(Ps), 1 if with_filter else 0))

    # -- clip planes (rtr.h section 6d)
    def set_clip_planes(self, planes):
        """Leaves out of every later frame the points outside any of up to MAX_CLIP_PLANES world-space half-spaces:
        planes is a (k, 4) array of {a, b, c, d} (rounded to float32), a point is kept iff ((a x + b y) + c z) + d >= 0
        in float32 for each of them.  None or an empty array clears them."""
        if planes is None:
            self._chk(self._lib.rtr_set_clip_planes(self._ctx, 0, None))
            return
        planes = np.ascontiguousarray(planes, dtype=np.float32)
        if planes.size == 0:
            self._chk(self._lib.rtr_set_clip_planes(self._ctx, 0, None))
            return
        if planes.ndim != 2 or planes.shape[1] != 4:
            raise ValueError("planes must have shape (k, 4)")
        self._chk(self._lib.rtr_set_clip_planes(self._ctx, planes.shape[0], _vp(planes)))

    def clip_planes(self):
        """The clip planes in force: float32 (k, 4), k = 0 when there are none."""
        out = np.zeros((L.MAX_CLIP_PLANES, 4), np.float32)
        k = C.c_int32()
        self._chk(self._lib.rtr_get_clip_planes(self._ctx, C.byref(k), _vp(out)))
        return out[:k.value].copy()

    # -- keep mask (rtr.h section 6e)
    def set_point_keep(self, keep):
        """Hides from every later frame the points whose keep bit is clear, by their upload index (the point pass's).
        keep: None (clears the mask), a bool array of length n, a uint32 word array of (n + 31) // 32 words (bit i % 32
        of word i // 32: point i is kept -- the layout of BUF_VISIBLE), or device memory holding such words: a torch
        tensor on the context's device, an object with __cuda_array_interface__ (device_buffer(BUF_VISIBLE) included)
        or an integer device pointer.  A bool torch tensor is packed on the host.  A cloud the library may sort needs
        option point_ids = 1."""
        if keep is None:
            self._chk(self._lib.rtr_set_point_keep(self._ctx, None, 0))
            return
        ptr, nwords, _hold = self._keep_words(keep)
        self._chk(self._lib.rtr_set_point_keep(self._ctx, ptr, nwords))

    def _keep_words(self, keep):
        """(pointer, nwords, owner) of a keep argument of set_point_keep / remove_points: device memory is passed as
        it is, a bool array is packed into upload-order words (owner: the host array, alive while the pointer is used)."""
        nwords = (self.num_points + 31) // 32
        if isinstance(keep, int):
            return C.c_void_p(keep), nwords, None
        if hasattr(keep, "__cuda_array_interface__") and not hasattr(keep, "data_ptr"):
            return C.c_void_p(keep.__cuda_array_interface__["data"][0]), nwords, keep
        if hasattr(keep, "data_ptr"):  # a torch tensor
            if keep.dtype.is_floating_point:
                raise ValueError("keep must be bool or 32-bit words")
            if keep.is_cuda and str(keep.dtype) != "torch.bool":
                import torch
                keep = keep.contiguous()
                torch.cuda.current_stream(keep.device).synchronize()  # (the words may still be on their way)
                if keep.numel() * keep.element_size() != 4 * nwords:
                    raise ValueError("keep must hold (n + 31) // 32 32-bit words")
                return C.c_void_p(keep.data_ptr()), nwords, keep
            keep = keep.cpu().numpy()
        keep = np.asarray(keep)
        if keep.dtype == bool:
            if keep.shape != (self.num_points,):
                raise ValueError("a bool keep mask must have shape (n,) = (%d,)" % self.num_points)
            words = np.packbits(np.concatenate([keep, np.zeros(32 * nwords - keep.size, bool)]),
                                bitorder="little").view("<u4")
        else:
            words = keep.astype("<u4", copy=False)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        return _vp(words), words.size, words

    def point_keep(self):
        """The keep mask in force as a bool array over the uploaded points, or None when none is set."""
        if not self.get_option("point_keep"):
            return None
        words = self.download(L.BUF_POINT_KEEP)
        return np.unpackbits(words.astype("<u4").view(np.uint8), bitorder="little")[:self.num_points].astype(bool)

    # -- selection (rtr.h section 6f)
    _SELECT_OPS = {"replace": L.SELECT_REPLACE, "add": L.SELECT_ADD, "subtract": L.SELECT_SUBTRACT,
                   "intersect": L.SELECT_INTERSECT, "toggle": L.SELECT_TOGGLE}

    def select_points(self, planes=None, P=None, rect=None, op="replace", outside=False, stats=True):
        """Selects on the device the points inside a region and combines them with the selection so far (BUF_SELECTION,
        upload-order words as set_point_keep / remove_points / transform_points take them).  planes: (k, 4) half-spaces
        {a, b, c, d} with the contract of set_clip_planes (None: no plane); P with rect = (x0, y0, x1, y1): also the
        points a frame with P splats onto a pixel x0 <= px < x1, y0 <= py < y1 at the context's resolution.  Neither:
        every point.  op: "replace", "add", "subtract", "intersect" or "toggle" (or the SELECT_* value); outside: the
        points NOT inside are the hits.  The context's own clip planes and keep mask are not looked at.
        stats: waits and returns (selected points after op, chunks decided outside on their boxes, chunks decided inside,
        chunks decoded); False: queued like point_pass, returns None."""
        k, pl = 0, None
        if planes is not None:
            pl = np.ascontiguousarray(planes, dtype=np.float32)
            if pl.size and (pl.ndim != 2 or pl.shape[1] != 4):
                raise ValueError("planes must have shape (k, 4)")
            k = pl.shape[0] if pl.size else 0
        if (P is None) != (rect is None):
            raise ValueError("P and rect come together")
        Pm = None if P is None else self._P(P)
        rc4 = None if rect is None else np.ascontiguousarray(rect, dtype=np.int32).reshape(4)
        code = self._SELECT_OPS[op] if isinstance(op, str) else int(op)
        if outside:
            code |= L.SELECT_OUTSIDE
        out = np.zeros(4, np.uint64) if stats else None
        self._chk(self._lib.rtr_select_points(self._ctx, k, _vp(pl) if k else None, _vp(Pm), _vp(rc4), code, _vp(out)))
        return tuple(int(v) for v in out) if stats else None

    def select_voxel_grid(self, cell, origin=(0, 0, 0), min_count=1, op="replace", outside=False, stats=True):
        """Selects on the device one point per cell of a regular grid (include/rtr.h section 6g) and combines the hits
        with the selection so far, as select_points does.  cell: the cell size, a scalar or three values (> 0);
        origin: a corner of cell (0, 0, 0).  The point of a cell with the smallest upload index is its representative,
        and it is a hit when the cell holds at least min_count points; points out of the grid (non-finite, or beyond
        2^20 cells from the origin) are cells of their own.  op / outside: as select_points.  The call always waits.
        stats: returns (selected points after op, occupied cells, cells with at least min_count points, points out of
        the grid); False: returns None."""
        c3 = np.ascontiguousarray(np.broadcast_to(np.asarray(cell, dtype=np.float32), (3,)))
        o3 = np.ascontiguousarray(origin, dtype=np.float32)
        if o3.shape != (3,):
            raise ValueError("origin must have three values")
        mc = int(min_count)
        if not 1 <= mc <= 0xFFFFFFFF:
            raise ValueError("min_count must be in 1 .. 2^32 - 1")
        code = self._SELECT_OPS[op] if isinstance(op, str) else int(op)
        if outside:
            code |= L.SELECT_OUTSIDE
        out = np.zeros(4, np.uint64) if stats else None
        self._chk(self._lib.rtr_select_voxel_grid(self._ctx, _vp(o3), _vp(c3), mc, code, _vp(out)))
        return tuple(int(v) for v in out) if stats else None

    def select_neighbours(self, radius, min_neighbours, op="replace", outside=False, stats=True):
        """Selects on the device the points with at least min_neighbours other points within `radius` (include/rtr.h
        section 6h, the radius outlier filter) and combines the hits with the selection so far, as select_points does.
        Neighbours: ((dx*dx + dy*dy) + dz*dz) <= radius*radius in float32, inclusive; never the point itself; a
        non-finite point has none.  outside: the outliers instead.  The call always waits.  stats: returns (selected
        points after op, points with at least min_neighbours neighbours, finite points with no neighbour at all,
        non-finite points); False: returns None."""
        r = float(radius)
        if not (np.isfinite(r) and r > 0):
            raise ValueError("radius must be finite and > 0")
        k = int(min_neighbours)
        if not 1 <= k <= 0xFFFFFFFF:
            raise ValueError("min_neighbours must be in 1 .. 2^32 - 1")
        code = self._SELECT_OPS[op] if isinstance(op, str) else int(op)
        if outside:
            code |= L.SELECT_OUTSIDE
        out = np.zeros(4, np.uint64) if stats else None
        self._chk(self._lib.rtr_select_neighbours(self._ctx, r, k, code, _vp(out)))
        return tuple(int(v) for v in out) if stats else None

    def select_statistical(self, k, radius, std_mul=1.0, threshold=None, op="replace", outside=False, mean_dist=False,
                           found=False, stats=True):
        """Selects on the device the points whose mean distance to their k nearest neighbours within `radius` is at most
        t = mu + std_mul * sigma, mu and sigma the mean and the sample standard deviation of that mean distance over the
        cloud (include/rtr_statistics.h section 6n, the statistical outlier filter), and combines the hits with the
        selection so far, as select_points does.  Neighbours: select_neighbours' relation; a point with fewer than k of
        them averages over those it has, a point with none (every non-finite one) has the mean +inf and is never a hit.
        k: 1 .. STAT_MAX_K.  threshold: t itself, in place of std_mul.  outside: the outliers instead.  The call always
        waits.  Returns a tuple: the stats when asked for -- (selected points after op, hits, finite points without a
        neighbour, non-finite points) --, then the moments (mu, sigma, t) as Python floats, then with mean_dist the
        float32 array of the mean distances and with found the uint32 array of min(k, neighbours), both in upload
        order."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError("k must be an integer")
        k = int(k)
        if not 1 <= k <= L.STAT_MAX_K:
            raise ValueError("k must be in 1 .. STAT_MAX_K (%d)" % L.STAT_MAX_K)
        r = float(radius)
        if not (np.isfinite(r) and r > 0):
            raise ValueError("radius must be finite and > 0")
        with np.errstate(over="ignore", under="ignore"):
            r2 = np.float32(r) * np.float32(r)
        if not (np.isfinite(r2) and r2 >= np.finfo(np.float32).tiny):
            raise ValueError("the square of radius must be a finite normal float32 number")
        mom = np.zeros(3, np.float64)
        flags = 0
        if threshold is not None:
            mom[2] = float(threshold)
            if np.isnan(mom[2]):
                raise ValueError("threshold must not be NaN")
            flags = L.STAT_THRESHOLD_GIVEN
            mul = 0.0
        else:
            mul = float(std_mul)
            if not np.isfinite(mul):
                raise ValueError("std_mul must be finite")
        code = self._SELECT_OPS[op] if isinstance(op, str) else int(op)
        if outside:
            code |= L.SELECT_OUTSIDE
        n = self.num_points
        md = np.empty(n, np.float32) if mean_dist else None
        fd = np.empty(n, np.uint32) if found else None
        out = np.zeros(4, np.uint64) if stats else None
        self._chk(self._lib.rtr_select_statistical(self._ctx, k, r, mul, flags, code, _vp(md), _vp(fd), _vp(mom), _vp(out)))
        res = [tuple(int(v) for v in out)] if stats else []
        res.append(tuple(float(v) for v in mom))
        if mean_dist:
            res.append(md)
        if found:
            res.append(fd)
        return tuple(res)

    def estimate_normals(self, k, radius, viewpoint=None, normals=True, curvature=True, found=False, device=False):
        """Estimates on the device the unit normal and the curvature of every resident point from a PCA over the point
        and its k nearest neighbours within `radius` (include/rtr_normals.h section 6o).  Neighbours:
        select_statistical's, the row ordered by (squared distance bits, upload index); a point with fewer than
        NORMAL_MIN_FOUND of them (every non-finite one) has the normal (0, 0, 0) and the curvature +inf.  k:
        1 .. NORMAL_MAX_K.  viewpoint: three finite floats towards which every normal is turned; None: the component of
        largest magnitude is positive.  The result depends on the coordinates and the upload order alone, bit for bit,
        and numpy float64 reproduces it (tests/normals_ref.py).  Nothing else changes: the selection, the keep mask and
        the clip planes play no part and stay as they are.  The call always waits.  Returns a tuple: with normals the
        (n, 3) float32 array, with curvature the (n,) float32 array of the surface variation lambda_min / (lambda_0 +
        lambda_1 + lambda_2), with found the (n,) uint32 array of min(k, neighbours) -- numpy arrays in upload order, or
        torch tensors on the context's device with device=True --, then the stats: (points with a normal, finite points
        without one, non-finite points, normals turned by the viewpoint)."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError("k must be an integer")
        k = int(k)
        if not 1 <= k <= L.NORMAL_MAX_K:
            raise ValueError("k must be in 1 .. NORMAL_MAX_K (%d)" % L.NORMAL_MAX_K)
        r = float(radius)
        if not (np.isfinite(r) and r > 0):
            raise ValueError("radius must be finite and > 0")
        with np.errstate(over="ignore", under="ignore"):
            r2 = np.float32(r) * np.float32(r)
        if not (np.isfinite(r2) and r2 >= np.finfo(np.float32).tiny):
            raise ValueError("the square of radius must be a finite normal float32 number")
        flags, vp = 0, None
        if viewpoint is not None:
            with np.errstate(over="ignore"):
                vp = np.ascontiguousarray(np.asarray(viewpoint, np.float64).astype(np.float32))
            if vp.shape != (3,) or not np.isfinite(vp).all():
                raise ValueError("viewpoint must be three finite float32 numbers")
            flags = L.NORMAL_VIEWPOINT
        n = self.num_points
        arrays, ptrs = [], []
        for want, shape, dt in ((normals, (n, 3), np.float32), (curvature, (n,), np.float32), (found, (n,), np.uint32)):
            if not want:
                ptrs.append(None)
            elif device:
                import torch
                a = torch.empty(shape, dtype=torch.uint32 if dt is np.uint32 else torch.float32, device="cuda:%d" % self.device)
                ptrs.append(C.c_void_p(a.data_ptr()))
                arrays.append(a)
            else:
                a = np.empty(shape, dt)
                ptrs.append(_vp(a))
                arrays.append(a)
        out = np.zeros(4, np.uint64)
        self._chk(self._lib.rtr_estimate_normals(self._ctx, k, r, flags, _vp(vp), ptrs[0], ptrs[1], ptrs[2], _vp(out)))
        arrays.append(tuple(int(v) for v in out))
        return tuple(arrays)

    def select_clusters(self, radius, min_points=1, max_points=0, seeded=False, op="replace", outside=False, labels=False,
                        stats=True):
        """Selects on the device the points whose connected cluster within `radius` (include/rtr.h section 6i, Euclidean
        clustering) holds at least min_points and, unless max_points is 0, at most max_points points, and combines the
        hits with the selection so far, as select_points does.  Clusters are the connected components of
        select_neighbours' relation; a point without neighbours (every non-finite one too) is a cluster of one.
        seeded: only the clusters that hold a point selected before the call.  outside: every other point instead.
        The call always waits.  labels: also the label of every point's cluster -- the smallest upload index among its
        members -- as a uint32 array in upload order.  stats: (selected points after op, clusters, clusters that hit,
        points of the largest cluster).  Returns the stats, (stats, labels) with labels, the labels alone with
        stats=False, or None with neither."""
        r = float(radius)
        if not (np.isfinite(r) and r > 0):
            raise ValueError("radius must be finite and > 0")
        lo, hi = int(min_points), int(max_points)
        if not 1 <= lo <= 0xFFFFFFFF:
            raise ValueError("min_points must be in 1 .. 2^32 - 1")
        if not 0 <= hi <= 0xFFFFFFFF or (hi != 0 and hi < lo):
            raise ValueError("max_points must be 0 (unbounded) or in min_points .. 2^32 - 1")
        code = self._SELECT_OPS[op] if isinstance(op, str) else int(op)
        if outside:
            code |= L.SELECT_OUTSIDE
        out = np.zeros(4, np.uint64) if stats else None
        lab = np.empty(self.num_points, np.uint32) if labels else None
        self._chk(self._lib.rtr_select_clusters(self._ctx, r, lo, hi, L.CLUSTER_SEEDED if seeded else 0, code, _vp(lab), _vp(out)))
        st = tuple(int(v) for v in out) if stats else None
        if labels:
            return (st, lab) if stats else lab
        return st

    @staticmethod
    def _curvature_source(arr, rows):
        """(pointer, owner) of `rows` packed float32 values: a numpy array (anything else numpy converts is converted),
        a torch tensor (host or device) or an object with __cuda_array_interface__; 1-D, or 2-D with one column."""
        if hasattr(arr, "data_ptr"):
            if arr.element_size() != 4 or not arr.dtype.is_floating_point:
                raise ValueError("curvature must hold float32 elements")
            if arr.is_cuda:
                import torch
                torch.cuda.current_stream(arr.device).synchronize()  # (the values may still be on their way)
            shape, packed, ptr = tuple(arr.shape), arr.is_contiguous(), arr.data_ptr()
        elif hasattr(arr, "__cuda_array_interface__"):
            cai = arr.__cuda_array_interface__
            if np.dtype(cai["typestr"]) != np.dtype(np.float32):
                raise ValueError("curvature must hold float32 elements")
            shape, ptr = tuple(cai["shape"]), cai["data"][0]
            packed = not cai.get("strides") or all(st == 4 for st in cai["strides"])
        else:
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            shape, packed, ptr = arr.shape, True, arr.ctypes.data
        if shape not in ((rows,), (rows, 1)) or not packed:
            raise ValueError("curvature must be %d packed float32 values" % rows)
        return C.c_void_p(ptr), arr

    def select_segments(self, radius, cos_angle, normals, curvature=None, max_curvature=float("inf"), min_points=1, max_points=0,
                        seeded=False, oriented=False, op="replace", outside=False, labels=False, stats=True):
        """Selects on the device the points whose smooth surface segment (include/rtr_segments.h section 6q, region
        growing over normals) holds at least min_points and, unless max_points is 0, at most max_points points, and
        combines the hits with the selection so far, as select_clusters does.  Segments are the connected components
        of: select_neighbours' relation within `radius`, AND |dot| >= cos_angle for the two points' normals (float32,
        (nx nx' + ny ny') + nz nz', every operation rounded on its own; oriented: dot >= cos_angle), AND, with
        `curvature`, both curvatures <= max_curvature.  normals: the (n, 3) float32 normals of the resident points in
        upload order, curvature: their n float32 curvatures or None -- numpy arrays, torch tensors (host or device) or
        objects with __cuda_array_interface__, as register_points takes its normals (estimate_normals(...,
        device=True) gives both without a copy); neither is written.  cos_angle: in (0, 1] as a float32.  A zero, NaN
        or infinite normal, a NaN curvature and a non-finite point make a segment of one.  seeded, outside, labels,
        stats and the return value: as select_clusters, with segments for clusters.  The call always waits."""
        r = float(radius)
        if not (np.isfinite(r) and r > 0):
            raise ValueError("radius must be finite and > 0")
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            ca = float(np.float32(cos_angle))
            mc = float(np.float32(max_curvature))
        if not (np.isfinite(ca) and 0 < ca <= 1):
            raise ValueError("cos_angle must be a finite float32 number in (0, 1]")
        if normals is None:
            raise ValueError("normals must be given: the (n, 3) float32 normals of the resident points")
        if curvature is not None and np.isnan(mc):
            raise ValueError("max_curvature must not be NaN")
        lo, hi = int(min_points), int(max_points)
        if not 1 <= lo <= 0xFFFFFFFF:
            raise ValueError("min_points must be in 1 .. 2^32 - 1")
        if not 0 <= hi <= 0xFFFFFFFF or (hi != 0 and hi < lo):
            raise ValueError("max_points must be 0 (unbounded) or in min_points .. 2^32 - 1")
        code = self._SELECT_OPS[op] if isinstance(op, str) else int(op)
        if outside:
            code |= L.SELECT_OUTSIDE
        n = self.num_points
        nptr, nstride, rows, nhold = self._write_source(normals, np.float32, "normals")
        if rows != n or (rows > 1 and nstride != 12):
            raise ValueError("normals must be %d packed rows of 3 float32" % n)
        cptr, chold = None, None
        if curvature is not None:
            cptr, chold = self._curvature_source(curvature, n)
        flags = (L.SEGMENT_SEEDED if seeded else 0) | (L.SEGMENT_ORIENTED if oriented else 0)
        out = np.zeros(4, np.uint64) if stats else None
        lab = np.empty(n, np.uint32) if labels else None
        self._chk(self._lib.rtr_select_segments(self._ctx, r, ca, nptr, cptr, mc if curvature is not None else 0.0, lo, hi, flags, code,
                                                _vp(lab), _vp(out)))
        del nhold, chold
        st = tuple(int(v) for v in out) if stats else None
        if labels:
            return (st, lab) if stats else lab
        return st

    def select_near(self, xyz, radius, op="replace", outside=False, near=False, given_only=False, stats=True):
        """Selects on the device the resident points that have one of the GIVEN points `xyz` within `radius` (include/rtr.h
        section 6k) and combines the hits with the selection so far, as select_points does.  xyz: float32 rows, (m, 3) or
        (m, 4) -- a numpy array, a torch tensor (host or device) or an object with __cuda_array_interface__, as
        write_points takes them; m = 0 is legal.  Near: ((dx*dx + dy*dy) + dz*dz) <= radius*radius in float32, inclusive,
        select_neighbours' relation between a resident and a given point; a non-finite point on either side is near
        nothing.  outside: the resident points near no given point instead.  near: also a bool array of m, True where
        the given point has a resident point within radius (every resident point counts).  given_only: only that
        array, the selection is neither read nor changed (op must be "replace", outside False).  The call always waits.
        stats: (selected points after op, resident points with a given point within radius, given points with a
        resident one within radius -- 0 without near --, non-finite given points).  Returns the stats, (stats, near
        array) with near or given_only, the array alone with stats=False, or None with neither."""
        r = float(radius)
        if not (np.isfinite(r) and r > 0):
            raise ValueError("radius must be finite and > 0")
        code = self._SELECT_OPS[op] if isinstance(op, str) else int(op)
        if outside:
            code |= L.SELECT_OUTSIDE
        if given_only and code != 0:
            raise ValueError("given_only leaves the selection alone: op must be 'replace' and outside False")
        ptr, stride, m, hold = self._write_source(xyz, np.float32, "xyz")
        if m >= 2 ** 32:
            raise ValueError("at most 2^32 - 1 given points")
        if m and (stride < 12 or stride % 4):
            raise ValueError("xyz rows must be at least 12 bytes apart, by a multiple of 4")
        want = bool(near or given_only)
        out = np.zeros(4, np.uint64) if stats else None
        words = np.zeros((m + 31) // 32, np.uint32) if want else None
        self._chk(self._lib.rtr_select_near(self._ctx, ptr if m else None, stride if m else 12, m, r,
                                            L.NEAR_GIVEN_ONLY if given_only else 0, code, _vp(words), _vp(out)))
        del hold
        st = tuple(int(v) for v in out) if stats else None
        if want:
            bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:m].astype(bool)
            return (st, bits) if stats else bits
        return st

    def nearest_points(self, xyz, radius, given=True, resident=False, stats=True):
        """Finds on the device, for every GIVEN point of `xyz`, the nearest resident point within `radius`, and for every
        resident point the nearest given one (include/rtr.h section 6l).  xyz: as select_near takes it -- float32 rows,
        (m, 3) or (m, 4), a numpy array, a torch tensor (host or device) or an object with __cuda_array_interface__;
        m = 0 is legal.  Candidates: ((dx*dx + dy*dy) + dz*dz) <= radius*radius in float32, inclusive, select_near's
        relation; of the candidates the smallest d2 wins, of equal d2 bits the smallest index.  given: (index, dist2)
        of m entries, the upload index of the nearest resident point and its squared distance bit for bit; resident:
        (index, dist2) of num_points entries in upload order, the given index of the nearest given point.  An entry
        without a candidate (every non-finite point) holds NEAREST_NONE and +inf.  Indices are uint32, distances
        float32; device input gives torch tensors on that device, anything else numpy arrays.  The selection, the keep
        mask and the clip planes play no part.  The call always waits.  stats: (given points with a nearest, resident
        points with one, non-finite given points, 0).  Returns the requested pairs and the stats flattened in the order
        given index, given dist2, resident index, resident dist2, stats; a single item alone; None with nothing."""
        r = float(radius)
        if not (np.isfinite(r) and r > 0):
            raise ValueError("radius must be finite and > 0")
        with np.errstate(over="ignore", under="ignore"):
            r2 = np.float32(r) * np.float32(r)
        if not (np.isfinite(r2) and r2 >= np.finfo(np.float32).tiny):
            raise ValueError("the square of radius must be a finite normal float32 number")
        ptr, stride, m, hold = self._write_source(xyz, np.float32, "xyz")
        if m >= 2 ** 32:
            raise ValueError("at most 2^32 - 1 given points")
        if m and (stride < 12 or stride % 4):
            raise ValueError("xyz rows must be at least 12 bytes apart, by a multiple of 4")
        n = self.num_points
        device = None
        if hasattr(xyz, "data_ptr"):
            device = xyz.device if xyz.is_cuda else None
        elif hasattr(xyz, "__cuda_array_interface__"):
            device = "cuda:%d" % self.device
        arrays, ptrs = [], []
        for want, rows in ((given, m), (given, m), (resident, n), (resident, n)):
            dt = (np.uint32, np.float32)[len(ptrs) % 2]
            if not want:
                ptrs.append(None)
            elif device is not None:
                import torch
                a = torch.empty(rows, dtype=torch.uint32 if dt is np.uint32 else torch.float32, device=device)
                arrays.append(a)
                ptrs.append(C.c_void_p(a.data_ptr()))
            else:
                a = np.empty(rows, dt)
                arrays.append(a)
                ptrs.append(_vp(a))
        out = np.zeros(4, np.uint64) if stats else None
        self._chk(self._lib.rtr_nearest_points(self._ctx, ptr if m else None, stride if m else 12, m, r, 0, ptrs[0], ptrs[1],
                                               ptrs[2], ptrs[3], _vp(out)))
        del hold
        if stats:
            arrays.append(tuple(int(v) for v in out))
        if not arrays:
            return None
        return arrays[0] if len(arrays) == 1 else tuple(arrays)

    @staticmethod
    def compose_pose(step, pose):
        """step o pose of two 3x4 (or 4x4) row-major float64 transforms, in register_points' fixed order: rotation part
        ((S_a0 P_0b + S_a1 P_1b) + S_a2 P_2b), translation the same with b = 3, + S_a3.  Returns a (3, 4) float64 array."""
        s = [float(v) for v in np.asarray(step, np.float64).reshape(-1)[:12]]
        p = [float(v) for v in np.asarray(pose, np.float64).reshape(-1)[:12]]
        out = np.empty((3, 4), np.float64)
        for a in range(3):
            for b in range(4):
                v = (s[4 * a] * p[b] + s[4 * a + 1] * p[4 + b]) + s[4 * a + 2] * p[8 + b]
                out[a, b] = v + s[4 * a + 3] if b == 3 else v
        return out

    def register_points(self, xyz, radius, point_to_plane=False, pose=None, normals=None):
        """One registration (ICP) step of the GIVEN points `xyz`, moved by `pose`, against the resident cloud, on the
        device (include/rtr_register.h section 6p).  xyz: as nearest_points takes it; it is never written.  pose: a (3, 4)
        or (4, 4) float64 transform with finite entries, or None for the identity; the posed points are formed in float64
        and rounded to float32.  Correspondences: nearest_points' given side on the posed points.  point_to_plane: with
        `normals`, the (n, 3) float32 normals of the resident points in upload order -- a numpy array, a torch tensor
        (host or device) or an object with __cuda_array_interface__ (estimate_normals(..., device=True) gives them
        without a copy); a pair whose normal is non-finite or (0, 0, 0) is dropped.  Returns (moments, step, stats):
        moments the REGISTER_MOMENTS float64 sums (pair count, means, cross sums, residual sum), step the (3, 4) float64
        transform that moves the POSED points onto their partners -- the identity when stats[3] is set --, stats (pairs
        used, finite posed points without a used pair, non-finite posed points, degenerate).  Every value is reproduced
        bit for bit by numpy float64 (tests/register_ref.py).  Nothing else changes; the call always waits."""
        r = float(radius)
        if not (np.isfinite(r) and r > 0):
            raise ValueError("radius must be finite and > 0")
        with np.errstate(over="ignore", under="ignore"):
            r2 = np.float32(r) * np.float32(r)
        if not (np.isfinite(r2) and r2 >= np.finfo(np.float32).tiny):
            raise ValueError("the square of radius must be a finite normal float32 number")
        ptr, stride, m, hold = self._write_source(xyz, np.float32, "xyz")
        if m >= 2 ** 32:
            raise ValueError("at most 2^32 - 1 given points")
        if m and (stride < 12 or stride % 4):
            raise ValueError("xyz rows must be at least 12 bytes apart, by a multiple of 4")
        T = None
        if pose is not None:
            T = np.asarray(pose, np.float64)
            if T.shape == (4, 4):
                if not (T[3, 0] == 0 and T[3, 1] == 0 and T[3, 2] == 0 and T[3, 3] == 1):
                    raise ValueError("the bottom row of a 4 x 4 pose must be exactly (0, 0, 0, 1)")
                T = T[:3]
            if T.shape != (3, 4) or not np.isfinite(T).all():
                raise ValueError("pose must be a finite (3, 4) or (4, 4) float64 array")
            T = np.ascontiguousarray(T).reshape(12)
        if point_to_plane and normals is None:
            raise ValueError("point_to_plane needs the resident points' normals")
        if normals is not None and not point_to_plane:
            raise ValueError("normals are read in point_to_plane mode only")
        nptr, nhold = None, None
        if point_to_plane:
            nptr, nstride, rows, nhold = self._write_source(normals, np.float32, "normals")
            if rows != self.num_points or (rows > 1 and nstride != 12):
                raise ValueError("normals must be %d packed rows of 3 float32" % self.num_points)
        mom, step, out = np.zeros(L.REGISTER_MOMENTS, np.float64), np.zeros(12, np.float64), np.zeros(4, np.uint64)
        self._chk(self._lib.rtr_register_points(self._ctx, ptr if m else None, stride if m else 12, m, r,
                                                L.REGISTER_POINT_TO_PLANE if point_to_plane else 0, _vp(T), nptr, _vp(mom), _vp(step),
                                                _vp(out)))
        del hold, nhold
        return mom, step.reshape(3, 4), tuple(int(v) for v in out)

    def nearest_k_points(self, xyz, k, radius, stats=True):
        """Finds on the device, for every GIVEN point of `xyz`, its `k` nearest resident points within `radius`
        (include/rtr.h section 6m).  xyz: as nearest_points takes it -- float32 rows, (m, 3) or (m, 4), a numpy array, a
        torch tensor (host or device) or an object with __cuda_array_interface__; m = 0 is legal.  k: 1 .. NEAREST_MAX_K.
        Candidates: nearest_points' relation.  Returns (index, dist2, found): index (m, k) uint32 and dist2 (m, k)
        float32, row j the candidates of given point j in ascending order of (dist2 bits, upload index), the first
        min(k, candidates) of them, NEAREST_NONE and +inf behind them; found (m,) uint32 the number of real entries of
        each row.  A given point coincident with a resident one finds it at +0.  Device input gives torch tensors on
        that device, anything else numpy arrays.  The selection, the keep mask and the clip planes play no part.  The
        call always waits.  stats: also, as a fourth item, (given points with found > 0, the sum of found, non-finite
        given points, given points with found == k)."""
        r = float(radius)
        if not (np.isfinite(r) and r > 0):
            raise ValueError("radius must be finite and > 0")
        with np.errstate(over="ignore", under="ignore"):
            r2 = np.float32(r) * np.float32(r)
        if not (np.isfinite(r2) and r2 >= np.finfo(np.float32).tiny):
            raise ValueError("the square of radius must be a finite normal float32 number")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError("k must be an integer")
        k = int(k)
        if not 1 <= k <= L.NEAREST_MAX_K:
            raise ValueError("k must be in 1 .. NEAREST_MAX_K (%d)" % L.NEAREST_MAX_K)
        ptr, stride, m, hold = self._write_source(xyz, np.float32, "xyz")
        if m >= 2 ** 32:
            raise ValueError("at most 2^32 - 1 given points")
        if m and (stride < 12 or stride % 4):
            raise ValueError("xyz rows must be at least 12 bytes apart, by a multiple of 4")
        device = None
        if hasattr(xyz, "data_ptr"):
            device = xyz.device if xyz.is_cuda else None
        elif hasattr(xyz, "__cuda_array_interface__"):
            device = "cuda:%d" % self.device
        arrays, ptrs = [], []
        for shape, dt in (((m, k), np.uint32), ((m, k), np.float32), ((m,), np.uint32)):
            if device is not None:
                import torch
                a = torch.empty(shape, dtype=torch.uint32 if dt is np.uint32 else torch.float32, device=device)
                ptrs.append(C.c_void_p(a.data_ptr()))
            else:
                a = np.empty(shape, dt)
                ptrs.append(_vp(a))
            arrays.append(a)
        out = np.zeros(4, np.uint64) if stats else None
        self._chk(self._lib.rtr_nearest_k_points(self._ctx, ptr if m else None, stride if m else 12, m, r, k, 0, ptrs[0], ptrs[1],
                                                 ptrs[2], _vp(out)))
        del hold
        if stats:
            arrays.append(tuple(int(v) for v in out))
        return tuple(arrays)

    # -- bands and the dominant plane (rtr.h section 6j)
    def count_in_bands(self, bands, selected=False, stats=True):
        """Counts on the device, for each band {a, b, c, d_lo, d_hi} of `bands` ((k, 5), 1 <= k <= MAX_BANDS), the points
        with u + d_lo >= 0 and -u + d_hi >= 0, u = (a*x + b*y) + c*z in float32 (include/rtr.h section 6j) -- the two
        planes {a, b, c, d_lo} and {-a, -b, -c, d_hi} of select_points, without touching the selection.  selected: only
        the currently selected points are counted (none without a selection).  The call always waits.  Returns a uint64
        array of k counts, or with stats (counts, (population size, (chunk, band) pairs decided outside on the chunk's
        box, pairs decided inside, pairs tested point by point))."""
        with np.errstate(over="ignore"):
            b = np.ascontiguousarray(bands, dtype=np.float32)
        if b.ndim != 2 or b.shape[1] != 5:
            raise ValueError("bands must have shape (k, 5)")
        if not 1 <= b.shape[0] <= L.MAX_BANDS:
            raise ValueError("bands must hold 1 .. %d bands" % L.MAX_BANDS)
        if not np.isfinite(b).all():
            raise ValueError("bands must be finite")
        if (b[:, :3] == 0).all(axis=1).any():
            raise ValueError("a band of bands has a = b = c = 0")
        counts = np.zeros(b.shape[0], np.uint64)
        out = np.zeros(4, np.uint64) if stats else None
        self._chk(self._lib.rtr_count_in_bands(self._ctx, b.shape[0], _vp(b), L.BANDS_SELECTED if selected else 0, _vp(counts),
                                               _vp(out)))
        return (counts, tuple(int(v) for v in out)) if stats else counts

    def fit_plane(self, dist, iterations=256, seed=0, selected=False):
        """Fits the dominant plane of the resident cloud by RANSAC on the device (include/rtr.h section 6j): `iterations`
        candidates through three sampled points each, scored by the points within `dist` (count_in_bands).  seed: the
        sampler's stream, any integer modulo 2^64.  selected: sample and count only the currently selected points.
        Neither changes the selection.  Returns (plane, inliers, stats): plane = float32 (a, b, c, d) with a unit normal
        whose (c, b, a) is lexicographically positive, inliers = its count, stats = (inliers, non-degenerate candidates,
        the winner's candidate number, population size).  Raises RuntimeError when every candidate is degenerate (fewer
        than three points, all samples collinear or coincident)."""
        with np.errstate(over="ignore"):
            d = float(np.float32(dist))  # (as the library takes it)
        if not (np.isfinite(d) and d >= 0):
            raise ValueError("dist must be finite and >= 0 in float32")
        it = int(iterations)
        if not 1 <= it <= L.MAX_BANDS:
            raise ValueError("iterations must be in 1 .. %d" % L.MAX_BANDS)
        plane = np.zeros(4, np.float32)
        out = np.zeros(4, np.uint64)
        self._chk(self._lib.rtr_fit_plane(self._ctx, d, it, int(seed) & 0xFFFFFFFFFFFFFFFF, L.BANDS_SELECTED if selected else 0,
                                          _vp(plane), _vp(out)))
        st = tuple(int(v) for v in out)
        if st[1] == 0:
            raise RuntimeError("fit_plane: every candidate was degenerate (population of %d points)" % st[3])
        return plane, st[0], st

    @staticmethod
    def plane_band(plane, dist):
        """The band {a, b, c, d + dist, dist - d} of fit_plane's plane, in float32 as the library forms it."""
        p = np.asarray(plane, dtype=np.float32).reshape(4)
        d = np.float32(dist)
        return np.array([p[0], p[1], p[2], p[3] + d, d - p[3]], dtype=np.float32)

    def selection(self):
        """The selection as a DeviceBuffer of upload-order words (pass it to remove_points, transform_points,
        set_point_keep or torch.as_tensor), or None when there is none."""
        if not self.get_option("selection"):
            return None
        return self.device_buffer(L.BUF_SELECTION)

    def clear_selection(self):
        self._chk(self._lib.rtr_clear_selection(self._ctx))

    # -- reading points back out (rtr.h section 2e)
    @staticmethod
    def _extract_dest(arr, dtype, min_cols, name):
        """(pointer, row stride in bytes, rows, owner) of an output of extract_points: a numpy array, a torch tensor or an
        object with __cuda_array_interface__; 2-D with at least min_cols contiguous columns of dtype (1-D for indices)."""
        dt = np.dtype(dtype)
        if hasattr(arr, "data_ptr"):  # a torch tensor (host or device)
            if arr.element_size() != dt.itemsize or arr.dtype.is_floating_point != (dt.kind == "f"):
                raise ValueError("out[%r] must hold %s elements" % (name, dt))
            shape, strides, ptr = tuple(arr.shape), tuple(st * dt.itemsize for st in arr.stride()), arr.data_ptr()
        elif hasattr(arr, "__cuda_array_interface__"):
            cai = arr.__cuda_array_interface__
            if np.dtype(cai["typestr"]).itemsize != dt.itemsize:
                raise ValueError("out[%r] must hold %s elements" % (name, dt))
            shape, ptr = tuple(cai["shape"]), cai["data"][0]
            strides = cai.get("strides") or tuple(int(np.prod(shape[i + 1:])) * dt.itemsize for i in range(len(shape)))
        else:
            if not isinstance(arr, np.ndarray) or arr.dtype != dt or not arr.flags.writeable:
                raise ValueError("out[%r] must be a writeable %s array" % (name, dt))
            shape, strides, ptr = arr.shape, arr.strides, arr.ctypes.data
        if len(shape) in (1, 2) and shape[0] == 0:  # (no rows: nothing is written, whatever strides the array reports)
            return C.c_void_p(ptr), max(min_cols, shape[-1] if len(shape) == 2 else 1) * dt.itemsize, 0, arr
        if min_cols == 1:
            if len(shape) != 1 or (shape[0] > 1 and strides[0] != dt.itemsize):
                raise ValueError("out[%r] must be a contiguous 1-D array" % name)
            return C.c_void_p(ptr), dt.itemsize, shape[0], arr
        if len(shape) != 2 or shape[1] < min_cols or strides[1] != dt.itemsize or strides[0] < min_cols * dt.itemsize:
            raise ValueError("out[%r] must be 2-D with at least %d contiguous columns" % (name, min_cols))
        return C.c_void_p(ptr), strides[0], shape[0], arr

    def count_selected(self, select):
        """The number of points `select` names (the forms of set_point_keep; None: every point): extract_points'
        count = 0 form, one pass over the words."""
        ptr, nwords, _hold = (None, 0, None) if select is None else self._keep_words(select)
        k = C.c_uint64()
        self._chk(self._lib.rtr_extract_points(self._ctx, ptr, nwords, 0, 0, None, 0, None, 0, None, C.byref(k)))
        return k.value

    def extract_points(self, select=None, first=0, count=None, xyz=True, rgb=True, indices=False, out=None):
        """Reads resident points back in UPLOAD order (include/rtr.h section 2e).  select: None = every point, else the
        forms of set_point_keep (a bool array of length n, uint32 words, device memory such as selection()); of the k
        selected points, in ascending upload index, those of ranks [first, first + count) come out (count None: to the
        last).  Returns the list of the streams asked for, in this order: xyz -> (k', 4) float32 (x, y, z, 1), rgb ->
        (k', 4) uint8 (c0, c1, c2, 255), indices -> (k',) uint32 upload indices.  Coordinates are the resident bits; the
        clip planes and the keep mask play no part; only the chunks holding a requested point are decoded.
        out: a dict with any of the keys "xyz", "rgb", "indices" naming caller arrays to fill instead -- numpy arrays,
        torch tensors (host or device) or objects with __cuda_array_interface__, 2-D with a row per point (at least 3
        columns; rows of exactly 4 columns get 1.0 / 255 in the fourth, wider rows keep what lies behind the first three)
        and 1-D uint32 for the indices; the xyz / rgb / indices flags are then ignored and the number of points written
        is returned.  A cloud the library sorted without point_ids = 1 gives every point in the resident order, and
        neither a selection nor indices."""
        ptr, nwords, _hold = (None, 0, None) if select is None else self._keep_words(select)
        k = C.c_uint64()
        self._chk(self._lib.rtr_extract_points(self._ctx, ptr, nwords, 0, 0, None, 0, None, 0, None, C.byref(k)))
        first = int(first)
        m = max(0, k.value - first)
        if count is not None:
            m = min(m, int(count))
        if out is None:
            dst = {}
            if xyz:
                dst["xyz"] = np.empty((m, 4), np.float32)
            if rgb:
                dst["rgb"] = np.empty((m, 4), np.uint8)
            if indices:
                dst["indices"] = np.empty(m, np.uint32)
        else:
            dst = dict(out)
            if set(dst) - {"xyz", "rgb", "indices"}:
                raise ValueError("out may hold the keys 'xyz', 'rgb' and 'indices'")
        if not dst:
            raise ValueError("extract_points: no stream asked for")
        px, sx, pc, sc, pi = None, 0, None, 0, None
        hold = []
        for name, dt, cols in (("xyz", np.float32, 3), ("rgb", np.uint8, 3), ("indices", np.uint32, 1)):
            if name not in dst:
                continue
            p, stride, rows, owner = self._extract_dest(dst[name], dt, cols, name)
            if rows < m:
                raise ValueError("out[%r] has %d rows, %d points are extracted" % (name, rows, m))
            hold.append(owner)
            if name == "xyz":
                px, sx = p, stride
            elif name == "rgb":
                pc, sc = p, stride
            else:
                pi = p
        if m:
            self._chk(self._lib.rtr_extract_points(self._ctx, ptr, nwords, first, m, px, sx, pc, sc, pi, None))
        if out is not None:
            return m
        return [dst[name] for name in ("xyz", "rgb", "indices") if name in dst]

    # -- writing points back (rtr.h section 2f)
    @staticmethod
    def _write_source(arr, dtype, name):
        """(pointer, row stride in bytes, rows, owner) of a stream of write_points: a numpy array (anything else numpy
        converts is converted), a torch tensor (host or device) or an object with __cuda_array_interface__; 2-D with a
        row per record and at least 3 contiguous columns of dtype."""
        dt = np.dtype(dtype)
        if hasattr(arr, "data_ptr"):  # a torch tensor (host or device)
            if arr.element_size() != dt.itemsize or arr.dtype.is_floating_point != (dt.kind == "f"):
                raise ValueError("%s must hold %s elements" % (name, dt))
            if arr.is_cuda:
                import torch
                torch.cuda.current_stream(arr.device).synchronize()  # (the records may still be on their way)
            shape, strides, ptr = tuple(arr.shape), tuple(st * dt.itemsize for st in arr.stride()), arr.data_ptr()
        elif hasattr(arr, "__cuda_array_interface__"):
            cai = arr.__cuda_array_interface__
            if np.dtype(cai["typestr"]).itemsize != dt.itemsize:
                raise ValueError("%s must hold %s elements" % (name, dt))
            shape, ptr = tuple(cai["shape"]), cai["data"][0]
            strides = cai.get("strides") or tuple(int(np.prod(shape[i + 1:])) * dt.itemsize for i in range(len(shape)))
        else:
            if not isinstance(arr, np.ndarray) or arr.dtype != dt:
                arr = np.ascontiguousarray(arr, dtype=dt)
            shape, strides, ptr = arr.shape, arr.strides, arr.ctypes.data
        if len(shape) != 2 or shape[1] < 3:
            raise ValueError("%s must be 2-D with a row per record and at least 3 columns" % name)
        if shape[0] > 0 and (strides[1] != dt.itemsize or (shape[0] > 1 and strides[0] < 3 * dt.itemsize)):
            raise ValueError("%s must have at least 3 contiguous columns per row" % name)
        stride = strides[0] if shape[0] > 1 else max(strides[0], shape[1] * dt.itemsize)
        return C.c_void_p(ptr), stride, shape[0], arr

    def write_points(self, xyz=None, rgb=None, select=None, first=0, broadcast=False):
        """Writes new coordinates and / or colours into resident points where they lie (include/rtr.h section 2f), the
        mirror image of extract_points: of the k points `select` names (None = every point, else the forms of
        set_point_keep, selection() included), in ascending upload index, the one of rank first + j takes row j.
        xyz: float32 rows, rgb: uint8 rows -- numpy arrays, torch tensors (host or device) or objects with
        __cuda_array_interface__, 2-D with a row per record and at least 3 columns (the row stride is the array's);
        None leaves that stream as it is resident.  broadcast = True: rgb is one colour, of shape (3,) or (1, 3 | 4),
        for every written point -- all of them from rank `first` on when xyz is None.  Coordinates are stored bit for
        bit.  Indices, the resident order, the keep mask and the selection stay; frames equal, bit for bit, those of one
        upload of the written cloud.  Returns the number of points written."""
        if xyz is None and rgb is None:
            raise ValueError("write_points: xyz and rgb are both None, nothing to write")
        hold, count = [], None
        px, sx, pc, sc = None, 0, None, 0
        if xyz is not None:
            px, sx, count, owner = self._write_source(xyz, np.float32, "xyz")
            hold.append(owner)
        if rgb is not None:
            if broadcast:
                if not (hasattr(rgb, "data_ptr") or hasattr(rgb, "__cuda_array_interface__")):
                    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
                    if rgb.shape == (3,) or rgb.shape == (4,):
                        rgb = rgb.reshape(1, -1)
                elif len(tuple(rgb.shape)) == 1:
                    rgb = rgb.reshape(1, -1)
            pc, sc, rows, owner = self._write_source(rgb, np.uint8, "rgb")
            hold.append(owner)
            if broadcast:
                if rows != 1:
                    raise ValueError("a broadcast rgb is one record: shape (3,) or (1, 3 | 4)")
                sc = 0
                if count is None:
                    count = 2 ** 64 - 1
            elif count is not None and rows != count:
                raise ValueError("xyz has %d rows and rgb %d: they must name the same points" % (count, rows))
            else:
                count = rows
        elif broadcast:
            raise ValueError("broadcast = True needs an rgb record")
        ptr, nwords, _hold = (None, 0, None) if select is None else self._keep_words(select)
        first = int(first)
        if count == 0:  # (no record: nothing to write, and an empty array need not have an address)
            return 0
        k = C.c_uint64()
        self._chk(self._lib.rtr_write_points(self._ctx, ptr, nwords, first, count, px, sx, pc, sc, C.byref(k)))
        return min(count, max(0, k.value - first))

    # -- point pass (rtr.h section 6b)
    def point_pass(self, P, ids=True, visible=True):
        """Per-pixel point IDs (BUF_POINT_ID: upload index, NO_POINT for none) and / or the per-point visibility
        mask (BUF_VISIBLE) of the frame in the depth buffer, made with P; queued behind it, read with download /
        device_buffer."""
        P = self._P(P)
        what = (L.POINTS_IDS if ids else 0) | (L.POINTS_VISIBLE if visible else 0)
        self._chk(self._lib.rtr_point_pass(self._ctx, _vp(P), what))

    # -- phases (multi-GPU: reduce the device buffers between them)
    def clear(self):
        self._chk(self._lib.rtr_clear(self._ctx))

    def min_depth_pass(self, P):
        P = self._P(P)
        self._chk(self._lib.rtr_min_depth_pass(self._ctx, _vp(P)))

    def accumulate_pass(self, P):
        P = self._P(P)
        self._chk(self._lib.rtr_accumulate_pass(self._ctx, _vp(P)))

    def resolve(self):
        self._chk(self._lib.rtr_resolve(self._ctx))

    def filter(self):
        self._chk(self._lib.rtr_filter(self._ctx))

    def resolve_range(self, first_pixel, count, acc_dev_ptr=None):
        self._chk(self._lib.rtr_resolve_range(self._ctx, C.c_void_p(acc_dev_ptr or 0), first_pixel, count))

    # -- buffers
    _BUF = {L.BUF_DEPTH: (np.uint32, "<u4", lambda w, h: (h, w)),
            L.BUF_ACCUM: (np.uint32, "<u4", lambda w, h: (h, w, 4)),
            L.BUF_IMAGE: (np.uint8, "|u1", lambda w, h: (h, w, 3)),
            L.BUF_TENSOR: (np.uint16, "<f2", lambda w, h: (1, 5, h, w)),
            L.BUF_MASK: (np.uint8, "|u1", lambda w, h: (h, w)),
            L.BUF_MINMAX: (np.uint32, "<u4", lambda w, h: (2,)),
            L.BUF_POINT_ID: (np.uint32, "<u4", lambda w, h: (h, w)),
            L.BUF_VISIBLE: (np.uint32, "<u4", lambda w, h, n: ((n + 31) // 32,)),  # (by the point count, not W / H)
            # (the last batch of views: by its count K)
            L.BUF_VIEW_DEPTH: (np.uint32, "<u4", lambda w, h, k: (k, h, w)),
            L.BUF_VIEW_IMAGE: (np.uint8, "|u1", lambda w, h, k: (k, h, w, 3)),
            L.BUF_VIEW_TENSOR: (np.uint16, "<f2", lambda w, h, k: (k, 5, h, w)),
            L.BUF_VIEW_MINMAX: (np.uint32, "<u4", lambda w, h, k: (k, 2)),
            L.BUF_POINT_KEEP: (np.uint32, "<u4", lambda w, h, n: ((n + 31) // 32,)),
            L.BUF_SELECTION: (np.uint32, "<u4", lambda w, h, n: ((n + 31) // 32,))}

    def _shape(self, which):
        shp = self._BUF[which][2]
        if which in (L.BUF_VISIBLE, L.BUF_POINT_KEEP, L.BUF_SELECTION):
            return shp(self.W, self.H, self.num_points)
        if L.BUF_VIEW_DEPTH <= which <= L.BUF_VIEW_MINMAX:
            return shp(self.W, self.H, self.get_option("views"))
        return shp(self.W, self.H)

    def device_buffer(self, which, typestr=None):
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._chk(self._lib.rtr_device_buffer(self._ctx, which, C.byref(ptr), C.byref(nbytes)))
        _, ts, _ = self._BUF[which]
        return DeviceBuffer(ptr.value, self._shape(which), typestr or ts)

    def download(self, which):
        dt = self._BUF[which][0]
        out = np.empty(self._shape(which), dt)
        self._chk(self._lib.rtr_download_buffer(self._ctx, which, _vp(out), out.nbytes))
        return out

    # -- peer-to-peer exchange (rtr.h section 5b)
    def p2p_export(self):
        """-> bytes: this rank's handle block (exchange it with the other ranks, then p2p_open)."""
        buf = C.create_string_buffer(L.P2P_HANDLES_BYTES)
        self._chk(self._lib.rtr_p2p_export(self._ctx, buf))
        return buf.raw

    def p2p_open(self, rank, world, handles):
        """handles: the `world` handle blocks in rank order."""
        assert len(handles) == world and all(len(h) == L.P2P_HANDLES_BYTES for h in handles)
        self._chk(self._lib.rtr_p2p_open(self._ctx, rank, world, C.create_string_buffer(b"".join(handles))))

    def p2p_close(self):
        self._chk(self._lib.rtr_p2p_close(self._ctx))

    def p2p_min_depth(self):
        self._chk(self._lib.rtr_p2p_min_depth(self._ctx))

    def p2p_sum_resolve(self):
        self._chk(self._lib.rtr_p2p_sum_resolve(self._ctx))

    def p2p_render(self, P, with_filter=False):
        P = self._P(P)
        self._chk(self._lib.rtr_p2p_render(self._ctx, _vp(P), 1 if with_filter else 0))

    def p2p_render_owned(self, P, with_filter=False, frame_owner=0):
        """Owner-computes sharded frame: afterwards only rank `frame_owner` holds the global frame."""
        P = self._P(P)
        self._chk(self._lib.rtr_p2p_render_owned(self._ctx, _vp(P), 1 if with_filter else 0, int(frame_owner)))

    def p2p_timeouts(self):
        n = C.c_uint32()
        self._chk(self._lib.rtr_p2p_status(self._ctx, C.byref(n)))
        return n.value

    # -- measurement
    def frame_stats(self):
        """Statistics of the last binned frame (synchronises): work items of the tile kernel, how many of
        them are slices of split tiles, in-frustum entries, entries of the heaviest tile, slice size,
        tile-store error bits of that frame (0 = none), split tiles, 256-point chunks with an in-frustum point
        (each loads 1 KiB of colours)."""
        out = np.zeros(8, np.uint32)
        self._chk(self._lib.rtr_frame_stats(self._ctx, _vp(out)))
        return {"items": int(out[0]), "split_items": int(out[1]), "entries": int(out[2]), "heaviest_tile": int(out[3]),
                "slice": int(out[4]), "errors": int(out[5]), "split_tiles": int(out[6]), "colour_chunks": int(out[7])}

    def timing_enable(self, on=True):
        """True / 1: every phase, 2: only the streaming point kernels, 3: those on every 4th launch, False / 0: off."""
        self._chk(self._lib.rtr_timing_enable(self._ctx, int(on)))

    def timing_reset(self):
        self._chk(self._lib.rtr_timing_reset(self._ctx))

    def timing(self):
        """-> {kernel name: (total_ms, launches)} (synchronises the stream)"""
        out = {}
        for k, name in enumerate(L.KERNEL_NAMES):
            ms, n = C.c_double(), C.c_uint64()
            self._chk(self._lib.rtr_timing_get(self._ctx, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out


class ProjectCloud:
    """Drop-in mirror of the reference class (project_cloud.h:11-19).

    ctor: the reference flattens its grid into float4 / uchar4 arrays
    (project_cloud.cu:191-192, Octreegrid.h:162-180); here the caller passes those
    flattened arrays (or tight xyz / rgb) directly.  `modelFilename` names a TorchScript file
    under $HOME/.render_cache like in the reference (project_cloud.cu:225-246); the U-Net itself
    is not part of this library -- computeFull only hands it the device tensor (zero copy) and
    post-processes its output (project_cloud.cu:471-487).  `set_model` accepts any callable
    instead of a file."""

    def __init__(self, vertices, colors, modelFilename="", device=0, reorder=True, point_ids=False):
        """reorder: True keeps the library's default upload policy (the cloud is Morton-sorted once when its
        256-point chunks are not spatially compact -- the grid's 0.25 m blocks are unordered inside); False never
        sorts.  Frames do not depend on the point order.  point_ids: a sorted cloud keeps its upload order resident
        (+4 B per point) so that computePointIds / visible_points work whatever the policy sorted; without it they
        work on clouds that were not sorted."""
        self.modelFilename = modelFilename
        self.model = None
        self._device = device
        self._bound_stream = None
        if modelFilename != "":
            import os
            import torch
            path = os.path.join(os.environ.get("HOME", ""), ".render_cache", modelFilename)
            if not os.path.exists(path):  # the reference prints this and exits (project_cloud.cu:232-236)
                raise FileNotFoundError("Model file does not exist: %s (export a TorchScript model for this "
                                        "camera resolution first)" % path)
            self.model = torch.jit.load(path, map_location="cuda:%d" % device)
        self._p = Projector(device)
        if not reorder:
            self._p.set_option("auto_reorder", 0)
        self._p.upload_points(vertices, colors, point_ids=bool(point_ids))

    def set_model(self, model):
        """Use `model` (a callable taking the fp16 {1,5,H,W} cuda tensor) in computeFull."""
        self.model = model

    @classmethod
    def from_grid(cls, grid, modelFilename="", device=0):
        """The reference constructor's argument: a block grid (project_cloud.cu:189-206);
        `grid` is a formats.Grid (CloudReader::loadCloud's result, cloudreader.cpp:180-216)."""
        return cls(grid.vertex_positions(), grid.vertex_colors(), modelFilename, device)

    def appendPoints(self, vertices, colors):
        """Appends points (the constructor's arrays: float4 / uchar4 or tight xyz / rgb) to the resident cloud without
        uploading it again.  computePointIds, visible_points and hidePoints indices continue across appends: the new
        points follow every point given so far."""
        self._p.append_points(vertices, colors)

    def appendGrid(self, grid):
        """appendPoints of a formats.Grid, flattened like from_grid (one registered scan per call)."""
        self._p.append_points(grid.vertex_positions(), grid.vertex_colors())

    @property
    def projector(self):
        return self._p

    def _frame(self, calibration, extrinsics, color, depth, filtered):
        if color is None and depth is None:  # project_cloud.cu:270-273
            return -1
        W, H = calibration.getWidth(), calibration.getHeight()
        for name, arr, shape, dt in (("color", color, (H, W, 3), np.uint8), ("depth", depth, (H, W), np.float32)):
            if arr is not None and (arr.dtype != dt or arr.shape != shape or not arr.flags.c_contiguous):
                raise ValueError("%s must be a C-contiguous %s array of shape %s (main.cpp:93-94)" % (name, dt, shape))
        self._p.set_resolution(W, H)  # project_cloud.cu:275-298
        P = compose_projection(calibration.getIntrinsicsMatrix(), extrinsics)  # project_cloud.cu:318
        fn = self._p._lib.rtr_project_filtered if filtered else self._p._lib.rtr_project
        self._p._chk(fn(self._p._ctx, _vp(P), _vp(color), _vp(depth)))
        return 1

    def setClipPlanes(self, planes):
        """Every later frame leaves out the points outside the world-space half-spaces `planes` ((k, 4), k <= 8, see
        Projector.set_clip_planes); None or empty clears them."""
        self._p.set_clip_planes(planes)

    def setClipBox(self, lo, hi, M=None):
        """Keeps only the points inside the box lo <= q <= hi, q = M p (M: 4x4 world -> box; None: the world axes,
        where the test is exactly lo <= p <= hi per axis, faces included).  See camera.clip_box_planes."""
        self._p.set_clip_planes(clip_box_planes(lo, hi, M))

    def clearClip(self):
        """No clip planes: the whole cloud again."""
        self._p.set_clip_planes(None)

    def setPointKeep(self, keep):
        """Every later frame leaves out the points whose keep bit is clear: a bool array over the uploaded vertices,
        uint32 words in the layout of visible_points' source (BUF_VISIBLE), or device memory holding them (see
        Projector.set_point_keep).  Needs point_ids=True when the cloud may be sorted."""
        self._p.set_point_keep(keep)

    def hidePoints(self, indices):
        """Hides the uploaded vertices `indices` as well, on top of the mask in force (none: every point kept)."""
        keep = self._p.point_keep()
        if keep is None:
            keep = np.ones(self._p.num_points, bool)
        keep[np.asarray(indices, dtype=np.int64)] = False
        self._p.set_point_keep(keep)

    def clearPointKeep(self):
        """No keep mask: every point again."""
        self._p.set_point_keep(None)

    def removePoints(self, indices):
        """Takes the uploaded vertices `indices` out of the resident cloud for good, giving their memory back; the
        others keep their order and are renumbered 0 .. n' - 1 (computePointIds, visible_points, hidePoints and later
        appends use the new indices)."""
        n = self._p.num_points
        idx = np.asarray(indices, dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= n):  # (as the C++ facade: no index counted from the end)
            raise IndexError("removePoints: indices must lie in [0, %d)" % n)
        keep = np.ones(n, bool)
        keep[idx] = False
        self._p.remove_points(keep)

    def transformPoints(self, M, first=0, count=None):
        """Moves the uploaded vertices [first, first + count) (default: to the last one) by the affine transform M, (3, 4)
        or (4, 4) with bottom row 0 0 0 1 (see Projector.transform_points) -- one re-registered scan.  Indices, order,
        colours and the keep mask stay; a range past the vertex count raises IndexError."""
        m = _affine_rows(M)
        n = self._p.num_points
        first = int(first)
        count = n - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > n:  # (as the C++ facade)
            raise IndexError("transformPoints: the range [%d, %d + %d) must lie in [0, %d)" % (first, first, count, n))
        if count == 0:
            return
        if first == 0 and count == n:  # (every point: no selection, so any cloud, sorted or not)
            self._p.transform_points(m.reshape(3, 4))
            return
        sel = np.zeros(n, bool)
        sel[first:first + count] = True
        self._p.transform_points(m.reshape(3, 4), sel)

    # -- selection (rtr.h section 6f): regions named on the device, then removed, hidden or moved without a host array
    def selectPlanes(self, planes, op="replace", outside=False):
        """Selects the uploaded vertices every half-space of `planes` ((k, 4), see Projector.select_points) keeps and
        combines them with the selection so far by op ("replace", "add", "subtract", "intersect", "toggle"); outside:
        the vertices NOT inside.  Returns the number selected afterwards.  Needs point_ids=True when the cloud may be
        sorted; the clip planes and the keep mask in force play no part."""
        return self._p.select_points(planes=planes, op=op, outside=outside)[0]

    def selectBox(self, lo, hi, M=None, op="replace", outside=False):
        """selectPlanes of the box lo <= q <= hi, q = M p (M: 4x4 world -> box; None: the world axes, exactly
        lo <= p <= hi per axis, faces included).  See camera.clip_box_planes."""
        return self.selectPlanes(clip_box_planes(lo, hi, M), op, outside)

    def selectRect(self, calibration, extrinsics, x0, y0, x1, y1, op="replace"):
        """Selects the vertices that computeRGBD with this calibration and pose splats onto a pixel x0 <= px < x1,
        y0 <= py < y1, hidden behind others or not (a rubber band on the screen).  Returns the number selected."""
        self._p.set_resolution(calibration.getWidth(), calibration.getHeight())
        P = compose_projection(calibration.getIntrinsicsMatrix(), extrinsics)
        return self._p.select_points(P=P, rect=(x0, y0, x1, y1), op=op)[0]

    def selectVoxelGrid(self, cell, origin=(0, 0, 0), min_count=1, op="replace", outside=False):
        """Selects one vertex per cell of a regular grid of cell size `cell` (a scalar or three values) -- the one with
        the smallest vertex index, where the cell holds at least min_count vertices (see Projector.select_voxel_grid).
        Returns the number selected afterwards."""
        return self._p.select_voxel_grid(cell, origin, min_count, op, outside)[0]

    def thin(self, cell):
        """Thins the resident cloud to one vertex per cell of size `cell` for good: selectVoxelGrid of everything but
        the representatives, then removeSelected.  Returns the number of vertices left."""
        self._p.select_voxel_grid(cell, outside=True, stats=False)
        self.removeSelected()
        return self._p.num_points

    def selectNeighbours(self, radius, min_neighbours, op="replace", outside=False):
        """Selects the vertices with at least min_neighbours other vertices within `radius` (outside: every vertex but
        those; see Projector.select_neighbours).  Returns the number selected afterwards."""
        return self._p.select_neighbours(radius, min_neighbours, op, outside)[0]

    def removeOutliers(self, radius, min_neighbours):
        """Takes the vertices with fewer than min_neighbours others within `radius` out of the resident cloud for good:
        selectNeighbours of the outliers, then removeSelected.  Returns the number removed."""
        gone = self._p.select_neighbours(radius, min_neighbours, outside=True)[0]
        self.removeSelected()
        return gone

    def selectStatistical(self, k, radius, std_mul=1.0, op="replace", outside=False):
        """Selects the vertices whose mean distance to their k nearest neighbours within `radius` is at most the cloud's
        average of it plus std_mul standard deviations (outside: every vertex but those; see
        Projector.select_statistical).  Returns the number selected afterwards."""
        return self._p.select_statistical(k, radius, std_mul, None, op, outside)[0][0]

    def removeStatisticalOutliers(self, k, radius, std_mul=1.0):
        """Takes the statistical outliers -- the vertices selectStatistical does not name, isolated and non-finite ones
        included -- out of the resident cloud for good: selectStatistical of the outliers, then removeSelected.
        Returns the number removed."""
        gone = self._p.select_statistical(k, radius, std_mul, outside=True)[0][0]
        self.removeSelected()
        return gone

    def estimateNormals(self, k, radius, viewpoint=None):
        """The unit normal (n, 3) and the curvature (n,) of every vertex, float32 in the order of the vertices, from
        its k nearest neighbours within `radius`; viewpoint: turned towards it (see Projector.estimate_normals).
        Returns (normals, curvature)."""
        return self._p.estimate_normals(k, radius, viewpoint)[:2]

    def selectClusters(self, radius, min_points=1, max_points=0, seeded=False, op="replace", outside=False):
        """Selects the vertices whose connected cluster within `radius` holds min_points .. max_points vertices (0: no
        upper bound; seeded: only clusters holding a selected vertex; see Projector.select_clusters).  Returns the
        number selected afterwards."""
        return self._p.select_clusters(radius, min_points, max_points, seeded, op, outside)[0]

    def growSelection(self, radius):
        """Grows the selection to every vertex connected to it by steps of at most `radius`.  Returns the number
        selected afterwards."""
        return self._p.select_clusters(radius, seeded=True)[0]

    def removeSmallClusters(self, radius, min_points):
        """Takes the clusters of fewer than min_points vertices within `radius` out of the resident cloud for good:
        selectClusters of everything else's complement, then removeSelected.  Returns the number removed."""
        gone = self._p.select_clusters(radius, min_points, outside=True)[0]
        self.removeSelected()
        return gone

    # -- smooth segments (rtr_segments.h section 6q)
    def selectSegments(self, radius, k, angle, max_curvature, min_points=1, max_points=0, seeded=False, op="replace", outside=False):
        """Selects the vertices whose smooth surface segment holds min_points .. max_points vertices (0: no upper bound;
        seeded: only segments holding a selected vertex): estimateNormals at (k, radius) into device memory, then
        Projector.select_segments at the same radius -- neighbours whose normals lie within `angle` (radians, up to
        sign) and whose curvatures are both <= max_curvature (inf: no limit) are joined.  cos_angle is the host's
        math.cos(angle) rounded to float32: this one value comes from libm, everything behind it is exact.  Returns the
        number selected afterwards."""
        import math
        normals, curvature, _ = self._p.estimate_normals(k, radius, device=True)
        return self._p.select_segments(radius, np.float32(math.cos(float(angle))), normals, curvature, max_curvature, min_points,
                                       max_points, seeded, False, op, outside)[0]

    def removeSmallSegments(self, radius, k, angle, max_curvature, min_points):
        """Takes the smooth segments of fewer than min_points vertices (selectSegments' arguments) out of the resident
        cloud for good: selectSegments of everything else's complement, then removeSelected.  Returns the number
        removed."""
        gone = self.selectSegments(radius, k, angle, max_curvature, min_points, outside=True)
        self.removeSelected()
        return gone

    # -- distance to given points (rtr.h section 6k)
    def selectNear(self, vertices, radius, op='replace', outside=False):
        """Selects the vertices that have one of the given `vertices` ((m, 3) or (m, 4) float32) within `radius`
        (outside: every vertex but those; see Projector.select_near).  Returns the number selected afterwards."""
        return self._p.select_near(vertices, radius, op, outside)[0]

    def appendNewPoints(self, vertices, colors, radius):
        """Appends of the given points (appendPoints' arrays) exactly those that have no resident vertex within `radius`,
        in their order: merging an overlapping scan without piling up duplicates.  The search leaves the selection as
        it is; appending even one point drops it, as appendPoints does (it stays when nothing is new).  A
        scan is not thinned against itself -- two new points closer than radius to each other are both appended: thin
        the scan first, or the cloud afterwards (selectVoxelGrid, thin).  Returns the number appended."""
        v = np.asarray(vertices)
        c = np.asarray(colors)
        if len(v) != len(c):
            raise ValueError("vertices has %d rows and colors %d" % (len(v), len(c)))
        near = self._p.select_near(v, radius, given_only=True, stats=False)
        new = ~near
        k = int(new.sum())
        if k:
            self.appendPoints(np.ascontiguousarray(v[new]), np.ascontiguousarray(c[new]))
        return k

    # -- the nearest vertex to given points (rtr.h section 6l)
    def nearestPoints(self, vertices, radius):
        """For every given vertex ((m, 3) or (m, 4) float32) the resident vertex closest to it within `radius` (see
        Projector.nearest_points).  Returns (index, dist2): the upload index (NEAREST_NONE: none within radius) and the
        squared distance (+inf then), float32 bit for bit."""
        return self._p.nearest_points(vertices, radius, stats=False)

    def nearestKPoints(self, vertices, k, radius):
        """The k nearest vertices to each row of `vertices` within `radius`, on the device (include/rtr.h section 6m,
        Projector.nearest_k_points).  Returns (index, dist2, found): (m, k) upload indices (NEAREST_NONE behind the real
        entries) and squared distances (+inf there), ascending by (dist2 bits, index), and the real entries per row."""
        return self._p.nearest_k_points(vertices, k, radius, stats=False)

    def matchPoints(self, vertices, radius):
        """nearestPoints with the matched vertices themselves: returns (index, dist2, xyz, rgb), xyz (m, 3) float32 and
        rgb (m, 3) uint8 the resident coordinates and colours of every winner, bit for bit; rows without a match are
        zero.  One extract of the distinct winners.  With a rigid fit of vertices[matched] onto xyz[matched] and
        transformPoints this is one ICP step."""
        index, dist2 = self.nearestPoints(vertices, radius)
        if hasattr(index, "cpu"):
            index, dist2 = index.cpu().numpy(), dist2.cpu().numpy()
        return (index, dist2) + self._gather_matched(index)

    # -- registering a scan (rtr_register.h section 6p)
    def registerPoints(self, vertices, radius, iterations=20, point_to_plane=False, normals=None, pose=None):
        """Aligns the scan `vertices` ((m, 3) or (m, 4) float32, host or device; never written) to the resident cloud by
        up to `iterations` steps of Projector.register_points, each composed onto the pose in float64
        (Projector.compose_pose).  point_to_plane with normals None: estimateNormals(16, radius) once, kept on the
        device.  Stops at a degenerate step, and at the first step whose pair count equals the previous one's while its
        rms residual did not fall (that step is not applied).  Returns (pose, rms, stats): the (4, 4) float64 pose that
        moves the scan onto the cloud, the rms residual of every call, and the last call's stats.  Every step is exact, so
        the whole loop is reproducible bit for bit; device vertices stay on the device."""
        cur = np.eye(4)[:3] if pose is None else np.asarray(pose, np.float64).reshape(-1)[:12].reshape(3, 4).copy()
        if point_to_plane and normals is None:
            normals = self._p.estimate_normals(16, radius, curvature=False, device=True)[0]
        at = L.REGISTER_MOMENTS - 1 if point_to_plane else 16  # (the residual sum's place among the moments)
        rms, stats, prev = [], (0, 0, 0, 0), None
        for _ in range(int(iterations)):
            mom, step, stats = self._p.register_points(vertices, radius, point_to_plane, cur, normals if point_to_plane else None)
            r = float(np.sqrt(mom[at] / mom[0])) if mom[0] > 0 else float("inf")
            rms.append(r)
            if stats[3]:
                break
            if prev is not None and stats[0] == prev[0] and not r < prev[1]:
                break
            prev = (stats[0], r)
            cur = Projector.compose_pose(step, cur)
        out = np.eye(4)
        out[:3] = cur
        return out, rms, stats

    def _gather_matched(self, index):
        m = index.shape[0]
        xyz, rgb = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.uint8)
        matched = index != L.NEAREST_NONE
        if matched.any():
            words = np.zeros((self._p.num_points + 31) // 32, np.uint32)
            win = np.unique(index[matched])
            np.bitwise_or.at(words, win >> 5, np.uint32(1) << (win & 31).astype(np.uint32))
            x, c, idx = self._p.extract_points(words, indices=True)  # (ascending upload index: idx equals win)
            at = np.searchsorted(idx, index[matched])
            xyz[matched], rgb[matched] = x[at, :3], c[at, :3]
        return xyz, rgb

    # -- the dominant plane (rtr.h section 6j)
    def fitPlane(self, dist, iterations=256, seed=0, selected=False):
        """RANSAC fit of the plane with the most vertices within `dist` (see Projector.fit_plane).  Returns
        (plane, inliers): float32 (a, b, c, d), unit normal pointing up, and the number of vertices within dist of it.
        selected: among the selected vertices only.  The selection stays as it is."""
        plane, inliers, _ = self._p.fit_plane(dist, iterations, seed, selected)
        return plane, inliers

    def countInBands(self, bands, selected=False):
        """The number of vertices in each band {a, b, c, d_lo, d_hi} of `bands` ((k, 5); see Projector.count_in_bands), as a
        uint64 array; selected: among the selected vertices only.  The selection stays as it is."""
        return self._p.count_in_bands(bands, selected, stats=False)

    def selectPlane(self, plane, dist, op="replace", outside=False):
        """Selects the vertices within `dist` of `plane` -- select_points with the two planes {a, b, c, d + dist} and
        {-a, -b, -c, dist - d} of the fit's band, so that with op "replace" the count is exactly fitPlane's -- and combines
        them with the selection so far by op; outside: every other vertex.  Returns the number selected afterwards."""
        b = Projector.plane_band(plane, dist)
        planes = np.array([[b[0], b[1], b[2], b[3]], [-b[0], -b[1], -b[2], b[4]]], dtype=np.float32)
        return self._p.select_points(planes=planes, op=op, outside=outside)[0]

    def segmentPlane(self, dist, iterations=256, seed=0):
        """Open3D's segment_plane: fitPlane, then selectPlane of it with "replace".  Returns (plane, inliers); the
        inliers are the selection.  Peeling a second plane off the rest:
            ground, _ = cloud.segmentPlane(0.03)
            cloud.selectPlanes(None, op="toggle")            # everything but the ground
            wall, _ = cloud.fitPlane(0.03, selected=True)"""
        plane, inliers = self.fitPlane(dist, iterations, seed)
        self.selectPlane(plane, dist)
        return plane, inliers

    def selectedCount(self):
        """The number of selected vertices (0 without a selection)."""
        if not self._p.get_option("selection"):
            return 0
        return self._p.select_points(op="add", outside=True)[0]  # (adds the complement of every point: nothing)

    def clearSelection(self):
        self._p.clear_selection()

    def _with_complement(self, fn):
        """fn(the words of everything but the selection), the inversion done on the device (SELECT_TOGGLE)."""
        if not self._p.get_option("selection"):
            self._p.select_points(op="subtract", stats=False)  # (none yet: an empty one)
        self._p.select_points(op="toggle", stats=False)
        try:
            fn(self._p.selection())
        finally:
            if self._p.get_option("selection"):  # (a removal drops it)
                self._p.select_points(op="toggle", stats=False)

    def removeSelected(self):
        """Takes the selected vertices out of the resident cloud for good (see removePoints); the others are renumbered
        and the selection is gone."""
        self._with_complement(self._p.remove_points)
        self._p.clear_selection()  # (also when nothing was selected)

    def hideSelected(self):
        """The keep mask becomes everything but the selection (a mask in force is replaced: add to the selection and
        hide again to hide more); the selection stays."""
        self._with_complement(self._p.set_point_keep)

    def transformSelected(self, M):
        """Moves the selected vertices by the affine transform M (see transformPoints); the selection stays, naming
        the same vertices where they now lie."""
        if self._p.get_option("selection"):
            self._p.transform_points(_affine_rows(M).reshape(3, 4), self._p.selection())

    # -- reading points back out (rtr.h section 2e)
    def extractSelected(self, indices=False):
        """The selected vertices in upload order: (vertices (k, 4) float32, colors (k, 4) uint8), with indices=True
        also their (k,) uint32 vertex indices -- the arrays the constructor and appendPoints take.  Nothing selected:
        empty arrays.  Vertices the clip planes or the keep mask hide are extracted like the others."""
        if not self._p.get_option("selection"):
            empty = [np.empty((0, 4), np.float32), np.empty((0, 4), np.uint8)] + ([np.empty(0, np.uint32)] if indices else [])
            return tuple(empty)
        return tuple(self._p.extract_points(self._p.selection(), indices=indices))

    def extractPoints(self, indices_or_mask):
        """The uploaded vertices a bool mask over them or an array of vertex indices names, in ASCENDING vertex index
        (an index given twice comes out once): (vertices (k, 4) float32, colors (k, 4) uint8)."""
        n = self._p.num_points
        sel = np.asarray(indices_or_mask)
        if sel.dtype != bool:
            idx = sel.astype(np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= n):  # (as removePoints: no index counted from the end)
                raise IndexError("extractPoints: indices must lie in [0, %d)" % n)
            sel = np.zeros(n, bool)
            sel[idx] = True
        return tuple(self._p.extract_points(sel))

    def extractAll(self):
        """Every vertex as it is resident now -- after appends, removals and moves -- in upload order:
        (vertices (n, 4) float32, colors (n, 4) uint8).  (A cloud sorted without point_ids=True comes in the sorted
        order.)"""
        return tuple(self._p.extract_points())

    def savePly(self, path, selected=False, bgr=True):
        """Writes every vertex (selected: the selected ones) to a binary PLY through formats.write_ply.  bgr: the
        colours were given in B, G, R order, as the reference's loader and formats.read_ply deliver them, and are
        written as red, green, blue; False writes the channels as they are.  Returns the number of vertices written."""
        from .formats import write_ply
        xyz, rgb = (self.extractSelected() if selected else self.extractAll())[:2]
        write_ply(path, xyz[:, :3], rgb[:, 2::-1] if bgr else rgb[:, :3])
        return xyz.shape[0]

    def commitPointKeep(self):
        """Removes the vertices the keep mask in force hides (see removePoints), then clears the mask: the frames stay
        what they were, the hidden vertices no longer cost memory or time.  Nothing happens without a mask."""
        keep = self._p.point_keep()
        if keep is None:
            return
        if not keep.all():
            self._p.remove_points(self._p.download(L.BUF_POINT_KEEP))
        self._p.set_point_keep(None)

    def computeRGBD(self, calibration, extrinsics, color, depth):
        """project_cloud.cu:268-312.  extrinsics = world->camera 4x4 (main.cpp:96)."""
        return self._frame(calibration, extrinsics, color, depth, False)

    def computeFilteredRGBD(self, calibration, extrinsics, color, depth):
        """project_cloud.cu:394-434."""
        return self._frame(calibration, extrinsics, color, depth, True)

    def computeFull(self, calibration, extrinsics, color, depth):
        """project_cloud.cu:437-493: projection + prefilter, then the model on the resident fp16
        tensor; color <- uint8(round(output * 255)) like cv::Mat::convertTo(CV_8UC3, 255.0),
        depth <- the prefiltered depth buffer.  Either output may be None; returns 1."""
        import torch
        if self.model is None:  # the reference warns in the ctor and then crashes in forward()
            raise L.RtrError(L.RTR_ERR_INVALID, "No model: computeFull needs modelFilename or set_model()")
        W, H = calibration.getWidth(), calibration.getHeight()
        for name, arr, shape, dt in (("color", color, (H, W, 3), np.uint8), ("depth", depth, (H, W), np.float32)):
            if arr is not None and (arr.dtype != dt or arr.shape != shape or not arr.flags.c_contiguous):
                raise ValueError("%s must be a C-contiguous %s array of shape %s (main.cpp:93-94)" % (name, dt, shape))
        dev = torch.device("cuda", self._device)
        with torch.cuda.device(dev):
            # kernels and the model share torch's current stream
            stream = torch.cuda.current_stream(dev).cuda_stream
            if self._bound_stream != stream:
                self._p.set_stream(stream)
                self._bound_stream = stream
            self._p.set_resolution(W, H)
            P = compose_projection(calibration.getIntrinsicsMatrix(), extrinsics)
            self._p.render(P, True)
            # (a frame that overflowed the adaptive extent pool is rendered again here, before the model reads it)
            self._p.synchronize()
            inp = torch.as_tensor(self._p.device_buffer(L.BUF_TENSOR), device=dev)  # zero copy (from_blob, :471)
            with torch.no_grad():
                out = self.model(inp)
            out = out[0].permute(1, 2, 0).contiguous()  # :475
            if color is not None:
                img = (out.float() * 255.0).round().clamp(0, 255).to(torch.uint8)  # convertTo(CV_8UC3, 255.0), :480
                color[...] = img.cpu().numpy()
            if depth is not None:
                depth[...] = self._p.download(L.BUF_DEPTH).view(np.float32)  # :485
        return 1

    def computeFullViews(self, calibration, extrinsics_list, colors, depths):
        """computeFull for K = len(extrinsics_list) <= MAX_VIEWS poses at once: one pass over the cloud, the model run
        ONCE on the [K,5,H,W] fp16 batch tensor (zero copy).  colors[v] / depths[v] (any may be None) receive view v's
        colour and prefiltered depth, as computeFull would for extrinsics_list[v].  Returns 1."""
        import torch
        if self.model is None:
            raise L.RtrError(L.RTR_ERR_INVALID, "No model: computeFullViews needs modelFilename or set_model()")
        K = len(extrinsics_list)
        if len(colors) != K or len(depths) != K:
            raise ValueError("colors and depths need one entry (or None) per extrinsics matrix")
        W, H = calibration.getWidth(), calibration.getHeight()
        for v in range(K):
            for name, arr, shape, dt in (("color", colors[v], (H, W, 3), np.uint8), ("depth", depths[v], (H, W), np.float32)):
                if arr is not None and (arr.dtype != dt or arr.shape != shape or not arr.flags.c_contiguous):
                    raise ValueError("%s[%d] must be a C-contiguous %s array of shape %s" % (name, v, dt, shape))
        dev = torch.device("cuda", self._device)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if self._bound_stream != stream:
                self._p.set_stream(stream)
                self._bound_stream = stream
            self._p.set_resolution(W, H)
            Kc = calibration.getIntrinsicsMatrix()
            Ps = np.stack([compose_projection(Kc, E) for E in extrinsics_list])
            self._p.render_views(Ps, True)
            # (a batch that overflowed the adaptive extent pools is rendered again here, before the model reads it)
            self._p.synchronize()
            inp = torch.as_tensor(self._p.device_buffer(L.BUF_VIEW_TENSOR), device=dev)  # zero copy, [K,5,H,W]
            with torch.no_grad():
                out = self.model(inp)
            need_depth = any(d is not None for d in depths)
            dall = self._p.download(L.BUF_VIEW_DEPTH).view(np.float32) if need_depth else None
            for v in range(K):
                if colors[v] is not None:
                    o = out[v].permute(1, 2, 0).contiguous()
                    colors[v][...] = (o.float() * 255.0).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
                if depths[v] is not None:
                    depths[v][...] = dall[v]
        return 1

    def _point_pass(self, calibration, extrinsics, filtered, ids, visible):
        W, H = calibration.getWidth(), calibration.getHeight()
        self._p.set_resolution(W, H)
        P = compose_projection(calibration.getIntrinsicsMatrix(), extrinsics)
        self._p.render(P, filtered)
        self._p.point_pass(P, ids=ids, visible=visible)

    def computePointIds(self, calibration, extrinsics, filtered=False):
        """Renders the frame (like computeRGBD / computeFilteredRGBD) and returns which point each pixel shows:
        int64 [H, W], the index into the uploaded vertex array, -1 for none (empty or prefiltered-away pixels).
        image[p] of an attribute array `a` is then a[ids[p]] where ids[p] >= 0."""
        self._point_pass(calibration, extrinsics, filtered, True, False)
        ids = self._p.download(L.BUF_POINT_ID)
        out = ids.astype(np.int64)
        out[ids == L.NO_POINT] = -1
        return out

    def visible_points(self, calibration, extrinsics, filtered=False):
        """Renders the frame and returns a bool mask over the uploaded vertices: True for the points that
        contributed to its colour (passed the z-buffer and depth window; after the prefilter, on a kept pixel)."""
        self._point_pass(calibration, extrinsics, filtered, False, True)
        words = self._p.download(L.BUF_VISIBLE)
        bits = np.unpackbits(words.astype("<u4").view(np.uint8), bitorder="little")
        return bits[:self._p.num_points].astype(bool)

    def tensor_device_buffer(self):
        """The planar fp16 {1,5,H,W} device tensor computeFull feeds to the U-Net
        (project_cloud.cu:471); valid after computeFilteredRGBD."""
        return self._p.device_buffer(L.BUF_TENSOR)
