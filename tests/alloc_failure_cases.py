"""The states and the calls of the failed-allocation sweep (tests/test_gpu_alloc_failure.py drives the library with them,
tests/test_alloc_failure_host.py checks this file, the header and the sources without a GPU; README_alloc_failure.md).

include/rtr.h says what every entry point leaves behind when an allocation fails.  Option "debug_alloc_fail" = k makes
the k-th allocation attempted from then on fail, once, on the host side (csrc/rtr_alloc_rule.h): a call that makes K0
allocations is run K0 times on K0 fresh contexts, failing at each of its sites in turn, and after each the context must be
what the call's contract says, must pass a health check, and must do the call again, exactly.

STATES: room_shell with N = 4099 points (17 chunks of 256, the last one of 3) at 64 x 48, resident in packed form only
("pack" = 2), as fp32 arrays ("pack" = 0), and Morton-sorted ("auto_reorder" = 1); option "point_ids" = 1 in all three,
so that rtr_reorder_points may run under the keep mask.  Each with a keep mask hiding two whole chunks and scattered
points, a selection made by rtr_select_points, and two clip planes in force: whether these survive a failure is then
visible.  The host statement of every state is edit_model.Model (nearest_model's subclass: one method per call).

CASES: every entry names its contract group, the rtr_* symbols it reaches, the states it runs on, a `call` (the library,
through the Projector) and an `expect` (the model and the references the call's own GPU test uses).  A call that
allocates nothing in a state is not in that state's list: NO_ALLOCATION says which and why.  NOT_SWEPT names every other
symbol of _lib.SYMBOLS with the reason.  numpy only at import time."""
import numpy as np

import edit_model as em
import helpers
import nearest_model as nm
import planes_ref
import point_pass_ref as ppr
import select_ref

N, W, H = 4099, 64, 48
SEED = 0xA110CA7E
HEALTH_POSE = 5
STATES = ("packed", "pack0", "sorted")
_FAMILY = {"packed": "pack2_ids", "pack0": "pack0", "sorted": "sorted_blocks"}
STATE_OPTIONS = {"packed": {"pack": 2, "auto_reorder": 0, "point_ids": 1},
                 "pack0": {"pack": 0, "auto_reorder": 0, "point_ids": 1},
                 "sorted": {"pack": 2, "auto_reorder": 1, "point_ids": 1}}
CLIP = np.array([[0.0, 0.0, 1.0, 3.5], [0.6, 0.0, -0.8, 4.0]], np.float32)  # (two slanted cuts through the room)
SELECT_PLANES = np.array([[1.0, 0.0, 0.0, 0.25]], np.float32)
RTR_ERR_HIP = -2
GROUPS = ("atomic", "replace", "reorder", "tolerant", "frame")


# ---- the states ---------------------------------------------------------------------------------------------------------
_cloud = {}


def base_cloud(orc):
    """xyz float32 (N, 3), rgb uint8 (N, 3) of the states' cloud (computed once, read only)."""
    if "base" not in _cloud:
        xyzw, rgba = orc.generate("room_shell", SEED, 0, N, N)
        _cloud["base"] = (np.ascontiguousarray(xyzw[:, :3]), np.ascontiguousarray(rgba[:, :3]))
    return _cloud["base"]


def keep_bits(n=N):
    """Two whole chunks hidden (3 and 9) and every 37th point."""
    i = np.arange(n)
    return ~(((i >= 768) & (i < 1024)) | ((i >= 2304) & (i < 2560)) | (i % 37 == 5))


def new_model(state, orc):
    m = nm.Model(_FAMILY[state])
    m.point_ids = True
    xyz, rgb = base_cloud(orc)
    m.upload(xyz, rgb)
    m.set_keep(keep_bits())
    m.select(SELECT_PLANES, "replace", False)
    m.clip = CLIP.copy()
    m.state, m.pack = state, STATE_OPTIONS[state]["pack"]
    return m


def copy_model(m):
    c = m.copy()
    c.point_ids, c.clip, c.state, c.pack = m.point_ids, m.clip.copy(), m.state, m.pack
    return c


def build(pkg, orc, state):
    """A fresh context in `state` and its model."""
    p = pkg.Projector(0)
    for k, v in STATE_OPTIONS[state].items():
        p.set_option(k, v)
    p.set_resolution(W, H)
    xyz, rgb = base_cloud(orc)
    p.upload_points(xyz, rgb)
    p.set_point_keep(keep_bits())
    p.select_points(planes=SELECT_PLANES)
    p.set_clip_planes(CLIP)
    return p, new_model(state, orc)


def drawn(model):
    """Upload indices of the points a frame draws: kept by the mask AND by every clip plane (rtr.h sections 6d, 6e)."""
    inside = np.ones(model.n, bool)
    x, y, z = (np.ascontiguousarray(model.xyz[:, k]) for k in range(3))
    with np.errstate(all="ignore"):
        for a, b, c, d in np.asarray(model.clip, np.float32).reshape(-1, 4):
            inside &= ((a * x + b * y) + c * z) + d >= np.float32(0)
    if model.keep is not None:
        inside &= model.keep
    return np.flatnonzero(inside)


def health_pose(model, k=HEALTH_POSE):
    """edit_model.pose_for's camera (an orbit round the drawable points) for a W x H frame: its pixel rows rescaled from
    edit_model's 160 x 128 frame to this one."""
    P = em.pose_for(model, k).astype(np.float64).reshape(4, 4)
    P[0] *= W / em.W
    P[1] *= H / em.H
    return P.astype(np.float32).reshape(16)


def frame_ref(orc, model, P, filtered=True, width=W, height=H):
    d = drawn(model)
    xyzw, rgba = helpers.cloud(model.xyz[d], model.rgb[d])
    r = orc.project(xyzw, rgba, P, width, height)
    out = {"depth_bits": r["depth_bits"].reshape(height, width), "img": r["img"]}
    if filtered:
        f = orc.filter(r["depth_bits"], r["img"])
        out = {"depth_bits": f["depth"].view(np.uint32).reshape(height, width), "img": f["img"], "tensor": f["tensor"],
               "minmax": np.asarray(f["minmax"]).view(np.uint32).reshape(2)}
    out["raw_depth_bits"] = r["depth_bits"]
    out["drawn"], out["xyzw"] = d, xyzw
    return out


def point_pass_ref(orc, model, P, ref):
    """(ids, visible words) in upload order of the model's cloud for the frame `ref` (frame_ref's)."""
    d = ref["drawn"]
    e_ids, e_vis = ppr.point_pass(orc, ref["xyzw"], P, W, H, ref["depth_bits"].reshape(-1))
    none = e_ids == ppr.NO_POINT
    ids = np.where(none, ppr.NO_POINT, d[np.where(none, 0, e_ids)] if d.size else ppr.NO_POINT).astype(np.uint32)
    seen = np.zeros(model.n, bool)
    seen[d] = ppr.unpack(e_vis, d.size)
    return ids.reshape(H, W), em.words_of(seen)


# ---- snapshots ----------------------------------------------------------------------------------------------------------
SNAPSHOT_OPTIONS = ("reordered", "packed", "point_keep", "selection", "views", "p2p_open")


def snapshot(pkg, p):
    """What a failed atomic call must leave word for word: the point count, the option read-backs, the clip planes, the
    keep and selection words, and every point with its index (coordinates as bit patterns)."""
    L = pkg._lib
    s = {"num_points": p.num_points, "clip": p.clip_planes().view(np.uint32)}
    for k in SNAPSHOT_OPTIONS:
        s[k] = p.get_option(k)
    s["keep_words"] = p.download(L.BUF_POINT_KEEP) if s["point_keep"] else None
    s["selection_words"] = p.download(L.BUF_SELECTION) if s["selection"] else None
    if s["num_points"]:
        xyz, rgb, idx = p.extract_points(indices=True)
        s["xyz_bits"], s["rgb"], s["indices"] = xyz.view(np.uint32).copy(), rgb.copy(), idx.copy()
    else:
        s["xyz_bits"] = s["rgb"] = s["indices"] = None
    return s


def model_snapshot(model):
    """The same for a model (views and p2p_open are the context's alone: 0)."""
    n = model.n
    s = {"num_points": n, "clip": np.asarray(model.clip, np.float32).view(np.uint32), "reordered": int(model.sorted),
         "packed": int(model.pack == 2 and n > 0), "point_keep": int(model.keep is not None),
         "selection": int(model.selection is not None), "views": 0, "p2p_open": 0}
    s["keep_words"] = em.words_of(model.keep) if model.keep is not None else None
    s["selection_words"] = select_ref.words(model.selection) if model.selection is not None else None
    if n:
        xyzw, rgba = helpers.cloud(model.xyz, model.rgb)
        s["xyz_bits"], s["rgb"], s["indices"] = xyzw.view(np.uint32), rgba, np.arange(n, dtype=np.uint32)
    else:
        s["xyz_bits"] = s["rgb"] = s["indices"] = None
    return s


def differences(a, b, ignore=()):
    """The keys under which two snapshots (or two result dicts) differ: arrays by dtype, shape and bits."""
    bad = sorted((set(a) ^ set(b)) - set(ignore))
    for k in sorted((set(a) & set(b)) - set(ignore)):
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            if x is None or y is None:
                bad.append(k)
                continue
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            if x.dtype.itemsize != y.dtype.itemsize or x.shape != y.shape or x.tobytes() != y.tobytes():
                bad.append(k)
        elif isinstance(x, (tuple, list)) or isinstance(y, (tuple, list)):
            if tuple(int(v) for v in x) != tuple(int(v) for v in y):
                bad.append(k)
        elif x is None or y is None:
            if x is not y:
                bad.append(k)
        elif x != y:
            bad.append(k)
    return bad


# ---- the cases ----------------------------------------------------------------------------------------------------------
class Case:
    """name; group; symbols: the rtr_* entry points the call goes through; states; call(cx) -> result dict (cx: a Ctx);
    expect(cx, model) -> result dict, applying the call to `model`; prepare(cx): what comes before the call on the context
    AND cx.model, outside the armed part.  A call whose caller outputs rtr.h promises untouched after an error goes
    through _raw, which pre-fills them with a sentinel and notes whether it is still there."""

    def __init__(self, name, group, symbols, call, expect, states=STATES, prepare=None):
        assert group in GROUPS
        self.name, self.group, self.symbols, self.states = name, group, tuple(symbols), tuple(states)
        self.call, self.expect, self.prepare = call, expect, prepare


class Ctx:
    def __init__(self, pkg, orc, p, model):
        self.pkg, self.orc, self.p, self.model, self.L = pkg, orc, p, model, pkg._lib
        self.note = {}


def _block(m, data, box=2):
    xyz, rgb = em.block({"m": m, "data": data, "box": box})
    return xyz, rgb


def _edit(fn_call, fn_model):
    """A call without outputs: the library side and the model side."""
    def call(cx):
        fn_call(cx)
        return {}

    def expect(cx, model):
        fn_model(cx, model)
        return {}
    return call, expect


def _append(m, data):
    xyz, rgb = None, None

    def blk():
        nonlocal xyz, rgb
        if xyz is None:
            xyz, rgb = _block(m, data)
        return xyz, rgb
    return _edit(lambda cx: cx.p.append_points(*blk()), lambda cx, mo: mo.append(*blk()))


def _remove(spec):
    return _edit(lambda cx: cx.p.remove_points(em.mask_bits(spec, cx.model)),
                 lambda cx, mo: mo.remove(em.mask_bits(spec, mo)))


_SEL = ("range", 100, 700)


def _write(coords):
    def rows(model):
        k = int(em.mask_bits(_SEL, model).sum())
        X, C = _block(k, 77, 1)
        return (X if coords else None), C
    return _edit(lambda cx: cx.p.write_points(*rows(cx.model), select=em.mask_bits(_SEL, cx.model)),
                 lambda cx, mo: mo.write(em.mask_bits(_SEL, mo), 0, *rows(mo)))


def _new_keep(model):
    return np.random.default_rng(11).random(model.n) < 0.7


def _radius(orc):
    """float of a float32: 1.0001 x the median distance of a point of the cloud to its 4th nearest."""
    if "radius" not in _cloud:
        p = base_cloud(orc)[0].astype(np.float64)
        d2 = ((p[:512, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        _cloud["radius"] = float(np.float32(1.0001 * np.median(np.sqrt(np.sort(d2, axis=1)[:, 4]))))
    return _cloud["radius"]


def _given(orc, m=300):
    """Given points of the near / nearest calls: half resident points displaced within the radius (every eighth
    coincident), half a block of their own."""
    if ("given", m) not in _cloud:
        xyz, r = base_cloud(orc)[0], _radius(orc)
        rng = np.random.default_rng(31)
        idx = rng.integers(N, size=m // 2)
        res = xyz[idx].astype(np.float64) + rng.uniform(-r, r, size=(m // 2, 3)) * (np.arange(m // 2) % 8 != 0)[:, None]
        _cloud[("given", m)] = np.ascontiguousarray(np.concatenate([res.astype(np.float32), _block(m - m // 2, 32, 0)[0]]))
    return _cloud[("given", m)]


SENTINEL_BYTE = 0xA5


def _raw(cx, fn, args, outputs):
    """One call through the C ABI itself with every caller output pre-filled with a sentinel.  args: the arguments behind
    the context, an output's name (a key of `outputs`: numpy arrays) standing for its pointer.  After an error
    cx.note["outputs_untouched"] says, output by output, whether every byte still holds the sentinel -- include/rtr.h
    promises that for these calls -- and the error is raised as the facade raises it.  -> outputs."""
    import ctypes as C
    for a in outputs.values():
        a.view(np.uint8).reshape(-1)[:] = SENTINEL_BYTE
    argv = [outputs[a].ctypes.data_as(C.c_void_p) if isinstance(a, str) else a for a in args]
    rc = getattr(cx.L.lib(), fn)(cx.p._ctx, *argv)
    if rc != 0:
        cx.note["outputs_untouched"] = {k: bool((a.view(np.uint8) == SENTINEL_BYTE).all()) for k, a in outputs.items()}
        cx.p._chk(rc)
    return outputs


def _ptr(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


def _stats(a):
    return tuple(int(v) for v in a)


def _analysis(kind):
    """The selecting analysis calls, against nearest_model.Model's methods."""
    def call(cx):
        r, L, n = _radius(cx.orc), cx.L, cx.model.n
        st = np.zeros(4, np.uint64)
        if kind == "voxel":
            cell, origin = np.full(3, 2 * r, np.float32), np.zeros(3, np.float32)
            _raw(cx, "rtr_select_voxel_grid", [_ptr(origin), _ptr(cell), 1, L.SELECT_ADD, "stats"], {"stats": st})
            return {"stats": _stats(st)}
        if kind == "neighbours":
            _raw(cx, "rtr_select_neighbours", [r, 4, L.SELECT_INTERSECT, "stats"], {"stats": st})
            return {"stats": _stats(st)}
        if kind == "clusters":
            lab = np.zeros(n, np.uint32)
            _raw(cx, "rtr_select_clusters", [r, 2, 0, 0, L.SELECT_REPLACE, "labels", "stats"], {"labels": lab, "stats": st})
            return {"stats": _stats(st), "labels": lab}
        G = _given(cx.orc)
        words = np.zeros((len(G) + 31) // 32, np.uint32)
        _raw(cx, "rtr_select_near", [_ptr(G), 12, len(G), r, 0, L.SELECT_ADD, "near_words", "stats"], {"near_words": words, "stats": st})
        return {"stats": _stats(st), "near": np.unpackbits(words.view(np.uint8), bitorder="little")[:len(G)].astype(bool)}

    def expect(cx, mo):
        r = _radius(cx.orc)
        if kind == "voxel":
            return {"stats": mo.voxel(2 * r, (0, 0, 0), 1, "add", False)["stats"]}
        if kind == "neighbours":
            return {"stats": mo.neighbours(r, 4, "intersect", False)["stats"]}
        if kind == "clusters":
            res = mo.clusters(r, 2, 0, False, "replace", False)
            return {"stats": res["stats"], "labels": res["labels"].astype(np.uint32)}
        res = mo.near(_given(cx.orc), r, "add", False, True, False)
        return {"stats": res["stats"], "near": res["near"]}
    return call, expect


def _bands(orc):
    if "bands" not in _cloud:
        xyz, r = base_cloud(orc)[0], _radius(orc)
        out = [[0.0, 1.0, 0.0, 0.5, 0.25]]
        for i in ((5, 900, 3000), (17, 2500, 4000)):
            pl = planes_ref.candidate(xyz[i[0]], xyz[i[1]], xyz[i[2]], list(i))
            out.append([float(v) for v in planes_ref.band_of(pl, np.float32(r))])
        _cloud["bands"] = np.ascontiguousarray(np.array(out, np.float32))
    return _cloud["bands"]


def _count_in_bands():
    def call(cx):
        b = _bands(cx.orc)
        counts, st = np.zeros(len(b), np.uint64), np.zeros(4, np.uint64)
        _raw(cx, "rtr_count_in_bands", [len(b), _ptr(b), cx.L.BANDS_SELECTED, "counts", "stats"], {"counts": counts, "stats": st})
        return {"counts": counts, "population": int(st[0])}

    def expect(cx, mo):
        res = mo.bands(_bands(cx.orc), True)
        return {"counts": np.asarray(res["counts"], np.uint64), "population": res["stats"][0]}
    return call, expect


def _fit_plane():
    def call(cx):
        plane, st = np.zeros(4, np.float32), np.zeros(4, np.uint64)
        _raw(cx, "rtr_fit_plane", [float(np.float32(_radius(cx.orc))), 16, 9, 0, "plane", "stats"], {"plane": plane, "stats": st})
        return {"plane": plane, "stats": _stats(st)}

    def expect(cx, mo):
        res = mo.fit_plane(_radius(cx.orc), 16, 9, False)
        assert res["error"] is None
        return {"plane": np.asarray(res["plane"], np.float32), "stats": res["stats"]}
    return call, expect


def _nearest():
    def call(cx):
        G, n = _given(cx.orc), cx.model.n
        out = {"resident_index": np.zeros(n, np.uint32), "resident_dist2": np.zeros(n, np.float32), "stats": np.zeros(4, np.uint64)}
        _raw(cx, "rtr_nearest_points", [_ptr(G), 12, len(G), _radius(cx.orc), 0, None, None, "resident_index", "resident_dist2", "stats"], out)
        return dict(out, stats=_stats(out["stats"]))

    def expect(cx, mo):
        res = mo.nearest(_given(cx.orc), _radius(cx.orc), False, True)
        return {"resident_index": res["resident"][0], "resident_dist2": res["resident"][1], "stats": res["stats"]}
    return call, expect


def _nearest_k(k):
    def call(cx):
        G = _given(cx.orc)
        m = len(G)
        out = {"index": np.zeros((m, k), np.uint32), "dist2": np.zeros((m, k), np.float32), "found": np.zeros(m, np.uint32),
               "stats": np.zeros(4, np.uint64)}
        _raw(cx, "rtr_nearest_k_points", [_ptr(G), 12, m, _radius(cx.orc), k, 0, "index", "dist2", "found", "stats"], out)
        return dict(out, stats=_stats(out["stats"]))

    def expect(cx, mo):
        res = mo.nearest_k(_given(cx.orc), _radius(cx.orc), k)
        return {"index": res["index"], "dist2": res["dist2"], "found": res["found"], "stats": res["stats"]}
    return call, expect


_EXTRACT_SEL = ("random", 41, 0.4)


def _extract(device):
    def call(cx):
        sel = em.mask_bits(_EXTRACT_SEL, cx.model)
        if not device:
            xyz, rgb, idx = cx.p.extract_points(sel, first=7, indices=True)
            return {"xyz": xyz, "rgb": rgb, "indices": idx}
        import torch
        k = int(sel.sum()) - 7
        dev = "cuda:%d" % cx.p.device
        out = {"xyz": torch.zeros((k, 4), dtype=torch.float32, device=dev), "rgb": torch.zeros((k, 4), dtype=torch.uint8, device=dev),
               "indices": torch.zeros(k, dtype=torch.int32, device=dev)}
        assert cx.p.extract_points(sel, first=7, out=out) == k
        return {"xyz": out["xyz"].cpu().numpy(), "rgb": out["rgb"].cpu().numpy(), "indices": out["indices"].cpu().numpy().view(np.uint32)}

    def expect(cx, mo):
        want = np.flatnonzero(em.mask_bits(_EXTRACT_SEL, mo))[7:]
        xyzw, rgba = helpers.cloud(mo.xyz[want], mo.rgb[want])
        return {"xyz": xyzw, "rgb": rgba, "indices": want.astype(np.uint32)}
    return call, expect


def _select_points_raw():
    """rtr_select_points where no selection exists yet (it allocates nothing otherwise), through the C ABI itself: rtr.h
    promises `stats` untouched after a failure, so the array is pre-filled with a sentinel."""
    SENTINEL = 0xDEADBEEFDEADBEEF

    def call(cx):
        import ctypes as C
        st = np.full(4, SENTINEL, np.uint64)
        rc = cx.L.lib().rtr_select_points(cx.p._ctx, 1, SELECT_PLANES.ctypes.data_as(C.c_void_p), None, None, cx.L.SELECT_ADD,
                                          st.ctypes.data_as(C.c_void_p))
        if rc != 0:
            cx.note["stats_untouched"] = bool((st == SENTINEL).all())
            cx.p._chk(rc)
        return {"stats0": int(st[0]), "chunks": int(st[1] + st[2] + st[3])}

    def expect(cx, mo):
        mo.select(SELECT_PLANES, "add", False)
        return {"stats0": int(mo.selection.sum()), "chunks": (mo.n + 255) // 256}

    def prepare(cx):
        cx.p.clear_selection()
        cx.model.selection = None
    return call, expect, prepare


def _extract_window(cx):
    cx.p.set_option("debug_extract_window", 300)


# -- cloud-replacing calls
def _upload(m, data):
    """Another room_shell (surfaces: its frames survive the prefilter), m points."""
    def rows(orc):
        if ("upload", m, data) not in _cloud:
            xyzw, rgba = orc.generate("room_shell", SEED + data, 0, m, m)
            _cloud[("upload", m, data)] = (np.ascontiguousarray(xyzw[:, :3]), np.ascontiguousarray(rgba[:, :3]))
        return _cloud[("upload", m, data)]
    return _edit(lambda cx: cx.p.upload_points(*rows(cx.orc)), lambda cx, mo: mo.upload(*rows(cx.orc)))


def _generate(count):
    def expect(cx, mo):
        xyzw, rgba = cx.orc.generate("room_shell", SEED + 1, 0, count, count)
        mo.upload(xyzw[:, :3], rgba[:, :3])
        return {}
    return (lambda cx: cx.p.generate_synthetic("room_shell", SEED + 1, 0, count, count) or {}), expect


def _download():
    def call(cx):
        xyzw, rgba = cx.p.download_points()
        return {"points": resident_rows(xyzw, rgba, cx.model.state)}

    def expect(cx, mo):
        xyzw, rgba = helpers.cloud(mo.xyz, mo.rgb)
        return {"points": resident_rows(xyzw, rgba, mo.state)}
    return call, expect


def resident_rows(xyzw, rgba, state):
    """The rows of rtr_download_points as one uint32 array: in the resident order where that is the upload order, else
    (a cloud the library sorted: a permutation of it) sorted row by row, so that equal sets of points compare equal."""
    rows = np.concatenate([np.ascontiguousarray(xyzw, np.float32).view(np.uint32), np.asarray(rgba, np.uint8).astype(np.uint32)], axis=1)
    if state == "sorted" and len(rows):
        rows = rows[np.lexsort(rows.T[::-1])]
    return rows


def _pack(value):
    def expect(cx, mo):
        mo.pack = value
        return {}
    return (lambda cx: cx.p.set_option("pack", value) or {}), expect


def _reorder():
    return _edit(lambda cx: cx.p.reorder_points(), lambda cx, mo: mo.reorder())


# -- frames
def _frame_buffers(cx, filtered):
    L = cx.L
    out = {"depth_bits": cx.p.download(L.BUF_DEPTH), "img": cx.p.download(L.BUF_IMAGE)}
    if filtered:
        out["tensor"] = cx.p.download(L.BUF_TENSOR).reshape(5, cx.p.H, cx.p.W)
        out["minmax"] = cx.p.download(L.BUF_MINMAX)
    return out


def _ref_frame(cx, mo, filtered, width=W, height=H, k=HEALTH_POSE + 1):
    ref = frame_ref(cx.orc, mo, _pose(mo, k, width, height), filtered, width, height)
    return {key: ref[key] for key in (("depth_bits", "img", "tensor", "minmax") if filtered else ("depth_bits", "img"))}


def _pose(mo, k, width=W, height=H):
    P = em.pose_for(mo, k).astype(np.float64).reshape(4, 4)
    P[0] *= width / em.W
    P[1] *= height / em.H
    return P.astype(np.float32).reshape(16)


def _render(filtered):
    def call(cx):
        cx.p.render(_pose(cx.model, HEALTH_POSE + 1), with_filter=filtered)
        return _frame_buffers(cx, filtered)
    return call, lambda cx, mo: _ref_frame(cx, mo, filtered)


W2, H2 = 96, 32


def _resolution_render():
    def call(cx):
        try:
            cx.p.set_resolution(W2, H2)
            cx.p.render(_pose(cx.model, HEALTH_POSE + 1, W2, H2), with_filter=True)
            return _frame_buffers(cx, True)
        finally:  # (the facade's W / H follow the call, not the context, when the call fails)
            cx.note["resolution"] = (W2, H2)
    return call, lambda cx, mo: _ref_frame(cx, mo, True, W2, H2)


def _project():
    def call(cx):
        img, depth = cx.p.project(_pose(cx.model, HEALTH_POSE + 1), filtered=True)
        return {"depth_bits": depth.view(np.uint32), "img": img}

    def expect(cx, mo):
        ref = _ref_frame(cx, mo, True)
        return {"depth_bits": ref["depth_bits"], "img": ref["img"]}
    return call, expect


def _project_async():
    def call(cx):
        cx.p.project_async(_pose(cx.model, HEALTH_POSE + 1), 1, filtered=True)
        cx.p.wait_outputs(1)
        img, depth = cx.p.host_output_buffers(1)
        return {"depth_bits": depth.view(np.uint32).copy(), "img": img.copy()}

    def expect(cx, mo):
        ref = _ref_frame(cx, mo, True)
        return {"depth_bits": ref["depth_bits"], "img": ref["img"]}
    return call, expect


def _point_pass():
    def call(cx):
        cx.p.point_pass(_pose(cx.model, HEALTH_POSE + 1))
        return {"ids": cx.p.download(cx.L.BUF_POINT_ID), "visible": cx.p.download(cx.L.BUF_VISIBLE)}

    def expect(cx, mo):
        P = _pose(mo, HEALTH_POSE + 1)
        ids, vis = point_pass_ref(cx.orc, mo, P, frame_ref(cx.orc, mo, P, True))
        return {"ids": ids, "visible": vis}

    def prepare(cx):  # (the frame the pass reads: rendered before, outside the armed part)
        cx.p.render(_pose(cx.model, HEALTH_POSE + 1), with_filter=True)
    return call, expect, prepare


VIEW_POSES = (HEALTH_POSE + 1, HEALTH_POSE + 2, HEALTH_POSE + 3)


def _render_views():
    def call(cx):
        L = cx.L
        cx.p.render_views(np.stack([_pose(cx.model, k) for k in VIEW_POSES]), with_filter=True)
        return {"views": cx.p.get_option("views"), "depth_bits": cx.p.download(L.BUF_VIEW_DEPTH), "img": cx.p.download(L.BUF_VIEW_IMAGE),
                "tensor": cx.p.download(L.BUF_VIEW_TENSOR), "minmax": cx.p.download(L.BUF_VIEW_MINMAX)}

    def expect(cx, mo):
        refs = [_ref_frame(cx, mo, True, k=k) for k in VIEW_POSES]
        out = {key: np.stack([r[key] for r in refs]) for key in ("depth_bits", "img", "tensor", "minmax")}
        out["views"] = len(VIEW_POSES)
        return out
    return call, expect


def _views_after_one():
    """render_views_3 behind a batch of ONE view that succeeded: "views" reads 1 before the armed call, so that the 0 it
    must read after a failure is the call's doing; the batch buffers grow from one view to three."""
    call, expect = _render_views()

    def prepare(cx):
        cx.p.render_views(_pose(cx.model, HEALTH_POSE + 4).reshape(1, 16), with_filter=True)
        assert cx.p.get_option("views") == 1
    return call, expect, prepare


def _p2p_export():
    def call(cx):
        blob = cx.p.p2p_export()
        return {"handles": len(blob), "p2p_open": cx.p.get_option("p2p_open")}
    return call, lambda cx, mo: {"handles": 9 * 64, "p2p_open": 0}


# -- tolerant: the second tile store and extent pool of option "overlap" (automatic), first allocated by the third
# consecutive filtered rtr_render of a context
def _overlap_third_frame():
    def call(cx):
        cx.p.render(_pose(cx.model, HEALTH_POSE + 1), with_filter=True)
        # (read at once: every other call, the downloads below among them, ends the streak and clears it)
        cx.note["overlap_active"] = cx.p.get_option("overlap_active")
        return _frame_buffers(cx, True)

    def expect(cx, mo):
        return _ref_frame(cx, mo, True)

    def prepare(cx):
        for k in (HEALTH_POSE + 2, HEALTH_POSE + 3):
            cx.p.render(_pose(cx.model, k), with_filter=True)
    return call, expect, prepare


def _c(name, group, symbols, pair, **kw):
    prepare = kw.pop("prepare", None)
    if len(pair) == 3:
        prepare = pair[2]
    return Case(name, group, symbols, pair[0], pair[1], prepare=prepare, **kw)


CASES = [
    # -- atomic: RTR_ERR_HIP and the snapshot afterwards is the snapshot before, word for word
    _c("append_1", "atomic", ["rtr_append_points"], _append(1, 21)),
    _c("append_300", "atomic", ["rtr_append_points"], _append(300, 22)),
    _c("append_past_headroom", "atomic", ["rtr_append_points"], _append(600, 23)),  # (more than N / 8: the arrays are reallocated)
    _c("remove_tail", "atomic", ["rtr_remove_points"], _remove(("drop_range", 3900, N))),
    _c("remove_one_per_chunk", "atomic", ["rtr_remove_points"], _remove(("drop_every", 256, 7))),
    _c("transform", "atomic", ["rtr_transform_points"],
       _edit(lambda cx: cx.p.transform_points(em.MATRICES["rigid"], em.mask_bits(_SEL, cx.model)),
             lambda cx, mo: mo.transform(em.MATRICES["rigid"], em.mask_bits(_SEL, mo)))),
    _c("write_coordinates", "atomic", ["rtr_write_points"], _write(True)),
    _c("write_colours", "atomic", ["rtr_write_points"], _write(False)),
    _c("set_point_keep", "atomic", ["rtr_set_point_keep"],
       _edit(lambda cx: cx.p.set_point_keep(_new_keep(cx.model)), lambda cx, mo: mo.set_keep(_new_keep(mo)))),
    _c("select_points_first", "atomic", ["rtr_select_points", "rtr_clear_selection"], _select_points_raw()),
    _c("select_voxel_grid", "atomic", ["rtr_select_voxel_grid"], _analysis("voxel")),
    _c("select_neighbours", "atomic", ["rtr_select_neighbours"], _analysis("neighbours")),
    _c("select_clusters_labels", "atomic", ["rtr_select_clusters"], _analysis("clusters")),
    _c("count_in_bands", "atomic", ["rtr_count_in_bands"], _count_in_bands()),
    _c("fit_plane", "atomic", ["rtr_fit_plane"], _fit_plane()),
    _c("select_near_words", "atomic", ["rtr_select_near"], _analysis("near")),
    _c("nearest_points_resident", "atomic", ["rtr_nearest_points"], _nearest()),
    _c("nearest_k_1", "atomic", ["rtr_nearest_k_points"], _nearest_k(1)),
    _c("nearest_k_64", "atomic", ["rtr_nearest_k_points"], _nearest_k(64)),
    _c("extract_host_windows", "atomic", ["rtr_extract_points"], _extract(False), prepare=_extract_window),
    _c("extract_device_windows", "atomic", ["rtr_extract_points"], _extract(True), prepare=_extract_window),
    # -- cloud-replacing: RTR_ERR_HIP with the old cloud intact or no points at all; RTR_OK where a best-effort site gave up
    _c("upload_other_size", "replace", ["rtr_upload_points"], _upload(3000, 51)),
    _c("upload_larger", "replace", ["rtr_upload_points"], _upload(5000, 53)),
    _c("upload_same_size", "replace", ["rtr_upload_points"], _upload(N, 52)),
    _c("generate_synthetic", "replace", ["rtr_generate_synthetic"], _generate(2000)),
    _c("download_points", "replace", ["rtr_download_points"], _download()),
    _c("pack_2_to_0", "replace", ["rtr_set_option"], _pack(0), states=("packed", "sorted")),
    _c("pack_0_to_2", "replace", ["rtr_set_option"], _pack(2), states=("pack0",)),
    # -- the sort on request: the error with the cloud intact, or success
    _c("reorder_points", "reorder", ["rtr_reorder_points"], _reorder()),
    # -- tolerant: RTR_OK, exact, the fallback visible
    _c("overlap_third_frame", "tolerant", ["rtr_render"], _overlap_third_frame(), states=("packed",)),
    # -- frame resources, made lazily: RTR_ERR_HIP, the cloud intact, and the call again is exact
    _c("render", "frame", ["rtr_render"], _render(False)),
    _c("render_filtered", "frame", ["rtr_render"], _render(True)),
    _c("set_resolution_render_filtered", "frame", ["rtr_set_resolution", "rtr_render"], _resolution_render(), states=("packed", "pack0")),
    _c("project_filtered_host", "frame", ["rtr_project_filtered"], _project(), states=("packed", "sorted")),
    _c("project_async_wait", "frame", ["rtr_project_async", "rtr_wait", "rtr_host_output_buffers"], _project_async(), states=("packed", "pack0")),
    _c("point_pass", "frame", ["rtr_point_pass"], _point_pass()),
    _c("render_views_3", "frame", ["rtr_render_views"], _render_views()),
    _c("render_views_3_after_1", "frame", ["rtr_render_views"], _views_after_one(), states=("packed",)),
    _c("p2p_export", "frame", ["rtr_p2p_export"], _p2p_export(), states=("packed",)),
]

# The caller outputs include/rtr.h promises untouched after an error, a failed allocation among them (sections 6g - 6i:
# "the selection and everything else are as they were, the caller's stats and labels included"; 6j: "with counts and stats
# untouched", "with plane and stats untouched"; 6k - 6m: "with nothing changed (... near_words and stats)", "(the four
# outputs and stats)", "(the three outputs and stats)"): these cases call through _raw, and the sweep asserts the sentinel.
# rtr_select_points' stats are asserted by select_points_first itself; rtr_extract_points' outputs are undefined (6e).
OUTPUTS_UNTOUCHED = {
    "select_voxel_grid": ("stats",), "select_neighbours": ("stats",), "select_clusters_labels": ("labels", "stats"),
    "count_in_bands": ("counts", "stats"), "fit_plane": ("plane", "stats"), "select_near_words": ("near_words", "stats"),
    "nearest_points_resident": ("resident_index", "resident_dist2", "stats"),
    "nearest_k_1": ("index", "dist2", "found", "stats"), "nearest_k_64": ("index", "dist2", "found", "stats"),
}

# Calls of the issue's list that allocate nothing in a state and are therefore not in that state's list
NO_ALLOCATION = {
    "select_points (a selection exists)": "every state holds a selection, and rtr_select_points allocates only the first "
                                          "selection's buffer: swept as select_points_first, behind rtr_clear_selection",
    "pack_0_to_2 on packed / sorted, pack_2_to_0 on pack0": "the option already has that value in those states' clouds",
}

# rtr_synchronize's repair of a frame that overflowed the adaptive pool needs a cloud of 2 000 000 points
# (pool_overflow_scenes.py): it is a case of its own in the GPU file, swept the same way on that cloud.
REPAIR_SYMBOLS = ("rtr_synchronize",)

# What the health check, the snapshots and the states' construction call on every context of the sweep, after a failure too
USED_BY_EVERY_CASE = ("rtr_create", "rtr_destroy", "rtr_last_error", "rtr_set_option", "rtr_get_option", "rtr_set_resolution",
                      "rtr_upload_points", "rtr_set_point_keep", "rtr_select_points", "rtr_set_clip_planes", "rtr_get_clip_planes",
                      "rtr_num_points", "rtr_extract_points", "rtr_download_buffer", "rtr_project_filtered", "rtr_point_pass",
                      "rtr_download_points")

NOT_SWEPT = {
    "rtr_abi_version": "a constant",
    "rtr_create": "out of scope: no context exists to arm the switch through (its allocations are all-or-nothing by reading)",
    "rtr_destroy": "frees only",
    "rtr_last_error": "reads a string",
    "rtr_default_params": "fills a struct",
    "rtr_set_params": "host state only",
    "rtr_get_params": "host state only",
    "rtr_set_stream": "host state only",
    "rtr_reset_stream": "host state only",
    "rtr_num_points": "reads a number",
    "rtr_compose_projection": "host arithmetic",
    "rtr_project": "rtr_project_filtered without the prefilter: the same sites, swept there and as render",
    "rtr_clear": "launches into the frame buffers rtr_set_resolution made",
    "rtr_min_depth_pass": "the pool and store of rtr_render (ensure_pool, ensure_store), swept there; mode 0 decodes through "
                          "ensure_soa, swept by download_points",
    "rtr_accumulate_pass": "as rtr_min_depth_pass",
    "rtr_resolve": "allocates nothing",
    "rtr_resolve_range": "allocates nothing",
    "rtr_filter": "the pyramid levels of render_filtered (ensure_levels)",
    "rtr_device_buffer": "hands out pointers",
    "rtr_download_buffer": "copies into the caller's memory; its repair is rtr_synchronize's",
    "rtr_timing_enable": "events only",
    "rtr_timing_reset": "host state only",
    "rtr_timing_get": "events only",
    "rtr_get_option": "reads; \"wide_chunks\" allocates one 16-byte scratch word pair, freed on every path",
    "rtr_stream_probe": "a measurement aid; decodes through ensure_soa, swept by download_points",
    "rtr_device_count": "no context",
    "rtr_p2p_open": "needs a second rank's handles for its mappings; its one allocation (the pointer table) was fixed by reading",
    "rtr_p2p_close": "frees only",
    "rtr_p2p_min_depth": "needs an open exchange; allocates nothing",
    "rtr_p2p_sum_resolve": "needs an open exchange; allocates nothing",
    "rtr_p2p_status": "reads a host word",
    "rtr_p2p_render": "needs an open exchange; the sites of rtr_render",
    "rtr_p2p_render_owned": "needs an open exchange; the sites of rtr_render",
    "rtr_frame_stats": "copies eight words out",
    "rtr_set_clip_planes": "host state only",
    "rtr_get_clip_planes": "host state only",
}


def swept_symbols():
    s = set(REPAIR_SYMBOLS)
    for c in CASES:
        s |= set(c.symbols)
    return s


def case_ids():
    return [(c.name, st) for c in CASES for st in c.states]


def by_name(name):
    return next(c for c in CASES if c.name == name)
