"""Writing points back (include/rtr.h section 2f), the parts a CPU can check: the exported symbol and its place in
_lib.SYMBOLS, the header's prototype, Projector.write_points' marshalling against a fake library (None streams, the
strides 12 / 16 / 28 and 3 / 4 / 7, a broadcast colour as stride 0, device pointers passed through, mismatched rows),
the host statement write_ref.written against a per-point loop, the sequences of write_model.py (pure, covering, the
model equal to the statement) and the poses of the GPU files: on every written cloud they check, the oracle's filtered
frame keeps at least 64 pixels whenever at least 256 finite points are drawable."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edit_model as em
import helpers
import write_cases as wc
import write_model as wm
import write_ref
from conftest import ROOT


def test_write_symbol_exported(pkg):
    L = pkg._lib
    assert "rtr_write_points" in L.SYMBOLS
    getattr(L.lib(), "rtr_write_points")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert re.search(r"\bT rtr_write_points$", nm, re.M)
    assert L.lib().rtr_abi_version() == 2


def test_write_header_declaration():
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    proto = ("int rtr_write_points(rtr_ctx *ctx, const uint32_t *select_words, uint64_t nwords, uint64_t first, "
             "uint64_t count, const float *xyz, size_t xyz_stride_bytes, const uint8_t *rgb, size_t rgb_stride_bytes, "
             "uint64_t *total);")
    assert proto in re.sub(r"\s+", " ", hdr)
    assert "#define RTR_ABI_VERSION 2" in hdr
    assert "2f. writing points back" in hdr
    hpp = open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read()
    for decl in ("uint64_t writeSelected(const std::vector<float>& vertices, const std::vector<uint8_t>& colors)",
                 "uint64_t writePoints(uint64_t first, uint64_t count, const std::vector<float>& vertices, const std::vector<uint8_t>& colors)",
                 "uint64_t colorSelected(uint8_t c0, uint8_t c1, uint8_t c2)"):
        assert decl in hpp, decl


# ---- Projector.write_points against a fake library ------------------------------------------------------------------
_DEVICE_PTR = 0x7000000


class _Lib:
    def __init__(self, k):
        self.calls, self.k = [], k

    def rtr_write_points(self, ctx, words, nwords, first, count, xyz, xs, rgb, rs, total):
        def ptr(p):
            return p.value if isinstance(p, C.c_void_p) else p

        def rows(p, stride, width, dt, n):
            """The first `width` elements of n records at `stride` bytes, read the way the library reads them."""
            if p is None or p >= _DEVICE_PTR and p < _DEVICE_PTR + (1 << 20):
                return p
            item = np.dtype(dt).itemsize
            raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), ((n - 1) * stride + width * item,)) if n else np.zeros(0, np.uint8)
            return np.array([raw[j * stride:j * stride + width * item].view(dt) for j in range(n)]).reshape(n, width)
        wp = ptr(words)
        w = wp if wp is None or wp == _DEVICE_PTR else np.ctypeslib.as_array(C.cast(wp, C.POINTER(C.c_uint32)), (nwords,)).copy()
        m = min(count, max(0, self.k - first))
        self.calls.append({"words": w, "nwords": nwords, "first": first, "count": count, "xs": xs, "rs": rs,
                           "xyz": rows(ptr(xyz), xs, 3, np.float32, m), "rgb": rows(ptr(rgb), rs, 3, np.uint8, 1 if rs == 0 and m else m)})
        C.cast(total, C.POINTER(C.c_uint64))[0] = self.k
        return 0


def _stub(pkg, n, k):
    class Stub:
        num_points = n
        _ctx = None
        _lib = _Lib(k)
        _keep_words = pkg.Projector._keep_words
        _write_source = staticmethod(pkg.Projector._write_source)

        def _chk(self, rc):
            assert rc == 0
    return Stub()


class _Device:
    """An object with __cuda_array_interface__: its pointer must reach the library untouched."""

    def __init__(self, shape, typestr, strides=None, offset=0):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (_DEVICE_PTR + offset, False), "version": 2,
                                         "strides": strides}


def test_write_points_marshals_streams_strides_and_selection(pkg):
    n, k = 70, 23
    sel = np.arange(n) % 3 == 1
    assert int(sel.sum()) == k
    s = _stub(pkg, n, k)
    wp = pkg.Projector.write_points
    rng = np.random.default_rng(1)
    for cols_x, cols_c in ((3, 3), (4, 4), (7, 7)):  # strides 12 / 16 / 28 and 3 / 4 / 7
        X = rng.standard_normal((k, cols_x)).astype(np.float32)
        Cc = rng.integers(0, 256, (k, cols_c), dtype=np.uint8)
        assert wp(s, X, Cc, sel) == k
        c = s._lib.calls[-1]
        assert (c["xs"], c["rs"], c["first"], c["count"], c["nwords"]) == (4 * cols_x, cols_c, 0, k, 3)
        assert np.array_equal(c["xyz"].view(np.uint32), X[:, :3].view(np.uint32)) and np.array_equal(c["rgb"], Cc[:, :3])
        assert np.array_equal(np.unpackbits(c["words"].view(np.uint8), bitorder="little")[:n].astype(bool), sel)
        # a view with a row stride of its own (every other row of a wider array): the stride is the array's
        wide = rng.standard_normal((2 * k, cols_x)).astype(np.float32)
        assert wp(s, wide[::2], None, sel, first=2) == k - 2
        c = s._lib.calls[-1]
        assert c["xs"] == 8 * cols_x and c["rs"] == 0 and c["rgb"] is None and c["first"] == 2 and c["count"] == k
        assert np.array_equal(c["xyz"].view(np.uint32), wide[::2][:k - 2, :3].view(np.uint32))
    # None streams
    X = rng.standard_normal((5, 3)).astype(np.float32)
    assert wp(s, X) == 5
    c = s._lib.calls[-1]
    assert c["words"] is None and c["nwords"] == 0 and c["rgb"] is None and c["count"] == 5
    Cc = rng.integers(0, 256, (9, 4), dtype=np.uint8)
    assert wp(s, None, Cc, sel, first=20) == 3  # (k - first = 3 of the 9 records)
    c = s._lib.calls[-1]
    assert c["xyz"] is None and c["xs"] == 0 and c["rs"] == 4 and np.array_equal(c["rgb"], Cc[:3, :3])
    # lists and float64 are converted; NaN payloads of float32 arrays pass bit for bit
    assert wp(s, [[1, 2, 3], [4, 5, 6]], [[7, 8, 9], [1, 2, 3]]) == 2
    assert np.array_equal(s._lib.calls[-1]["xyz"], np.float32([[1, 2, 3], [4, 5, 6]]))
    odd = np.array([[0x7FC00001, 0x80000000, 0x00000001]], np.uint32).view(np.float32)
    wp(s, odd)
    assert np.array_equal(s._lib.calls[-1]["xyz"].view(np.uint32), odd.view(np.uint32))
    # a broadcast colour: stride 0, one record, to the last selected point
    for colour in (np.uint8([1, 2, 3]), np.uint8([[1, 2, 3]]), np.uint8([[1, 2, 3, 255]]), [1, 2, 3]):
        assert wp(s, None, colour, sel, broadcast=True) == k
        c = s._lib.calls[-1]
        assert c["rs"] == 0 and c["count"] == 2 ** 64 - 1 and np.array_equal(c["rgb"], [[1, 2, 3]])
    assert wp(s, X, np.uint8([1, 2, 3]), sel, first=1, broadcast=True) == 5
    assert s._lib.calls[-1]["count"] == 5 and s._lib.calls[-1]["rs"] == 0
    # device memory is passed through: the selection and both streams
    dx, dc = _Device((k, 4), "<f4"), _Device((k, 4), "|u1", offset=4096)
    assert wp(s, dx, dc, _DEVICE_PTR) == k
    c = s._lib.calls[-1]
    assert c["words"] == _DEVICE_PTR and c["xyz"] == _DEVICE_PTR and c["rgb"] == _DEVICE_PTR + 4096 and (c["xs"], c["rs"]) == (16, 4)
    assert wp(s, _Device((k, 3), "<f4", strides=(28, 4)), None, sel) == k
    assert s._lib.calls[-1]["xs"] == 28
    # one stream on the host, the other on the device
    assert wp(s, dx, rng.integers(0, 256, (k, 3), dtype=np.uint8), sel) == k
    assert s._lib.calls[-1]["xyz"] == _DEVICE_PTR and s._lib.calls[-1]["rgb"].shape == (k, 3)


def test_write_points_argument_rules(pkg):
    s = _stub(pkg, 70, 23)
    wp = pkg.Projector.write_points
    calls = len(s._lib.calls)
    with pytest.raises(ValueError):
        wp(s)  # both streams None
    with pytest.raises(ValueError):
        wp(s, np.zeros((4, 3), np.float32), np.zeros((5, 3), np.uint8))  # mismatched rows
    with pytest.raises(ValueError):
        wp(s, np.zeros((4, 2), np.float32))  # fewer than 3 columns
    with pytest.raises(ValueError):
        wp(s, np.zeros(12, np.float32))  # not 2-D
    with pytest.raises(ValueError):
        wp(s, np.zeros((3, 4, 3), np.float32))
    with pytest.raises(ValueError):
        wp(s, np.zeros((4, 6), np.float32)[:, ::2])  # columns not contiguous
    with pytest.raises(ValueError):
        wp(s, None, np.zeros((2, 3), np.uint8), broadcast=True)  # a broadcast colour is ONE record
    with pytest.raises(ValueError):
        wp(s, np.zeros((4, 3), np.float32), broadcast=True)  # nothing to broadcast
    with pytest.raises(ValueError):
        wp(s, np.zeros((4, 3), np.float32), None, np.ones(69, bool))  # the selection's own rule
    assert len(s._lib.calls) == calls


# ---- the host statement ---------------------------------------------------------------------------------------------
def _loop(xyz, rgb, sel, first, X, Cc):
    xyz, rgb = xyz.copy(), rgb.copy()
    n = xyz.shape[0]
    one = Cc is not None and np.ndim(Cc) == 1
    count = len(X) if X is not None else (n if one else len(Cc))
    rank, touched = 0, []
    for i in range(n):
        if sel is not None and not sel[i]:
            continue
        j = rank - first
        rank += 1
        if j < 0 or j >= count:
            continue
        touched.append(i)
        if X is not None:
            for a in range(3):
                xyz[i, a] = X[j][a]
        if Cc is not None:
            for a in range(3):
                rgb[i, a] = Cc[a] if one else Cc[j][a]
    return xyz, rgb, np.array(touched, np.int64)


def test_written_equals_the_per_point_loop():
    rng = np.random.default_rng(2)
    for n in (1, 2, 31, 32, 33, 70, 257, 600):
        xyzw, rgba = helpers.random_cloud(n, n)
        for sel in (None, rng.random(n) < 0.4, np.zeros(n, bool), np.ones(n, bool), np.arange(n) == n - 1):
            k = n if sel is None else int(sel.sum())
            for first, count in wc.windows(k) + [(0, k + 3), (1, 2)]:
                X, Cc = wc.records("specials", count, first)
                for xs, cs in ((X, Cc), (X, None), (None, Cc), (None, np.uint8([4, 5, 6])), (X, np.uint8([4, 5, 6]))):
                    got = write_ref.written(xyzw, rgba, sel, first, xs, cs)
                    want = _loop(xyzw, rgba, sel, first, xs, cs)
                    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (n, first, count)
                    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (n, first, count)
                    assert np.array_equal(got[0][:, 3], xyzw[:, 3]) and np.array_equal(got[1][:, 3], rgba[:, 3])  # (further columns stay)
    # the inputs are not changed
    xyzw, rgba = helpers.random_cloud(40, 1)
    keep = xyzw.copy(), rgba.copy()
    write_ref.written(xyzw, rgba, None, 0, np.zeros((40, 3), np.float32), np.zeros((40, 3), np.uint8))
    assert np.array_equal(xyzw, keep[0]) and np.array_equal(rgba, keep[1])


# ---- the sequences of write_model.py ----------------------------------------------------------------------------------
def test_write_sequences_are_pure_cover_the_forms_and_match_the_statement():
    for family in wm.WRITE_FAMILIES:
        streams, sources, forms, hits = set(), set(), set(), 0
        can_sort = em.allows_reorder(family) or em.FAMILIES[family].get("auto_reorder") == 1
        for seed in wm.SEEDS:
            recs = wm.sequence(seed, family, wm.STEPS)
            assert recs == wm.sequence(seed, family, wm.STEPS) and len(recs) == wm.STEPS
            model = wm.Model(family)
            for rec in recs:
                args = wm.materialize(rec, model)
                before = model.copy()
                wm.apply(model, rec, args)
                assert 0 <= model.n <= em.N_MAX
                if rec["call"] != "write":
                    continue
                st = rec["state"]
                assert st["masked"] == (before.keep is not None) and st["sorted"] == before.sorted
                x1, c1, idx = write_ref.written(before.xyz, before.rgb, args["bits"], args["first"], args["X"], args["C"])
                assert idx.size == st["points"]
                assert np.array_equal(model.xyz.view(np.uint32), x1.view(np.uint32)) and np.array_equal(model.rgb, c1)
                assert np.array_equal(model.keep, before.keep) if before.keep is not None else model.keep is None
                assert st["behind"] == bool(idx.size and (idx.max() // 256 + 1) * 256 < before.n)
                streams.add(rec["streams"]); sources.add(rec["source"]); forms.add(rec["form"])
                hits += bool(st["points"] and st["behind"] and st["masked"] and (st["sorted"] or not can_sort))
        assert streams == set(wm.STREAMS) and sources == {"host", "device"}, (family, streams, sources)
        assert {"bool", "words", None} <= forms, (family, forms)
        assert hits, family  # (a write behind a mask, in front of resident points, on a sorted cloud where one can be)


# ---- the poses of the GPU files ---------------------------------------------------------------------------------------
def _filled(orc, model, k):
    d = model.drawable()
    xyzw, rgba = helpers.cloud(model.xyz[d], model.rgb[d])
    r = orc.project(xyzw, rgba, em.pose_for(model, k), em.W, em.H)
    f = orc.filter(r["depth_bits"], r["img"])
    finite = int(np.isfinite(xyzw[:, :3]).all(1).sum())
    kept = (f["depth"] > 0) & (f["depth"].view(np.uint32) != orc.EMPTY_DEPTH)  # (removed pixels hold -1, empty ones EMPTY_DEPTH)
    return finite, int(kept.sum())


def test_every_checked_frame_of_the_write_cases_shows_something(orc):
    frames = nontrivial = 0
    for n in wc.COUNTS:
        for name in wc.names(n):
            for j, (st, model) in enumerate(wc.replay(name, n)):
                finite, kept = _filled(orc, model, j)
                frames += 1
                if finite >= 256:
                    nontrivial += 1
                    assert kept >= 64, (name, n, j, finite, kept)
    assert nontrivial >= frames // 2, (frames, nontrivial)


def test_every_checked_frame_of_the_write_sequences_shows_something(orc):
    for family in wm.WRITE_FAMILIES:
        for seed in wm.SEEDS:
            recs, model = wm.sequence(seed, family, wm.STEPS), wm.Model(family)
            checks = {i: [i] for i in wm.frame_steps(wm.STEPS)}
            checks[wm.STEPS - 1] = checks.get(wm.STEPS - 1, []) + em.final_poses(wm.STEPS)
            for i, rec in enumerate(recs):
                wm.apply(model, rec, wm.materialize(rec, model))
                for k in checks.get(i, []):
                    finite, kept = _filled(orc, model, k)
                    if finite >= 256:
                        assert kept >= 64, (family, seed, i, k, finite, kept)
