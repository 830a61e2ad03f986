"""rtr_select_segments (include/rtr_segments.h section 6q) without a GPU: the exported symbol, its own symbol list and
the unchanged ABI version; the header's prototype as a C99 consumer sees it and rtr.h's silence about it; the two
references of segments_ref.py against each other and against hand-written labels on the special clouds of
segments_cases.py; the zero-normal substitution of the library's gather; the pinned counts of the cases the GPU tests
use; Projector.select_segments' marshalling and argument validation against a fake library; the facade declarations in
both languages."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import clusters_ref as cr
import normals_ref as nref
import segments_cases as sc
import segments_ref as sg
from conftest import ROOT

f32 = np.float32


def test_segments_symbol_has_a_list_of_its_own(pkg):
    L = pkg._lib
    assert L.SEGMENTS_SYMBOLS == ["rtr_select_segments"]
    assert all("rtr_select_segments" not in s for s in (L.SYMBOLS, L.STATISTICS_SYMBOLS, L.NORMALS_SYMBOLS, L.REGISTER_SYMBOLS))
    assert L.STATISTICS_SYMBOLS == ["rtr_select_statistical"] and L.NORMALS_SYMBOLS == ["rtr_estimate_normals"]
    assert L.REGISTER_SYMBOLS == ["rtr_register_points"] and len(L.SYMBOLS) == 67
    assert hasattr(L.lib(), "rtr_select_segments")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert re.search(r"\bT rtr_select_segments$", nm, re.M)
    assert L.lib().rtr_abi_version() == 2 == L.ABI_VERSION
    assert (L.SEGMENT_SEEDED, L.SEGMENT_ORIENTED) == (1, 2)
    assert "SEGMENTS_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    at = L.lib().rtr_select_segments.argtypes
    assert len(at) == 12 and [k for k, t in enumerate(at) if t is C.c_float] == [1, 2, 5] and at[6] is C.c_uint32 and at[7] is C.c_uint32


def test_segments_header_declaration(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "rtr_segments.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int rtr_select_segments(rtr_ctx *ctx, float radius, float cos_angle, const float *normals, const float *curvature, "
            "float max_curvature, uint32_t min_points, uint32_t max_points, int flags, int op, uint32_t *labels, uint64_t stats[4]);") in flat
    assert re.search(r"#define RTR_SEGMENT_SEEDED\s+1\b", hdr) and re.search(r"#define RTR_SEGMENT_ORIENTED\s+2\b", hdr)
    assert '#include "rtr.h"' in hdr and "RTR_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    text = re.sub(r"[\s*]+", " ", hdr)
    for want in ("6q. selection by smooth segment", "((dx dx + dy dy) + dz dz) <= r2", "curvature[i] <= max_curvature", "A NaN curvature fails",
                 "dot = (nx_i nx_j + ny_i ny_j) + nz_i nz_j", "no FMA", "fabsf(dot) >= cos_angle", "RTR_SEGMENT_ORIENTED iff dot >= cos_angle",
                 "A NaN dot fails", "NOT checked for unit length", "connected components", "smallest upload index", "section 6i's, word for word",
                 "never written", "at most 32 B per point", "adds no option key", "normals == NULL", "NaN max_curvature", "unknown bits in flags",
                 "<= 0 or > 1", "ALWAYS waits"):
        assert want in text, want
    rtr_h = open(os.path.join(ROOT, "include", "rtr.h")).read()
    assert "#define RTR_ABI_VERSION 2" in rtr_h
    assert not re.search(r"rtr_select_segments|RTR_SEGMENT|rtr_segments\.h|\b6q\b", rtr_h)  # (rtr.h knows nothing of the call)
    src = tmp_path / "segments_abi.c"  # the prototype as a C99 consumer sees it, through this header alone
    src.write_text('#include "rtr_segments.h"\n'
                   "typedef int (*fn_t)(rtr_ctx *, float, float, const float *, const float *, float, uint32_t, uint32_t, int, int, uint32_t *, uint64_t[4]);\n"
                   "int main(void) { fn_t f = rtr_select_segments; return f == 0 || RTR_SEGMENT_SEEDED != RTR_CLUSTER_SEEDED || RTR_SEGMENT_ORIENTED != 2\n"
                   "                  || RTR_ABI_VERSION != 2; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "segments_abi.o")])


def test_facade_declarations_in_both_languages(pkg):
    hpp = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read())
    for decl in ("uint64_t selectSegments(float radius, uint32_t k, float angle, float max_curvature, uint32_t min_points = 1, "
                 "uint32_t max_points = 0, bool seeded = false, int op = RTR_SELECT_REPLACE, bool outside = false, uint32_t* labels = nullptr)",
                 "uint64_t removeSmallSegments(float radius, uint32_t k, float angle, float max_curvature, uint32_t min_points)",
                 '#include "rtr_segments.h"', "comes from libm", "no device allocator"):
        assert decl in hpp, decl
    pc = pkg.ProjectCloud
    assert list(inspect.signature(pc.selectSegments).parameters)[:6] == ["self", "radius", "k", "angle", "max_curvature", "min_points"]
    assert inspect.signature(pc.selectSegments).parameters["min_points"].default == 1
    assert list(inspect.signature(pc.removeSmallSegments).parameters) == ["self", "radius", "k", "angle", "max_curvature", "min_points"]
    assert "libm" in pc.selectSegments.__doc__ and "device=True" in inspect.getsource(pc.selectSegments)
    sig = inspect.signature(pkg.Projector.select_segments)
    assert list(sig.parameters) == ["self", "radius", "cos_angle", "normals", "curvature", "max_curvature", "min_points", "max_points", "seeded",
                                    "oriented", "op", "outside", "labels", "stats"]
    assert sig.parameters["max_curvature"].default == np.inf and sig.parameters["curvature"].default is None


# ---- the reference on special clouds ----------------------------------------------------------------------------------
def _args(case):
    return (case["xyz"], sc.R, case["cos_angle"], case["normals"], case["curvature"], case["max_curvature"], case["oriented"])


@pytest.mark.parametrize("name", sorted(sc.special_clouds()))
def test_both_references_give_the_labels_written_down_by_hand(name):
    case = sc.special_clouds()[name]
    with np.errstate(invalid="ignore"):
        a, b = sg.labels(*_args(case)), sg.labels_brute(*_args(case))
    assert a.dtype == np.uint32 and np.array_equal(a, case["labels"]), (name, a)
    assert np.array_equal(b, case["labels"]), (name, b)


@pytest.mark.parametrize("name", sorted(sc.special_clouds()))
def test_the_zero_normal_of_the_gather_gives_the_same_edges(name):
    case = sc.special_clouds()[name]
    xyz, r, cos_angle, normals, curvature, max_curvature, oriented = _args(case)
    with np.errstate(invalid="ignore"):
        want = sg.adjacency_brute(xyz, r, cos_angle, normals, curvature, max_curvature, oriented)
        got = sg.adjacency_brute(xyz, r, cos_angle, sg.gathered(normals, curvature, max_curvature), None, np.inf, oriented)
    assert np.array_equal(want, got) and np.array_equal(want, want.T)  # (and the relation is symmetric)
    if curvature is not None:
        assert not sg.gathered(normals, curvature, max_curvature)[~sg.usable(xyz.shape[0], curvature, max_curvature)].any()


def test_what_the_special_clouds_are_built_to_show():
    s = sc.special_clouds()
    assert sc.R * sc.R == f32(0.015625) and float(sc.R) ** 2 == 0.015625  # (the radius and its square are exact)
    up, tilt = f32([0, 0, 1]), s["fold_at_threshold"]["normals"][5]
    assert sg.dot(up, tilt) == sc.C08 == s["fold_at_threshold"]["cos_angle"]  # exactly the threshold: joined
    below = sg.dot(up, s["fold_one_ulp_below"]["normals"][5])
    assert below == np.nextafter(sc.C08, f32(0)) and below < sc.C08  # one ulp below: split
    assert sg.dot(s["fold_oriented"]["normals"][0], s["fold_oriented"]["normals"][5]) == sc.C08
    lim = s["curvature_at_limit"]["max_curvature"]
    assert s["curvature_at_limit"]["curvature"][2] == lim and s["curvature_next_float"]["curvature"][2] == np.nextafter(lim, f32(1))
    # the sheets: by |dot| the opposite normals agree; plain clustering gives the same single cluster
    assert (cr.labels(s["sheets"]["xyz"], sc.R) == 0).all()
    with np.errstate(invalid="ignore"):
        bad = s["bad_normals_and_curvature"]
        d = sg.dot(bad["normals"][:, None, :], bad["normals"][None, :, :])
        assert np.isnan(d[3]).all() and np.isnan(d[5, [0, 6]]).all() and (d[1] == 0).sum() == 9  # NaN, inf * 0, the zero normal
        assert (cr.labels(bad["xyz"], sc.R) == 0).all()  # (every point is every other's neighbour)


def test_constant_normals_without_curvature_are_plain_clustering(orc):
    n = 6001
    xyzw, _ = orc.generate("room_shell", 3, 0, n, n)
    for nrm in (f32([0, 0, 1]), f32([0.6, 0, -0.8]), f32([1, 1, 1])):  # (|n|^2 = 3: unit length is not asked for)
        for r in (0.08, 0.2):
            lab = sg.labels(xyzw, r, 0.99, np.tile(nrm, (n, 1)))
            assert np.array_equal(lab, cr.labels(xyzw, r)) and 1 < (lab == np.arange(n)).sum() < n
    # ... while a cos_angle above the normals' own square keeps nothing
    assert np.array_equal(sg.labels(xyzw, 0.2, 1.0, np.tile(f32([0.6, 0, 0.6]), (n, 1))), np.arange(n))


def test_subsampled_cases_agree_with_the_brute_reference(orc):
    for name, (scene, n, radius, _) in sc.CASES.items():
        xyzw, _, normals, curvature, max_curvature = sc.make(orc, nref, name)
        sub = np.sort(np.random.default_rng(5).choice(n, 3000, replace=False))
        args = (xyzw[sub], 3 * radius, sc.COS_ANGLE, normals[sub], None if curvature is None else curvature[sub], max_curvature)
        a, b = sg.labels(*args), sg.labels_brute(*args)
        assert np.array_equal(a, b) and 100 < (a == np.arange(3000)).sum() < 3000, name


@pytest.fixture(scope="module")
def case_labels(orc):
    out = {}
    for name, (scene, n, radius, _) in sc.CASES.items():
        xyzw, _, normals, curvature, max_curvature = sc.make(orc, nref, name)
        out[name] = (xyzw, curvature, sg.labels(xyzw, radius, sc.COS_ANGLE, normals, curvature, max_curvature))
    return out


def test_the_pinned_counts_of_the_gpu_cases_hold(case_labels):
    spread = 0
    for name, (segments, segments2, largest, hit_counts) in sc.PINS.items():
        scene, n, radius, max_curvature = sc.CASES[name]
        xyzw, curvature, lab = case_labels[name]
        sz = sg.sizes(lab)
        roots = lab == np.arange(n)
        got = tuple(int(sg.hits(lab, lo, hi).sum()) for lo, hi in sc.WINDOWS)
        assert (int(roots.sum()), int((roots & (sz >= 2)).sum()), int(sz.max()), got) == (segments, segments2, largest, hit_counts), name
        for w in sc.SPREAD[name]:
            assert sc.spread_holds(segments2, largest, got[sc.WINDOWS.index(w)], n), (name, w)
            spread += 1
        if name in sc.FACES:
            assert tuple(sorted(np.bincount(lab)[np.unique(lab)])[::-1][:6]) == sc.FACES[name]
        if name in sc.USABLE:
            assert int(sg.usable(n, curvature, max_curvature).sum()) == sc.USABLE[name]
    assert spread == 4 and (50, 0) in sc.SPREAD["room"] and set(sc.PINS) == set(sc.CASES) == set(sc.SPREAD)
    assert sc.PINS["box"][2] <= 11
    # what the call is for: plain clustering at the same radius has one cluster above 85 % of the points
    xyzw = case_labels["room"][0]
    plain = cr.labels(xyzw, sc.CASES["room"][2])
    n = plain.size
    assert (int((plain == np.arange(n)).sum()), int(cr.sizes(plain).max())) == sc.PLAIN_ROOM and cr.sizes(plain).max() > 0.85 * n
    assert sc.PINS["room"][2] < 0.25 * n  # ... against faces


# ---- Projector.select_segments against a fake library -----------------------------------------------------------------
class _Lib:
    def __init__(self):
        self.calls = []

    def rtr_select_segments(self, ctx, radius, cos_angle, normals, curvature, max_curvature, min_points, max_points, flags, op, labels, stats):
        ptr = lambda p: p if p is None else (p.value if isinstance(p, C.c_void_p) else C.cast(p, C.c_void_p).value)  # noqa: E731
        self.calls.append({"radius": radius, "cos": cos_angle, "normals": ptr(normals), "curvature": ptr(curvature), "max_curvature": max_curvature,
                           "min": min_points, "max": max_points, "flags": flags, "op": op, "labels": labels is not None, "stats": stats is not None})
        if stats is not None:
            out = C.cast(stats, C.POINTER(C.c_uint64))
            for k in range(4):
                out[k] = 20 + k
        if labels is not None:
            out = C.cast(labels, C.POINTER(C.c_uint32))
            for k in range(5):
                out[k] = 4 - k
        return 0


class _Cai:  # an object with __cuda_array_interface__ (a device array as cupy or numba hand it over)
    def __init__(self, shape, ptr, typestr="<f4", strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


def _stub(pkg):
    class Stub:
        _ctx = None
        _lib = _Lib()
        _SELECT_OPS = pkg.Projector._SELECT_OPS
        num_points = 5
        select_segments = pkg.Projector.select_segments
        _write_source = staticmethod(pkg.Projector._write_source)
        _curvature_source = staticmethod(pkg.Projector._curvature_source)

        def _chk(self, rc):
            assert rc == 0
    return Stub()


def test_select_segments_marshals_and_validates(pkg):
    import torch
    L = pkg._lib
    s = _stub(pkg)
    nrm = np.arange(15, dtype=f32).reshape(5, 3)
    curv = np.arange(5, dtype=f32)
    cos = f32(0.9659258)
    assert s.select_segments(0.05, cos, nrm) == (20, 21, 22, 23)
    assert s._lib.calls[-1] == {"radius": 0.05, "cos": float(cos), "normals": nrm.ctypes.data, "curvature": None, "max_curvature": 0.0, "min": 1,
                                "max": 0, "flags": 0, "op": L.SELECT_REPLACE, "labels": False, "stats": True}
    assert s.select_segments(f32(0.25), 0.5, nrm, curv, 0.02, np.uint32(2), np.uint32(49), seeded=True, oriented=True, op="toggle",
                             outside=True, stats=False) is None
    assert s._lib.calls[-1] == {"radius": 0.25, "cos": 0.5, "normals": nrm.ctypes.data, "curvature": curv.ctypes.data, "max_curvature": float(f32(0.02)),
                                "min": 2, "max": 49, "flags": L.SEGMENT_SEEDED | L.SEGMENT_ORIENTED, "op": L.SELECT_TOGGLE | L.SELECT_OUTSIDE,
                                "labels": False, "stats": False}
    assert s.select_segments(0.1, 1.0, nrm, oriented=True, stats=False) is None and s._lib.calls[-1]["flags"] == L.SEGMENT_ORIENTED
    assert s.select_segments(0.1, 1.0, nrm, seeded=True, stats=False) is None and s._lib.calls[-1]["flags"] == L.SEGMENT_SEEDED
    st, lab = s.select_segments(0.1, cos, nrm, curv, np.inf, 50, labels=True)
    assert st == (20, 21, 22, 23) and lab.dtype == np.uint32 and list(lab) == [4, 3, 2, 1, 0] and s._lib.calls[-1]["max_curvature"] == np.inf
    lab = s.select_segments(0.1, cos, nrm, curv, -np.inf, 3, 3, labels=True, stats=False)
    assert isinstance(lab, np.ndarray) and list(lab) == [4, 3, 2, 1, 0] and s._lib.calls[-1]["max_curvature"] == -np.inf
    for op in ("add", "subtract", "intersect"):
        s.select_segments(1, cos, nrm, op=op)
        assert s._lib.calls[-1]["op"] == pkg.Projector._SELECT_OPS[op]
    # both array kinds: torch tensors in host memory, objects with __cuda_array_interface__, lists numpy converts
    tn, tc = torch.from_numpy(nrm), torch.from_numpy(curv)
    s.select_segments(0.1, cos, tn, tc, 0.5)
    assert (s._lib.calls[-1]["normals"], s._lib.calls[-1]["curvature"]) == (tn.data_ptr(), tc.data_ptr())
    s.select_segments(0.1, cos, _Cai((5, 3), 0x7000), _Cai((5,), 0x9000), 0.5)
    assert (s._lib.calls[-1]["normals"], s._lib.calls[-1]["curvature"]) == (0x7000, 0x9000)
    s.select_segments(0.1, cos, nrm.tolist(), curv.reshape(5, 1), 0.5)
    assert s._lib.calls[-1]["normals"] not in (None, nrm.ctypes.data)
    made = len(s._lib.calls)
    for radius in (0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="radius"):
            s.select_segments(radius, cos, nrm)
    for bad in (0, -0.0, -0.5, 1.0000001, 2, np.nan, np.inf, -np.inf, 1e-60):  # (1e-60 is 0 as a float32)
        with pytest.raises(ValueError, match="cos_angle"):
            s.select_segments(0.1, bad, nrm)
    with pytest.raises(ValueError, match="normals"):
        s.select_segments(0.1, cos, None)
    for bad in (nrm[:4], np.zeros((5, 4), f32), np.zeros(15, f32), np.zeros((6, 3), f32), torch.zeros((5, 3), dtype=torch.float64),
                _Cai((5, 3), 0x7000, strides=(16, 4)), _Cai((4, 3), 0x7000)):
        with pytest.raises(ValueError, match="normals"):
            s.select_segments(0.1, cos, bad)
    for bad in (curv[:4], np.zeros((5, 2), f32), np.zeros(6, f32), torch.zeros(5, dtype=torch.float64), torch.zeros(10)[::2],
                _Cai((5,), 0x9000, "<f8"), _Cai((5,), 0x9000, strides=(8,))):
        with pytest.raises(ValueError, match="curvature"):
            s.select_segments(0.1, cos, nrm, bad, 0.5)
    with pytest.raises(ValueError, match="max_curvature"):
        s.select_segments(0.1, cos, nrm, curv, np.nan)
    s.select_segments(0.1, cos, nrm, None, np.nan)  # (not read without a curvature array)
    assert s._lib.calls[-1]["max_curvature"] == 0.0 and len(s._lib.calls) == made + 1
    for k in (0, -1, 2 ** 32):
        with pytest.raises(ValueError, match="min_points"):
            s.select_segments(0.1, cos, nrm, min_points=k)
    for lo, hi in ((2, 1), (50, 49), (1, -1), (1, 2 ** 32)):
        with pytest.raises(ValueError, match="max_points"):
            s.select_segments(0.1, cos, nrm, min_points=lo, max_points=hi)
    with pytest.raises(KeyError):
        s.select_segments(0.1, cos, nrm, op="xor")
    assert len(s._lib.calls) == made + 1
