"""rtr_select_voxel_grid (include/rtr.h section 6g) without a GPU: the exported symbol, its place in _lib.SYMBOLS, the
header prototype compiled as C99 and the facade declarations; Projector.select_voxel_grid against a fake library
(scalar and 3-vector cells, op names, outside, stats=False, the argument errors); the numpy reference of voxel_ref.py
against a per-point dictionary loop; the identity of the statistics."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import voxel_ref as vr
from conftest import ROOT


def test_voxel_symbol_exported(pkg):
    L = pkg._lib
    assert "rtr_select_voxel_grid" in L.SYMBOLS
    getattr(L.lib(), "rtr_select_voxel_grid")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert re.search(r"\bT rtr_select_voxel_grid$", nm, re.M)
    assert L.lib().rtr_abi_version() == 2


def test_voxel_header_declaration(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    proto = ("int rtr_select_voxel_grid(rtr_ctx *ctx, const float origin[3], const float cell[3], uint32_t min_count, "
             "int op, uint64_t stats[4]);")
    assert proto in re.sub(r"\s+", " ", hdr)
    assert "#define RTR_ABI_VERSION 2" in hdr
    assert "6g. selection by density" in hdr
    assert hdr.index("6f. selection") < hdr.index("6g. selection by density") < hdr.index("7. measurement")
    src = tmp_path / "voxel_abi.c"  # the prototype as a C99 consumer sees it
    src.write_text('#include "rtr.h"\n'
                   "typedef int (*fn_t)(rtr_ctx *, const float[3], const float[3], uint32_t, int, uint64_t[4]);\n"
                   "int main(void) { fn_t f = rtr_select_voxel_grid; return f == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "voxel_abi.o")])
    hpp = open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read()
    flat = re.sub(r"\s+", " ", hpp)
    for decl in ("uint64_t selectVoxelGrid(const float cell[3], const float origin[3] = nullptr, uint32_t min_count = 1, "
                 "int op = RTR_SELECT_REPLACE, bool outside = false)", "uint64_t thin(float cell)"):
        assert decl in flat, decl


# ---- Projector.select_voxel_grid against a fake library ---------------------------------------------------------------
class _Lib:
    def __init__(self):
        self.calls = []

    def rtr_select_voxel_grid(self, ctx, origin, cell, min_count, op, stats):
        f3 = lambda p: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), (3,)).copy()  # noqa: E731
        self.calls.append({"origin": f3(origin), "cell": f3(cell), "min_count": min_count, "op": op, "stats": stats is not None})
        if stats is not None:
            out = C.cast(stats, C.POINTER(C.c_uint64))
            for k in range(4):
                out[k] = 10 + k
        return 0


def _stub(pkg):
    class Stub:
        _ctx = None
        _lib = _Lib()
        _SELECT_OPS = pkg.Projector._SELECT_OPS
        select_voxel_grid = pkg.Projector.select_voxel_grid

        def _chk(self, rc):
            assert rc == 0
    return Stub()


def test_select_voxel_grid_marshals_cells_ops_and_stats(pkg):
    L = pkg._lib
    s = _stub(pkg)
    f = np.float32
    assert s.select_voxel_grid(0.05) == (10, 11, 12, 13)
    call = s._lib.calls[-1]
    assert np.array_equal(call["cell"], f([0.05, 0.05, 0.05])) and np.array_equal(call["origin"], f([0, 0, 0]))
    assert call["min_count"] == 1 and call["op"] == L.SELECT_REPLACE and call["stats"]
    assert s.select_voxel_grid((0.25, 0.5, 0.125), origin=(0.013, -0.4, 0), min_count=3, op="add", outside=True) == (10, 11, 12, 13)
    call = s._lib.calls[-1]
    assert np.array_equal(call["cell"], f([0.25, 0.5, 0.125])) and np.array_equal(call["origin"], f([0.013, -0.4, 0]))
    assert call["min_count"] == 3 and call["op"] == (L.SELECT_ADD | L.SELECT_OUTSIDE)
    for name, code in (("replace", 0), ("add", 1), ("subtract", 2), ("intersect", 3), ("toggle", 8)):
        s.select_voxel_grid(np.float64(1000), op=name)
        assert s._lib.calls[-1]["op"] == code and np.array_equal(s._lib.calls[-1]["cell"], f([1000, 1000, 1000]))
        s.select_voxel_grid(1, op=code, outside=True)
        assert s._lib.calls[-1]["op"] == code | 4
    assert s.select_voxel_grid(np.float32([1, 2, 3]), stats=False) is None
    assert not s._lib.calls[-1]["stats"] and np.array_equal(s._lib.calls[-1]["cell"], f([1, 2, 3]))
    assert s.select_voxel_grid(1, min_count=0xFFFFFFFF) and s._lib.calls[-1]["min_count"] == 0xFFFFFFFF


def test_select_voxel_grid_argument_rules(pkg):
    s = _stub(pkg)
    before = len(s._lib.calls)
    for kw in (dict(cell=(1, 2)), dict(cell=(1, 2, 3, 4)), dict(cell=1, origin=(0, 0)), dict(cell=1, origin=0.5),
               dict(cell=1, min_count=0), dict(cell=1, min_count=-1), dict(cell=1, min_count=1 << 32)):
        with pytest.raises(ValueError):
            s.select_voxel_grid(**kw)
    with pytest.raises(KeyError):
        s.select_voxel_grid(1, op="xor")
    assert len(s._lib.calls) == before  # (none of them reached the library)


# ---- the reference ------------------------------------------------------------------------------------------------------
def _cloud():
    rng = np.random.default_rng(5)
    pts = (rng.normal(size=(3000, 3)) * [2, 1.5, 0.5]).astype(np.float32)
    pts[rng.choice(np.arange(100, 2990), 100, replace=False)] = pts[:100]  # (100 exact duplicates)
    pts[[2997, 2998, 2999]] = [[np.nan, 0, 0], [0, np.inf, 0], [3e6, 0, 0]]
    return pts


def test_voxel_ref_equals_the_per_point_loop():
    pts = _cloud()
    for cell, origin in ((0.25, (0, 0, 0)), (0.05, (0.013, -0.4, 0)), ((0.25, 0.5, 0.125), (0.013, -0.4, 0)), (1000, (0, 0, 0))):
        for mc in (1, 2, 3, 257):
            hit, st = vr.select(pts, cell, origin, mc)
            hit2, st2 = vr.select_loop(pts, cell, origin, mc)
            assert np.array_equal(hit, hit2) and st == st2, (cell, mc)
    hit, st = vr.select(pts, 0.25)
    assert st[2] == 2 + (1 if 3e6 * 4 >= 2 ** 20 else 0) and hit[[2997, 2998, 2999]].all()
    assert not vr.select(pts, 0.25, min_count=2)[0][[2997, 2998, 2999]].any()
    dup = vr.select(pts, 1e-3)[0]  # (cells so small that only the exact duplicates share one)
    assert int((~dup).sum()) == 100 and dup[:100].all()


def test_stats_identity_and_counts():
    pts = _cloud()
    for cell in (0.05, 0.25, 1000):
        seen = None
        for mc in (1, 2, 3, 257):
            hit, (cells, full, out) = vr.select(pts, cell, (0.013, -0.4, 0), mc)
            assert int(hit.sum()) == full + (out if mc == 1 else 0)
            assert out == (3 if 3e6 / cell >= 2 ** 20 else 2) and full <= cells  # (NaN, inf, and 3e6 where it is past 2^20 cells) and (seen is None or full <= seen)
            assert mc != 1 or full == cells
            seen = full
    # keys_u64: bit 63 exactly for the points out of the grid, and equal keys exactly for equal cells
    k = vr.keys_u64(pts, 0.25)
    ok, key = vr.cells(pts, 0.25)
    assert np.array_equal((k >> np.uint64(63)).astype(bool), ~ok) and np.array_equal(k[ok], key[ok].astype(np.uint64))
