"""rtr_select_neighbours (include/rtr.h section 6h) without a GPU: the exported symbol and the ABI version, the header's
prototype and its statement of the neighbour relation, the facade declarations; the two numpy references of
neighbours_ref.py against each other (their grids differ from the library's) and on special coordinates; the hit counts
of the scenes the GPU tests use, pinned and spread; Projector.select_neighbours' argument validation against a fake
library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import neighbours_cases as nc
import neighbours_ref as nr
from conftest import ROOT


def test_neighbours_symbol_exported(pkg):
    L = pkg._lib
    assert "rtr_select_neighbours" in L.SYMBOLS
    getattr(L.lib(), "rtr_select_neighbours")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert re.search(r"\bT rtr_select_neighbours$", nm, re.M)
    assert L.lib().rtr_abi_version() == 2


def test_neighbours_header_declaration(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    assert "int rtr_select_neighbours(rtr_ctx *ctx, float radius, uint32_t min_neighbours, int op, uint64_t stats[4]);" in \
        re.sub(r"\s+", " ", hdr)
    assert "#define RTR_ABI_VERSION 2" in hdr
    assert hdr.index("6g. selection by density") < hdr.index("6h. selection by neighbour count") < hdr.index("7. measurement")
    sec = flat[flat.index("6h. selection by neighbour count"):flat.index("int rtr_select_neighbours(")]
    for text in ("((dx dx + dy dy) + dz dz) <= r2", "r2 = radius radius, rounded once to fp32 on the host", "no FMA",
                 "The comparison is inclusive", "never its own neighbour", "has no neighbours and is nobody's neighbour",
                 "O(m^2)", "56 B per point", "RTR_ERR_UNSUPPORTED"):
        assert text in sec, text
    src = tmp_path / "neighbours_abi.c"  # the prototype as a C99 consumer sees it
    src.write_text('#include "rtr.h"\n'
                   "typedef int (*fn_t)(rtr_ctx *, float, uint32_t, int, uint64_t[4]);\n"
                   "int main(void) { fn_t f = rtr_select_neighbours; return f == 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "neighbours_abi.o")])
    hpp = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read())
    for decl in ("uint64_t selectNeighbours(float radius, uint32_t min_neighbours, int op = RTR_SELECT_REPLACE, bool outside = false)",
                 "uint64_t removeOutliers(float radius, uint32_t min_neighbours)"):
        assert decl in hpp, decl


def test_option_keys_are_documented():
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    for key in ("neighbours_keys_us", "neighbours_sort_us", "neighbours_count_us"):
        assert '"%s"' % key in hdr, key


# ---- the reference against itself -------------------------------------------------------------------------------------
def _clouds():
    rng = np.random.default_rng(5)
    f = np.float32
    box = rng.uniform(-1, 1, (3000, 3)).astype(f)
    sheet = np.c_[rng.uniform(-2, 2, (4000, 2)), rng.normal(0, 0.01, 4000)].astype(f)
    lattice = (np.stack(np.meshgrid(*[np.arange(-7, 8)] * 3), -1).reshape(-1, 3) * 0.1).astype(f)  # spacing = the radius
    far = (rng.uniform(-1, 1, (2500, 3)) + [5000.0, -7000.0, 123.0]).astype(f)
    dup = np.concatenate([box[:1500], box[:700], box[:1]])
    return {"box": (box, 0.1), "sheet": (sheet, 0.05), "lattice": (lattice, 0.1), "far": (far, 0.11), "dup": (dup, 0.08)}


@pytest.mark.parametrize("name", sorted(_clouds()))
def test_brute_force_and_buckets_agree(name):
    xyz, r = _clouds()[name]
    a, b = nr.counts_brute(xyz, r), nr.counts_bucket(xyz, r)
    assert np.array_equal(a, b), np.flatnonzero(a != b)[:5]
    assert 0 < (a >= 4).sum() < xyz.shape[0] or name == "lattice", name
    assert (a > 0).any()


def test_the_lattice_has_its_six_neighbours_exactly_where_fp32_says():
    xyz, r = _clouds()["lattice"]
    cnt = nr.counts_brute(xyz, r)
    d2 = nr._d2(xyz[:, None, :], xyz[None, :, :])
    want = (d2 <= nr.r2_of(r)).sum(axis=1) - 1
    assert np.array_equal(cnt, want) and cnt.max() <= 6 and cnt.min() >= 0 and len(set(cnt)) > 1


def test_reference_on_special_coordinates():
    f = np.float32
    big = np.finfo(f).max
    xyz = f([[0, 0, 0], [0.05, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [-big, 0, 0], [big, 0, 0],
             [0, 0, 0]])
    cnt = nr.counts_brute(xyz, 0.05)
    # the two coincident points, their neighbour at exactly the radius; the two +FLT_MAX points are neighbours of each
    # other (d2 == 0) and of nobody else: FLT_MAX - -FLT_MAX overflows and fails by itself
    assert list(cnt) == [2, 2, 0, 0, 0, 1, 0, 1, 2]
    hit, st = nr.select(xyz, 0.05, 2)
    assert list(hit) == [True, True] + [False] * 6 + [True] and st == (3, 1, 3)
    assert np.array_equal(nr.words(hit), np.uint32([0b100000011]))


def test_threshold_is_inclusive_and_one_ulp_sharp():
    f = np.float32
    r = f(0.05)
    for base in f([0.0, 1.0, -3.0, 17.25]):
        at = f(base + r)  # (rounded: the distance seen in fp32 is at - base, not r)
        d = f(at - base)
        pair = f([[base, 0, 0], [at, 0, 0]])
        assert bool(nr.counts_brute(pair, r)[0]) == bool(f(d * d) <= nr.r2_of(r))
    a, b = f(0.05), np.nextafter(f(0.05), f(1))
    assert list(nr.counts_brute(f([[0, 0, 0], [a, 0, 0]]), r)) == [1, 1]
    assert list(nr.counts_brute(f([[0, 0, 0], [b, 0, 0]]), r)) == [0, 0]


@pytest.fixture(scope="module")
def scene_counts(orc):
    out = {}
    for scene, (n, radii) in nc.SCENES.items():
        xyzw, _ = orc.generate(scene, nc.SEED, 0, n, n)
        for r in radii:
            out[(scene, r)] = (n, nr.counts(xyzw, r))
    return out


def test_the_reference_spreads_the_scenes_of_the_gpu_tests(scene_counts):
    spread = 0
    for key, (n, cnt) in scene_counts.items():
        got = tuple(int((cnt >= k).sum()) for k in nc.KS)
        assert got == nc.PINS[key], (key, got)
        for k, hits, kind in zip(nc.KS, got, nc.KINDS[key]):
            assert nc.kind_holds(kind, hits, n), (key, k, hits, kind)
            spread += kind == "spread"
    assert spread == 8


# ---- Projector.select_neighbours against a fake library ---------------------------------------------------------------
class _Lib:
    def __init__(self):
        self.calls = []

    def rtr_select_neighbours(self, ctx, radius, min_neighbours, op, stats):
        self.calls.append({"radius": radius, "k": min_neighbours, "op": op, "stats": stats is not None})
        if stats is not None:
            out = C.cast(stats, C.POINTER(C.c_uint64))
            for k in range(4):
                out[k] = 20 + k
        return 0


def _stub(pkg):
    class Stub:
        _ctx = None
        _lib = _Lib()
        _SELECT_OPS = pkg.Projector._SELECT_OPS
        select_neighbours = pkg.Projector.select_neighbours

        def _chk(self, rc):
            assert rc == 0
    return Stub()


def test_select_neighbours_marshals_and_validates(pkg):
    L = pkg._lib
    s = _stub(pkg)
    assert s.select_neighbours(0.05, 4) == (20, 21, 22, 23)
    assert s._lib.calls[-1] == {"radius": 0.05, "k": 4, "op": L.SELECT_REPLACE, "stats": True}
    assert s.select_neighbours(np.float32(0.25), np.uint32(2), op="toggle", outside=True, stats=False) is None
    assert s._lib.calls[-1] == {"radius": 0.25, "k": 2, "op": L.SELECT_TOGGLE | L.SELECT_OUTSIDE, "stats": False}
    for op in ("add", "subtract", "intersect"):
        s.select_neighbours(1, 1, op=op)
        assert s._lib.calls[-1]["op"] == pkg.Projector._SELECT_OPS[op]
    made = len(s._lib.calls)
    for radius in (0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="radius"):
            s.select_neighbours(radius, 1)
    for k in (0, -1, 2 ** 32):
        with pytest.raises(ValueError, match="min_neighbours"):
            s.select_neighbours(0.1, k)
    with pytest.raises(KeyError):
        s.select_neighbours(0.1, 1, op="xor")
    assert len(s._lib.calls) == made
    assert L.lib().rtr_select_neighbours.argtypes[1] is C.c_float
