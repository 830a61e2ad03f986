"""rtr_count_in_bands and rtr_fit_plane (include/rtr.h section 6j) without a GPU: the exported symbols, their place in
_lib.SYMBOLS, the header prototypes compiled as C99 and the section's place, the facade declarations;
Projector.count_in_bands and Projector.fit_plane against a fake library (argument packing, `selected`, every error raised
before the library is reached); planes_ref.in_band against select_ref's two-plane test; the sampler's first draws pinned."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import planes_ref as pr
import select_ref as sr
from conftest import ROOT
from test_gpu_select import _specials


def test_planes_symbols_exported(pkg):
    L = pkg._lib
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    for name in ("rtr_count_in_bands", "rtr_fit_plane"):
        assert name in L.SYMBOLS
        getattr(L.lib(), name)
        assert re.search(r"\bT %s$" % name, nm, re.M)
    assert L.lib().rtr_abi_version() == 2
    assert L.BANDS_SELECTED == 1 and L.MAX_BANDS == 4096 == pr.MAX_BANDS
    kernels = open(os.path.join(os.path.dirname(pkg.LIB_PATH), "..", "csrc", "rtr_kernels.h")).read()
    assert "constexpr int kBandPass = 64;" in kernels  # (the pass width B of tests/test_gpu_planes.py)


def test_planes_header_declarations(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int rtr_count_in_bands(rtr_ctx *ctx, uint32_t count, const float *bands /* count x 5, host */, int flags, "
            "uint64_t *counts /* count, host */, uint64_t stats[4]);") in flat
    assert ("int rtr_fit_plane(rtr_ctx *ctx, float dist, uint32_t iterations, uint64_t seed, int flags, float plane[4], "
            "uint64_t stats[4]);") in flat
    assert "#define RTR_MAX_BANDS 4096" in hdr and re.search(r"#define RTR_BANDS_SELECTED 1\b", hdr)
    assert "#define RTR_ABI_VERSION 2" in hdr
    assert hdr.index("6i. selection by connected cluster") < hdr.index("/* ---- 6j.") < hdr.index("7. measurement")
    assert "{-a, -b, -c, d_hi}" in hdr and "negation commutes with round-to-nearest" in hdr  # (the stated equivalence)
    src = tmp_path / "planes_abi.c"  # the prototypes as a C99 consumer sees them
    src.write_text('#include "rtr.h"\n'
                   "typedef int (*count_t)(rtr_ctx *, uint32_t, const float *, int, uint64_t *, uint64_t[4]);\n"
                   "typedef int (*fit_t)(rtr_ctx *, float, uint32_t, uint64_t, int, float[4], uint64_t[4]);\n"
                   "int main(void) { count_t f = rtr_count_in_bands; fit_t g = rtr_fit_plane;\n"
                   "  return (f == 0) + (g == 0) + (RTR_MAX_BANDS != 4096) + (RTR_BANDS_SELECTED != 1); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "planes_abi.o")])
    hpp = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read())
    for decl in ("Plane fitPlane(float dist, uint32_t iterations = 256, uint64_t seed = 0, bool selected = false, uint64_t stats[4] = nullptr)",
                 "uint64_t selectPlane(const float plane[4], float dist, int op = RTR_SELECT_REPLACE, bool outside = false)",
                 "Plane segmentPlane(float dist, uint32_t iterations = 256, uint64_t seed = 0)",
                 "std::vector<uint64_t> countInBands(const float* bands, uint32_t count, bool selected = false, uint64_t stats[4] = nullptr)"):
        assert decl in hpp, decl


def test_python_facade_declarations(pkg):
    import inspect
    sig = lambda f: str(inspect.signature(f))  # noqa: E731
    assert sig(pkg.Projector.count_in_bands) == "(self, bands, selected=False, stats=True)"
    assert sig(pkg.Projector.fit_plane) == "(self, dist, iterations=256, seed=0, selected=False)"
    assert sig(pkg.ProjectCloud.fitPlane) == "(self, dist, iterations=256, seed=0, selected=False)"
    assert sig(pkg.ProjectCloud.selectPlane) == "(self, plane, dist, op='replace', outside=False)"
    assert sig(pkg.ProjectCloud.countInBands) == "(self, bands, selected=False)"
    assert sig(pkg.ProjectCloud.segmentPlane) == "(self, dist, iterations=256, seed=0)"
    assert "fitPlane(0.03, selected=True)" in pkg.ProjectCloud.segmentPlane.__doc__  # (peeling a second plane)


# ---- the Projector methods against a fake library -------------------------------------------------------------------
class _Lib:
    def __init__(self):
        self.calls = []
        self.good = 7  # non-degenerate candidates rtr_fit_plane reports

    def rtr_count_in_bands(self, ctx, count, bands, flags, counts, stats):
        b = np.ctypeslib.as_array(C.cast(bands, C.POINTER(C.c_float)), (count, 5)).copy()
        self.calls.append({"fn": "count", "count": count, "bands": b, "flags": flags, "stats": stats is not None})
        out = C.cast(counts, C.POINTER(C.c_uint64))
        for k in range(count):
            out[k] = 100 + k
        if stats is not None:
            st = C.cast(stats, C.POINTER(C.c_uint64))
            for k in range(4):
                st[k] = 10 + k
        return 0

    def rtr_fit_plane(self, ctx, dist, iterations, seed, flags, plane, stats):
        self.calls.append({"fn": "fit", "dist": dist, "iterations": iterations, "seed": seed, "flags": flags})
        pl = C.cast(plane, C.POINTER(C.c_float))
        st = C.cast(stats, C.POINTER(C.c_uint64))
        for k in range(4):
            pl[k] = 0.25 * (k + 1) if self.good else 0.0
        st[0], st[1], st[2], st[3] = (55 if self.good else 0), self.good, (3 if self.good else 0), 99
        return 0


def _stub(pkg):
    class Stub:
        _ctx = None
        _lib = _Lib()
        count_in_bands = pkg.Projector.count_in_bands
        fit_plane = pkg.Projector.fit_plane

        def _chk(self, rc):
            assert rc == 0
    return Stub()


def test_count_in_bands_marshals_bands_flag_and_stats(pkg):
    L = pkg._lib
    s = _stub(pkg)
    bands = [[0, 0, 1, -0.27, 0.33], [0.6, 0, 0.8, 1.5, -1.25], [1, 0, 0, 0, 0]]
    counts, st = s.count_in_bands(bands)
    call = s._lib.calls[-1]
    assert counts.dtype == np.uint64 and list(counts) == [100, 101, 102] and st == (10, 11, 12, 13)
    assert call["count"] == 3 and np.array_equal(call["bands"], np.float32(bands)) and call["flags"] == 0 and call["stats"]
    counts = s.count_in_bands(np.float64(bands)[:1], selected=True, stats=False)
    call = s._lib.calls[-1]
    assert list(counts) == [100] and call["count"] == 1 and call["flags"] == L.BANDS_SELECTED and not call["stats"]
    big = np.tile(np.float32([[0, 0, 1, 0, 0]]), (L.MAX_BANDS, 1))
    assert s.count_in_bands(big, stats=False).shape == (L.MAX_BANDS,) and s._lib.calls[-1]["count"] == L.MAX_BANDS
    strided = np.zeros((4, 10), np.float32)
    strided[:, ::2] = np.float32(bands + [[0, 1, 0, 2, 3]])
    s.count_in_bands(strided[:, ::2])  # (a view: made contiguous before it is passed)
    assert np.array_equal(s._lib.calls[-1]["bands"], strided[:, ::2])


def test_count_in_bands_argument_rules(pkg):
    L = pkg._lib
    s = _stub(pkg)
    ok = [0, 0, 1, 0, 0]
    for bands in ([ok[:4]], ok, np.zeros((0, 5)), np.tile([ok], (L.MAX_BANDS + 1, 1)), [[0, 0, 0, 1, 1]], [ok, [0, 0, 0, 0, 0]],
                  [[np.nan, 0, 1, 0, 0]], [[0, 0, 1, np.inf, 0]], [[0, 0, 1, 0, -np.inf]], [[1e39, 0, 1, 0, 0]], np.zeros((2, 5, 1))):
        with pytest.raises(ValueError):
            s.count_in_bands(bands)
    assert s._lib.calls == []  # (none of them reached the library)


def test_fit_plane_marshals_and_raises_on_no_candidate(pkg):
    L = pkg._lib
    s = _stub(pkg)
    plane, inliers, st = s.fit_plane(0.03)
    call = s._lib.calls[-1]
    assert plane.dtype == np.float32 and list(plane) == [0.25, 0.5, 0.75, 1.0] and inliers == 55 and st == (55, 7, 3, 99)
    assert call == {"fn": "fit", "dist": float(np.float32(0.03)), "iterations": 256, "seed": 0, "flags": 0}
    s.fit_plane(np.float32(0), iterations=1, seed=(1 << 64) - 1, selected=True)
    assert s._lib.calls[-1] == {"fn": "fit", "dist": 0.0, "iterations": 1, "seed": (1 << 64) - 1, "flags": L.BANDS_SELECTED}
    s.fit_plane(1.5, L.MAX_BANDS, -1)  # (seeds are taken modulo 2^64)
    assert s._lib.calls[-1]["seed"] == (1 << 64) - 1 and s._lib.calls[-1]["iterations"] == L.MAX_BANDS
    s.fit_plane(1.5, seed=(1 << 64) + 5)
    assert s._lib.calls[-1]["seed"] == 5
    before = len(s._lib.calls)
    for kw in (dict(dist=-1e-9), dict(dist=np.nan), dict(dist=np.inf), dict(dist=0.1, iterations=0),
               dict(dist=0.1, iterations=L.MAX_BANDS + 1), dict(dist=0.1, iterations=-3)):
        with pytest.raises(ValueError):
            s.fit_plane(**kw)
    assert len(s._lib.calls) == before
    s._lib.good = 0
    with pytest.raises(RuntimeError, match="degenerate"):
        s.fit_plane(0.03)


def test_plane_band_is_the_headers_rule(pkg):
    rng = np.random.default_rng(2)
    for _ in range(200):
        pl, d = rng.normal(size=4).astype(np.float32), np.float32(abs(rng.normal()) * 0.1)
        assert np.array_equal(pkg.Projector.plane_band(pl, d).view(np.uint32), pr.band_of(pl, d).view(np.uint32))
    b = pr.band_of([0, 0, 1, -0.3], 0.03)
    assert b[3] == np.float32(-0.3) + np.float32(0.03) and b[4] == np.float32(0.03) - np.float32(-0.3)


# ---- the reference ----------------------------------------------------------------------------------------------------
def test_in_band_is_select_refs_two_plane_test(pkg, orc):
    rng = np.random.default_rng(31)
    sp = _specials()
    pts = (rng.normal(size=(3000, 3)) * [3, 2, 1]).astype(np.float32)
    rows = rng.choice(3000, 600, replace=False)
    pts[rows, rng.integers(0, 3, 600)] = rng.choice(sp, 600)
    pts[rows[:60]] = rng.choice(sp, (60, 3))
    seen = 0
    for k in range(50):
        nrm = rng.normal(size=3)
        if k % 5 == 0:
            nrm[rng.integers(0, 3)] = 0  # (a zero coefficient: 0 x inf is NaN)
        if k % 10 == 1:
            nrm = np.eye(3)[k % 3] * rng.choice([-1, 1])  # (axis-aligned)
        d, w = rng.normal() * 2, abs(rng.normal()) * [0, 0.02, 0.05, 1, 30][k % 5]
        band = np.float32([nrm[0], nrm[1], nrm[2], d + w, w - d])
        got = pr.in_band(pts, band)
        want = sr.inside(pkg, orc, pts, pr.two_planes(band))
        assert np.array_equal(got, want), (k, band)
        assert not got[~np.isfinite(pts).all(axis=1) & np.isnan(pts).any(axis=1)].any()
        assert list(pr.counts(pts, [band])) == [int(want.sum())]
        half = np.arange(3000) % 2 == 0
        assert list(pr.counts(pts, [band], half)) == [int((want & half).sum())]
        seen += int(want.sum())
    assert seen > 3000


def test_sampler_first_draws_are_pinned():
    assert [pr.draw(0, t) for t in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [pr.draw(1, t) for t in range(3)] == [0x910A2DEC89025CC1, 0xBEEB8DA1658EEC67, 0xF893A2EEFB32555E]
    assert [pr.draw((1 << 64) - 1, t) for t in range(3)] == [0xE4D971771B652C20, 0xE99FF867DBF682C9, 0x382FF84CB27281E9]
    r = pr.ranks(0, 2, 1000)
    assert [list(map(int, row)) for row in r] == [[pr.draw(0, 3 * c + j) % 1000 for j in range(3)] for c in range(2)]
    assert int(r[0][0]) == 0xE220A8397B1DCDAF % 1000


def test_fit_reference_on_a_small_plane():
    rng = np.random.default_rng(4)
    n = 4000
    pts = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    on = rng.random(n) < 0.5
    pts[on, 2] = np.float32(0.3) + rng.uniform(-0.01, 0.01, int(on.sum())).astype(np.float32)
    plane, st = pr.fit(pts, 0.03, 64, 1)
    assert st[0] >= 0.9 * on.sum() and st[1] == 64 and st[3] == n and plane[2] > 0.99 and abs(plane[3] + 0.3) < 0.02
    assert st[0] == int(pr.in_band(pts, pr.band_of(plane, 0.03)).sum())
    assert pr.fit(pts[:2], 0.03, 16)[1] == (0, 0, 0, 2)  # (fewer than three points: every candidate is degenerate)
    same = np.repeat(pts[:1], 50, axis=0)
    assert pr.fit(same, 0.03, 16)[1] == (0, 0, 0, 50) and not pr.fit(same, 0.03, 16)[0].any()
    plane2, st2 = pr.fit(pts, 0.03, 64, 1, ~pr.in_band(pts, pr.band_of(plane, 0.03)))
    assert st2[3] == n - st[0] and st2[0] < st[0]
