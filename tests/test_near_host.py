"""rtr_select_near (include/rtr.h section 6k) without a GPU: the exported symbol and the ABI version, the header's
prototype and its statements of the relation, the span rule, the GIVEN_ONLY rule, the scratch and the option keys, the
facade declarations and signatures; the two numpy references of near_ref.py against each other (their grid differs from
the library's), on special coordinates, at the threshold and across the edge of the library's span; the counts of the
cases the GPU tests use, pinned and spread; Projector.select_near's marshalling and argument validation against a fake
library; ProjectCloud.appendNewPoints against a stub."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import near_cases as nc
import near_ref as nr
from conftest import ROOT

f32 = np.float32


def test_near_symbol_exported(pkg):
    L = pkg._lib
    assert "rtr_select_near" in L.SYMBOLS and L.SYMBOLS.index("rtr_select_near") == len(L.SYMBOLS) - 1
    assert L.NEAR_GIVEN_ONLY == 1
    getattr(L.lib(), "rtr_select_near")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert re.search(r"\bT rtr_select_near$", nm, re.M)
    assert L.lib().rtr_abi_version() == 2
    at = L.lib().rtr_select_near.argtypes
    assert at[2] is C.c_size_t and at[3] is C.c_uint64 and at[4] is C.c_float and len(at) == 9


def test_near_header_declaration(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    assert ("int rtr_select_near(rtr_ctx *ctx, const float *xyz, size_t xyz_stride_bytes, uint64_t count, float radius, "
            "int flags, int op, uint32_t *near_words, uint64_t stats[4]);") in re.sub(r"\s+", " ", hdr)
    assert "#define RTR_NEAR_GIVEN_ONLY 1" in hdr and "#define RTR_ABI_VERSION 2" in hdr
    assert hdr.index("/* ---- 6j.") < hdr.index("/* ---- 6k.") < hdr.index("int rtr_select_near(") < hdr.index("7. measurement")
    sec = flat[flat.index("---- 6k."):flat.index("int rtr_select_near(")]
    for text in (
            # the relation
            "((dx dx + dy dy) + dz dz) <= r2", "r2 = radius radius, rounded once to fp32 on the host", "no FMA",
            "The comparison is inclusive", "negation is exact and the squares are equal", "There is no self-exclusion",
            "A non-finite point on either side is near nothing", "bit-for-bit reference",
            # the span rule
            "Only the GIVEN points must lie inside the span", "RESIDENT points may lie anywhere",
            "more than one cell beyond the span is near no given point", "and then hits",
            # GIVEN_ONLY
            "the selection is neither read, changed nor created", "op must be 0 and near_words must not be NULL",
            "but not with RTR_NEAR_GIVEN_ONLY",
            # the given side, the stats
            "the keep mask, the clip planes and the selection are ignored", "Bits past count are clear",
            "written only when the call succeeds", "[3] the non-finite given points", "[0] = [1] = 0",
            # the scratch and the cost
            "56 B per GIVEN point", "(n + 31) / 32 hit words", "(count + 31) / 32 near words",
            "nothing is proportional to n beyond the hit words", "never decoded", "O(pile x candidates)",
            # errors
            "RTR_ERR_INVALID", "RTR_ERR_UNSUPPORTED", "RTR_ERR_HIP", "before the first selection word changes"):
        assert text in sec, text
    for key in ("near_given_us", "near_sweep_us", "near_pair_tests_k", "near_chunks_skipped", "near_chunks_decoded"):
        assert '"%s"' % key in sec, key
    assert "near_chunks_skipped + near_chunks_decoded = (n + 255) / 256" in sec
    src = tmp_path / "near_abi.c"  # the prototype as a C99 consumer sees it
    src.write_text('#include "rtr.h"\n'
                   "typedef int (*fn_t)(rtr_ctx *, const float *, size_t, uint64_t, float, int, int, uint32_t *, uint64_t[4]);\n"
                   "int main(void) { fn_t f = rtr_select_near; return f == 0 || RTR_NEAR_GIVEN_ONLY != 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "near_abi.o")])
    hpp = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read())
    for decl in ("uint64_t selectNear(const float* xyz, size_t xyz_stride_bytes, size_t m, float radius, int op = RTR_SELECT_REPLACE, "
                 "bool outside = false, std::vector<uint32_t>* near_words = nullptr)",
                 "size_t appendNewPoints(const float* xyz, size_t xyz_stride_bytes, const uint8_t* rgb, size_t rgb_stride_bytes, "
                 "size_t m, float radius)",
                 "// selectNear (section 6k)", "// appendNewPoints appends only"):
        assert decl in hpp, decl


def test_the_cell_proof_covers_the_edge_of_the_span(pkg):
    txt = re.sub(r"[\s/]+", " ", open(os.path.join(os.path.dirname(pkg.LIB_PATH), "..", "csrc", "rtr_neighbour_cell.h")).read())
    for text in ("Across the span's edge", "|t| <= 2^20 + 1", "2^-53 |t|", "BY CELL INDEX"):
        assert text in txt, text


def test_python_signatures(pkg):
    sig = inspect.signature(pkg.Projector.select_near)
    assert str(sig) == "(self, xyz, radius, op='replace', outside=False, near=False, given_only=False, stats=True)"
    assert str(inspect.signature(pkg.ProjectCloud.selectNear)) == "(self, vertices, radius, op='replace', outside=False)"
    assert str(inspect.signature(pkg.ProjectCloud.appendNewPoints)) == "(self, vertices, colors, radius)"
    doc = pkg.ProjectCloud.appendNewPoints.__doc__
    assert "not thinned against itself" in doc and "selectVoxelGrid" in doc


# ---- the reference against itself -------------------------------------------------------------------------------------
def _clouds():
    """name -> (resident, given, radius): the clouds of test_neighbours_host.py, each against 300 .. 1000 given points
    that lie partly on it and partly off it."""
    rng = np.random.default_rng(6)
    box = rng.uniform(-1, 1, (3000, 3)).astype(f32)
    sheet = np.c_[rng.uniform(-2, 2, (4000, 2)), rng.normal(0, 0.01, 4000)].astype(f32)
    lattice = (np.stack(np.meshgrid(*[np.arange(-7, 8)] * 3), -1).reshape(-1, 3) * 0.1).astype(f32)  # spacing = the radius
    far = (rng.uniform(-1, 1, (2500, 3)) + [5000.0, -7000.0, 123.0]).astype(f32)
    dup = np.concatenate([box[:1500], box[:700], box[:1]])

    def given(cloud, m, jitter, lo, hi):
        pick = cloud[rng.integers(0, cloud.shape[0], m // 2)] + rng.normal(0, jitter, (m // 2, 3))
        return np.concatenate([pick, rng.uniform(lo, hi, (m - m // 2, 3))]).astype(f32)

    return {"box": (box, given(box, 700, 0.05, -1.5, 1.5), 0.1),
            "sheet": (sheet, given(sheet, 1000, 0.03, -2.5, 2.5), 0.05),
            "lattice": (lattice, np.concatenate([lattice[::7][:200] + f32([0.1, 0, 0]), given(lattice, 300, 0.05, -1, 1)]), 0.1),
            "far": (far, given(far, 300, 0.06, -1, 1) + f32([0, 0, 0]), 0.11),
            "dup": (dup, np.concatenate([box[:300], given(box, 400, 0.04, -1, 1)]), 0.08)}


@pytest.mark.parametrize("name", sorted(_clouds()))
def test_brute_force_and_buckets_agree(name):
    A, G, r = _clouds()[name]
    assert 300 <= G.shape[0] <= 1000
    h0, n0 = nr.near_brute(A, G, r)
    h1, n1 = nr.near_bucket(A, G, r)
    assert np.array_equal(h0, h1), np.flatnonzero(h0 != h1)[:5]
    assert np.array_equal(n0, n1), np.flatnonzero(n0 != n1)[:5]
    assert 0 < h0.sum() < A.shape[0] and 0 < n0.sum() < G.shape[0], name
    # both directions are one relation
    d2 = nr._d2(A[:, None, :], G[None, :, :]) <= nr.r2_of(r)
    assert np.array_equal(h0, d2.any(axis=1)) and np.array_equal(n0, d2.any(axis=0))


def test_reference_on_special_coordinates():
    big = np.finfo(f32).max
    A = f32([[0, 0, 0], [0.05, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [-big, 0, 0], [1, 1, 1]])
    G = f32([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [0.2, 0, 0], [np.nan, np.nan, np.nan]])
    hit, near = nr.near_brute(A, G, 0.05)
    # the coincident pair (no self-exclusion) and the point at exactly the radius; +FLT_MAX is near +FLT_MAX (d2 == 0);
    # non-finite points are near nothing on either side, even where they coincide
    assert list(hit) == [True, True, False, False, False, True, False, False]
    assert list(near) == [True, False, False, False, True, False, False]
    assert nr.stats(hit, near, G, hit) == (3, 3, 2, 4)
    assert nr.stats(hit, None, G, ~hit)[::2] == (5, 0)
    assert np.array_equal(nr.words(near), np.uint32([0b0010001]))
    h2, n2 = nr.near_bucket(A[:5], G[:4], 0.05)
    assert list(h2) == list(hit[:5]) and list(n2) == list(near[:4])
    e = nr.near_brute(A, np.zeros((0, 3), f32), 0.05)
    assert not e[0].any() and e[1].shape == (0,)


def test_threshold_is_inclusive_and_one_ulp_sharp():
    r = f32(0.05)
    for base in f32([0.0, 1.0, -3.0, 17.25]):
        at = f32(base + r)  # (rounded: the distance seen in fp32 is at - base, not r)
        d = f32(at - base)
        want = bool(f32(d * d) <= nr.r2_of(r))
        for A, G in (([[base, 0, 0]], [[at, 0, 0]]), ([[at, 0, 0]], [[base, 0, 0]])):  # (the direction does not matter)
            hit, near = nr.near_brute(f32(A), f32(G), r)
            assert bool(hit[0]) == want and bool(near[0]) == want
    a, b = f32(0.05), np.nextafter(f32(0.05), f32(1))
    assert [list(v) for v in nr.near_brute(f32([[0, 0, 0]]), f32([[a, 0, 0]]), r)] == [[True], [True]]
    assert [list(v) for v in nr.near_brute(f32([[0, 0, 0]]), f32([[b, 0, 0]]), r)] == [[False], [False]]


def span_edge_pairs(radius):
    """(resident, given, cells): given points in the last and the first in-span cell of the library's grid (edge h =
    radius * (1 + 2^-10), cells -(2^20 - 1) .. 2^20 - 2), resident points from just inside to three cells beyond it."""
    r = float(f32(radius))
    h = r * (1.0 + 1.0 / 1024.0)
    G, A = [], []
    for sign, edge in ((1.0, (2 ** 20 - 1) * h), (-1.0, -(2 ** 20 - 1) * h)):
        for axis in range(3):
            for back in (0.01, 0.3, 0.6, 0.99):  # the given point: `back` cells inside the edge
                g = np.zeros(3)
                g[axis] = edge - sign * back * h
                g[(axis + 1) % 3] = 0.3 * r
                G.append(g)
            for out in (-0.5, -0.01, 0.01, 0.3, 0.7, 0.99, 1.01, 1.5, 2.5, 3.0):  # the resident point: `out` cells beyond
                a = np.zeros(3)
                a[axis] = edge + sign * out * h
                a[(axis + 1) % 3] = 0.3 * r
                A.append(a)
    A, G = f32(A), f32(G)

    def cell(p):
        return np.floor(p.astype(np.float64) / h)
    qg = cell(G)  # (fp32 is coarse out there, 1/16 at 2^20: a given point rounded across the edge is left out)
    G = G[((qg >= -(2 ** 20 - 1)) & (qg <= 2 ** 20 - 2)).all(axis=1)]
    return A, G, (cell(A), cell(G))


@pytest.mark.parametrize("radius", [0.05, 1.0, 0.37])
def test_reference_across_the_edge_of_the_span(radius):
    A, G, (qa, qg) = span_edge_pairs(radius)
    lo, hi = -(2 ** 20 - 1), 2 ** 20 - 2
    assert ((qg >= lo) & (qg <= hi)).all() and G.shape[0] >= 18, "every given point has a cell"
    assert (qg[:, :] == hi).any() and (qg[:, :] == lo).any(), "the last and the first in-span cell"
    beyond = ((qa < lo) | (qa > hi)).any(axis=1)
    assert beyond.sum() >= 30 and (~beyond).sum() >= 6
    near = nr._d2(A[:, None, :], G[None, :, :]) <= nr.r2_of(radius)
    hit, given = nr.near_brute(A, G, radius)
    assert np.array_equal(hit, near.any(axis=1)) and np.array_equal(given, near.any(axis=0))
    # a resident point one cell beyond the span is near a given point in the last cell: it must hit
    assert (hit & beyond).any() and (hit & ~beyond).any() and (~hit & beyond).any()
    # every accepted pair has cells at most one apart on every axis, and no resident point more than one cell out is near
    i, j = np.nonzero(near)
    assert (np.abs(qa[i] - qg[j]) <= 1).all()
    far = ((qa < lo - 1) | (qa > hi + 1)).any(axis=1)
    assert far.any() and not hit[far].any()


@pytest.fixture(scope="module")
def scene_clouds(orc):
    return {s: (orc.generate(s, nc.SEED, 0, n, n)[0], orc.generate(s, nc.GIVEN_SEED, 0, n, n)[0]) for s, n in nc.SCENES.items()}


def test_the_reference_reproduces_the_pinned_cases_and_they_spread(scene_clouds):
    res = giv = 0
    for case in nc.CASES:
        scene, take, radius, count, hits, nears = case
        A, second = scene_clouds[scene]
        G = nc.given(case, second)
        assert G.shape[0] == count, case
        hit, near = nr.near_brute(A, G, radius)
        assert (int(hit.sum()), int(near.sum())) == (hits, nears), case
        hb, nb = nr.near_bucket(A, G, radius)
        assert np.array_equal(hit, hb) and np.array_equal(near, nb), case
        res += nc.spread(hits, A.shape[0])
        giv += nc.spread(nears, count)
    # a kernel that answers all or nothing must not pass
    assert res >= 6 and giv >= 6, (res, giv)
    assert (res, giv) == (8, 7)


# ---- Projector.select_near against a fake library ---------------------------------------------------------------------
class _Lib:
    def __init__(self):
        self.calls = []
        self.near_bits = None

    def rtr_select_near(self, ctx, xyz, stride, count, radius, flags, op, near_words, stats):
        pts = None
        if count:
            addr = xyz.value if isinstance(xyz, C.c_void_p) else xyz
            raw = (C.c_char * ((count - 1) * stride + 12)).from_address(addr)
            rows = np.frombuffer(raw, np.uint8)
            pts = np.stack([rows[j * stride:j * stride + 12].view(np.float32) for j in range(count)])
        self.calls.append({"xyz": pts, "null": xyz is None, "stride": stride, "count": count, "radius": radius, "flags": flags,
                           "op": op, "near": near_words is not None, "stats": stats is not None})
        if near_words is not None:
            out = C.cast(near_words, C.POINTER(C.c_uint32))
            for j in range(count):
                if self.near_bits[j]:
                    out[j // 32] |= 1 << (j % 32)
        if stats is not None:
            out = C.cast(stats, C.POINTER(C.c_uint64))
            for k in range(4):
                out[k] = 30 + k
        return 0


def _stub(pkg):
    class Stub:
        _ctx = None
        _lib = _Lib()
        _SELECT_OPS = pkg.Projector._SELECT_OPS
        _write_source = staticmethod(pkg.Projector._write_source)
        select_near = pkg.Projector.select_near

        def _chk(self, rc):
            assert rc == 0
    return Stub()


def test_select_near_marshals_and_validates(pkg):
    L = pkg._lib
    s = _stub(pkg)
    rng = np.random.default_rng(2)
    tight = rng.normal(size=(70, 3)).astype(f32)
    wide = np.c_[tight, np.ones(70, f32)]
    s._lib.near_bits = rng.integers(0, 2, 70).astype(bool)
    assert s.select_near(tight, 0.05) == (30, 31, 32, 33)
    call = s._lib.calls[-1]
    assert np.array_equal(call.pop("xyz"), tight)
    assert call == {"null": False, "stride": 12, "count": 70, "radius": 0.05, "flags": 0, "op": L.SELECT_REPLACE, "near": False,
                    "stats": True}
    st, bits = s.select_near(wide, np.float32(0.25), op="toggle", outside=True, near=True)
    call = s._lib.calls[-1]
    assert np.array_equal(call.pop("xyz"), tight) and st == (30, 31, 32, 33)
    assert call == {"null": False, "stride": 16, "count": 70, "radius": 0.25, "flags": 0, "op": L.SELECT_TOGGLE | L.SELECT_OUTSIDE,
                    "near": True, "stats": True}
    assert bits.dtype == bool and np.array_equal(bits, s._lib.near_bits)
    bits = s.select_near(wide[::2], 1, given_only=True, stats=False)  # (a row stride of 32 bytes)
    call = s._lib.calls[-1]
    assert np.array_equal(call.pop("xyz"), tight[::2]) and np.array_equal(bits, s._lib.near_bits[:35])
    assert call == {"null": False, "stride": 32, "count": 35, "radius": 1.0, "flags": L.NEAR_GIVEN_ONLY, "op": 0, "near": True,
                    "stats": False}
    assert s.select_near(tight.tolist(), 0.5, stats=False) is None  # (anything numpy converts)
    assert np.array_equal(s._lib.calls[-1]["xyz"], tight)
    for op in ("add", "subtract", "intersect"):
        s.select_near(tight, 1, op=op)
        assert s._lib.calls[-1]["op"] == pkg.Projector._SELECT_OPS[op]
    st, bits = s.select_near(np.zeros((0, 3), f32), 0.1, near=True)  # (no given point)
    assert bits.shape == (0,) and s._lib.calls[-1]["count"] == 0 and s._lib.calls[-1]["null"]
    made = len(s._lib.calls)
    for radius in (0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="radius"):
            s.select_near(tight, radius)
    with pytest.raises(KeyError):
        s.select_near(tight, 0.1, op="xor")
    for kw in ({"op": "add"}, {"outside": True}):
        with pytest.raises(ValueError, match="given_only"):
            s.select_near(tight, 0.1, given_only=True, **kw)
    for bad in (np.zeros((5, 2), f32), np.zeros(6, f32), np.zeros((2, 3, 3), f32), np.zeros((8, 4), f32)[:, ::2]):
        with pytest.raises(ValueError, match="xyz"):
            s.select_near(bad, 0.1)
    assert len(s._lib.calls) == made


def test_append_new_points_appends_exactly_the_clear_rows_in_order(pkg):
    rng = np.random.default_rng(3)
    v = rng.normal(size=(37, 4)).astype(f32)
    c = rng.integers(0, 256, (37, 4)).astype(np.uint8)
    near = rng.integers(0, 2, 37).astype(bool)
    log = []

    class P:
        def select_near(self, xyz, radius, op="replace", outside=False, near=False, given_only=False, stats=True):
            log.append(("near", radius, op, outside, given_only, stats))
            assert np.array_equal(xyz, v)
            return near_bits

    class Stub:
        _p = P()
        appendNewPoints = pkg.ProjectCloud.appendNewPoints

        def appendPoints(self, vertices, colors):
            log.append(("append", vertices.copy(), colors.copy()))

    near_bits = near
    assert Stub().appendNewPoints(v, c, 0.02) == int((~near).sum())
    assert log[0] == ("near", 0.02, "replace", False, True, False) and len(log) == 2
    assert np.array_equal(log[1][1], v[~near]) and np.array_equal(log[1][2], c[~near])
    log.clear()
    near_bits = np.ones(37, bool)  # (a scan that adds nothing: no append at all)
    assert Stub().appendNewPoints(v, c, 0.02) == 0 and len(log) == 1
    with pytest.raises(ValueError, match="rows"):
        Stub().appendNewPoints(v, c[:5], 0.02)
