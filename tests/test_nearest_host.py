"""rtr_nearest_points (include/rtr.h section 6l) without a GPU: the exported symbol, its place in SYMBOLS and the ABI
version, the header's prototype and its statements of the tie rule, NONE and +inf, denormals, the scratch and the option
keys, the facade declarations and signatures; the two numpy references of nearest_ref.py against each other and against
near_ref.py's bits, on special coordinates, at the threshold and on the tie lattice of nearest_cases.py;
Projector.nearest_points' marshalling and argument validation against a fake library; ProjectCloud.matchPoints against a
stub."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import near_cases as nc
import near_ref as nr
import nearest_cases as ncs
import nearest_ref as nf
from conftest import ROOT
from test_near_host import _clouds

f32 = np.float32
KEYS = ("nearest_given_us", "nearest_sweep_us", "nearest_pair_tests_k", "nearest_chunks_skipped", "nearest_chunks_decoded")


def test_nearest_symbol_exported(pkg):
    L = pkg._lib
    assert L.SYMBOLS.index("rtr_nearest_points") == L.SYMBOLS.index("rtr_select_near") - 1 == len(L.SYMBOLS) - 2
    assert L.NEAREST_NONE == 0xFFFFFFFF == nf.NONE
    getattr(L.lib(), "rtr_nearest_points")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert re.search(r"\bT rtr_nearest_points$", nm, re.M)
    assert L.lib().rtr_abi_version() == 2 and L.ABI_VERSION == 2
    at = L.lib().rtr_nearest_points.argtypes
    assert at[2] is C.c_size_t and at[3] is C.c_uint64 and at[4] is C.c_float and len(at) == 11


def test_nearest_header_declaration(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    proto = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("int rtr_nearest_points("):], flags=re.S)
    assert re.sub(r"\s+", " ", proto).startswith(
        "int rtr_nearest_points(rtr_ctx *ctx, const float *xyz, size_t xyz_stride_bytes, uint64_t count, float radius, int flags, "
        "uint32_t *given_index, float *given_dist2, uint32_t *resident_index, float *resident_dist2, uint64_t stats[4]);")
    assert "#define RTR_NEAREST_NONE 0xFFFFFFFFu" in hdr and "#define RTR_ABI_VERSION 2" in hdr
    assert hdr.index("int rtr_select_near(") < hdr.index("/* ---- 6l.") < hdr.index("int rtr_nearest_points(") < hdr.index("7. measurement")
    sec = flat[flat.index("---- 6l."):flat.index("int rtr_nearest_points(")]
    for text in (
            # the relation and the tie rule
            "d2 = ((dx dx + dy dy) + dz dz)", "no FMA", "d2 <= r2, inclusive", "rounded once to fp32 on the host", "bit-for-bit reference",
            "of several candidates with the same d2 bits, the smallest upload index wins", "ties to the smallest given index",
            # NONE and +inf, denormals
            "gets RTR_NEAREST_NONE and +inf (0x7F800000)", "every non-finite one among them", "the kernels do not flush denormals",
            "a coincident point gives +0", "RTR_NEAREST_NONE is never a real index",
            # who counts, the outputs
            "the keep mask, the clip planes and the selection are ignored", "indexed by UPLOAD index",
            "each of the four pointers may be NULL on its own", "all four NULL is legal", "written only when the call succeeds",
            "flags must be 0", "[2] the non-finite given points, [3] 0", "equals rtr_select_near's stats[2]",
            # why no coordinates
            "keeps no map from upload to resident index", "hold a distance and an index and nothing more",
            # the rules of section 6k, stated again
            "not on the resident order, the library's sort, the packed form, any option, the internal grid or the order of the given points",
            "the given outputs permute with them", "neither read, changed nor created", 'needs option "point_ids" = 1',
            "the call ALWAYS waits for its own work",
            # the scratch
            "8 B per GIVEN point for the given slots", "8 B per RESIDENT point only when a resident output is asked for",
            "Everything is allocated before anything is written",
            # errors
            "RTR_ERR_INVALID", "RTR_ERR_UNSUPPORTED", "RTR_ERR_HIP", "n or count >= 2^32"):
        assert text.lower() in sec.lower(), text
    for key in KEYS:
        assert '"%s"' % key in sec and '"%s"' % key in hdr[:hdr.index("/* ---- 6l.")], key
    assert "nearest_chunks_skipped + nearest_chunks_decoded = (n + 255) / 256" in sec
    src = tmp_path / "nearest_abi.c"  # the prototype as a C99 consumer sees it
    src.write_text('#include "rtr.h"\n'
                   "typedef int (*fn_t)(rtr_ctx *, const float *, size_t, uint64_t, float, int, uint32_t *, float *, uint32_t *, float *,\n"
                   "                    uint64_t[4]);\n"
                   "int main(void) { fn_t f = rtr_nearest_points; return f == 0 || RTR_NEAREST_NONE != 0xFFFFFFFFu; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "nearest_abi.o")])
    hpp = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read())
    for decl in ("Nearest nearestPoints(const float* xyz, size_t xyz_stride_bytes, size_t m, float radius)",
                 "Match matchPoints(const float* xyz, size_t xyz_stride_bytes, size_t m, float radius)",
                 "// nearestPoints (section 6l)", "// matchPoints also returns"):
        assert decl in hpp, decl


def test_python_signatures(pkg):
    assert str(inspect.signature(pkg.Projector.nearest_points)) == "(self, xyz, radius, given=True, resident=False, stats=True)"
    assert str(inspect.signature(pkg.ProjectCloud.nearestPoints)) == "(self, vertices, radius)"
    assert str(inspect.signature(pkg.ProjectCloud.matchPoints)) == "(self, vertices, radius)"
    doc = pkg.Projector.nearest_points.__doc__
    assert "smallest index" in doc and "NEAREST_NONE" in doc and "+inf" in doc


# ---- the reference against itself -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_clouds()))
def test_brute_force_and_buckets_agree(name):
    A, G, r = _clouds()[name]  # (test_near_host.py's five kinds of cloud)
    b, k = nf.nearest_brute(A, G, r), nf.nearest_bucket(A, G, r)
    assert nf.same(b[:4], k[:4]) and b[4] == k[4]
    assert 0 < b[4][0] < G.shape[0] and 0 < b[4][1] < A.shape[0], name
    # who has a nearest is section 6k's relation: near_ref's hit and near bits
    hit, near = nr.near_brute(A, G, r)
    assert np.array_equal(b[0] != nf.NONE, near) and np.array_equal(b[2] != nf.NONE, hit)
    assert np.array_equal(np.isfinite(b[1]), near) and np.array_equal(np.isfinite(b[3]), hit)
    assert b[4] == (int(near.sum()), int(hit.sum()), 0, 0)
    # the definition, spelled out point by point on a few of them
    d2 = nf._d2(A[:, None, :], G[None, :, :])
    for j in np.flatnonzero(near)[:40]:
        col = np.where(d2[:, j] <= nf.r2_of(r), d2[:, j], f32(np.inf))
        i = int(b[0][j])
        assert col[i] == col.min() == b[1][j] and not (col[:i] == col[i]).any()
    if name == "dup":  # (coincident resident points: the first of them wins, at d2 = +0)
        zero = np.flatnonzero(nf.bits(b[1]) == 0)
        assert zero.size >= 300 and (b[0][zero] < 1500).all()


@pytest.fixture(scope="module")
def scene_clouds(orc):
    return {s: (orc.generate(s, nc.SEED, 0, n, n)[0], orc.generate(s, nc.GIVEN_SEED, 0, n, n)[0]) for s, n in nc.SCENES.items()}


def test_the_reference_agrees_with_near_ref_on_the_pinned_cases(scene_clouds):
    for case in nc.CASES:  # (the ten cases of the GPU tests; test_near_host.py pins their counts and their spread)
        A, second = scene_clouds[case[0]]
        G = nc.given(case, second)
        gi, gd, ri, rd, st = nf.nearest_bucket(A, G, case[2])
        hit, near = nr.near_bucket(A, G, case[2])
        assert np.array_equal(gi != nf.NONE, near) and np.array_equal(ri != nf.NONE, hit), case
        assert np.array_equal(np.isfinite(gd), near) and np.array_equal(np.isfinite(rd), hit), case
        assert st == (case[5], case[4], 0, 0), case
        if case[3] < 300:
            assert nf.same(nf.nearest_brute(A, G, case[2])[:4], (gi, gd, ri, rd)), case


def test_reference_on_special_coordinates():
    big = np.finfo(f32).max
    A = f32([[0, 0, 0], [0.05, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [-big, 0, 0], [1, 1, 1]])
    G = f32([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [0.2, 0, 0], [np.nan, np.nan, np.nan], [0.03, 0, 0]])
    gi, gd, ri, rd, st = nf.nearest_brute(A, G, 0.05)
    N, inf = nf.NONE, np.inf
    # a coincident pair is at +0; +FLT_MAX is nearest to +FLT_MAX (d2 == 0); a non-finite point on either side has no nearest
    # and is nobody's, even where two coincide; (0.03, 0, 0) is nearer to (0.05, 0, 0) than to the origin
    assert list(gi) == [0, N, N, N, 5, N, N, 1]
    d = f32(0.05) - f32(0.03)
    assert list(nf.bits(gd)) == [0, nf.INF_BITS, nf.INF_BITS, nf.INF_BITS, 0, nf.INF_BITS, nf.INF_BITS, int(nf.bits(d * d)[0])]
    assert list(ri) == [0, 7, N, N, N, 4, N, N] and list(rd[[2, 3, 4, 6, 7]]) == [inf] * 5 and nf.bits(rd)[0] == 0
    assert st == (3, 3, 4, 0)
    k = nf.nearest_bucket(A[:5], G[[0, 1, 2, 3, 7]], 0.05)
    b = nf.nearest_brute(A[:5], G[[0, 1, 2, 3, 7]], 0.05)
    assert nf.same(k[:4], b[:4]) and k[4] == b[4] == (2, 2, 3, 0)
    e = nf.nearest_brute(A, np.zeros((0, 3), f32), 0.05)
    assert e[0].shape == e[1].shape == (0,) and (e[2] == N).all() and np.isinf(e[3]).all() and e[4] == (0, 0, 0, 0)


def test_threshold_is_inclusive_and_one_ulp_sharp():
    r = f32(0.05)
    a, b = f32(0.05), np.nextafter(f32(0.05), f32(1))
    at = nf.nearest_brute(f32([[0, 0, 0]]), f32([[a, 0, 0]]), r)
    assert list(at[0]) == [0] and list(at[2]) == [0] and nf.bits(at[1])[0] == nf.bits(at[3])[0] == nf.bits(nf.r2_of(r))[0]
    off = nf.nearest_brute(f32([[0, 0, 0]]), f32([[b, 0, 0]]), r)
    assert list(off[0]) == [nf.NONE] and list(off[2]) == [nf.NONE] and nf.bits(off[1])[0] == nf.bits(off[3])[0] == nf.INF_BITS
    for base in f32([0.0, 1.0, -3.0, 17.25]):  # (rounded: the distance seen in fp32 is at - base, not r; both ways round)
        far = f32(base + r)
        d = f32(far - base)
        want = bool(f32(d * d) <= nf.r2_of(r))
        for A, G in (([[base, 0, 0]], [[far, 0, 0]]), ([[far, 0, 0]], [[base, 0, 0]])):
            got = nf.nearest_brute(f32(A), f32(G), r)
            assert (got[0][0] != nf.NONE) == want == (got[2][0] != nf.NONE)
            if want:
                assert nf.bits(got[1])[0] == nf.bits(got[3])[0] == nf.bits(f32(d * d))[0]


@pytest.mark.parametrize("order", ncs.TIE_ORDERS)
def test_every_answer_on_the_lattice_is_a_tie(order):
    A, G = ncs.tie_lattice(order)
    assert np.array_equal(A * 256, np.round(A * 256)) and np.array_equal(G * 256, np.round(G * 256)) and np.abs(A).max() <= 16
    tg, tr = ncs.tie_counts(A, G)
    # EVERY given point has at least two resident points at its bitwise-minimal d2: a kernel that ignores the tie rule
    # cannot pass test_gpu_nearest.py's lattice test by luck
    assert (tg >= 2).all() and (tg == 8).sum() == 288 and tg[288] == 3
    assert (tr == 3).sum() == 2, "two resident points with three given points at the same distance"
    b, k = nf.nearest_brute(A, G, ncs.TIE_RADIUS), nf.nearest_bucket(A, G, ncs.TIE_RADIUS)
    assert nf.same(b[:4], k[:4]) and b[4] == k[4] == (G.shape[0], A.shape[0], 0, 0)
    d = A[:, None, :] - G[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    for j in range(G.shape[0]):  # the winner is the smallest upload index of the tie
        ties = np.flatnonzero(d2[:, j] == d2[:, j].min())
        assert b[0][j] == ties[0] and ties.size == tg[j]
    assert nf.bits(b[1])[288] == 0 and (nf.bits(b[1])[:288] == nf.bits(f32(48 / 65536))[0]).all()
    lone = np.flatnonzero(tr == 3)
    assert (b[2][lone] == 289).all(), "the smallest given index of the three coincident given points"
    if order != "beside":  # the eight of a cell are spread: other lanes, other chunks
        first = b[0][:288]
        spread = np.array([np.flatnonzero(d2[:, j] == d2[:, j].min()) for j in range(288)])
        assert (spread.max(axis=1) - first >= 64).all()
    if order in ("chunks", "random"):
        assert (np.array([len(set(s // 256)) for s in spread]) >= 3).all()


# ---- Projector.nearest_points against a fake library ------------------------------------------------------------------
class _Lib:
    def __init__(self, n):
        self.calls, self.n = [], n

    def rtr_nearest_points(self, ctx, xyz, stride, count, radius, flags, gi, gd, ri, rd, stats):
        pts = None
        if count:
            addr = xyz.value if isinstance(xyz, C.c_void_p) else xyz
            raw = (C.c_char * ((count - 1) * stride + 12)).from_address(addr)
            rows = np.frombuffer(raw, np.uint8)
            pts = np.stack([rows[j * stride:j * stride + 12].view(np.float32) for j in range(count)])
        self.calls.append({"xyz": pts, "null": xyz is None, "stride": stride, "count": count, "radius": radius, "flags": flags,
                           "out": tuple(p is not None for p in (gi, gd, ri, rd)), "stats": stats is not None})
        for p, rows, base, ct in ((gi, count, 100, C.c_uint32), (gd, count, 0.5, C.c_float), (ri, self.n, 200, C.c_uint32),
                                  (rd, self.n, 0.25, C.c_float)):
            if p is not None:
                out = C.cast(p, C.POINTER(ct))
                for j in range(rows):
                    out[j] = base + j
        if stats is not None:
            out = C.cast(stats, C.POINTER(C.c_uint64))
            for k in range(4):
                out[k] = 30 + k
        return 0


def _stub(pkg, n):
    class Stub:
        _ctx = None
        _lib = _Lib(n)
        device = 0
        num_points = n
        _write_source = staticmethod(pkg.Projector._write_source)
        nearest_points = pkg.Projector.nearest_points

        def _chk(self, rc):
            assert rc == 0
    return Stub()


def test_nearest_points_marshals_and_validates(pkg):
    n = 9
    s = _stub(pkg, n)
    rng = np.random.default_rng(2)
    tight = rng.normal(size=(70, 3)).astype(f32)
    wide = np.c_[tight, np.ones(70, f32)]
    want = {"gi": np.arange(70, dtype=np.uint32) + 100, "gd": np.arange(70, dtype=f32) + f32(0.5),
            "ri": np.arange(n, dtype=np.uint32) + 200, "rd": np.arange(n, dtype=f32) + f32(0.25)}
    for rows, stride, m in ((tight, 12, 70), (wide, 16, 70), (wide[::2], 32, 35)):
        for given in (True, False):
            for resident in (True, False):
                for stats in (True, False):
                    got = s.nearest_points(rows, np.float32(0.25), given=given, resident=resident, stats=stats)
                    call = s._lib.calls[-1]
                    assert np.array_equal(call.pop("xyz"), tight[::2] if stride == 32 else tight)
                    assert call == {"null": False, "stride": stride, "count": m, "radius": 0.25, "flags": 0,
                                    "out": (given, given, resident, resident), "stats": stats}
                    exp = ([want["gi"][:m], want["gd"][:m]] if given else []) + ([want["ri"], want["rd"]] if resident else []) + \
                          ([(30, 31, 32, 33)] if stats else [])
                    if not exp:
                        assert got is None
                        continue
                    got = got if len(exp) > 1 else (got,)
                    assert len(got) == len(exp)
                    for g, e in zip(got, exp):
                        if isinstance(e, tuple):
                            assert g == e
                        else:
                            assert g.dtype == e.dtype and np.array_equal(g, e)
    gi, gd, st = s.nearest_points(tight.tolist(), 0.5)  # (anything numpy converts)
    assert np.array_equal(s._lib.calls[-1]["xyz"], tight)
    gi, gd, ri, rd, st = s.nearest_points(np.zeros((0, 3), f32), 0.1, resident=True)  # (no given point)
    assert gi.shape == gd.shape == (0,) and ri.shape == (n,) and s._lib.calls[-1]["count"] == 0 and s._lib.calls[-1]["null"]
    assert s._lib.calls[-1]["stride"] == 12
    made = len(s._lib.calls)
    for radius in (0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="radius"):
            s.nearest_points(tight, radius)
    for radius in (1e-30, 1e-20, 2e19, 3e38):
        with pytest.raises(ValueError, match="square of radius"):
            s.nearest_points(tight, radius)
    for bad in (np.zeros((5, 2), f32), np.zeros(6, f32), np.zeros((2, 3, 3), f32), np.zeros((8, 4), f32)[:, ::2]):
        with pytest.raises(ValueError, match="xyz"):
            s.nearest_points(bad, 0.1)
    assert len(s._lib.calls) == made, "no argument error reaches the library"


def test_match_points_gathers_the_winners_with_one_extract(pkg):
    L = pkg._lib
    rng = np.random.default_rng(3)
    n, m = 500, 41
    xyz = rng.normal(size=(n, 4)).astype(f32)
    rgb = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    index = rng.integers(0, n, m).astype(np.uint32)
    index[5] = index[6] = index[7]  # (several given points with one winner)
    index[[0, 11, 40]] = L.NEAREST_NONE
    dist2 = rng.random(m).astype(f32)
    log = []

    class P:
        num_points = n

        def nearest_points(self, v, radius, given=True, resident=False, stats=True):
            log.append(("nearest", radius, given, resident, stats))
            return index, dist2

        def extract_points(self, select=None, first=0, count=None, xyz=True, rgb=True, indices=False, out=None):
            log.append(("extract", indices))
            sel = np.unpackbits(select.view(np.uint8), bitorder="little")[:n].astype(bool)
            at = np.flatnonzero(sel)
            return [P.x[at], P.c[at], at.astype(np.uint32)]
    P.x, P.c = xyz, rgb

    class Stub:
        _p = P()
        nearestPoints = pkg.ProjectCloud.nearestPoints
        matchPoints = pkg.ProjectCloud.matchPoints
        _gather_matched = pkg.ProjectCloud._gather_matched

    gi, gd, mx, mc = Stub().matchPoints(np.zeros((m, 3), f32), 0.02)
    assert log == [("nearest", 0.02, True, False, False), ("extract", True)]
    has = index != L.NEAREST_NONE
    assert gi is index and gd is dist2 and mx.shape == (m, 3) and mc.shape == (m, 3)
    assert np.array_equal(mx[has].view(np.uint32), xyz[index[has], :3].copy().view(np.uint32)) and np.array_equal(mc[has], rgb[index[has], :3])
    assert not mx[~has].any() and not mc[~has].any()
    log.clear()
    index[:] = L.NEAREST_NONE  # (no match at all: rows of zeros, and no extract)
    gi, gd, mx, mc = Stub().matchPoints(np.zeros((m, 3), f32), 0.02)
    assert len(log) == 1 and not mx.any() and not mc.any()
