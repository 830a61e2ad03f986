"""rtr_nearest_k_points (include/rtr.h section 6m) without a GPU: the exported symbol, its place in SYMBOLS and the ABI
version, the header's prototype and its statements of the order, the fill, found, k = 1, the self-query rule, the
scratch, the option keys and the errors, the facade declarations and signatures; the two numpy references of
nearest_k_ref.py against each other, against nearest_ref.py (column 0) and near_ref.py (found > 0), on the tie lattice of
nearest_cases.py and on special coordinates; Projector.nearest_k_points' marshalling and argument validation against a
fake library."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import near_ref as nr
import nearest_cases as ncs
import nearest_k_ref as kf
import nearest_ref as nf
from conftest import ROOT
from test_near_host import _clouds

f32 = np.float32
KEYS = ("nearest_k_given_us", "nearest_k_sweep_us", "nearest_k_pair_tests_k", "nearest_k_chunks_skipped", "nearest_k_chunks_decoded",
        "nearest_k_cascades_k")


def test_nearest_k_symbol_exported(pkg):
    L = pkg._lib
    assert L.SYMBOLS.index("rtr_nearest_k_points") == L.SYMBOLS.index("rtr_nearest_points") - 1 == len(L.SYMBOLS) - 3
    assert L.NEAREST_MAX_K == 64 == kf.MAX_K and L.NEAREST_NONE == kf.NONE
    getattr(L.lib(), "rtr_nearest_k_points")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert re.search(r"\bT rtr_nearest_k_points$", nm, re.M)
    assert L.lib().rtr_abi_version() == 2 and L.ABI_VERSION == 2
    at = L.lib().rtr_nearest_k_points.argtypes
    assert at[2] is C.c_size_t and at[3] is C.c_uint64 and at[4] is C.c_float and at[5] is C.c_uint32 and at[6] is C.c_int and len(at) == 11


def test_nearest_k_header_declaration(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    proto = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("int rtr_nearest_k_points("):], flags=re.S)
    assert re.sub(r"\s+", " ", proto).startswith(
        "int rtr_nearest_k_points(rtr_ctx *ctx, const float *xyz, size_t xyz_stride_bytes, uint64_t count, float radius, uint32_t k, "
        "int flags, uint32_t *index, float *dist2, uint32_t *found, uint64_t stats[4]);")
    assert "#define RTR_NEAREST_MAX_K 64" in hdr and "#define RTR_ABI_VERSION 2" in hdr
    assert hdr.index("int rtr_nearest_points(") < hdr.index("/* ---- 6m.") < hdr.index("int rtr_nearest_k_points(") < hdr.index("7. measurement")
    sec = flat[flat.index("---- 6m."):flat.index("int rtr_nearest_k_points(")]
    for text in (
            # what section 6l's rules cover, said once
            "Section 6l's rules apply unchanged to", "the span rule", "no FMA", "denormals kept", "EVERY resident point counts",
            "the order of the given points", "the rows permute with them", "the call ALWAYS waits for its own work", '"point_ids" = 1',
            # the order, the fill, found, k = 1
            "in ascending order of (d2 bits, upload index)", "the first min(k, candidates) of them",
            "the remaining entries of the row are RTR_NEAREST_NONE and +inf (0x7F800000)", "found[j] = the number of real entries of row j",
            "a stable sort on (bits, index) is a bit-for-bit reference", "nothing has a tolerance",
            "With k = 1 the row equals rtr_nearest_points' given_index[j] and given_dist2[j] bit for bit",
            # self queries
            "is its own neighbour at +0", "ask for k + 1", "drop from each row the entry whose index is the point's own",
            "not the row's first entry", "a coincident duplicate with a smaller upload index sorts before",
            # no resident side, k, flags, the outputs
            "There is no resident side", "k is 1 .. RTR_NEAREST_MAX_K", "flags must be 0", "may be NULL on its own",
            "all three NULL is legal", "written only when the call succeeds",
            # stats
            "[0] the given points with found > 0", "rtr_select_near's stats[2]", "[1] the sum of found", "[2] the non-finite given points",
            "[3] the given points with found == k", "All four are exact and independent of the form of the cloud",
            # how, and the scratch
            "no lock, no retry, no wave waiting for another", "56 B per given point", "8 k B per given point for the rows",
            "a staging copy of every output that lies in host memory", "Everything is allocated before anything is written",
            # errors
            "section 6l's list as it is", "k == 0 or k > RTR_NEAREST_MAX_K -> RTR_ERR_INVALID", "RTR_ERR_UNSUPPORTED", "RTR_ERR_HIP",
            "names the argument", "it depends on timing"):
        assert text.lower() in sec.lower(), text
    for key in KEYS:
        assert '"%s"' % key in sec and '"%s"' % key in hdr[:hdr.index("/* ---- 6l.")], key
    src = tmp_path / "nearest_k_abi.c"  # the prototype as a C99 consumer sees it
    src.write_text('#include "rtr.h"\n'
                   "typedef int (*fn_t)(rtr_ctx *, const float *, size_t, uint64_t, float, uint32_t, int, uint32_t *, float *, uint32_t *,\n"
                   "                    uint64_t[4]);\n"
                   "int main(void) { fn_t f = rtr_nearest_k_points; return f == 0 || RTR_NEAREST_MAX_K != 64; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "nearest_k_abi.o")])
    hpp = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read())
    for decl in ("NearestK nearestKPoints(const float* xyz, size_t xyz_stride_bytes, size_t m, uint32_t k, float radius)",
                 "struct NearestK {", "std::vector<uint32_t> found;", "uint32_t k;", "// nearestKPoints (section 6m)"):
        assert decl in hpp, decl


def test_python_signatures(pkg):
    assert str(inspect.signature(pkg.Projector.nearest_k_points)) == "(self, xyz, k, radius, stats=True)"
    assert str(inspect.signature(pkg.ProjectCloud.nearestKPoints)) == "(self, vertices, k, radius)"
    doc = pkg.Projector.nearest_k_points.__doc__
    assert "ascending" in doc and "NEAREST_NONE" in doc and "+inf" in doc and "found" in doc


# ---- the reference against itself -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_clouds()))
def test_brute_force_and_buckets_agree(name):
    A, G, r = _clouds()[name]  # (test_near_host.py's five kinds of cloud)
    pairs = kf.candidate_pairs(A, G, r)
    one = nf.nearest_brute(A, G, r)
    _, near = nr.near_brute(A, G, r)
    for k in (1, 2, 5, 64):
        b, q = kf.nearest_k_brute(A, G, r, k), kf.rows_of_pairs(pairs, G.shape[0], k, G)
        assert kf.same(b[:3], q[:3]) and b[3] == q[3], (name, k)
        assert kf.same((b[0][:, 0], b[1][:, 0]), one[:2]), "column 0 is rtr_nearest_points' answer"
        assert np.array_equal(b[2] > 0, near), "found > 0 is section 6k's near bit"
        assert b[3][0] == int(near.sum()) and b[3][1] == int(b[2].sum()) and b[3][2] == 0 and b[3][3] == int((b[2] == k).sum())
        # the rows: real entries first, sorted by (bits, index) strictly, NONE and +inf behind them
        col = np.arange(k)[None, :]
        real = col < b[2][:, None]
        assert np.array_equal(b[0] != kf.NONE, real) and np.array_equal(np.isfinite(b[1]), real)
        key = (kf.bits(b[1]).astype(np.uint64) << np.uint64(32)) | b[0]
        assert (key[:, 1:] > key[:, :-1])[real[:, 1:]].all()
        assert (kf.bits(b[1])[~real] == kf.INF_BITS).all()
    if name == "dup":  # (coincident resident points: both copies of a pair at d2 = +0, the smaller index first)
        two = kf.nearest_k_brute(A, G, r, 2)
        zero = np.flatnonzero((kf.bits(two[1])[:, :2] == 0).all(axis=1) & (two[2] >= 2))
        assert zero.size >= 300 and (two[0][zero, 0] < two[0][zero, 1]).all()


@pytest.mark.parametrize("order", ncs.TIE_ORDERS)
def test_the_lattice_returns_the_smallest_indices_of_a_tie(order):
    A, G = ncs.tie_lattice(order)
    tg, _ = ncs.tie_counts(A, G)
    assert (tg == 8).sum() == 288 and (tg[:288] == 8).all()
    d = A[:, None, :] - G[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    ties = np.array([np.flatnonzero(d2[:, j] == d2[:, j].min()) for j in range(288)])  # (ascending upload indices)
    pairs = kf.candidate_pairs(A, G, ncs.TIE_RADIUS)
    for k in (1, 3, 7, 8, 9):
        b, q = kf.nearest_k_brute(A, G, ncs.TIE_RADIUS, k), kf.rows_of_pairs(pairs, G.shape[0], k, G)
        assert kf.same(b[:3], q[:3]) and b[3] == q[3], (order, k)
        # the eight resident points of a cell lie at ONE d2 bit pattern: k < 8 must return the k smallest upload indices
        # of the tie, k = 9 must find eight
        assert (b[2][:288] == min(k, 8)).all()
        assert np.array_equal(b[0][:288, :min(k, 8)], ties[:, :min(k, 8)])
        assert (kf.bits(b[1])[:288, :min(k, 8)] == kf.bits(f32(48 / 65536))[0]).all()
        if k == 9:
            assert (b[0][:288, 8] == kf.NONE).all() and (kf.bits(b[1])[:288, 8] == kf.INF_BITS).all()
        assert b[2][288] == min(k, 3) and not kf.bits(b[1])[288, :min(k, 3)].any()  # (the pile: three at +0)


def test_reference_on_special_coordinates():
    big = np.finfo(f32).max
    A = f32([[0, 0, 0], [0.05, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [-big, 0, 0], [1, 1, 1], [0, 0, 0]])
    G = f32([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [0.2, 0, 0], [np.nan, np.nan, np.nan], [0.03, 0, 0]])
    N = kf.NONE
    idx, d2, found, st = kf.nearest_k_brute(A, G, 0.05, 3)
    # the origin finds both coincident points at +0, the smaller index first, then (0.05, 0, 0) at the radius; +FLT_MAX
    # finds +FLT_MAX at +0; a non-finite point on either side is nobody's candidate
    assert idx.tolist() == [[0, 8, 1], [N] * 3, [N] * 3, [N] * 3, [5, N, N], [N] * 3, [N] * 3, [1, 0, 8]]
    assert list(found) == [3, 0, 0, 0, 1, 0, 0, 3] and st == (3, 7, 4, 2)
    assert list(kf.bits(d2)[0]) == [0, 0, int(kf.bits(kf.r2_of(0.05))[0])] and list(kf.bits(d2)[4]) == [0, kf.INF_BITS, kf.INF_BITS]
    q = kf.nearest_k_bucket(A[:5], G[[0, 1, 2, 3, 7]], 0.05, 3)
    b = kf.nearest_k_brute(A[:5], G[[0, 1, 2, 3, 7]], 0.05, 3)
    assert kf.same(q[:3], b[:3]) and q[3] == b[3] == (2, 4, 3, 0)
    e = kf.nearest_k_brute(A, np.zeros((0, 3), f32), 0.05, 4)
    assert e[0].shape == e[1].shape == (0, 4) and e[2].shape == (0,) and e[3] == (0, 0, 0, 0)


# ---- Projector.nearest_k_points against a fake library ----------------------------------------------------------------
class _Lib:
    def __init__(self):
        self.calls = []

    def rtr_nearest_k_points(self, ctx, xyz, stride, count, radius, k, flags, index, dist2, found, stats):
        pts = None
        if count:
            addr = xyz.value if isinstance(xyz, C.c_void_p) else xyz
            raw = (C.c_char * ((count - 1) * stride + 12)).from_address(addr)
            rows = np.frombuffer(raw, np.uint8)
            pts = np.stack([rows[j * stride:j * stride + 12].view(np.float32) for j in range(count)])
        self.calls.append({"xyz": pts, "null": xyz is None, "stride": stride, "count": count, "radius": radius, "k": k, "flags": flags,
                           "out": tuple(p is not None for p in (index, dist2, found)), "stats": stats is not None})
        for p, words, base, ct in ((index, count * k, 100, C.c_uint32), (dist2, count * k, 0.5, C.c_float), (found, count, 7, C.c_uint32)):
            if p is not None:
                out = C.cast(p, C.POINTER(ct))
                for j in range(words):
                    out[j] = base + j
        if stats is not None:
            out = C.cast(stats, C.POINTER(C.c_uint64))
            for q in range(4):
                out[q] = 30 + q
        return 0


def _stub(pkg):
    class Stub:
        _ctx = None
        _lib = _Lib()
        device = 0
        num_points = 9
        _write_source = staticmethod(pkg.Projector._write_source)
        nearest_k_points = pkg.Projector.nearest_k_points

        def _chk(self, rc):
            assert rc == 0
    return Stub()


def test_nearest_k_points_marshals_and_validates(pkg):
    s = _stub(pkg)
    rng = np.random.default_rng(2)
    tight = rng.normal(size=(70, 3)).astype(f32)
    wide = np.c_[tight, np.ones(70, f32)]
    for rows, stride, m in ((tight, 12, 70), (wide, 16, 70), (wide[::2], 32, 35)):
        for k in (1, 5, 64):
            for stats in (True, False):
                got = s.nearest_k_points(rows, k, np.float32(0.25), stats=stats)
                call = s._lib.calls[-1]
                assert np.array_equal(call.pop("xyz"), tight[::2] if stride == 32 else tight)
                assert call == {"null": False, "stride": stride, "count": m, "radius": 0.25, "k": k, "flags": 0, "out": (True,) * 3,
                                "stats": stats}
                assert len(got) == (4 if stats else 3)
                index, dist2, found = got[:3]
                assert index.dtype == np.uint32 and dist2.dtype == f32 and found.dtype == np.uint32
                assert index.shape == dist2.shape == (m, k) and found.shape == (m,)
                assert np.array_equal(index, (np.arange(m * k, dtype=np.uint32) + 100).reshape(m, k))  # (row j at [j * k])
                assert np.array_equal(dist2, (np.arange(m * k, dtype=f32) + f32(0.5)).reshape(m, k))
                assert np.array_equal(found, np.arange(m, dtype=np.uint32) + 7)
                assert not stats or got[3] == (30, 31, 32, 33)
    s.nearest_k_points(tight.tolist(), np.int64(3), 0.5)  # (anything numpy converts; a numpy integer)
    assert np.array_equal(s._lib.calls[-1]["xyz"], tight) and s._lib.calls[-1]["k"] == 3
    index, dist2, found, st = s.nearest_k_points(np.zeros((0, 3), f32), 4, 0.1)  # (no given point)
    assert index.shape == dist2.shape == (0, 4) and found.shape == (0,)
    assert s._lib.calls[-1]["count"] == 0 and s._lib.calls[-1]["null"] and s._lib.calls[-1]["stride"] == 12
    made = len(s._lib.calls)
    for radius in (0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="radius"):
            s.nearest_k_points(tight, 3, radius)
    for radius in (1e-30, 1e-20, 2e19, 3e38):
        with pytest.raises(ValueError, match="square of radius"):
            s.nearest_k_points(tight, 3, radius)
    for k in (0, -1, 65, 2 ** 32 + 1):
        with pytest.raises(ValueError, match="k must be in 1"):
            s.nearest_k_points(tight, k, 0.1)
    for k in (2.0, "3", None, True):
        with pytest.raises(TypeError, match="k must be an integer"):
            s.nearest_k_points(tight, k, 0.1)
    for bad in (np.zeros((5, 2), f32), np.zeros(6, f32), np.zeros((2, 3, 3), f32), np.zeros((8, 4), f32)[:, ::2]):
        with pytest.raises(ValueError, match="xyz"):
            s.nearest_k_points(bad, 3, 0.1)
    assert len(s._lib.calls) == made, "no argument error reaches the library"


def test_project_cloud_forwards(pkg):
    log = []

    class P:
        def nearest_k_points(self, v, k, radius, stats=True):
            log.append((k, radius, stats))
            return "index", "dist2", "found"

    class Stub:
        _p = P()
        nearestKPoints = pkg.ProjectCloud.nearestKPoints

    assert Stub().nearestKPoints(np.zeros((3, 3), f32), 5, 0.02) == ("index", "dist2", "found") and log == [(5, 0.02, False)]
