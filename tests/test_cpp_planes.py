"""rtr_fit_plane in C++ (include/rtr.h section 6j).  CPU: the sampler and the candidate arithmetic of
csrc/rtr_plane_fit.h built with plain g++ -ffp-contract=off -fno-fast-math as a stand-alone program
(tests/cpp/plane_fit_check.cpp) and compared bit for bit with planes_ref.py on 20 000 triples -- magnitudes from
subnormal to 1e30, collinear and coincident triples, repeated ranks, non-finite samples, every branch of the orientation
rule -- the same program once more under -fsanitize=address,undefined, and the facade's calls of
include/rtr_project_cloud.hpp compiled and linked against librtr_hip.so.  GPU: fitPlane, selectPlane, segmentPlane and
countInBands through the C++ facade give the reference's planes, counts and words, and the Python facade gives the same."""
import os
import subprocess

import numpy as np
import pytest

import planes_ref as pr
import select_ref as sr
from conftest import ROOT

CSRC = os.path.join(ROOT, "real-time-neural-rendering-of-lidar-point-clouds_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "plane_fit_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC]
SEED, DRAWS, DIST = 0x1234_5678_9ABC_DEF0, 64, np.float32(0.03)


def triples():
    """(points float32 [k, 3, 3], ranks uint64 [k, 3], groups): the 20 000 triples."""
    rng = np.random.default_rng(23)
    f = np.float32
    k = 20_000
    mag = (10.0 ** rng.uniform(-45, 30, (k, 1, 1))).astype(np.float64)  # one magnitude per triple: subnormal .. 1e30
    pts = (rng.normal(size=(k, 3, 3)) * mag).astype(f)
    near = slice(0, 6000)  # clouds of ordinary size
    pts[near] = (rng.normal(size=(6000, 3, 3)) * [4, 3, 1]).astype(f)
    ranks = rng.integers(0, 1 << 40, (k, 3)).astype(np.uint64)
    groups = {}
    g = groups["collinear"] = slice(6000, 6600)  # p2 = p0 + 2 (p1 - p0), exactly (small integers)
    a, d = rng.integers(-50, 50, (600, 3)), rng.integers(-9, 9, (600, 3))
    pts[g, 0], pts[g, 1], pts[g, 2] = a, a + d, a + 2 * d
    g = groups["coincident"] = slice(6600, 7000)
    pts[g, 1] = pts[g, 0]
    pts[6800:7000, 2] = pts[6800:7000, 0]
    g = groups["repeated_rank"] = slice(7000, 7600)
    ranks[7000:7200, 1] = ranks[7000:7200, 0]
    ranks[7200:7400, 2] = ranks[7200:7400, 0]
    ranks[7400:7600, 2] = ranks[7400:7600, 1]
    g = groups["non_finite"] = slice(7600, 8200)
    bad = rng.choice(f([np.nan, np.inf, -np.inf]), 600)
    pts[g].reshape(600, 9)[np.arange(600), rng.integers(0, 9, 600)] = bad  # (a view: written in place)
    # the orientation rule: normals with c < 0, c == 0 and b < 0, c == b == 0 and a < 0, and their mirror images
    g = groups["orientation"] = slice(8200, 9400)
    o = rng.integers(-20, 20, (1200, 3)).astype(f)
    s = rng.integers(1, 9, (1200, 2)).astype(f)
    e1, e2 = np.zeros((1200, 3), f), np.zeros((1200, 3), f)
    e1[0:200, 0], e2[0:200, 1] = s[0:200, 0], s[0:200, 1]            # n = +z
    e1[200:400, 1], e2[200:400, 0] = s[200:400, 0], s[200:400, 1]    # n = -z
    e1[400:600, 2], e2[400:600, 0] = s[400:600, 0], s[400:600, 1]    # n = +y, c == 0
    e1[600:800, 0], e2[600:800, 2] = s[600:800, 0], s[600:800, 1]    # n = -y
    e1[800:1000, 1], e2[800:1000, 2] = s[800:1000, 0], s[800:1000, 1]      # n = +x, c == b == 0
    e1[1000:1200, 2], e2[1000:1200, 1] = s[1000:1200, 0], s[1000:1200, 1]  # n = -x
    pts[g, 0], pts[g, 1], pts[g, 2] = o, o + e1, o + e2
    groups["huge"] = slice(9400, 9500)  # offsets beyond fp32: a far point and a steep normal
    pts[9400:9500] = rng.uniform(-3.3e38, 3.3e38, (100, 3, 3)).astype(f)
    far, step = f(3.3e38) * rng.choice(f([-1, 1]), (50, 1)), (10.0 ** rng.uniform(30, 37, (50, 1))).astype(f)
    zero = np.zeros((50, 1), f)
    pts[9450:9500, 0] = far  # the corner (+-3.3e38) x 3 with the normal along the diagonal: |D| = sqrt(3) x 3.3e38
    pts[9450:9500, 1] = far + np.concatenate([step, -step, zero], axis=1)
    pts[9450:9500, 2] = far + np.concatenate([zero, step, -step], axis=1)
    return pts, ranks, groups


def run(exe, tmp_path, pts, ranks):
    k = pts.shape[0]
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.uint64(SEED).tobytes() + np.uint64(DRAWS).tobytes() + np.float32(DIST).tobytes() + np.uint64(k).tobytes())
        rec = np.zeros(k, dtype=[("p", "<f4", 9), ("r", "<u8", 3)])
        rec["p"], rec["r"] = pts.reshape(k, 9), ranks
        assert rec.dtype.itemsize == 60
        fh.write(rec.tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], text=True).split()
    raw = open(tmp_path / "out.bin", "rb").read()
    z = np.frombuffer(raw[:8 * DRAWS], "<u8")
    res = np.frombuffer(raw[8 * DRAWS:], dtype=[("ok", "<u4"), ("plane", "<f4", 4), ("band", "<f4", 5)])
    assert out[0] == "ok" and int(out[1]) == k == res.size and int(out[2]) == int(res["ok"].sum())
    return z, res


def compare(z, res, pts, ranks, groups):
    assert [int(v) for v in z] == [pr.draw(SEED, t) for t in range(DRAWS)]
    want_ok = np.zeros(len(pts), bool)
    flips = {"c": 0, "b": 0, "a": 0}
    for i in range(len(pts)):
        pl = pr.candidate(pts[i, 0], pts[i, 1], pts[i, 2], [int(r) for r in ranks[i]])
        want_ok[i] = pl is not None
        assert bool(res["ok"][i]) == want_ok[i], i
        if pl is None:
            assert not res["plane"][i].any() and not res["band"][i].any()
            continue
        assert np.array_equal(res["plane"][i].view(np.uint32), pl.view(np.uint32)), (i, res["plane"][i], pl)
        assert np.array_equal(res["band"][i].view(np.uint32), pr.band_of(pl, DIST).view(np.uint32)), i
        assert (pl[2], pl[1], pl[0]) > (0, 0, 0), (i, pl)  # (c, b, a) lexicographically positive
        flips["c" if pl[2] != 0 else ("b" if pl[1] != 0 else "a")] += 1
    for name in ("collinear", "coincident", "repeated_rank", "non_finite"):
        assert not want_ok[groups[name]].any(), name
    assert want_ok[groups["orientation"]].all() and flips["b"] >= 400 and flips["a"] >= 400
    assert want_ok[9400:9450].sum() > 25 and not want_ok[9450:9500].any()  # (offsets that fit fp32, and offsets that do not)
    assert want_ok[:6000].all() and want_ok[9500:].sum() > 9000  # (tiny triangles whose squares underflow are degenerate)
    assert not want_ok[9500:].all()


@pytest.fixture(scope="module")
def data():
    return triples()


def test_plane_fit_header_matches_the_reference_bit_for_bit(tmp_path, data):
    exe = str(tmp_path / "plane_fit_check")
    subprocess.check_call(["g++", "-O2"] + FLAGS + [SRC, "-o", exe])
    pts, ranks, groups = data
    z, res = run(exe, tmp_path, pts, ranks)
    compare(z, res, pts, ranks, groups)


def test_plane_fit_header_under_the_sanitizers(tmp_path, data):
    """The same stand-alone program built with -fsanitize=address,undefined: a clean run, and the same bytes."""
    exe = str(tmp_path / "plane_fit_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS + [SRC, "-o", exe])
    pts, ranks, groups = data
    z, res = run(exe, tmp_path, pts, ranks)
    plain = str(tmp_path / "plane_fit_check")
    subprocess.check_call(["g++", "-O2"] + FLAGS + [SRC, "-o", plain])
    sub = tmp_path / "plain"
    sub.mkdir()
    z2, res2 = run(plain, sub, pts, ranks)
    assert np.array_equal(z, z2) and res.tobytes() == res2.tobytes()


def test_plane_fit_header_is_plain_cpp():
    src = open(os.path.join(CSRC, "rtr_plane_fit.h")).read()
    for name in ("uint64_t plane_draw(uint64_t seed, uint64_t t)", "bool plane_candidate(", "void plane_band("):
        assert name in src, name
    assert "__global__" not in src and "#include <hip" not in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "rtr_planes.hip" in mk and "rtr_plane_fit.h" in mk and "-ffp-contract=off" in mk


def _build(tmp_path, pkg):
    exe = str(tmp_path / "planes_facade_check")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "planes_facade_check.cpp"), "-o", exe, pkg.LIB_PATH,
                           "-Wl,-rpath," + libdir])
    return exe


def test_cpp_planes_facade_compiles_and_links(tmp_path, pkg):
    assert os.path.exists(_build(tmp_path, pkg))


@pytest.mark.gpu
def test_cpp_planes_match_the_reference_and_the_python_facade(tmp_path, pkg, orc):
    exe = _build(tmp_path, pkg)
    n, dist, iters, seed = 60_001, np.float32(0.03), 48, 5
    xyzw, rgba = orc.generate("room_shell", 15, 0, n, n)
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(n).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "args.bin", "wb") as f:
        f.write(np.float32(dist).tobytes() + np.uint32(iters).tobytes() + np.uint64(seed).tobytes())
    out = str(tmp_path / "out")
    subprocess.check_call([exe, str(tmp_path / "cloud.bin"), str(tmp_path / "args.bin"), out], timeout=300)
    fit_t = np.dtype([("plane", "<f4", 4), ("v", "<u8", 5)])
    rd = lambda ext, dt: np.fromfile(out + ext, dtype=dt)  # noqa: E731
    plane0, st0 = pr.fit(xyzw, dist, iters, seed)
    got0 = rd(".fit0", fit_t)[0]
    assert np.array_equal(got0["plane"].view(np.uint32), plane0.view(np.uint32))
    assert tuple(int(v) for v in got0["v"]) == (st0[0],) + st0 and 3 <= st0[0] < n
    in0 = pr.in_band(xyzw, pr.band_of(plane0, dist))
    assert int(in0.sum()) == st0[0]
    rest = ~in0
    plane1, st1 = pr.fit(xyzw, dist, iters, seed + 1, rest)
    got1 = rd(".fit1", fit_t)[0]
    assert np.array_equal(got1["plane"].view(np.uint32), plane1.view(np.uint32))
    assert tuple(int(v) for v in got1["v"]) == (st1[0],) + st1 and st1[3] == int(rest.sum())
    assert list(rd(".counts", np.uint64)) == [st0[0], st0[0], int(rest.sum()), st1[0]]
    assert np.array_equal(rd(".words0", np.uint32), sr.words(in0))
    assert np.array_equal(rd(".words1", np.uint32), sr.words(in0))
    # the Python facade: the same planes, counts and words
    pc = pkg.ProjectCloud(xyzw, rgba, point_ids=True)
    pl, inl = pc.fitPlane(dist, iters, seed)
    assert np.array_equal(pl.view(np.uint32), plane0.view(np.uint32)) and inl == st0[0]
    assert pc.projector.get_option("selection") == 0
    assert pc.selectPlane(pl, dist) == st0[0]
    assert np.array_equal(pc.projector.download(pkg._lib.BUF_SELECTION), sr.words(in0))
    assert pc.selectPlane(pl, dist, outside=True) == n - st0[0]
    pc.clearSelection()
    pl, inl = pc.segmentPlane(dist, iters, seed)
    assert inl == st0[0] and np.array_equal(pc.projector.download(pkg._lib.BUF_SELECTION), sr.words(in0))
    assert pc.selectPlanes(None, op="toggle") == int(rest.sum())
    pl1, inl1 = pc.fitPlane(dist, iters, seed + 1, selected=True)
    assert np.array_equal(pl1.view(np.uint32), plane1.view(np.uint32)) and inl1 == st1[0]
    assert np.array_equal(pc.projector.download(pkg._lib.BUF_SELECTION), sr.words(rest))
