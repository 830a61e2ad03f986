"""rtr_select_clusters (include/rtr.h section 6i) without a GPU: the exported symbol and the ABI version, the header's
prototype and its statement of the relation, the label rule, the seeded rule and the cost; the facade declarations; the
two references of clusters_ref.py against each other, against scipy where it is installed, and on special coordinates;
the pinned counts of the scenes the GPU tests use; Projector.select_clusters' marshalling and argument validation
against a fake library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clusters_cases as cc
import clusters_ref as cr
import neighbours_ref as nr
from conftest import ROOT
from test_neighbours_host import _clouds

f32 = np.float32


def test_clusters_symbol_exported(pkg):
    L = pkg._lib
    assert "rtr_select_clusters" in L.SYMBOLS
    assert hasattr(L.lib(), "rtr_select_clusters")
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    assert re.search(r"\bT rtr_select_clusters$", nm, re.M)
    assert L.lib().rtr_abi_version() == 2
    assert L.CLUSTER_SEEDED == 1


def test_clusters_header_declaration(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    assert ("int rtr_select_clusters(rtr_ctx *ctx, float radius, uint32_t min_points, uint32_t max_points, int flags, int op, "
            "uint32_t *labels, uint64_t stats[4]);") in re.sub(r"\s+", " ", hdr)
    assert "#define RTR_ABI_VERSION 2" in hdr and re.search(r"#define RTR_CLUSTER_SEEDED\s+1\b", hdr)
    assert hdr.index("6h. selection by neighbour count") < hdr.index("6i. selection by connected cluster") < hdr.index("7. measurement")
    assert hdr.index("int rtr_select_neighbours(") < hdr.index("6i. selection by connected cluster")
    sec = flat[flat.index("6i. selection by connected cluster"):flat.index("int rtr_select_clusters(")]
    for text in ("Neighbour relation: exactly section 6h's", "((dx dx + dy dy) + dz dz) <= r2", "r2 = radius radius, rounded once to fp32 on the host",
                 "no FMA", "inclusive", "coincident points are neighbours", "never its own neighbour", "a non-finite point has no neighbours",
                 "connected components", "cluster of one", "smallest upload index among its members",
                 "selected BEFORE this call", "a selection that does not exist yet is empty, so nothing hits",
                 "max_points == 0 (unbounded)", "NO early exit", "O(m^2)", "56 B per point", "RTR_ERR_UNSUPPORTED",
                 "written only when the call succeeds", "[1] clusters, [2] clusters that hit", "largest cluster",
                 "unknown bits in flags", "max_points != 0 && max_points < min_points", "ALWAYS waits"):
        assert text in sec, text
    src = tmp_path / "clusters_abi.c"  # the prototype as a C99 consumer sees it
    src.write_text('#include "rtr.h"\n'
                   "typedef int (*fn_t)(rtr_ctx *, float, uint32_t, uint32_t, int, int, uint32_t *, uint64_t[4]);\n"
                   "int main(void) { fn_t f = rtr_select_clusters; return f == 0 || RTR_CLUSTER_SEEDED != 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "clusters_abi.o")])
    hpp = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtr_project_cloud.hpp")).read())
    for decl in ("uint64_t selectClusters(float radius, uint32_t min_points = 1, uint32_t max_points = 0, bool seeded = false, "
                 "int op = RTR_SELECT_REPLACE, bool outside = false, uint32_t* labels = nullptr)",
                 "uint64_t growSelection(float radius)", "uint64_t removeSmallClusters(float radius, uint32_t min_points)"):
        assert decl in hpp, decl


def test_option_keys_are_documented():
    hdr = open(os.path.join(ROOT, "include", "rtr.h")).read()
    for key in ("clusters_keys_us", "clusters_sort_us", "clusters_label_us", "clusters_pair_tests_k"):
        assert '"%s"' % key in hdr, key


# ---- the reference against itself -------------------------------------------------------------------------------------
def _partition(lab):
    """the clusters as a canonical set of member tuples"""
    order = np.argsort(lab, kind="stable")
    cuts = np.flatnonzero(np.diff(lab[order])) + 1
    return sorted(tuple(g) for g in np.split(order, cuts))


@pytest.mark.parametrize("name", sorted(_clouds()))
def test_propagation_and_brute_force_agree(name):
    xyz, r = _clouds()[name]
    a, b = cr.labels(xyz, r), cr.labels_brute(xyz, r)
    assert a.dtype == np.uint32 and np.array_equal(a, b), np.flatnonzero(a != b)[:5]
    n = xyz.shape[0]
    assert (a <= np.arange(n)).all() and np.array_equal(a[a], a)  # (a label is a member, and its own label)
    sz = cr.sizes(a)
    assert sz.sum() == (sz.astype(np.int64) ** 2)[a == np.arange(n)].sum() and sz.min() >= 1
    # the pairs are the relation: their counts are neighbours_ref's
    i, j = cr.pairs(xyz, r)
    assert np.array_equal(np.bincount(i, minlength=n), nr.counts_brute(xyz, r)) and (a[i] == a[j]).all()


@pytest.mark.parametrize("name", sorted(_clouds()))
def test_reference_equals_scipy(name):
    sp = pytest.importorskip("scipy.sparse")
    cg = pytest.importorskip("scipy.sparse.csgraph")
    xyz, r = _clouds()[name]
    n = xyz.shape[0]
    i, j = cr.pairs(xyz, r)
    ncomp, comp = cg.connected_components(sp.coo_matrix((np.ones(i.size, np.int8), (i, j)), shape=(n, n)).tocsr(), directed=False)
    lab = cr.labels(xyz, r)
    assert ncomp == cr.stats(lab, cr.hits(lab))[0]
    assert _partition(lab) == _partition(comp)  # by partition
    first = np.full(ncomp, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    assert np.array_equal(first[comp].astype(np.uint32), lab)  # by label: the smallest member index


def test_hits_and_stats_of_a_small_forest():
    lab = np.uint32([0, 0, 2, 0, 4, 4, 6, 2, 0])  # clusters {0, 1, 3, 8}, {2, 7}, {4, 5}, {6}
    assert list(cr.sizes(lab)) == [4, 4, 2, 4, 2, 2, 1, 2, 4]
    assert cr.hits(lab).all() and list(np.flatnonzero(cr.hits(lab, 2))) == [0, 1, 2, 3, 4, 5, 7, 8]
    assert list(np.flatnonzero(cr.hits(lab, 2, 2))) == [2, 4, 5, 7] and not cr.hits(lab, 5).any()
    seeds = np.zeros(9, bool)
    assert not cr.hits(lab, seeds=seeds).any()  # (seeded without a selection: nothing)
    seeds[[7, 6]] = True
    assert list(np.flatnonzero(cr.hits(lab, seeds=seeds))) == [2, 6, 7]
    assert list(np.flatnonzero(cr.hits(lab, 2, seeds=seeds))) == [2, 7]
    assert cr.stats(lab, cr.hits(lab, 2)) == (4, 3, 4) and cr.stats(lab, cr.hits(lab, 1, 1)) == (4, 1, 4)


def test_reference_on_special_coordinates():
    big = np.finfo(f32).max
    xyz = f32([[0, 0, 0], [0.05, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [-big, 0, 0], [big, 0, 0],
               [0, 0, 0], [np.nan, 0, 0], [0.1, 0, 0]])
    # NaN / +-inf points are singletons labelled by themselves, also two NaN points at "the same place"; the two
    # +FLT_MAX points are one cluster (d2 == 0), -FLT_MAX alone; 0 -- 0.05 -- 0.1 is a chain with the coincident origin
    lab = cr.labels_brute(xyz, 0.05)
    assert list(lab) == [0, 0, 2, 3, 4, 5, 6, 5, 0, 9, 0]
    assert list(cr.sizes(lab)) == [4, 4, 1, 1, 1, 2, 1, 2, 4, 1, 4]
    hit = cr.hits(lab, 2)
    assert cr.stats(lab, hit) == (7, 2, 4) and list(np.flatnonzero(~hit)) == [2, 3, 4, 6, 9]
    # two coincident piles without FLT_MAX: each a cluster, apart
    piles = np.concatenate([np.tile(f32([[1, 2, 3]]), (40, 1)), np.tile(f32([[1, 2, 3.5]]), (7, 1))])[np.random.default_rng(1).permutation(47)]
    lab = cr.labels(piles, 0.05)
    assert np.array_equal(lab, cr.labels_brute(piles, 0.05)) and sorted(np.bincount(lab)[np.unique(lab)]) == [7, 40]
    assert cr.hits(lab, 8).sum() == 40 and cr.hits(lab, 1, 7).sum() == 7


def test_threshold_joins_or_splits_by_one_ulp():
    r = f32(0.05)
    a, b = f32(0.05), np.nextafter(f32(0.05), f32(1))
    for fn in (cr.labels, cr.labels_brute):
        assert list(fn(f32([[0, 0, 0], [a, 0, 0]]), r)) == [0, 0]
        assert list(fn(f32([[0, 0, 0], [b, 0, 0]]), r)) == [0, 1]
        assert list(fn(f32([[b, 0, 0], [0, 0, 0], [a, 0, 0]]), r)) == [0, 0, 0]  # (b is no neighbour of the origin, but of a: joined through it)


@pytest.fixture(scope="module")
def scene_labels(orc):
    out = {}
    for scene, (n, radii) in cc.SCENES.items():
        xyzw, _ = orc.generate(scene, cc.SEED, 0, n, n)
        for r in radii + ((cc.EVERYTHING[1],) if scene == cc.EVERYTHING[0] else ()):
            out[(scene, r)] = (n, cr.labels(xyzw, r))
    return out


def test_the_pinned_counts_of_the_gpu_scenes_hold(scene_labels):
    spread = 0
    for key, (clusters, clusters2, largest, hits) in cc.PINS.items():
        n, lab = scene_labels[key]
        sz = cr.sizes(lab)
        roots = lab == np.arange(n)
        got = tuple(int(cr.hits(lab, lo, hi).sum()) for lo, hi in cc.WINDOWS)
        assert (int(roots.sum()), int((roots & (sz >= 2)).sum()), int(sz.max()), got) == (clusters, clusters2, largest, hits), key
        assert got[0] == n
        for w in cc.SPREAD[key]:
            assert cc.spread_holds(clusters2, largest, got[cc.WINDOWS.index(w)], n), (key, w)
            spread += 1
    assert spread == 9 and set(cc.PINS) == set(cc.SPREAD) == {(s, r) for s, (_, rr) in cc.SCENES.items() for r in rr}
    for (scene, r, lo, hi), pin in cc.NAMED_PINS.items():
        n, lab = scene_labels[(scene, r)]
        hit = cr.hits(lab, lo, hi)
        st = cr.stats(lab, hit)
        assert (st[0], st[2], int(hit.sum())) == pin
    assert cc.NOTHING[2] > cc.SCENES[cc.NOTHING[0]][0] and cc.NAMED_PINS[cc.EVERYTHING][0] == 1


# ---- Projector.select_clusters against a fake library -----------------------------------------------------------------
class _Lib:
    def __init__(self):
        self.calls = []

    def rtr_select_clusters(self, ctx, radius, min_points, max_points, flags, op, labels, stats):
        self.calls.append({"radius": radius, "min": min_points, "max": max_points, "flags": flags, "op": op,
                           "labels": labels is not None, "stats": stats is not None})
        if stats is not None:
            out = C.cast(stats, C.POINTER(C.c_uint64))
            for k in range(4):
                out[k] = 20 + k
        if labels is not None:
            out = C.cast(labels, C.POINTER(C.c_uint32))
            for k in range(5):
                out[k] = 4 - k
        return 0


def _stub(pkg):
    class Stub:
        _ctx = None
        _lib = _Lib()
        _SELECT_OPS = pkg.Projector._SELECT_OPS
        num_points = 5
        select_clusters = pkg.Projector.select_clusters

        def _chk(self, rc):
            assert rc == 0
    return Stub()


def test_select_clusters_marshals_and_validates(pkg):
    L = pkg._lib
    s = _stub(pkg)
    assert s.select_clusters(0.05) == (20, 21, 22, 23)
    assert s._lib.calls[-1] == {"radius": 0.05, "min": 1, "max": 0, "flags": 0, "op": L.SELECT_REPLACE, "labels": False, "stats": True}
    assert s.select_clusters(np.float32(0.25), np.uint32(2), np.uint32(49), seeded=True, op="toggle", outside=True, stats=False) is None
    assert s._lib.calls[-1] == {"radius": 0.25, "min": 2, "max": 49, "flags": L.CLUSTER_SEEDED, "op": L.SELECT_TOGGLE | L.SELECT_OUTSIDE,
                                "labels": False, "stats": False}
    st, lab = s.select_clusters(0.1, 50, labels=True)
    assert st == (20, 21, 22, 23) and lab.dtype == np.uint32 and list(lab) == [4, 3, 2, 1, 0] and s._lib.calls[-1]["labels"]
    lab = s.select_clusters(0.1, 3, 3, labels=True, stats=False)
    assert isinstance(lab, np.ndarray) and list(lab) == [4, 3, 2, 1, 0] and s._lib.calls[-1]["stats"] is False
    for op in ("add", "subtract", "intersect"):
        s.select_clusters(1, op=op)
        assert s._lib.calls[-1]["op"] == pkg.Projector._SELECT_OPS[op]
    made = len(s._lib.calls)
    for radius in (0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="radius"):
            s.select_clusters(radius)
    for k in (0, -1, 2 ** 32):
        with pytest.raises(ValueError, match="min_points"):
            s.select_clusters(0.1, k)
    for lo, hi in ((2, 1), (50, 49), (1, -1), (1, 2 ** 32)):
        with pytest.raises(ValueError, match="max_points"):
            s.select_clusters(0.1, lo, hi)
    with pytest.raises(KeyError):
        s.select_clusters(0.1, op="xor")
    assert len(s._lib.calls) == made
    at = L.lib().rtr_select_clusters.argtypes
    assert at[1] is C.c_float and at[2] is C.c_uint32 and at[3] is C.c_uint32 and len(at) == 8
