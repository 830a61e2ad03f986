"""The rules the selecting calls share (include/rtr.h sections 6f - 6k; csrc/rtr_select_api.hip), pinned ACROSS the calls
where the per-call files pin them one call at a time: a selection that does not exist yet counts as empty for every call
and every op, a span failure on a context without a selection makes none and touches no caller array, and every
caller-owned array may be left out or live in host or device memory.  Two clouds -- n = 257 (two chunks, the second
ragged) and n = 20 001 -- each in upload order (auto_reorder = 0) and sorted by the library with point_ids = 1; the hit
sets come from the brute-force references of the per-call files, combined with the op in numpy."""
import ctypes as C

import numpy as np
import pytest

import clusters_ref as cr
import near_ref as nr
import neighbours_ref as nbr
import select_ref as sr
import voxel_ref as vr
from test_gpu_select import OPS, _new, _sel

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = {257: 1.0, 20_001: 0.15}  # n -> the radius of its neighbour, cluster and near calls
FORMS = {"upload_order": ({"auto_reorder": 0}, False), "sorted": ({"point_ids": 1}, True)}
PLANES = f32([[1, 0, 0, 0]])
NOTHING = f32([[0, 0, 1, -100]])  # (no point of the room is inside)
K, WINDOW = 4, (5, 1000)  # min_neighbours; min_points, max_points
CALLS = ("points", "voxel", "neighbours", "clusters", "near")
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def clouds(pkg, orc):
    """n -> the cloud, the given points and the five hit sets (before OUTSIDE): computed once, never changed."""
    out = {}
    for n, r in SIZES.items():
        xyzw, rgba = orc.generate("room_shell", 0x5E1EC7, 0, n, n)
        G = np.ascontiguousarray(orc.generate("room_shell", 0x5E1EC8, 0, n, n)[0][:max(n // 8, 40), :3])
        lab = cr.labels(xyzw, r)
        near_hit, near_bits = nr.near_brute(xyzw, G, r / 2)
        hits = {"points": np.asarray(pkg.clip_keep(PLANES, xyzw), bool), "voxel": vr.select(xyzw, 4 * r)[0],
                "neighbours": nbr.select(xyzw, r, K)[0], "clusters": cr.hits(lab, *WINDOW), "near": near_hit}
        for name, hit in hits.items():
            assert 0 < hit.sum() < n, (n, name)
        assert 0 < near_bits.sum() < G.shape[0]
        out[n] = dict(xyzw=xyzw, rgba=rgba, r=r, G=G, hits=hits, labels=lab, near_bits=near_bits)
    return out


def _call(p, c, name, **kw):
    r = c["r"]
    if name == "points":
        return p.select_points(planes=PLANES, **kw)
    if name == "voxel":
        return p.select_voxel_grid(4 * r, **kw)
    if name == "neighbours":
        return p.select_neighbours(r, K, **kw)
    if name == "clusters":
        return p.select_clusters(r, *WINDOW, **kw)
    return p.select_near(c["G"], r / 2, **kw)


CASES = [(n, form) for n in SIZES for form in FORMS]


@pytest.mark.parametrize("n,form", CASES)
def test_a_selection_that_does_not_exist_counts_as_empty_for_every_call_and_op(pkg, clouds, n, form):
    c = clouds[n]
    options, sort = FORMS[form]
    p = _new(pkg, options, c["xyzw"], c["rgba"], sort=sort)
    try:
        assert p.get_option("reordered") == int(sort)
        for name in CALLS:
            for op in OPS:
                for outside in (False, True):
                    what = (n, form, name, op, outside)
                    want = sr.combine(op, np.zeros(n, bool), c["hits"][name] != outside)
                    p.clear_selection()
                    assert p.get_option("selection") == 0
                    st_none = _call(p, c, name, op=op, outside=outside)
                    assert p.get_option("selection") == 1, what
                    words_none = p.download(pkg._lib.BUF_SELECTION).copy()
                    assert p.select_points(planes=NOTHING)[0] == 0 and not _sel(pkg, p, n).any()
                    st_empty = _call(p, c, name, op=op, outside=outside)
                    words_empty = p.download(pkg._lib.BUF_SELECTION)
                    assert np.array_equal(words_none, words_empty) and st_none == st_empty, what
                    assert np.array_equal(words_none, sr.words(want)) and st_none[0] == int(want.sum()), what
    finally:
        p.close()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n,form", CASES)
def test_a_span_failure_without_a_selection_makes_none_and_writes_no_caller_array(pkg, clouds, n, form):
    L = pkg._lib
    c = clouds[n]
    r = c["r"]
    options, sort = FORMS[form]
    far = f32(2.0 ** 20 * r * 1.0011)  # (finite, beyond the span of the neighbour grid: test_gpu_neighbours.py)
    moved = c["xyzw"].copy()
    moved[n // 2, 1] = far
    G = c["G"].copy()
    G[7, 2] = -f32(2.0 ** 20 * (r / 2) * 1.0011)
    m = G.shape[0]
    p = _new(pkg, options, moved, c["rgba"], sort=sort)
    try:
        lib, ctx = p._lib, p._ctx
        st = np.full(4, SENTINEL, np.uint64)
        labels = np.full(n, SENTINEL, np.uint32)
        words = np.full((m + 31) // 32, SENTINEL, np.uint32)
        for op in (L.SELECT_REPLACE, L.SELECT_ADD, L.SELECT_TOGGLE | L.SELECT_OUTSIDE):
            calls = {"neighbours": lambda: lib.rtr_select_neighbours(ctx, r, K, op, _vp(st)),
                     "clusters": lambda: lib.rtr_select_clusters(ctx, r, WINDOW[0], WINDOW[1], 0, op, _vp(labels), _vp(st)),
                     "near": lambda: lib.rtr_select_near(ctx, _vp(G), 12, m, r / 2, 0, op, _vp(words), _vp(st))}
            for name, call in calls.items():
                assert p.get_option("selection") == 0
                assert call() == L.RTR_ERR_UNSUPPORTED, (name, op)
                text = lib.rtr_last_error(ctx).decode()
                assert "rtr_select_" + name in text and "span" in text, text
                assert p.get_option("selection") == 0 and p.selection() is None, (name, op)
                assert (st == SENTINEL).all() and (labels == SENTINEL).all() and (words == SENTINEL).all(), (name, op)
    finally:
        p.close()


@pytest.mark.parametrize("n,form", CASES)
def test_every_caller_array_may_be_left_out_or_lie_in_host_or_device_memory(pkg, clouds, n, form):
    import torch
    L = pkg._lib
    c = clouds[n]
    r, G, hits = c["r"], c["G"], c["hits"]
    m = G.shape[0]
    options, sort = FORMS[form]
    p = _new(pkg, options, c["xyzw"], c["rgba"], sort=sort)
    try:
        lib, ctx = p._lib, p._ctx
        # stats = NULL: the same words as with them (the first test has pinned those to the references)
        for name in CALLS:
            p.clear_selection()
            assert _call(p, c, name, op="add", stats=False) is None
            assert np.array_equal(_sel(pkg, p, n), hits[name]), name
        band = f32([[1, 0, 0, 0.5, 0.5]])
        counts, _ = p.count_in_bands(band)
        assert np.array_equal(p.count_in_bands(band, stats=False), counts) and 0 < counts[0] < n
        plane, inliers, _ = p.fit_plane(0.05, iterations=16, seed=3)
        got = np.zeros(4, f32)
        assert lib.rtr_fit_plane(ctx, 0.05, 16, 3, 0, _vp(got), None) == L.RTR_OK
        assert np.array_equal(got.view(np.uint32), plane.view(np.uint32)) and inliers > 0
        # the labels and the near words: host memory and device memory hold the same, and nothing beside them is written
        st_host, st_dev = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        lab_host = np.full(n + 1, SENTINEL, np.uint32)
        lab_dev = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda:0")
        assert lib.rtr_select_clusters(ctx, r, WINDOW[0], WINDOW[1], 0, 0, _vp(lab_host), _vp(st_host)) == L.RTR_OK
        sel_host = p.download(L.BUF_SELECTION).copy()
        assert lib.rtr_select_clusters(ctx, r, WINDOW[0], WINDOW[1], 0, 0, C.c_void_p(lab_dev.data_ptr()), _vp(st_dev)) == L.RTR_OK
        assert np.array_equal(lab_dev.cpu().numpy().view(np.uint32), lab_host) and np.array_equal(st_host, st_dev)
        assert np.array_equal(lab_host[:n], c["labels"]) and lab_host[n] == SENTINEL
        assert np.array_equal(p.download(L.BUF_SELECTION), sel_host) and np.array_equal(sel_host, sr.words(hits["clusters"]))
        gw = (m + 31) // 32
        near_host = np.full(gw + 1, SENTINEL, np.uint32)
        near_dev = torch.full((gw + 1,), SENTINEL, dtype=torch.int32, device="cuda:0")
        assert lib.rtr_select_near(ctx, _vp(G), 12, m, r / 2, 0, 0, _vp(near_host), _vp(st_host)) == L.RTR_OK
        sel_host = p.download(L.BUF_SELECTION).copy()
        assert lib.rtr_select_near(ctx, _vp(G), 12, m, r / 2, 0, 0, C.c_void_p(near_dev.data_ptr()), _vp(st_dev)) == L.RTR_OK
        assert np.array_equal(near_dev.cpu().numpy().view(np.uint32), near_host) and np.array_equal(st_host, st_dev)
        assert np.array_equal(near_host[:gw], nr.words(c["near_bits"])) and near_host[gw] == SENTINEL
        assert np.array_equal(p.download(L.BUF_SELECTION), sel_host) and np.array_equal(sel_host, sr.words(hits["near"]))
        assert tuple(int(v) for v in st_host) == nr.stats(hits["near"], c["near_bits"], G, hits["near"])
    finally:
        p.close()
