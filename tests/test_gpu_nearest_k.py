"""The k nearest resident points to each given point on the GPU (include/rtr.h section 6m): rtr_nearest_k_points' three
arrays and its statistics compared exactly -- np.array_equal on the indices, on the uint32 view of the distances and on
found, no tolerance anywhere -- with the numpy float32 reference of tests/nearest_k_ref.py: in every form the cloud can
take, at the smallest shapes with every combination of requested outputs, against rtr_nearest_points and rtr_select_near
on the same context, on a lattice where eight candidates tie, on rows that every chunk's waves insert into at once, at
subnormal and zero distances, on section 6k's remaining ground (the threshold, special coordinates, the span's edge,
chunks that are never decoded), whatever the order and the memory of the given points, with everything else the context
holds left alone, and on the error paths."""
import ctypes as C
import itertools

import numpy as np
import pytest

import near_cases as nc
import near_ref as nr
import nearest_cases as ncs
import nearest_k_ref as kf
from test_gpu_near import _ragged
from test_gpu_nearest import FIXED_FORMS, _cloud
from test_gpu_neighbours import _edge_cloud
from test_gpu_select import FORMS, _new, _sel

pytestmark = pytest.mark.gpu

f32 = np.float32
NONE = kf.NONE


def _chunks(n):
    return (n + 255) // 256


def _check(p, n, G, r, k, ref, what):
    """the three arrays and the stats against ref = nearest_k_ref's four"""
    idx, d2, found, st = p.nearest_k_points(G, k, r)
    assert idx.dtype == np.uint32 and d2.dtype == f32 and found.dtype == np.uint32, what
    assert idx.shape == d2.shape == (len(G), k) and found.shape == (len(G),), what
    for name, got, want in zip(("index", "dist2", "found"), (idx, d2, found), ref[:3]):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (what, k, name, bad[:5], [got[tuple(b)] for b in bad[:5]], [want[tuple(b)] for b in bad[:5]])
    assert st == ref[3], (what, k, st, ref[3])
    assert p.get_option("nearest_k_chunks_skipped") + p.get_option("nearest_k_chunks_decoded") == _chunks(n), what


@pytest.fixture(scope="module")
def cases(orc):
    """scene -> (xyzw, rgba); case -> (given, {k: nearest_k_ref's four}): computed once, never changed."""
    clouds, ref = {}, {}
    for scene, n in nc.SCENES.items():
        clouds[scene] = orc.generate(scene, nc.SEED, 0, n, n)
        second = orc.generate(scene, nc.GIVEN_SEED, 0, n, n)[0]
        for case in nc.CASES:
            if case[0] == scene:
                G = np.ascontiguousarray(nc.given(case, second))
                pairs = kf.candidate_pairs(clouds[scene][0], G, case[2])
                want = {k: kf.rows_of_pairs(pairs, G.shape[0], k, G) for k in (1, 4, 64)}
                assert (G.shape[0], want[1][3][0]) == (case[3], case[5])  # (test_near_host.py pins these counts, and their spread)
                ref[case] = (G, want)
    return clouds, ref


@pytest.mark.parametrize("form", sorted(FORMS))
def test_all_three_arrays_and_stats_match_the_reference_in_every_form(pkg, cases, form):
    options, sort = FORMS[form]
    clouds, ref = cases
    for scene, n in nc.SCENES.items():
        xyzw, rgba = clouds[scene]
        opts = dict(options)
        if scene == "uniform_box" and form not in ("hash_unpacked",):
            opts["point_ids"] = 1  # (the library sorts a hash-ordered cloud)
        p = _new(pkg, opts, xyzw, rgba, sort=sort)
        try:
            if form == "sorted":
                assert p.get_option("reordered") == 1
            for case in nc.CASES:
                if case[0] != scene:
                    continue
                G, want = ref[case]
                for k in (1, 4, 64):
                    for rows in (G, np.ascontiguousarray(G[:, :3])):  # (float4 and tight rows)
                        _check(p, n, rows, case[2], k, want[k], (form, case, rows.shape))
                        assert p.get_option("nearest_k_given_us") > 0 and p.get_option("nearest_k_sweep_us") > 0
                        assert p.get_option("nearest_k_pair_tests_k") > 0 and p.get_option("nearest_k_chunks_decoded") > 0
                        assert p.get_option("nearest_k_cascades_k") >= 0  # (depends on timing: never compared with anything)
        finally:
            p.close()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4099])
def test_smallest_shapes_and_every_combination_of_outputs(pkg, orc, n):
    L = pkg._lib
    some = False
    for count in (0, 1, 63, 64, 65, 257):
        xyzw, rgba, r, G = _ragged(orc, n, count)  # (test_gpu_near: half of the given points beside a resident one)
        pairs = kf.candidate_pairs(xyzw, G, r)
        want = {k: kf.rows_of_pairs(pairs, count, k, G) for k in (1, 2, 17, 64)}
        if n * count <= 70_000:
            assert all(kf.same(kf.nearest_k_brute(xyzw, G, r, k)[:3], want[k][:3]) for k in (2, 17))
        assert count < 63 or n < 63 or 0 < want[1][3][0] < count
        assert n >= 64 or want[64][3][3] == 0, "k > n: no row can be full"
        some = some or want[1][3][0] > 0
        for name, options, sort in FIXED_FORMS:
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                for k in (1, 2, 17, 64):
                    _check(p, n, G, r, k, want[k], (n, count, name))
                # each combination of NULL outputs over the C ABI, stats only among them
                k = 17
                for asked in itertools.product((False, True), repeat=3):
                    out = [np.full((count, k), 7, np.uint32), np.full((count, k), 7, f32), np.full(count, 7, np.uint32)]
                    st = np.full(4, 7, np.uint64)
                    ptrs = [C.c_void_p(a.ctypes.data) if ask else None for a, ask in zip(out, asked)]
                    rc = p._lib.rtr_nearest_k_points(p._ctx, C.c_void_p(G.ctypes.data) if count else None, 12, count, r, k, 0, *ptrs,
                                                     C.c_void_p(st.ctypes.data))
                    assert rc == L.RTR_OK, (n, count, name, asked)
                    assert tuple(int(v) for v in st) == want[k][3], (n, count, name, asked)
                    for a, ask, w in zip(out, asked, want[k][:3]):  # (an output that was not asked for is not there to be written)
                        assert np.array_equal(a.view(np.uint32), w.view(np.uint32)) if ask else (a == 7).all(), (n, count, name, asked)
                got = p.nearest_k_points(G, 2, r, stats=False)
                assert len(got) == 3 and kf.same(got, want[2][:3])
            finally:
                p.close()
    assert some


def test_agreement_with_the_existing_calls_on_the_same_context(pkg, cases):
    clouds, ref = cases
    xyzw, rgba = clouds["room_shell"]
    for name, options, sort in FIXED_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for case in nc.CASES[:3]:
                G = ref[case][0]
                st6k, near = p.select_near(G, case[2], near=True, given_only=True)
                gi, gd, st6l = p.nearest_points(G, case[2])
                idx, d2, found, st = p.nearest_k_points(G, 1, case[2])
                assert np.array_equal(idx[:, 0], gi) and np.array_equal(d2[:, 0].view(np.uint32), gd.view(np.uint32)), (name, case)
                assert np.array_equal(found > 0, near) and (st[0], st[2]) == (st6k[2], st6k[3]) == (st6l[0], st6l[2]), (name, case)
                idx, d2, found, st = p.nearest_k_points(G, 4, case[2])
                assert np.array_equal(idx[:, 0], gi) and np.array_equal(found > 0, near) and st[0] == st6k[2], (name, case)
                assert p.get_option("selection") == 0, "no selection is created"
        finally:
            p.close()


@pytest.mark.parametrize("order", ncs.TIE_ORDERS)
def test_eight_way_ties_come_back_in_index_order(pkg, orc, order):
    A, G = ncs.tie_lattice(order)
    n = A.shape[0]
    pairs = kf.candidate_pairs(A, G, ncs.TIE_RADIUS)
    want = {k: kf.rows_of_pairs(pairs, G.shape[0], k, G) for k in (3, 8, 9)}
    # (pinned without a GPU in test_nearest_k_host.py: eight candidates at one d2 bit pattern per cell)
    assert (want[3][2][:288] == 3).all() and (want[9][2][:288] == 8).all() and (want[9][0][:288, 8] == NONE).all()
    assert (kf.bits(want[8][1])[:288] == kf.bits(f32(48 / 65536))[0]).all() and (np.diff(want[8][0][:288].astype(np.int64), axis=1) > 0).all()
    xyzw, rgba = _cloud(orc, A)
    for name, options, sort in FIXED_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            if sort:
                assert p.get_option("reordered") == 1
            for k in (3, 8, 9):
                _check(p, n, G, ncs.TIE_RADIUS, k, want[k], (order, name))
        finally:
            p.close()


def _contended():
    """4099 resident points, all within the radius of three given points, one of which coincides with a resident point; a
    third of the resident points are pairwise duplicates (d2 ties across chunks); shuffled upload order"""
    rng = np.random.default_rng(77)
    n = 4099
    A = rng.normal(0, 0.05, (n, 3)).clip(-0.2, 0.2).astype(f32)
    half = n // 6
    A[half:2 * half] = A[:half]  # (pairwise duplicates: 2 * half of the points, a third)
    A = A[rng.permutation(n)]
    G = f32([[0.01, 0, 0], A[1234], [-0.02, 0.03, 0.01]])
    r = f32(0.5)  # (every pair is within 0.35 + 0.04 of each other)
    return np.ascontiguousarray(A), np.ascontiguousarray(G), r


def test_rows_that_every_chunk_inserts_into_at_once(pkg, orc):
    A, G, r = _contended()
    n = A.shape[0]
    want = {k: kf.nearest_k_brute(A, G, r, k) for k in (1, 2, 16, 64)}
    d2 = kf._d2(A[:, None, :], G[None, :, :])
    assert (d2 <= kf.r2_of(r)).all(), "every resident point is a candidate of every given point: all 17 chunks insert into all three rows"
    assert (want[64][2] == 64).all() and kf.bits(want[2][1])[1, 0] == 0
    b = kf.bits(want[64][1])
    assert ((b[:, 1:] == b[:, :-1]).sum(axis=1) >= 5).all(), "ties within the rows"
    tie = b[:, 1:] == b[:, :-1]
    i64 = want[64][0].astype(np.int64)
    assert (np.abs(i64[:, 1:] - i64[:, :-1])[tie] >= 256).any(), "... across chunks"
    xyzw, rgba = _cloud(orc, A)
    p = _new(pkg, {"auto_reorder": 0, "pack": 0}, xyzw, rgba)  # (unsorted, unpacked: the chunks as uploaded)
    try:
        for k in (1, 2, 16, 64):
            first = None
            for again in range(3):
                _check(p, n, G, r, k, want[k], ("contended", again))
                assert p.get_option("nearest_k_chunks_decoded") == _chunks(n) == 17
                got = p.nearest_k_points(G, k, r, stats=False)
                first = first or got
                assert kf.same(got, first), "identical each time"
    finally:
        p.close()


def test_subnormal_and_zero_distances_are_kept_bit_for_bit(pkg, orc):
    tiny = f32(2.0 ** -70)
    A = np.zeros((300, 3), f32)
    A[:, 0] = np.arange(300) + 10  # (far from the origin: only points 7 and 299 are candidates)
    A[7] = (tiny, 0, 0)
    A[299] = (0, tiny, 0)
    G = f32([[0, 0, 0], [tiny, 0, 0], [0, 2 * tiny, 0]])
    want = kf.nearest_k_brute(A, G, 0.05, 3)
    sub = int(f32(2.0 ** -140).view(np.uint32))
    two = int(f32(2.0 ** -139).view(np.uint32))
    five = int((f32(2.0 ** -140) + f32(2.0 ** -138)).view(np.uint32))
    assert sub == 0x200 and want[0].tolist() == [[7, 299, NONE], [7, 299, NONE], [299, 7, NONE]]
    assert kf.bits(want[1])[:, :2].tolist() == [[sub, sub], [0, two], [sub, five]] and list(want[2]) == [2, 2, 2]
    xyzw, rgba = _cloud(orc, A)
    for name, options, sort in FIXED_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(p, 300, G, 0.05, 3, want, name)
        finally:
            p.close()


def test_the_threshold_is_exact(pkg, orc):
    xyz, r, want = _edge_cloud()  # (test_gpu_neighbours: 2160 isolated pairs at, and one ulp beyond, the radius)
    ends = (xyz[0::2], xyz[1::2])
    want = want[0::2]
    for a, g in ((0, 1), (1, 0)):  # (both ways round)
        A, G = ends[a], np.ascontiguousarray(ends[g])
        ref = kf.nearest_k_brute(A, G, r, 2)
        assert np.array_equal(ref[2], want.astype(np.uint32)) and np.array_equal(ref[0][want, 0], np.flatnonzero(want))  # (every pair alone)
        xyzw, rgba = _cloud(orc, A)
        for name, options, sort in FIXED_FORMS:
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                _check(p, A.shape[0], G, r, 2, ref, (name, a))
            finally:
                p.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_special_coordinates_on_either_side(pkg, orc, axis):
    n, m, k = 4099, 600, 2
    xyzw, rgba = orc.generate("room_shell", 300 + axis, 0, n, n)
    xyzw = xyzw.copy()
    rng = np.random.default_rng(axis)
    at = rng.choice(np.arange(300, 1500), 16, replace=False)
    big = np.finfo(f32).max
    xyzw[at[:9], axis] = np.tile(f32([np.nan, np.inf, -np.inf]), 3)  # (inside otherwise ordinary chunks: the per-point path)
    xyzw[at[9:13], axis] = f32([1e30, -1e30, big, -big])  # (finite and far beyond the span: legal on the resident side)
    G = (xyzw[rng.choice(np.arange(1500, n), m, replace=False), :3] + rng.normal(0, 0.05, (m, 3))).astype(f32)
    G[:9] = xyzw[at[:9], :3]  # coincident with the non-finite resident points: nobody's candidate all the same
    G[9:12, (axis + 1) % 3] = f32([np.nan, np.inf, -np.inf])
    G[12] = xyzw[at[14], :3]  # coincident with a finite resident point
    r = 0.15
    want = kf.nearest_k_brute(xyzw, G, r, k)
    assert (want[2][:12] == 0).all() and (want[0][:12] == NONE).all() and want[0][12, 0] == at[14] and kf.bits(want[1])[12, 0] == 0
    assert not np.isin(want[0], at[:13]).any() and want[3][2] == 12 and 0 < want[3][0] < m and 0 < want[3][3] < want[3][0]
    for name, options, sort in FIXED_FORMS + (("default", {}, False),):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(p, n, G, r, k, want, (axis, name))
            none = kf.nearest_k_brute(xyzw, G[:12], r, k)  # twelve given points that are all non-finite: nothing is found
            _check(p, n, G[:12], r, k, none, (axis, name, "all non-finite"))
            assert none[3] == (0, 0, 12, 0) and p.get_option("nearest_k_chunks_skipped") == _chunks(n)
        finally:
            p.close()
    # a finite GIVEN coordinate beyond the span fails the call with the outputs and stats as they were
    p = _new(pkg, {}, xyzw, rgba)
    try:
        for what, v in {"1e30": 1e30, "-FLT_MAX": -big, "beyond": 2.0 ** 20 * r * 1.0011}.items():
            moved = G.copy()
            moved[77, axis] = f32(v)
            out = [np.full((m, k), 7, np.uint32), np.full((m, k), 7, f32), np.full(m, 7, np.uint32), np.full(4, 7, np.uint64)]
            rc = p._lib.rtr_nearest_k_points(p._ctx, C.c_void_p(moved.ctypes.data), 12, m, r, k, 0, *[C.c_void_p(a.ctypes.data) for a in out])
            assert rc == pkg._lib.RTR_ERR_UNSUPPORTED and "span" in p._lib.rtr_last_error(p._ctx).decode(), what
            assert all((a == 7).all() for a in out), what
        edge = G.copy()  # a given coordinate within 2^20 radius of the origin is inside the span
        edge[77, axis], edge[78, axis] = f32(2.0 ** 20 * r), f32(-(2.0 ** 20) * r)
        _check(p, n, edge, r, k, kf.nearest_k_brute(xyzw, edge, r, k), (axis, "edge of the span"))
    finally:
        p.close()


def test_chunks_far_from_the_given_points_are_never_decoded(pkg, orc):
    n, k = 120_001, 2
    xyzw, rgba = orc.generate("room_shell", 7, 0, n, n)
    centre = xyzw[777, :3]
    G = np.ascontiguousarray(xyzw[np.linalg.norm(xyzw[:, :3] - centre, axis=1) < 0.4, :3] + f32(0.003))  # (the ball)
    two = np.concatenate([G, G[:50] - 2 * (centre - xyzw[:, :3].mean(axis=0))]).astype(f32)  # (a second spot: the box between is empty)
    r = 0.03
    want = kf.nearest_k_bucket(xyzw, two, r, k)
    hit, _ = nr.near_bucket(xyzw, two, r)  # (on the CPU: so few resident points lie near a given one that most chunks cannot)
    assert 0 < hit.sum() < n // 20 and want[3][0] > 0 and 0 < want[3][3] < want[3][0]
    for name, options, sort in (("sorted", {"point_ids": 1}, True), ("sorted_unpacked", {"point_ids": 1, "pack": 0}, True)):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(p, n, two, r, k, want, name)
            skipped, decoded = p.get_option("nearest_k_chunks_skipped"), p.get_option("nearest_k_chunks_decoded")
            assert decoded >= 1 and skipped > 0.5 * _chunks(n), (name, skipped, decoded)
        finally:
            p.close()


def test_the_order_and_the_memory_of_the_given_points_do_not_matter(pkg, orc):
    import torch
    L = pkg._lib
    n, m, k = 40_001, 3001, 6
    xyzw, rgba = orc.generate("room_shell", 7, 0, n, n)
    G = np.ascontiguousarray(orc.generate("room_shell", 8, 0, n, n)[0][:m])
    G[100:200] = G[:100]  # (copies: two rows that every accepted pair of theirs goes into side by side)
    r = 0.06
    want = kf.nearest_k_bucket(xyzw, G, r, k)
    assert 0.05 * m < want[3][0] < 0.95 * m and 0 < want[3][3] < want[3][0]
    perm = np.random.default_rng(1).permutation(m)
    wp = kf.nearest_k_bucket(xyzw, G[perm], r, k)
    assert kf.same(wp[:3], (want[0][perm], want[1][perm], want[2][perm])) and wp[3] == want[3]
    for name, options, sort in FIXED_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(p, n, G, r, k, want, name)
            _check(p, n, G[perm], r, k, wp, (name, "permuted"))  # (the rows permute with the given points)
            # device memory: the given points as a torch tensor, float4 rows and tight ones; device input gives device output
            for rows in (torch.from_numpy(G).cuda(), torch.from_numpy(np.ascontiguousarray(G[:, :3])).cuda()):
                got = p.nearest_k_points(rows, k, r)
                assert all(t.is_cuda for t in got[:3]) and got[0].dtype == torch.uint32 and got[1].dtype == torch.float32
                assert got[0].shape == got[1].shape == (m, k) and got[2].shape == (m,)
                assert kf.same([t.cpu().numpy() for t in got[:3]], want[:3]) and got[3] == want[3], (name, "device")
            # all three outputs into device memory over the C ABI: the element behind each is untouched
            dev = [torch.full((w + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for w in (m * k, m * k, m)]
            st = np.zeros(4, np.uint64)
            assert p._lib.rtr_nearest_k_points(p._ctx, C.c_void_p(rows.data_ptr()), 12, m, r, k, 0, *[C.c_void_p(t.data_ptr()) for t in dev],
                                               st.ctypes.data_as(C.c_void_p)) == L.RTR_OK
            host = [t.cpu().numpy().view(np.uint32) for t in dev]
            assert kf.same([h[:-1] for h in host], [w.reshape(-1) for w in want[:3]]) and all(h[-1] == 0x5A5A5A5A for h in host), name
            assert tuple(int(v) for v in st) == want[3]
        finally:
            p.close()


def test_the_call_moves_nothing_else(pkg, orc):
    L = pkg._lib
    n, W, H, k = 60_001, 320, 240, 5
    xyzw, rgba = orc.generate("room_shell", 88, 0, n, n)
    G = np.ascontiguousarray(orc.generate("room_shell", 89, 0, n, n)[0][:5003])
    P, P2 = pkg.orbit_projection(40, W, H), pkg.orbit_projection(41, W, H)
    keep = np.arange(n) % 3 != 0
    planes = f32([[0, 0, 1, 100], [1, 0, 0, 50]])
    p = _new(pkg, {}, xyzw, rgba, W, H)
    try:
        def state():
            return [p.download(b).copy() for b in (L.BUF_DEPTH, L.BUF_IMAGE, L.BUF_TENSOR, L.BUF_VISIBLE, L.BUF_POINT_ID, L.BUF_POINT_KEEP,
                                                   L.BUF_SELECTION)] + \
                   [p.clip_planes(), p.frame_stats(), p.get_option("p2p_open"), p.get_option("packed"), p.get_option("reordered"),
                    p.get_option("point_keep"), p.get_option("selection"), p.num_points, p.get_option("resident_millibytes_per_point")]

        def same(a, b):
            return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

        p.set_clip_planes(planes)
        p.set_point_keep(keep)
        p.p2p_open(0, 1, [p.p2p_export()])  # (the one-rank form of test_gpu_p2p.py: a rank maps its own buffers)
        p.p2p_render(P, True)
        p.point_pass(P)
        p.select_points(planes=f32([[0, 1, 0, 0]]), stats=False)
        assert 0 < _sel(pkg, p, n).sum() < n
        before = state()
        for r in (0.05, 0.09):
            want = kf.nearest_k_bucket(xyzw, G, r, k)  # (every resident point counts: hidden, clipped and unselected ones too)
            assert 0 < want[3][0] and 0 < want[3][3] < want[3][0]
            _check(p, n, G, r, k, want, r)
        assert same(before, state()) and p.get_option("p2p_open") == 1
        p.p2p_close()
        p.set_clip_planes(None)
        p.set_point_keep(None)
        # a context without a selection gets none
        p.clear_selection()
        p.nearest_k_points(G, k, 0.05)
        assert p.get_option("selection") == 0 and p.selection() is None
        # issued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.nearest_k_points(G, k, 0.05)
        p.wait_outputs(0)
        o = orc.project(xyzw, rgba, P2, W, H)
        assert np.array_equal(depth.view(np.uint32), o["depth_bits"]) and np.array_equal(img, o["img"])
    finally:
        p.close()


def test_errors_leave_everything_intact(pkg, orc):
    L = pkg._lib
    n, m, k = 20_001, 1001, 4
    xyzw, rgba = orc.generate("room_shell", 4, 0, n, n)
    G = np.ascontiguousarray(orc.generate("room_shell", 3, 0, n, n)[0][:m, :3])
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    fresh = pkg.Projector(0)
    try:
        with pytest.raises(pkg.RtrError) as e:
            fresh.nearest_k_points(G, k, 0.25)
        assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        lib, ctx = p._lib, p._ctx
        den = np.array([1], np.uint32).view(f32)[0]
        out = [np.full((m, 64), 7, np.uint32), np.full((m, 64), 7, f32), np.full(m, 7, np.uint32), np.full(4, 7, np.uint64)]

        def call(xyz, stride, count, radius, kk, flags):
            return lib.rtr_nearest_k_points(ctx, vp(xyz), stride, count, radius, kk, flags, *[vp(a) for a in out])

        # (xyz, stride, count, radius, k, flags, what the message names)
        bad = [(G, 12, m, v, k, 0, "radius") for v in (0.0, -0.0, -0.25, np.nan, np.inf, -np.inf)]
        bad += [(G, 12, m, v, k, 0, "square of radius") for v in (float(den), 1e-20, 1e-30, 2e19, 3e38)]
        bad += [(None, 12, m, 0.1, k, 0, "xyz is NULL")]
        bad += [(G, s, m, 0.1, k, 0, "xyz_stride_bytes") for s in (0, 4, 8, 11, 13, 14, 18)]
        bad += [(G, 12, m, 0.1, kk, 0, "k outside") for kk in (0, 65, 66, 1000, 2 ** 32 - 1)]
        bad += [(G, 12, m, 0.1, k, f, "flags") for f in (1, 2, 3, -1, 1 << 16)]
        for case in bad:
            assert call(*case[:6]) == L.RTR_ERR_INVALID, case[1:6]
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_nearest_k_points" in text and case[6] in text, (case[1:6], text)
            assert all((a == 7).all() for a in out), case[1:6]
        assert call(G, 12, 2 ** 32, 0.1, k, 0) == L.RTR_ERR_UNSUPPORTED and all((a == 7).all() for a in out)  # 2^32 given points or more
        assert p.get_option("selection") == 0
        # count == 0: xyz may be NULL, nothing is found, no output has an entry to write
        assert call(None, 12, 0, 0.1, k, 0) == L.RTR_OK
        assert tuple(out[3]) == (0, 0, 0, 0) and all((a == 7).all() for a in out[:3])
        assert p.get_option("nearest_k_chunks_skipped") == _chunks(n)
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        out[3][...] = 7
        assert call(G, 12, m, 0.1, k, 0) == L.RTR_ERR_INVALID and "point_ids" in lib.rtr_last_error(ctx).decode()
        assert all((a == 7).all() for a in out)
        with pytest.raises(pkg.RtrError) as e:
            p.nearest_k_points(G, k, 0.1)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
    finally:
        p.close()
