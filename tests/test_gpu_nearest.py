"""The nearest resident point to each given point on the GPU (include/rtr.h section 6l): rtr_nearest_points' four arrays
and its statistics compared exactly -- np.array_equal on the indices and on the uint32 view of the distances, no
tolerance anywhere -- with the numpy float32 reference of tests/nearest_ref.py: in every form the cloud can take, at the
smallest shapes on both sides with every combination of requested outputs, against rtr_select_near on the same context,
on a lattice where every answer is an eight-way tie, at subnormal and zero distances, on section 6k's remaining ground
(the threshold, special coordinates, the span's edge, chunks that are never decoded), whatever the order and the memory
of the given points, with everything else the context holds left alone, and on the error paths."""
import ctypes as C

import numpy as np
import pytest

import near_cases as nc
import nearest_cases as ncs
import nearest_ref as nf
from test_gpu_near import _ragged
from test_gpu_neighbours import _edge_cloud
from test_gpu_select import FORMS, _new, _sel
from test_near_host import span_edge_pairs

pytestmark = pytest.mark.gpu

f32 = np.float32
NONE = nf.NONE
# the forms whose resident order the test decides: packed and not as uploaded, and sorted by the library
FIXED_FORMS = (("packed", {"auto_reorder": 0, "pack": 2}, False), ("pack0", {"auto_reorder": 0, "pack": 0}, False),
               ("sorted", {"point_ids": 1}, True))


def _chunks(n):
    return (n + 255) // 256


def _check(p, n, G, r, ref, what):
    """both sides and the stats against ref = nearest_ref's five"""
    gi, gd, ri, rd, st = p.nearest_points(G, r, given=True, resident=True)
    assert gi.dtype == np.uint32 and gd.dtype == f32 and ri.dtype == np.uint32 and rd.dtype == f32, what
    assert gi.shape == gd.shape == (len(G),) and ri.shape == rd.shape == (n,), what
    for name, got, want in zip(("given_index", "given_dist2", "resident_index", "resident_dist2"), (gi, gd, ri, rd), ref[:4]):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (what, name, bad[:5], got[bad[:5]], want[bad[:5]])
    assert st == ref[4], (what, st, ref[4])
    assert p.get_option("nearest_chunks_skipped") + p.get_option("nearest_chunks_decoded") == _chunks(n), what


def _cloud(orc, A, seed=9):
    n = A.shape[0]
    xyzw, rgba = orc.generate("room_shell", seed, 0, n, n)
    xyzw = xyzw.copy()
    xyzw[:, :3] = A
    return xyzw, rgba


@pytest.fixture(scope="module")
def cases(orc):
    """scene -> (xyzw, rgba); case -> (given, nearest_ref's five): computed once, never changed."""
    clouds, ref = {}, {}
    for scene, n in nc.SCENES.items():
        clouds[scene] = orc.generate(scene, nc.SEED, 0, n, n)
        second = orc.generate(scene, nc.GIVEN_SEED, 0, n, n)[0]
        for case in nc.CASES:
            if case[0] == scene:
                G = np.ascontiguousarray(nc.given(case, second))
                want = nf.nearest_bucket(clouds[scene][0], G, case[2])
                assert (G.shape[0], want[4][1], want[4][0]) == case[3:]  # (test_near_host.py pins these counts, and their spread)
                ref[case] = (G, want)
    return clouds, ref


@pytest.mark.parametrize("form", sorted(FORMS))
def test_all_four_arrays_and_stats_match_the_reference_in_every_form(pkg, cases, form):
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
                for rows in (G, np.ascontiguousarray(G[:, :3])):  # (float4 and tight rows)
                    _check(p, n, rows, case[2], want, (form, case, rows.shape))
                    assert p.get_option("nearest_given_us") > 0 and p.get_option("nearest_sweep_us") > 0
                    assert p.get_option("nearest_pair_tests_k") > 0 and p.get_option("nearest_chunks_decoded") > 0
        finally:
            p.close()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4099])
def test_smallest_shapes_and_every_combination_of_outputs(pkg, orc, n):
    some = False
    for count in (0, 1, 63, 64, 65, 257):
        xyzw, rgba, r, G = _ragged(orc, n, count)  # (test_gpu_near: half of the given points beside a resident one)
        want = nf.nearest_brute(xyzw, G, r)
        assert count < 63 or n < 63 or (0 < want[4][0] < count and 0 < want[4][1] < n)
        some = some or want[4][0] > 0
        for name, options, sort in FIXED_FORMS:
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                what = (n, count, name)
                _check(p, n, G, r, want, what)
                gi, gd, st = p.nearest_points(G, r)  # (the given side alone: the sweep without its resident half)
                assert nf.same((gi, gd), want[:2]) and st == want[4], what
                ri, rd, st = p.nearest_points(G, r, given=False, resident=True)
                assert nf.same((ri, rd), want[2:4]) and st == want[4], what
                assert p.nearest_points(G, r, given=False) == want[4], what  # (stats only: both sides are computed)
                assert p.nearest_points(G, r, given=False, stats=False) is None
                gi, gd = p.nearest_points(G, r, stats=False)
                assert nf.same((gi, gd), want[:2]), what
            finally:
                p.close()
    assert some


def test_agreement_with_select_near_on_the_same_context(pkg, cases):
    clouds, ref = cases
    scene = "room_shell"
    xyzw, rgba = clouds[scene]
    n = xyzw.shape[0]
    for name, options, sort in FIXED_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            for case in nc.CASES[:3]:
                G = ref[case][0]
                st6k, near = p.select_near(G, case[2], near=True)
                hit = _sel(pkg, p, n)
                gi, gd, ri, rd, st = p.nearest_points(G, case[2], resident=True)
                assert np.array_equal(gi != NONE, near) and np.array_equal(ri != NONE, hit), (name, case)
                assert np.array_equal(np.isinf(gd), ~near) and np.array_equal(np.isinf(rd), ~hit), (name, case)
                assert (st[0], st[1], st[2]) == (st6k[2], st6k[1], st6k[3]), (name, case)
                assert np.array_equal(_sel(pkg, p, n), hit), "the selection is not touched"
        finally:
            p.close()


@pytest.mark.parametrize("order", ncs.TIE_ORDERS)
def test_ties_go_to_the_smallest_index(pkg, orc, order):
    A, G = ncs.tie_lattice(order)
    n = A.shape[0]
    want = nf.nearest_brute(A, G, ncs.TIE_RADIUS)
    tg, tr = ncs.tie_counts(A, G)
    assert (tg >= 2).all() and (tg == 8).sum() == 288 and (tr == 3).sum() == 2  # (pinned without a GPU in test_nearest_host.py)
    assert want[4] == (G.shape[0], n, 0, 0)
    assert nf.bits(want[1])[288] == 0 and (nf.bits(want[1])[:288] == nf.bits(f32(48 / 65536))).all()
    xyzw, rgba = _cloud(orc, A)
    for name, options, sort in FIXED_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            if sort:
                assert p.get_option("reordered") == 1
            _check(p, n, G, ncs.TIE_RADIUS, want, (order, name))
            gi, gd = p.nearest_points(G, ncs.TIE_RADIUS, stats=False)  # (the kernel without its resident half)
            assert nf.same((gi, gd), want[:2]), (order, name)
        finally:
            p.close()


def test_subnormal_and_zero_distances_are_kept_bit_for_bit(pkg, orc):
    tiny = f32(2.0 ** -70)
    A = np.zeros((300, 3), f32)
    A[:, 0] = np.arange(300) + 10  # (far from the origin: only points 7 and 299 are candidates)
    A[7] = (tiny, 0, 0)
    A[299] = (0, tiny, 0)
    G = f32([[0, 0, 0], [tiny, 0, 0], [0, 2 * tiny, 0]])
    want = nf.nearest_brute(A, G, 0.05)
    sub = int(f32(2.0 ** -140).view(np.uint32))
    assert sub == 0x200 and list(want[0]) == [7, 7, 299] and list(nf.bits(want[1])) == [sub, 0, sub]
    assert list(want[2][[7, 299]]) == [1, 0] and list(nf.bits(want[3])[[7, 299]]) == [0, sub]
    xyzw, rgba = _cloud(orc, A)
    for name, options, sort in FIXED_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(p, 300, G, 0.05, want, name)
        finally:
            p.close()


def test_the_threshold_is_exact_on_both_sides(pkg, orc):
    xyz, r, want = _edge_cloud()  # (test_gpu_neighbours: 2160 isolated pairs at, and one ulp beyond, the radius)
    ends = (xyz[0::2], xyz[1::2])
    want = want[0::2]
    for a, g in ((0, 1), (1, 0)):  # (both ways round)
        A, G = ends[a], np.ascontiguousarray(ends[g])
        ref = nf.nearest_brute(A, G, r)
        assert np.array_equal(ref[0] != NONE, want) and np.array_equal(ref[2] != NONE, want)
        assert np.array_equal(ref[0][want], np.flatnonzero(want))  # (every pair alone)
        xyzw, rgba = _cloud(orc, A)
        for name, options, sort in FIXED_FORMS:
            p = _new(pkg, options, xyzw, rgba, sort=sort)
            try:
                _check(p, A.shape[0], G, r, ref, (name, a))
            finally:
                p.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_special_coordinates_on_either_side(pkg, orc, axis):
    n, m = 4099, 600
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
    want = nf.nearest_brute(xyzw, G, r)
    assert (want[0][:12] == NONE).all() and np.isinf(want[1][:12]).all() and want[0][12] == at[14] and nf.bits(want[1])[12] == 0
    assert (want[2][at[:13]] == NONE).all() and want[4][2] == 12 and 0 < want[4][0] < m and 0 < want[4][1] < n
    for name, options, sort in FIXED_FORMS + (("default", {}, False),):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(p, n, G, r, want, (axis, name))
            none = nf.nearest_brute(xyzw, G[:12], r)  # given points that are all non-finite: nothing has a nearest
            _check(p, n, G[:12], r, none, (axis, name, "all non-finite"))
            assert none[4] == (0, 0, 12, 0) and p.get_option("nearest_chunks_skipped") == _chunks(n)
        finally:
            p.close()
    # a finite GIVEN coordinate beyond the span fails the call with the outputs and stats as they were
    p = _new(pkg, {}, xyzw, rgba)
    try:
        for what, v in {"1e30": 1e30, "-FLT_MAX": -big, "beyond": 2.0 ** 20 * r * 1.0011}.items():
            moved = G.copy()
            moved[77, axis] = f32(v)
            out = [np.full(m, 7, np.uint32), np.full(m, 7, f32), np.full(n, 7, np.uint32), np.full(n, 7, f32), np.full(4, 7, np.uint64)]
            rc = p._lib.rtr_nearest_points(p._ctx, C.c_void_p(moved.ctypes.data), 12, m, r, 0, *[C.c_void_p(a.ctypes.data) for a in out])
            assert rc == pkg._lib.RTR_ERR_UNSUPPORTED and "span" in p._lib.rtr_last_error(p._ctx).decode(), what
            assert all((a == 7).all() for a in out), what
        edge = G.copy()  # a given coordinate within 2^20 radius of the origin is inside the span
        edge[77, axis], edge[78, axis] = f32(2.0 ** 20 * r), f32(-(2.0 ** 20) * r)
        _check(p, n, edge, r, nf.nearest_brute(xyzw, edge, r), (axis, "edge of the span"))
    finally:
        p.close()


@pytest.mark.parametrize("radius", [0.05, 1.0, 0.37])
def test_resident_points_across_the_edge_of_the_span(pkg, orc, radius):
    A, G, (qa, qg) = span_edge_pairs(radius)  # (test_near_host.py)
    n = A.shape[0]
    G = np.ascontiguousarray(G)
    want = nf.nearest_brute(A, G, radius)
    beyond = ((qa < -(2 ** 20 - 1)) | (qa > 2 ** 20 - 2)).any(axis=1)
    hit = want[2] != NONE
    assert (hit & beyond).any() and (~hit & beyond).any()
    xyzw, rgba = _cloud(orc, A, 5)
    for name, options, sort in FIXED_FORMS + (("default", {}, False),):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(p, n, G, radius, want, (name, radius))
        finally:
            p.close()
    # one resident point per chunk beyond the span, the chunks' boxes reaching across its edge: a larger cloud around them
    m = 4099
    more, rgba = orc.generate("room_shell", 6, 0, m, m)
    more = more.copy()
    more[::41][:n, :3] = A
    w2 = nf.nearest_brute(more, G, radius)
    for name, options, sort in FIXED_FORMS:
        p = _new(pkg, options, more, rgba, sort=sort)
        try:
            _check(p, m, G, radius, w2, (name, radius, "mixed"))
        finally:
            p.close()


def test_chunks_far_from_the_given_points_are_never_decoded(pkg, orc):
    n = 120_001
    xyzw, rgba = orc.generate("room_shell", 7, 0, n, n)
    centre = xyzw[777, :3]
    G = np.ascontiguousarray(xyzw[np.linalg.norm(xyzw[:, :3] - centre, axis=1) < 0.4, :3] + f32(0.003))
    two = np.concatenate([G, G[:50] - 2 * (centre - xyzw[:, :3].mean(axis=0))]).astype(f32)  # (a second spot: the box between is empty)
    r = 0.03
    want = nf.nearest_bucket(xyzw, two, r)
    assert 0 < want[4][1] < n // 20 and want[4][0] > 0
    for name, options, sort in (("sorted", {"point_ids": 1}, True), ("sorted_unpacked", {"point_ids": 1, "pack": 0}, True)):
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(p, n, two, r, want, name)
            skipped, decoded = p.get_option("nearest_chunks_skipped"), p.get_option("nearest_chunks_decoded")
            assert decoded >= 1 and skipped > 0.5 * _chunks(n), (name, skipped, decoded)
        finally:
            p.close()


def test_the_order_and_the_memory_of_the_given_points_do_not_matter(pkg, orc):
    import torch
    L = pkg._lib
    n, m = 40_001, 3001
    xyzw, rgba = orc.generate("room_shell", 7, 0, n, n)
    G = np.ascontiguousarray(orc.generate("room_shell", 8, 0, n, n)[0][:m])
    G[100:200] = G[:100]  # (copies: the resident side's ties)
    r = 0.06
    want = nf.nearest_bucket(xyzw, G, r)
    assert 0.05 * n < want[4][1] < 0.95 * n and 0.05 * m < want[4][0] < 0.95 * m
    perm = np.random.default_rng(1).permutation(m)
    wp = nf.nearest_bucket(xyzw, G[perm], r)
    assert nf.same((wp[0], wp[1]), (want[0][perm], want[1][perm])) and np.array_equal(nf.bits(wp[3]), nf.bits(want[3]))
    for name, options, sort in FIXED_FORMS:
        p = _new(pkg, options, xyzw, rgba, sort=sort)
        try:
            _check(p, n, G, r, want, name)
            _check(p, n, G[perm], r, wp, (name, "permuted"))  # (the given outputs permute, the resident indices map through it)
            # device memory: the given points as a torch tensor, float4 rows and tight ones; device input gives device output
            for rows in (torch.from_numpy(G).cuda(), torch.from_numpy(np.ascontiguousarray(G[:, :3])).cuda()):
                got = p.nearest_points(rows, r, resident=True)
                assert all(t.is_cuda for t in got[:4]) and got[0].dtype == torch.uint32 and got[1].dtype == torch.float32
                assert nf.same([t.cpu().numpy() for t in got[:4]], want[:4]) and got[4] == want[4], (name, "device")
            # all four outputs into device memory over the C ABI: the element behind each is untouched
            dev = [torch.full((k + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for k in (m, m, n, n)]
            st = np.zeros(4, np.uint64)
            assert p._lib.rtr_nearest_points(p._ctx, C.c_void_p(rows.data_ptr()), 12, m, r, 0, *[C.c_void_p(t.data_ptr()) for t in dev],
                                             st.ctypes.data_as(C.c_void_p)) == L.RTR_OK
            host = [t.cpu().numpy().view(np.uint32) for t in dev]
            assert nf.same([h[:-1] for h in host], want[:4]) and all(h[-1] == 0x5A5A5A5A for h in host), name
            assert tuple(int(v) for v in st) == want[4]
        finally:
            p.close()


def test_the_call_moves_nothing_else(pkg, orc):
    L = pkg._lib
    n, W, H = 60_001, 320, 240
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
            want = nf.nearest_bucket(xyzw, G, r)  # (every resident point counts: hidden, clipped and unselected ones too)
            assert 0 < want[4][1] < n
            _check(p, n, G, r, want, r)
        assert same(before, state()) and p.get_option("p2p_open") == 1
        p.p2p_close()
        p.set_clip_planes(None)
        p.set_point_keep(None)
        # a context without a selection gets none
        p.clear_selection()
        p.nearest_points(G, 0.05)
        assert p.get_option("selection") == 0 and p.selection() is None
        # issued between rtr_project_async and rtr_wait: the slot's frame is exact
        img, depth = p.host_output_buffers(0)
        p.project_async(P2, 0, filtered=False)
        p.nearest_points(G, 0.05)
        p.wait_outputs(0)
        o = orc.project(xyzw, rgba, P2, W, H)
        assert np.array_equal(depth.view(np.uint32), o["depth_bits"]) and np.array_equal(img, o["img"])
    finally:
        p.close()


def test_errors_leave_everything_intact(pkg, orc):
    L = pkg._lib
    n, m = 20_001, 1001
    xyzw, rgba = orc.generate("room_shell", 4, 0, n, n)
    G = np.ascontiguousarray(orc.generate("room_shell", 3, 0, n, n)[0][:m, :3])
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    fresh = pkg.Projector(0)
    try:
        with pytest.raises(pkg.RtrError) as e:
            fresh.nearest_points(G, 0.25)
        assert e.value.code == L.RTR_ERR_INVALID and "no cloud" in str(e.value)
    finally:
        fresh.close()
    p = _new(pkg, {}, xyzw, rgba)
    try:
        lib, ctx = p._lib, p._ctx
        den = np.array([1], np.uint32).view(f32)[0]
        out = [np.full(m, 7, np.uint32), np.full(m, 7, f32), np.full(n, 7, np.uint32), np.full(n, 7, f32), np.full(4, 7, np.uint64)]

        def call(xyz, stride, count, radius, flags):
            return lib.rtr_nearest_points(ctx, vp(xyz), stride, count, radius, flags, *[vp(a) for a in out])

        # (xyz, stride, count, radius, flags, what the message names)
        bad = [(G, 12, m, v, 0, "radius") for v in (0.0, -0.0, -0.25, np.nan, np.inf, -np.inf)]
        bad += [(G, 12, m, v, 0, "square of radius") for v in (float(den), 1e-20, 1e-30, 2e19, 3e38)]
        bad += [(None, 12, m, 0.1, 0, "xyz is NULL")]
        bad += [(G, s, m, 0.1, 0, "xyz_stride_bytes") for s in (0, 4, 8, 11, 13, 14, 18)]
        bad += [(G, 12, m, 0.1, f, "flags") for f in (1, 2, 3, -1, 1 << 16)]
        for case in bad:
            assert call(*case[:5]) == L.RTR_ERR_INVALID, case[1:5]
            text = lib.rtr_last_error(ctx).decode()
            assert "rtr_nearest_points" in text and case[5] in text, (case[1:5], text)
            assert all((a == 7).all() for a in out), case[1:5]
        assert call(G, 12, 2 ** 32, 0.1, 0) == L.RTR_ERR_UNSUPPORTED and all((a == 7).all() for a in out)  # 2^32 given points or more
        assert p.get_option("selection") == 0
        # count == 0: xyz may be NULL, nothing has a nearest; the resident arrays are written all the same
        assert call(None, 12, 0, 0.1, 0) == L.RTR_OK
        assert tuple(out[4]) == (0, 0, 0, 0) and (out[2] == NONE).all() and np.isinf(out[3]).all() and (out[0] == 7).all()
        assert p.get_option("nearest_chunks_skipped") == _chunks(n)
        # a cloud sorted without point_ids has lost its upload order
        p.reorder_points()
        for a in out:
            a[...] = 7
        assert call(G, 12, m, 0.1, 0) == L.RTR_ERR_INVALID and "point_ids" in lib.rtr_last_error(ctx).decode()
        assert all((a == 7).all() for a in out)
        with pytest.raises(pkg.RtrError) as e:
            p.nearest_points(G, 0.1)
        assert e.value.code == L.RTR_ERR_INVALID and "point_ids" in str(e.value)
    finally:
        p.close()
