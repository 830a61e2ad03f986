"""Every entry point against a failed device allocation (include/rtr.h: each call says what it leaves behind; option
"debug_alloc_fail"; tests/alloc_failure_cases.py: the states, the calls, their contracts; README_alloc_failure.md).

For each call and each state it applies to: (1) on a fresh context in that state the call, unarmed, equals its reference,
and K0 = the allocations it attempted (the difference of "debug_alloc_count") is at least 1; (2) for k = 1 .. K0, on
another fresh context in the same state, "debug_alloc_fail" = k is armed, the call is made, the switch must have fired,
and the return code and the context's state must be what the call's contract says; (3) on that context, disarmed, a
health check -- a filtered frame and its point pass against the oracle on the points the state draws, and
rtr_download_points of everything; (4) the call again, unarmed: RTR_OK and its reference; (5) the context is destroyed;
(6) at the end "debug_alloc_live", read through a long-lived observer context, is what it was before the case.

A fresh context per k, not one context swept upward: a failed call may rightly keep what it made lazily, so only on a
fresh context is site k of the sweep site k of the unarmed run, and every site hit exactly once.  The switch is a
host-side return value: nothing is requested from the device and nothing is launched for the allocation that fails."""
import numpy as np
import pytest

import alloc_failure_cases as afc
import pool_overflow_scenes as pos

pytestmark = pytest.mark.gpu

K0_SEEN = {}  # (case, state) -> K0, printed by the last test (the table of README_alloc_failure.md)


@pytest.fixture(scope="module")
def observer(pkg):
    """A context that lives through every case and only reads the process-wide counters."""
    p = pkg.Projector(0)
    yield p
    p.close()


def _count(p):
    return p.get_option("debug_alloc_count")


def _same(got, want, what, ignore=()):
    bad = afc.differences(got, want, ignore)
    assert not bad, (what, bad)


def _health(pkg, orc, p, model, what):
    """Step 3: a filtered frame and its point pass at a pose of edit_model.pose_for against the oracle on the drawable
    points, bit for bit; rtr_download_points of everything against the model (this is what walks ensure_soa)."""
    L = pkg._lib
    p.set_resolution(afc.W, afc.H)
    P = afc.health_pose(model)
    ref = afc.frame_ref(orc, model, P, True)
    img, depth = p.project(P, filtered=True)
    got = {"depth_bits": depth.view(np.uint32), "img": img, "tensor": p.download(L.BUF_TENSOR).reshape(5, afc.H, afc.W),
           "minmax": p.download(L.BUF_MINMAX)}
    _same(got, {k: ref[k] for k in got}, ("health frame", what))
    assert p.frame_stats()["errors"] == 0, ("health frame_stats", what)
    if model.n == 0:
        return
    p.point_pass(P)
    ids, vis = afc.point_pass_ref(orc, model, P, ref)
    _same({"ids": p.download(L.BUF_POINT_ID), "visible": p.download(L.BUF_VISIBLE)}, {"ids": ids, "visible": vis},
          ("health point pass", what))
    xyzw, rgba = p.download_points()
    mx, mc = afc.helpers.cloud(model.xyz, model.rgb)
    state = "sorted" if p.get_option("reordered") else "upload"
    assert np.array_equal(afc.resident_rows(xyzw, rgba, state), afc.resident_rows(mx, mc, state)), ("health download", what)


def _matches_model(pkg, p, model, what, ignore=("views", "p2p_open")):
    _same(afc.snapshot(pkg, p), afc.model_snapshot(model), what, ignore)


def _armed_call(case, cx, k):
    """The call with the switch armed at k: (code, message, result); the switch must have fired."""
    p = cx.p
    p.set_option("debug_alloc_fail", k)
    code, text, result = 0, "", None
    try:
        result = case.call(cx)
    except cx.L.RtrError as e:
        code, text = e.code, str(e)
    left = p.get_option("debug_alloc_fail")
    p.set_option("debug_alloc_fail", 0)
    assert left == 0, ("the switch did not fire: the call made fewer allocations than the unarmed run", case.name, k, left)
    if code != 0:
        assert code == afc.RTR_ERR_HIP, (case.name, k, code, text)
        assert text.split(":", 1)[1].strip(), ("rtr_last_error is empty", case.name, k)
    return code, text, result


def _sweep(pkg, orc, observer, case, state):
    live0 = observer.get_option("debug_alloc_live")
    # (1) unarmed: the reference, and K0
    p, model = afc.build(pkg, orc, state)
    try:
        cx = afc.Ctx(pkg, orc, p, model)
        if case.prepare:
            case.prepare(cx)
        after = afc.copy_model(model)
        want = case.expect(cx, after)
        c0 = _count(p)
        got = case.call(cx)
        K0 = _count(p) - c0
        _same(got, want, ("unarmed", case.name, state))
        if case.group in ("atomic", "replace", "reorder"):
            _matches_model(pkg, p, after, ("unarmed state", case.name, state))
        if case.name == "overlap_third_frame":
            assert cx.note["overlap_active"] == 1, "the third frame of the streak did not engage the overlap"
    finally:
        p.close()
    assert K0 >= 1, ("the call allocates nothing in this state: take it off the state's list by name", case.name, state)
    K0_SEEN[(case.name, state)] = K0
    outcomes = []
    # (2) .. (5) one fresh context per site
    for k in range(1, K0 + 1):
        what = (case.name, state, "k", k, "of", K0)
        p, model = afc.build(pkg, orc, state)
        try:
            cx = afc.Ctx(pkg, orc, p, model)
            if case.group == "tolerant":  # (its preparation is a streak of frames, which any other call would end)
                before = afc.snapshot(pkg, p)
                case.prepare(cx)
            else:
                if case.prepare:
                    case.prepare(cx)
                before = afc.snapshot(pkg, p)
            code, text, result = _armed_call(case, cx, k)
            now = _contract(pkg, orc, case, cx, before, code, result, what)
            outcomes.append((code, now.n, p.get_option("packed"), p.get_option("reordered")))
            cx.model = now
            _health(pkg, orc, p, now, what)                              # (3)
            if case.group == "tolerant":
                continue  # (the call is a place in a streak, which the health check has ended: nothing to repeat)
            if "resolution" in cx.note:
                p.W, p.H = afc.W, afc.H
            if case.prepare:
                case.prepare(cx)
            again = afc.copy_model(now)
            want = case.expect(cx, again)
            got = case.call(cx)                                          # (4): raises unless RTR_OK
            _same(got, want, ("again", what))
            if case.group in ("atomic", "replace", "reorder"):
                _matches_model(pkg, p, again, ("state after the call again", what))
        finally:
            p.close()                                                    # (5)
    assert observer.get_option("debug_alloc_live") == live0, ("allocations leaked", case.name, state)   # (6)
    return outcomes


def _contract(pkg, orc, case, cx, before, code, result, what):
    """The return code and state the call's contract allows after a failed allocation; -> the model the context now equals."""
    p, model = cx.p, cx.model
    snap = afc.snapshot(pkg, p)
    if case.group == "atomic":
        assert code == afc.RTR_ERR_HIP, ("an atomic call must report the failed allocation", what, code)
        _same(snap, before, ("atomic: the snapshot changed", what))
        if "stats_untouched" in cx.note:
            assert cx.note["stats_untouched"], ("rtr.h promises stats untouched", what)
        if case.name in afc.OUTPUTS_UNTOUCHED:  # (rtr.h promises the caller's outputs untouched: the sentinel is still there)
            assert set(cx.note["outputs_untouched"]) == set(afc.OUTPUTS_UNTOUCHED[case.name]), what
            assert all(cx.note["outputs_untouched"].values()), ("a caller output was written", cx.note["outputs_untouched"], what)
        return model
    if case.group == "frame":
        assert code == afc.RTR_ERR_HIP, ("a frame resource that cannot be made is an error", what, code)
        _same(snap, before, ("frame: the cloud changed", what), ("views",))
        if case.name.startswith("render_views_3"):
            assert snap["views"] == 0, ("no batch is current after a failed allocation", what)
            assert before["views"] == (1 if case.name.endswith("after_1") else 0), what
        if case.name == "point_pass":  # (no pass has run on this context: both buffers read as before any pass)
            for which in (cx.L.BUF_POINT_ID, cx.L.BUF_VISIBLE):
                with pytest.raises(cx.L.RtrError) as e:
                    p.device_buffer(which)
                assert e.value.code == cx.L.RTR_ERR_INVALID, (which, what)
        return model
    if case.group == "tolerant":
        assert code == 0, ("a best-effort site must give up quietly", what, code)
        want = case.expect(cx, afc.copy_model(model))
        _same(result, want, ("tolerant: the frame", what))
        assert cx.note["overlap_active"] == 0, ("the fallback must be visible", what)
        _same(snap, before, ("tolerant: the cloud changed", what))
        return model
    after = afc.copy_model(model)
    want = case.expect(cx, after)
    if code == 0:
        # a best-effort site inside the call gave up (the packing, the sort behind an upload, the measure of the order):
        # exact results, the new state, and only "packed" / "reordered" may read 0 where the model says 1
        _same(result, want, ("best effort: the result", what))
        _same(snap, afc.model_snapshot(after), ("best effort: the state", what), ("views", "p2p_open", "packed", "reordered"))
        assert snap["packed"] <= int(after.pack == 2) and snap["reordered"] <= int(after.sorted), what
        after.sorted = bool(snap["reordered"])  # (the option "pack" stays what it is: the next packing tries again)
        if case.group == "reorder":
            assert snap["reordered"] == 1, ("a sort that succeeded", what)
        return after
    if snap["num_points"] == before["num_points"] and case.group in ("replace", "reorder") and not afc.differences(snap, before):
        if case.name.startswith("pack_"):  # (the option keeps its previous value with the cloud's form)
            assert p.get_option("pack") == afc.STATE_OPTIONS[model.state]["pack"], what
        return model  # the old cloud, intact
    assert case.group == "replace", ("the sort must leave the cloud intact", what, afc.differences(snap, before))
    empty = afc.copy_model(model)
    empty.upload(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    empty.sorted = False
    assert snap["num_points"] == 0, ("neither the old cloud intact nor an empty context", what, afc.differences(snap, before))
    _same(snap, afc.model_snapshot(empty), ("the context of an upload of 0 points", what), ("views", "p2p_open"))
    return empty


@pytest.mark.parametrize("name,state", [i for i in afc.case_ids() if afc.by_name(i[0]).group == "atomic"])
def test_atomic_calls_leave_everything_as_it_was(pkg, orc, observer, name, state):
    _sweep(pkg, orc, observer, afc.by_name(name), state)


@pytest.mark.parametrize("name,state", [i for i in afc.case_ids() if afc.by_name(i[0]).group == "replace"])
def test_cloud_replacing_calls_leave_the_old_cloud_or_none(pkg, orc, observer, name, state):
    case = afc.by_name(name)
    outcomes = _sweep(pkg, orc, observer, case, state)
    if name.startswith("upload") or name == "generate_synthetic":
        # the sweep has been through the allocation of the cloud itself and through the best-effort packing behind it
        # (a generated cloud that fits the fp32 arrays of the "pack" = 0 state allocates nothing that is not best effort)
        if not (name == "generate_synthetic" and state == "pack0"):
            assert any(code != 0 for code, *_ in outcomes), outcomes
        # (in the sorted state the sort packs, and where that gives up the upload itself packs once more: never visible)
        if state == "packed":
            assert any(code == 0 and packed == 0 for code, _, packed, _ in outcomes), ("pack_cloud was not reached", outcomes)
        if state == "sorted":
            assert any(code == 0 and reordered == 0 for code, _, _, reordered in outcomes), ("auto_reorder was not reached", outcomes)


@pytest.mark.parametrize("name,state", [i for i in afc.case_ids() if afc.by_name(i[0]).group == "reorder"])
def test_reorder_points_fails_whole_or_succeeds(pkg, orc, observer, name, state):
    outcomes = _sweep(pkg, orc, observer, afc.by_name(name), state)
    assert any(code != 0 for code, *_ in outcomes), outcomes


@pytest.mark.parametrize("name,state", [i for i in afc.case_ids() if afc.by_name(i[0]).group == "tolerant"])
def test_tolerant_sites_give_up_quietly(pkg, orc, observer, name, state):
    _sweep(pkg, orc, observer, afc.by_name(name), state)


@pytest.mark.parametrize("name,state", [i for i in afc.case_ids() if afc.by_name(i[0]).group == "frame"])
def test_frame_resources_fail_whole_and_come_back(pkg, orc, observer, name, state):
    _sweep(pkg, orc, observer, afc.by_name(name), state)


# ---- the repair of a frame that overflowed the adaptive extent pool, inside rtr_synchronize (pool_overflow_scenes.py) --------
@pytest.fixture(scope="module")
def big(pkg, orc):
    xyzw, rgba = pos.cloud(orc)
    P = pos.p_one(orc)[0]
    ref = orc.project(xyzw, rgba, P, pos.W, pos.H)
    return xyzw, rgba, P, ref


def test_repair_in_synchronize_fails_whole_and_comes_back(pkg, orc, observer, big):
    """The first frame after the upload overflows the adaptive pool; rtr_synchronize sizes the pool for the worst case and
    renders the frame again.  That allocation failing: RTR_ERR_HIP, the cloud intact, and the frame rendered again exact."""
    xyzw, rgba, P, ref = big
    L = pkg._lib
    live0 = observer.get_option("debug_alloc_live")

    def fresh():
        p = pkg.Projector(0)
        pos.prepare(pkg, orc, p, xyzw, rgba, "first")
        p.render(P)
        return p

    def exact(p, what):
        assert np.array_equal(p.download(L.BUF_DEPTH).reshape(-1), ref["depth_bits"].reshape(-1)), ("depth", what)
        assert np.array_equal(p.download(L.BUF_IMAGE), ref["img"]), ("image", what)
        pos.no_errors(p)

    p = fresh()
    try:
        before = pos.footprint(p)
        c0 = _count(p)
        p.synchronize()
        K0 = _count(p) - c0
        pos.assert_overflowed(p, before, "unarmed")
        exact(p, "unarmed")
    finally:
        p.close()
    assert K0 >= 1
    K0_SEEN[("synchronize_repair", "2e6 points")] = K0
    for k in range(1, K0 + 1):
        p = fresh()
        try:
            p.set_option("debug_alloc_fail", k)
            with pytest.raises(L.RtrError) as e:
                p.synchronize()
            assert p.get_option("debug_alloc_fail") == 0
            assert e.value.code == afc.RTR_ERR_HIP and str(e.value).split(":", 1)[1].strip(), (k, str(e.value))
            assert p.num_points == pos.N and p.get_option("packed") in (0, 1)
            p.render(P)          # the frame again: the pool is made worst-case sized this time
            p.synchronize()
            exact(p, ("again", k))
            P2 = pkg.orbit_projection(3, pos.W, pos.H)
            img, depth = p.project(P2)
            r2 = orc.project(xyzw, rgba, P2, pos.W, pos.H)
            assert np.array_equal(depth.view(np.uint32).reshape(-1), r2["depth_bits"].reshape(-1)) and np.array_equal(img, r2["img"]), k
        finally:
            p.close()
    assert observer.get_option("debug_alloc_live") == live0


def test_steady_state_frames_allocate_nothing(pkg, orc):
    """The shipped frame path must not slow down: the wrapper costs one relaxed load and two increments per allocation,
    and a steady-state frame makes none -- "debug_alloc_count" does not move across 10 renders."""
    p, model = afc.build(pkg, orc, "packed")
    try:
        P = afc.health_pose(model)
        for _ in range(4):  # (the streak engages the overlap at the third frame: its second store and pool are made there)
            p.render(P, with_filter=True)
        p.synchronize()
        c0 = _count(p)
        for _ in range(10):
            p.render(P, with_filter=True)
        p.synchronize()
        assert _count(p) == c0
        assert p.get_option("debug_alloc_fail") == 0
    finally:
        p.close()


def test_k0_table(observer):
    """Prints call x state x K0 as the sweep found them (README_alloc_failure.md holds the table)."""
    print()
    for (name, state), k0 in sorted(K0_SEEN.items()):
        print("K0 %-34s %-12s %d" % (name, state, k0))
    assert observer.get_option("debug_alloc_fail") == 0
