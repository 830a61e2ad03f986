"""rtr_select_segments against a failed device allocation (include/rtr_segments.h section 6q, "Errors"; option
"debug_alloc_fail"; README_alloc_failure.md): the sweep of test_gpu_alloc_failure.py on this call, in the three states
of alloc_failure_cases.py, with its states, snapshot, sentinel-filled raw call and health check.  The normals and the
curvature lie in HOST memory, so that the two staging buffers are among the allocation sites.

Per state: (1) unarmed on a fresh context the call equals the reference (segments_ref.py) and K0 = the allocations it
attempted is at least 1; (2) for k = 1 .. K0 on another fresh context "debug_alloc_fail" = k fires inside the call, which
returns RTR_ERR_HIP with a message, the snapshot is intact -- the selection word for word --, and every byte of labels
and stats still holds the sentinel, and the caller's normals and curvature are as they were; (3) the health check is
exact; (4) the call again is exact; (5), (6) the context goes and "debug_alloc_live" is back where it was."""
import numpy as np
import pytest

import alloc_failure_cases as afc
import normals_ref as nref
import segments_cases as sc
import segments_ref as sg
import select_ref as sr
from test_gpu_alloc_failure import _count, _health, _same

pytestmark = pytest.mark.gpu

K = 8
LIMIT = np.float32(0.05)
WINDOW = (2, 0)
OUTPUTS = ("labels", "stats")
K0_SEEN = {}


@pytest.fixture(scope="module")
def observer(pkg):
    """A context that lives through every case and only reads the process-wide counters."""
    p = pkg.Projector(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def ref(orc):
    xyz = afc.base_cloud(orc)[0]
    r = afc._radius(orc)
    est = nref.estimate(xyz, r, K)
    lab = sg.labels(xyz, r, sc.COS_ANGLE, est["normals"], est["curvature"], LIMIT)
    hit = sg.hits(lab, *WINDOW)
    roots = lab == np.arange(afc.N)
    assert (roots & (sg.sizes(lab) >= 2)).sum() >= 20 and 0.05 * afc.N < hit.sum() < 0.95 * afc.N
    assert 0 < sg.usable(afc.N, est["curvature"], LIMIT).sum() < afc.N
    return {"normals": est["normals"], "curvature": est["curvature"], "labels": lab, "hit": hit, "stats": sg.stats(lab, hit)}


def _call(cx, ref):
    n, L = cx.model.n, cx.L
    out = {"labels": np.zeros(n, np.uint32), "stats": np.zeros(4, np.uint64)}
    afc._raw(cx, "rtr_select_segments", [afc._radius(cx.orc), float(sc.COS_ANGLE), afc._ptr(ref["normals"]), afc._ptr(ref["curvature"]), float(LIMIT),
                                         WINDOW[0], WINDOW[1], 0, L.SELECT_ADD, "labels", "stats"], out)
    return out


def _exact(pkg, p, got, ref, before, what):
    n = afc.N
    want = sr.unpack(before["selection_words"], n) | ref["hit"]
    assert np.array_equal(got["labels"], ref["labels"]), what
    assert tuple(int(v) for v in got["stats"]) == (int(want.sum()),) + ref["stats"], what
    assert np.array_equal(p.download(pkg._lib.BUF_SELECTION), sg.words(want)), what


@pytest.mark.parametrize("state", afc.STATES)
def test_a_failed_allocation_leaves_everything_as_it_was(pkg, orc, observer, ref, state):
    live0 = observer.get_option("debug_alloc_live")
    inputs = (ref["normals"].copy(), ref["curvature"].copy())
    p, model = afc.build(pkg, orc, state)
    try:
        cx = afc.Ctx(pkg, orc, p, model)
        before = afc.snapshot(pkg, p)
        c0 = _count(p)
        got = _call(cx, ref)
        K0 = _count(p) - c0
        _exact(pkg, p, got, ref, before, ("unarmed", state))
        after = afc.snapshot(pkg, p)
        after["selection_words"] = before["selection_words"]
        _same(after, before, ("the call changed more than the selection", state))
    finally:
        p.close()
    assert K0 >= 3  # (the normal records and the two staging buffers at the least)
    K0_SEEN[state] = K0
    for k in range(1, K0 + 1):
        what = (state, "k", k, "of", K0)
        p, model = afc.build(pkg, orc, state)
        try:
            cx = afc.Ctx(pkg, orc, p, model)
            before = afc.snapshot(pkg, p)
            p.set_option("debug_alloc_fail", k)
            with pytest.raises(pkg.RtrError) as e:
                _call(cx, ref)
            left = p.get_option("debug_alloc_fail")
            p.set_option("debug_alloc_fail", 0)
            assert left == 0, ("the switch did not fire: the call made fewer allocations than the unarmed run", what)
            assert e.value.code == afc.RTR_ERR_HIP and str(e.value).split(":", 1)[1].strip(), (what, str(e.value))
            _same(afc.snapshot(pkg, p), before, ("the snapshot changed", what))
            assert set(cx.note["outputs_untouched"]) == set(OUTPUTS) and all(cx.note["outputs_untouched"].values()), \
                ("a caller output was written", cx.note["outputs_untouched"], what)
            assert nref.same_bits(ref["normals"], inputs[0]) and nref.same_bits(ref["curvature"], inputs[1]), what
            _health(pkg, orc, p, model, what)
            again = _call(cx, ref)
            _exact(pkg, p, again, ref, before, ("again", what))
        finally:
            p.close()
    assert observer.get_option("debug_alloc_live") == live0, ("allocations leaked", state)


def test_k0_table(observer):
    """Prints state x K0 as the sweep found them (README_segments.md holds the row)."""
    print()
    for state, k0 in sorted(K0_SEEN.items()):
        print("K0 %-28s %-12s %d" % ("select_segments", state, k0))
    assert observer.get_option("debug_alloc_fail") == 0
