"""rtr_estimate_normals against a failed device allocation (include/rtr_normals.h section 6o, "Errors"; option
"debug_alloc_fail"; README_alloc_failure.md): the sweep of test_gpu_alloc_failure.py on this call, in the three states
of alloc_failure_cases.py, with its states, snapshot, sentinel-filled raw call and health check.

Per state: (1) unarmed on a fresh context the call equals the reference (normals_ref.py) and K0 = the allocations it
attempted is at least 1; (2) for k = 1 .. K0 on another fresh context "debug_alloc_fail" = k fires inside the call, which
returns RTR_ERR_HIP with a message, the snapshot is intact -- the selection word for word --, and every byte of normals,
curvature, found and stats still holds the sentinel; (3) the health check is exact; (4) the call again is exact; (5),
(6) the context goes and "debug_alloc_live" is back where it was."""
import numpy as np
import pytest

import alloc_failure_cases as afc
import normals_ref as nf
from test_gpu_alloc_failure import _count, _health, _same

pytestmark = pytest.mark.gpu

K = 8
VIEW = np.float32([0.0, 0.0, 1.5])
OUTPUTS = ("normals", "curvature", "found", "stats")
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
    e = nf.estimate(xyz, afc._radius(orc), K, VIEW)
    assert 0.05 * afc.N < e["stats"][0] < afc.N and 0 < (e["found"] < K).sum() and 0 < e["stats"][3] < e["stats"][0]
    return e


def _call(cx):
    n, L = cx.model.n, cx.L
    out = {"normals": np.zeros((n, 3), np.float32), "curvature": np.zeros(n, np.float32), "found": np.zeros(n, np.uint32),
           "stats": np.zeros(4, np.uint64)}
    afc._raw(cx, "rtr_estimate_normals", [K, afc._radius(cx.orc), L.NORMAL_VIEWPOINT, afc._ptr(VIEW), "normals", "curvature", "found", "stats"], out)
    return out


def _exact(got, e, what):
    assert np.array_equal(got["found"], e["found"]), what
    assert nf.same_bits(got["normals"], e["normals"]) and nf.same_bits(got["curvature"], e["curvature"]), what
    assert tuple(int(v) for v in got["stats"]) == e["stats"], what


@pytest.mark.parametrize("state", afc.STATES)
def test_a_failed_allocation_leaves_everything_as_it_was(pkg, orc, observer, ref, state):
    live0 = observer.get_option("debug_alloc_live")
    p, model = afc.build(pkg, orc, state)
    try:
        cx = afc.Ctx(pkg, orc, p, model)
        before = afc.snapshot(pkg, p)
        c0 = _count(p)
        got = _call(cx)
        K0 = _count(p) - c0
        _exact(got, ref, ("unarmed", state))
        _same(afc.snapshot(pkg, p), before, ("the call itself changed the snapshot", state))  # (a pure analysis call)
    finally:
        p.close()
    assert K0 >= 1
    K0_SEEN[state] = K0
    for k in range(1, K0 + 1):
        what = (state, "k", k, "of", K0)
        p, model = afc.build(pkg, orc, state)
        try:
            cx = afc.Ctx(pkg, orc, p, model)
            before = afc.snapshot(pkg, p)
            p.set_option("debug_alloc_fail", k)
            with pytest.raises(pkg.RtrError) as e:
                _call(cx)
            left = p.get_option("debug_alloc_fail")
            p.set_option("debug_alloc_fail", 0)
            assert left == 0, ("the switch did not fire: the call made fewer allocations than the unarmed run", what)
            assert e.value.code == afc.RTR_ERR_HIP and str(e.value).split(":", 1)[1].strip(), (what, str(e.value))
            _same(afc.snapshot(pkg, p), before, ("the snapshot changed", what))
            assert set(cx.note["outputs_untouched"]) == set(OUTPUTS) and all(cx.note["outputs_untouched"].values()), \
                ("a caller output was written", cx.note["outputs_untouched"], what)
            _health(pkg, orc, p, model, what)
            again = _call(cx)
            _exact(again, ref, ("again", what))
        finally:
            p.close()
    assert observer.get_option("debug_alloc_live") == live0, ("allocations leaked", state)


def test_k0_table(observer):
    """Prints state x K0 as the sweep found them (README_normals.md holds the row)."""
    print()
    for state, k0 in sorted(K0_SEEN.items()):
        print("K0 %-28s %-12s %d" % ("estimate_normals", state, k0))
    assert observer.get_option("debug_alloc_fail") == 0
