"""rtr_register_points against a failed device allocation (include/rtr_register.h section 6p, "Errors"; option
"debug_alloc_fail"; README_alloc_failure.md): the sweep of test_gpu_alloc_failure.py on this call, in both modes and the
three states of alloc_failure_cases.py, with its states, snapshot, sentinel-filled raw call and health check.

Per state and mode: (1) unarmed on a fresh context the call equals the reference (register_ref.py) and K0 = the
allocations it attempted is at least 1; (2) for k = 1 .. K0 on another fresh context "debug_alloc_fail" = k fires inside
the call, which returns RTR_ERR_HIP with a message, the snapshot is intact -- the selection word for word --, and every
byte of moments, step and stats still holds the sentinel; (3) the health check is exact; (4) the call again is exact;
(5), (6) the context goes and "debug_alloc_live" is back where it was."""
import numpy as np
import pytest

import alloc_failure_cases as afc
import register_cases as rc
import register_ref as rr
from test_gpu_alloc_failure import _count, _health, _same

pytestmark = pytest.mark.gpu

OUTPUTS = ("moments", "step", "stats")
POSE = np.ascontiguousarray(rc.GENERAL_POSE).reshape(12)
K0_SEEN = {}


@pytest.fixture(scope="module")
def observer(pkg):
    """A context that lives through every case and only reads the process-wide counters."""
    p = pkg.Projector(0)
    yield p
    p.close()


def _normals():
    return rc._unit(np.random.default_rng(17).normal(size=(afc.N, 3)))


@pytest.fixture(scope="module")
def refs(orc):
    xyz, G, r = afc.base_cloud(orc)[0], afc._given(orc), afc._radius(orc)
    out = {plane: rr.register(xyz, G, r, plane, POSE, _normals() if plane else None) for plane in (0, 1)}
    assert all(50 < e[2][0] < len(G) and e[2][3] == 0 for e in out.values())
    return out


def _call(cx, plane):
    G, nrm = afc._given(cx.orc), _normals()
    out = {"moments": np.zeros(32, np.float64), "step": np.zeros(12, np.float64), "stats": np.zeros(4, np.uint64)}
    afc._raw(cx, "rtr_register_points", [afc._ptr(G), 12, len(G), afc._radius(cx.orc), plane, afc._ptr(POSE), afc._ptr(nrm) if plane else None,
                                         "moments", "step", "stats"], out)
    return out


def _exact(got, e, what):
    assert np.array_equal(rr.bits64(got["moments"]), rr.bits64(e[0])) and np.array_equal(rr.bits64(got["step"]), rr.bits64(e[1])), what
    assert tuple(int(v) for v in got["stats"]) == e[2], what


@pytest.mark.parametrize("plane", [0, 1], ids=["point", "plane"])
@pytest.mark.parametrize("state", afc.STATES)
def test_a_failed_allocation_leaves_everything_as_it_was(pkg, orc, observer, refs, state, plane):
    live0 = observer.get_option("debug_alloc_live")
    p, model = afc.build(pkg, orc, state)
    try:
        cx = afc.Ctx(pkg, orc, p, model)
        before = afc.snapshot(pkg, p)
        c0 = _count(p)
        got = _call(cx, plane)
        K0 = _count(p) - c0
        _exact(got, refs[plane], ("unarmed", state, plane))
        _same(afc.snapshot(pkg, p), before, ("the call itself changed the snapshot", state))  # (a pure analysis call)
    finally:
        p.close()
    assert K0 >= 1
    K0_SEEN[(state, plane)] = K0
    for k in range(1, K0 + 1):
        what = (state, plane, "k", k, "of", K0)
        p, model = afc.build(pkg, orc, state)
        try:
            cx = afc.Ctx(pkg, orc, p, model)
            before = afc.snapshot(pkg, p)
            p.set_option("debug_alloc_fail", k)
            with pytest.raises(pkg.RtrError) as e:
                _call(cx, plane)
            left = p.get_option("debug_alloc_fail")
            p.set_option("debug_alloc_fail", 0)
            assert left == 0, ("the switch did not fire: the call made fewer allocations than the unarmed run", what)
            assert e.value.code == afc.RTR_ERR_HIP and str(e.value).split(":", 1)[1].strip(), (what, str(e.value))
            _same(afc.snapshot(pkg, p), before, ("the snapshot changed", what))
            assert set(cx.note["outputs_untouched"]) == set(OUTPUTS) and all(cx.note["outputs_untouched"].values()), \
                ("a caller output was written", cx.note["outputs_untouched"], what)
            _health(pkg, orc, p, model, what)
            again = _call(cx, plane)
            _exact(again, refs[plane], ("again", what))
        finally:
            p.close()
    assert observer.get_option("debug_alloc_live") == live0, ("allocations leaked", state)


def test_k0_table(observer):
    """Prints state x mode x K0 as the sweep found them (README_register.md holds the rows)."""
    print()
    for (state, plane), k0 in sorted(K0_SEEN.items()):
        print("K0 %-28s %-12s %-6s %d" % ("register_points", state, "plane" if plane else "point", k0))
    assert observer.get_option("debug_alloc_fail") == 0
