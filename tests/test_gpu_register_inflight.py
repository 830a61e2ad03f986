"""rtr_register_points behind an overlapped streak that is still in flight (include/rtr_register.h section 6p,
"Ordering"): the engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug
(streak_ctx.Ctx.run_plugged), `not event.query()` asserted directly in front of the call, then the call, which queues
behind the streak and waits for it.  The queued frames equal the oracle's, moments, step and stats equal the reference
(register_ref.py) bit for bit, no selection appears, and the next streak equals the oracle's on the same cloud."""
import numpy as np
import pytest

import nearest_ref as nr
import register_cases as rc
import register_ref as rr
import test_gpu_inflight_streak as inflight
from streak_ctx import Ctx, Scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(pkg, orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Scene(pkg, orc, name)
        return cache[name]
    return get


_refs = {}


def _register(radius, plane, posed):
    def kind(c, s, P):
        res = np.ascontiguousarray(s.xyzw[:, :3])
        scan = rc.unmoved(res[::23], rc.MOTION)
        nrm = rc._unit(np.random.default_rng(s.n).normal(size=res.shape) + np.float64([0, 0, 2.0]))
        pose = rc.GENERAL_POSE if posed else None
        key = (s.n, radius, plane, posed)
        if key not in _refs:
            with np.errstate(all="ignore"):
                _refs[key] = rr.register(res, scan, radius, plane, pose, nrm if plane else None, finder=nr.nearest_bucket)
        ref = _refs[key]
        assert ref[2][0] > 0.2 * scan.shape[0] and ref[2][3] == 0
        yield
        mom, step, st = c.p.register_points(scan, radius, bool(plane), pose, nrm if plane else None)
        assert st == ref[2], (st, ref[2])
        assert np.array_equal(rr.bits64(mom), rr.bits64(ref[0])) and np.array_equal(rr.bits64(step).reshape(-1), rr.bits64(ref[1]))
        assert c.p.get_option("selection") == 0
        yield s, "run"
    return kind


KINDS = {"point_10cm": _register(0.1, 0, False),
         "plane_10cm_posed": _register(0.1, 1, True),
         "point_5cm_posed": _register(0.05, 0, True)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_register_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_register_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, _register(0.1, 1, False), ("plane_10cm", "overlap = 1"), mode=1)
    finally:
        c.close()
