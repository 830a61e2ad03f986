"""rtr_nearest_points behind an overlapped streak that is still in flight (include/rtr.h section 6l, "Ordering"): the
engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug (streak_ctx.Ctx.run_plugged),
`not event.query()` asserted directly in front of the call, then the call, which queues behind the streak and waits for
it.  The queued frames equal the oracle's, all four arrays and the statistics equal the reference (nearest_ref.py), and
the next streak equals the oracle's on the same cloud."""
import pytest

import nearest_ref as nf
import test_gpu_inflight_streak as inflight
from streak_ctx import Ctx, Scene
from test_gpu_near_inflight import given_of

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


def _nearest(radius, resident):
    def kind(c, s, P):
        G = given_of(s)
        key = (s.n, radius)
        if key not in _refs:
            _refs[key] = nf.nearest_bucket(s.xyzw, G, radius)
        want = _refs[key]
        assert 0.05 * G.shape[0] < want[4][0] < 0.95 * G.shape[0] and 0.05 * s.n < want[4][1] < 0.95 * s.n
        yield
        got = c.p.nearest_points(G, radius, resident=resident)
        assert got[-1] == want[4], got[-1]
        assert nf.same(got[:-1], want[:4] if resident else want[:2])
        assert c.p.get_option("selection") == 0
        yield s, "run"
    return kind


KINDS = {"given_4cm": _nearest(0.04, False), "both_6cm": _nearest(0.06, True)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_nearest_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_nearest_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, _nearest(0.04, True), ("both_4cm", "overlap = 1"), mode=1)
    finally:
        c.close()
