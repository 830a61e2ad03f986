"""rtr_nearest_k_points behind an overlapped streak that is still in flight (include/rtr.h section 6m, the ordering of
section 6l): the engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug
(streak_ctx.Ctx.run_plugged), `not event.query()` asserted directly in front of the call, then the call, which queues
behind the streak and waits for it.  The queued frames equal the oracle's, the three arrays and the statistics equal the
reference (nearest_k_ref.py), and the next streak equals the oracle's on the same cloud."""
import pytest

import nearest_k_ref as kf
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


def _nearest_k(radius, k):
    def kind(c, s, P):
        G = given_of(s)
        key = (s.n, radius, k)
        if key not in _refs:
            _refs[key] = kf.nearest_k_bucket(s.xyzw, G, radius, k)
        want = _refs[key]
        assert 0.05 * G.shape[0] < want[3][0] < 0.95 * G.shape[0] and want[3][1] > want[3][0]
        yield
        got = c.p.nearest_k_points(G, k, radius)
        assert got[3] == want[3], got[3]
        assert kf.same(got[:3], want[:3])
        assert c.p.get_option("selection") == 0
        yield s, "run"
    return kind


KINDS = {"k3_4cm": _nearest_k(0.04, 3), "k16_6cm": _nearest_k(0.06, 16)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_nearest_k_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()
