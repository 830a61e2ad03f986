"""rtr_select_near behind an overlapped streak that is still in flight (include/rtr.h section 6k, "Ordering"): the engine
of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug (streak_ctx.Ctx.run_plugged),
`not event.query()` asserted directly in front of the call, then the call, which queues behind the streak and waits for
it.  The queued frames equal the oracle's, the words, the near bits and the statistics equal the reference (near_ref.py),
and the next streak equals the oracle's on the same cloud."""
import numpy as np
import pytest

import near_ref as nr
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


def given_of(s):
    """every 13th point of the scene, moved by 3 cm along x and every other one of those by 20 cm more on all axes: some
    of them near the cloud, some not, and near a part of it"""
    g = s.xyzw[::13, :3] + np.float32([0.03, 0, 0])
    g[1::2] += np.float32([0.2, -0.2, 0.2])
    return np.ascontiguousarray(g)


def _near(radius, op, outside, given_only=False):
    def kind(c, s, P):
        L = c.pkg._lib
        G = given_of(s)
        key = (s.n, radius)
        if key not in _refs:
            _refs[key] = nr.near_bucket(s.xyzw, G, radius)
        hit, near = _refs[key]
        assert 0.05 * s.n < hit.sum() < 0.95 * s.n and 0.05 * G.shape[0] < near.sum() < 0.95 * G.shape[0]
        want = hit != outside  # (replace, toggle and add alike: no selection before it)
        yield
        st, bits = c.p.select_near(G, radius, op=op, outside=outside, near=True, given_only=given_only)
        assert np.array_equal(bits, near)
        if given_only:
            assert st == (0, 0, int(near.sum()), 0) and c.p.get_option("selection") == 0
        else:
            assert st == nr.stats(hit, near, G, want), st
            assert np.array_equal(c.p.download(L.BUF_SELECTION), nr.words(want))
            c.p.clear_selection()
        yield s, "run"
    return kind


KINDS = {"near_4cm": _near(0.04, "replace", False),
         "far_toggled": _near(0.06, "toggle", True),
         "given_only_4cm": _near(0.04, "replace", False, given_only=True)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_near_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_near_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, _near(0.04, "add", False), ("4cm_add", "overlap = 1"), mode=1)
    finally:
        c.close()
