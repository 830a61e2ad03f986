"""rtr_select_neighbours behind an overlapped streak that is still in flight (include/rtr.h section 6h, "Ordering"): the
engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug (streak_ctx.Ctx.run_plugged),
`not event.query()` asserted directly in front of the call, then the call, which queues behind the streak and waits for
it.  The queued frames equal the oracle's, the words and the statistics equal the reference (neighbours_ref.py), and the
next streak equals the oracle's on the same cloud."""
import numpy as np
import pytest

import neighbours_ref as nr
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


_counts = {}


def _neighbours(radius, k, op, outside):
    def kind(c, s, P):
        L = c.pkg._lib
        key = (s.n, radius)
        if key not in _counts:
            _counts[key] = nr.counts(s.xyzw, radius)
        hit, ref = nr.select(s.xyzw, radius, k, _counts[key])
        assert 0.05 * s.n < hit.sum() < 0.95 * s.n
        want = hit != outside  # (replace, toggle and add alike: no selection before it)
        yield
        st = c.p.select_neighbours(radius, k, op=op, outside=outside)
        assert st == (int(want.sum()),) + ref, (st, ref)
        assert np.array_equal(c.p.download(L.BUF_SELECTION), nr.words(want))
        c.p.clear_selection()
        yield s, "run"
    return kind


KINDS = {"pairs_5cm": _neighbours(0.05, 2, "replace", False),
         "outliers_toggled": _neighbours(0.1, 4, "toggle", True),
         "add_5cm": _neighbours(0.05, 1, "add", False)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_neighbours_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_neighbours_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, _neighbours(0.05, 4, "replace", False), ("5cm_4", "overlap = 1"), mode=1)
    finally:
        c.close()
