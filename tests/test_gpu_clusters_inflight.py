"""rtr_select_clusters behind an overlapped streak that is still in flight (include/rtr.h section 6i, "Ordering"): the
engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug (streak_ctx.Ctx.run_plugged),
`not event.query()` asserted directly in front of the call, then the call, which queues behind the streak and waits for
it.  The queued frames equal the oracle's, the words, the labels and the statistics equal the reference
(clusters_ref.py), and the next streak equals the oracle's on the same cloud."""
import numpy as np
import pytest

import clusters_ref as cr
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


_labels = {}


def _clusters(radius, lo, hi, op, outside):
    def kind(c, s, P):
        L = c.pkg._lib
        key = (s.n, radius)
        if key not in _labels:
            _labels[key] = cr.labels(s.xyzw, radius)
        lab = _labels[key]
        hit = cr.hits(lab, lo, hi)
        ref = cr.stats(lab, hit)
        assert 0.05 * s.n < hit.sum() < 0.95 * s.n and ref[0] >= 20
        want = hit != outside  # (replace, toggle and add alike: no selection before it)
        yield
        st, got = c.p.select_clusters(radius, lo, hi, op=op, outside=outside, labels=True)
        assert st == (int(want.sum()),) + ref, (st, ref)
        assert np.array_equal(c.p.download(L.BUF_SELECTION), cr.words(want))
        assert np.array_equal(got, lab)
        c.p.clear_selection()
        yield s, "run"
    return kind


KINDS = {"pairs_5cm": _clusters(0.05, 2, 0, "replace", False),
         "small_toggled": _clusters(0.05, 2, 4, "toggle", True),
         "add_5_and_more": _clusters(0.05, 5, 0, "add", False)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_clusters_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_clusters_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, _clusters(0.05, 50, 0, "replace", False), ("5cm_50", "overlap = 1"), mode=1)
    finally:
        c.close()
