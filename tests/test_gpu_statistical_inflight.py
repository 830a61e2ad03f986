"""rtr_select_statistical behind an overlapped streak that is still in flight (include/rtr_statistics.h section 6n,
"Ordering"): the engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug
(streak_ctx.Ctx.run_plugged), `not event.query()` asserted directly in front of the call, then the call, which queues
behind the streak and waits for it.  The queued frames equal the oracle's, the words, both arrays and the statistics
equal the reference (statistical_ref.py), and the next streak equals the oracle's on the same cloud."""
import numpy as np
import pytest

import neighbours_ref as nr
import statistical_ref as sf
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


_rows = {}


def _statistical(radius, k, std_mul, op, outside):
    def kind(c, s, P):
        L = c.pkg._lib
        key = (s.n, radius)
        if key not in _rows:
            _rows[key] = sf.rows(s.xyzw, radius, 16)
        ref = sf.select(s.xyzw, radius, k, std_mul, rows_found=_rows[key])
        assert 0.05 * s.n < ref["hit"].sum() < 0.95 * s.n
        want = ref["hit"] != outside  # (replace, toggle and add alike: no selection before it)
        yield
        st, mom, md, fd = c.p.select_statistical(k, radius, std_mul, op=op, outside=outside, mean_dist=True, found=True)
        assert st == (int(want.sum()),) + ref["stats"], (st, ref["stats"])
        assert np.array_equal(fd, ref["found"]) and np.array_equal(md.view(np.uint32), ref["mean"].view(np.uint32))
        tol = sf.moments_tolerance(int((fd > 0).sum()))
        assert all(abs(g - w) <= tol * abs(w) for g, w in zip(mom, ref["moments"])), (mom, ref["moments"])
        assert np.array_equal(c.p.download(L.BUF_SELECTION), nr.words(want))
        c.p.clear_selection()
        yield s, "run"
    return kind


KINDS = {"k8_5cm": _statistical(0.05, 8, 1.0, "replace", False),
         "outliers_toggled": _statistical(0.1, 16, 0.5, "toggle", True),
         "add_k1": _statistical(0.05, 1, 1.0, "add", False)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_statistical_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_statistical_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, _statistical(0.05, 8, 0.5, "replace", False), ("k8_half_sigma", "overlap = 1"), mode=1)
    finally:
        c.close()
