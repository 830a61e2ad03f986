"""rtr_estimate_normals behind an overlapped streak that is still in flight (include/rtr_normals.h section 6o,
"Ordering"): the engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug
(streak_ctx.Ctx.run_plugged), `not event.query()` asserted directly in front of the call, then the call, which queues
behind the streak and waits for it.  The queued frames equal the oracle's, the three arrays and the statistics equal the
reference (normals_ref.py) bit for bit, no selection appears, and the next streak equals the oracle's on the same cloud."""
import numpy as np
import pytest

import normals_ref as nf
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


def _normals(radius, k, viewpoint):
    def kind(c, s, P):
        key = (s.n, radius)
        if key not in _rows:
            _rows[key] = nf.rows(s.xyzw, radius, 16)
        ref = nf.estimate(s.xyzw, radius, k, viewpoint, rows_k=_rows[key])
        assert 0.05 * s.n < ref["stats"][0] and (viewpoint is None or 0 < ref["stats"][3] < ref["stats"][0])
        yield
        nrm, curv, fd, st = c.p.estimate_normals(k, radius, viewpoint, found=True)
        assert st == ref["stats"], (st, ref["stats"])
        assert np.array_equal(fd, ref["found"]) and nf.same_bits(nrm, ref["normals"]) and nf.same_bits(curv, ref["curvature"])
        assert c.p.get_option("selection") == 0
        yield s, "run"
    return kind


KINDS = {"k8_5cm": _normals(0.05, 8, None),
         "k16_towards": _normals(0.1, 16, (0.0, 0.0, 1.5)),
         "k2_towards": _normals(0.05, 2, (1.0, -2.0, 0.5))}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_normals_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_normals_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, _normals(0.05, 8, (0.0, 0.0, 1.5)), ("k8_towards", "overlap = 1"), mode=1)
    finally:
        c.close()
