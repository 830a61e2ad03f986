"""rtr_select_voxel_grid behind an overlapped streak that is still in flight (include/rtr.h section 6g, "Ordering"): the
engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug (streak_ctx.Ctx.run_plugged),
`not event.query()` asserted directly in front of the call, then the call, which queues behind the streak and waits for
it.  The queued frames equal the oracle's, the words and the statistics equal the reference (voxel_ref.py), and the next
streak equals the oracle's on the same cloud."""
import numpy as np
import pytest

import test_gpu_inflight_streak as inflight
import voxel_ref as vr
from streak_ctx import Ctx, Scene

pytestmark = pytest.mark.gpu

ORIGIN = (0.013, -0.4, 0)


@pytest.fixture(scope="module")
def scenes(pkg, orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Scene(pkg, orc, name)
        return cache[name]
    return get


def _voxel(cell, min_count, op, outside):
    def kind(c, s, P):
        L = c.pkg._lib
        hit, ref = vr.select(s.xyzw, cell, ORIGIN, min_count)
        assert 0 < hit.sum() < s.n
        want = {"replace": hit != outside, "toggle": hit != outside, "add": hit != outside}[op]  # (no selection before it)
        yield
        st = c.p.select_voxel_grid(cell, ORIGIN, min_count, op=op, outside=outside)
        assert st == (int(want.sum()),) + ref, (st, ref)
        assert np.array_equal(c.p.download(L.BUF_SELECTION), vr.words(want))
        c.p.clear_selection()
        yield s, "run"
    return kind


KINDS = {"thin_5cm": _voxel(0.05, 1, "replace", False),
         "stragglers_outside": _voxel((0.25, 0.5, 0.125), 3, "toggle", True),
         "add_10cm_pairs": _voxel(0.1, 2, "add", False)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_voxel_grid_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_voxel_grid_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, KINDS["thin_5cm"], ("thin_5cm", "overlap = 1"), mode=1)
    finally:
        c.close()
