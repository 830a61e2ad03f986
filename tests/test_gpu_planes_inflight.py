"""rtr_count_in_bands and rtr_fit_plane behind an overlapped streak that is still in flight (include/rtr.h section 6j,
"Ordering"): the engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug
(streak_ctx.Ctx.run_plugged), `not event.query()` asserted directly in front of the call, then the call, which queues
behind the streak and waits for it.  The queued frames equal the oracle's, the counts, the plane and the statistics equal
the reference (planes_ref.py), and the next streak equals the oracle's on the same cloud."""
import numpy as np
import pytest

import planes_ref as pr
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


def _bands(xyzw):
    rng = np.random.default_rng(19)
    out = [np.float32([0, 0, 1, 1000, 1000]), np.float32([0, 0, 1, -1000, 2000])]
    while len(out) < 70:  # (more than one pass)
        i = rng.choice(len(xyzw), 3, replace=False)
        pl = pr.candidate(xyzw[i[0], :3], xyzw[i[1], :3], xyzw[i[2], :3], [0, 1, 2])
        if pl is not None:
            out.append(pr.band_of(pl, np.float32([0.02, 0.05, 0.3][len(out) % 3])))
    return np.array(out, np.float32)


def _count(selected):
    def kind(c, s, P):
        bands = _bands(s.xyzw)
        sel = s.xyzw[:, 0] >= np.float32(0.1)
        want = pr.counts(s.xyzw[:, :3], bands, sel if selected else None)
        assert want[0] == (sel.sum() if selected else s.n) and want[1] == 0 and (want[2:] > 0).sum() > 30
        if selected:  # (queued in front of the streak's frames: a selection changes no frame)
            assert c.p.select_points(planes=np.float32([[1, 0, 0, -0.1]]))[0] == int(sel.sum())
        yield
        counts, st = c.p.count_in_bands(bands, selected=selected)
        assert np.array_equal(counts, want), np.flatnonzero(counts != want)[:5]
        assert st[0] == (int(sel.sum()) if selected else s.n) and st[1] + st[2] + st[3] == ((s.n + 255) // 256) * len(bands)
        if selected:
            c.p.clear_selection()
        else:
            assert c.p.selection() is None
        yield s, "run"
    return kind


def _fit(dist, iterations, seed):
    def kind(c, s, P):
        want, wst = pr.fit(s.xyzw, np.float32(dist), iterations, seed)
        assert wst[1] > iterations // 2 and wst[0] >= 1
        yield
        plane, inliers, st = c.p.fit_plane(dist, iterations, seed)
        assert np.array_equal(plane.view(np.uint32), want.view(np.uint32)) and st == wst and inliers == wst[0], (plane, st, want, wst)
        assert c.p.selection() is None
        yield s, "run"
    return kind


KINDS = {"count_all": _count(False), "count_selected": _count(True), "fit_3cm": _fit(0.03, 70, 2), "fit_thin": _fit(0, 5, 11)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bands_and_fit_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_fit_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, KINDS["fit_3cm"], ("fit_3cm", "overlap = 1"), mode=1)
    finally:
        c.close()
