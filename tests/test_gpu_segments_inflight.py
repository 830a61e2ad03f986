"""rtr_select_segments behind an overlapped streak that is still in flight (include/rtr_segments.h section 6q, "the
ordering and the waits"): the engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug
(streak_ctx.Ctx.run_plugged), `not event.query()` asserted directly in front of the call, then the call, which queues
behind the streak and waits for it.  The queued frames equal the oracle's, the words, the labels and the statistics
equal the reference (segments_ref.py) -- with the normals and the curvature in host and in device memory --, and the
next streak equals the oracle's on the same cloud."""
import numpy as np
import pytest

import clusters_ref as cr
import normals_ref as nref
import segments_cases as sc
import segments_ref as sg
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


_inputs, _labels = {}, {}


def _segments(radius, max_curvature, lo, hi, op, outside, device):
    def kind(c, s, P):
        import torch
        L = c.pkg._lib
        key = (s.n, radius)
        if key not in _inputs:
            est = nref.estimate(s.xyzw, radius, 12)
            _inputs[key] = (est["normals"], est["curvature"], cr.pairs(s.xyzw, radius))
        normals, curvature, near = _inputs[key]
        if key + (max_curvature,) not in _labels:
            _labels[key + (max_curvature,)] = sg.labels(s.xyzw, radius, sc.COS_ANGLE, normals, None if max_curvature is None else curvature,
                                                        np.inf if max_curvature is None else max_curvature, near=near)
        lab = _labels[key + (max_curvature,)]
        hit = sg.hits(lab, lo, hi)
        ref = sg.stats(lab, hit)
        assert 0.02 * s.n < hit.sum() < 0.98 * s.n and ref[0] >= 20
        want = hit != outside  # (replace, toggle and add alike: no selection before it)
        nrm, curv = normals, None if max_curvature is None else curvature
        if device:  # (uploaded before the plug: the copies are not what is in flight)
            nrm = torch.from_numpy(nrm).to("cuda:0")
            curv = None if curv is None else torch.from_numpy(curv).to("cuda:0")
            torch.cuda.synchronize()
        yield
        st, got = c.p.select_segments(radius, sc.COS_ANGLE, nrm, curv, np.inf if max_curvature is None else max_curvature, lo, hi, op=op,
                                      outside=outside, labels=True)
        assert st == (int(want.sum()),) + ref, (st, ref)
        assert np.array_equal(c.p.download(L.BUF_SELECTION), sg.words(want))
        assert np.array_equal(got, lab)
        c.p.clear_selection()
        yield s, "run"
    return kind


KINDS = {"faces_host": _segments(0.09, None, 50, 0, "replace", False, False),
         "small_toggled_device": _segments(0.09, None, 2, 49, "toggle", True, True),
         "smooth_add_device": _segments(0.09, 0.02, 50, 0, "add", False, True)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_segments_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_segments_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, _segments(0.06, 0.02, 50, 0, "replace", False, False), ("6cm_smooth_50", "overlap = 1"), mode=1)
    finally:
        c.close()
