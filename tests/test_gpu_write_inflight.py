"""rtr_write_points behind an overlapped streak that is still in flight (include/rtr.h section 2f, "Ordering"): the
engine of test_gpu_inflight_streak.py -- an unplugged streak, the same streak behind a plug (streak_ctx.Ctx.run_plugged),
`not event.query()` asserted directly in front of the call, then the write of both streams.  The queued frames equal the
oracle's on the OLD cloud, the resident cloud read back equals the host statement (write_ref.written), and the next
streak equals the oracle's on the NEW cloud."""
import numpy as np
import pytest

import test_gpu_inflight_streak as inflight
import write_ref
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


def _write(name, sel_of, device):
    def kind(c, s, P):
        sel = sel_of(s.n)
        k = s.n if sel is None else int(sel.sum())
        rng = np.random.default_rng(k)
        lo, hi = s.xyzw[:, :3].min(0), s.xyzw[:, :3].max(0)
        X = rng.uniform(lo, hi, (k, 3)).astype(np.float32)  # (inside the room: the streak's poses see the new points)
        C = rng.integers(0, 256, (k, 3), dtype=np.uint8)
        x1, c1, idx = write_ref.written(s.xyzw, s.rgba, sel, 0, X, C)
        new = s.but(name, xyzw=x1, rgba=c1)
        src_x, src_c = X, C
        if device:
            import torch
            src_x = torch.from_numpy(X).to(torch.device("cuda", 0))
            torch.cuda.synchronize()
        yield
        assert c.p.write_points(src_x, src_c, sel) == idx.size == k, name
        inflight._resident_is(c, new, name)
        yield new, "run"
    return kind


KINDS = {"write_all_host": _write("write_all_host", lambda n: None, False),
         "write_random_mixed": _write("write_random_mixed", lambda n: np.random.default_rng(11).random(n) < 0.3, True),
         "write_last_chunks": _write("write_last_chunks", lambda n: np.arange(n) >= n - 700, True)}


@pytest.mark.parametrize("m", [3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_write_behind_a_streak_in_flight(pkg, scenes, kind, m):
    scene = scenes("96x64")
    c = Ctx(pkg, scene)
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, m, KINDS[kind], (kind, m))
    finally:
        c.close()


def test_write_behind_a_streak_with_explicit_overlap(pkg, scenes):
    scene = scenes("208x112")
    c = Ctx(pkg, scene, {"overlap": 1})
    try:
        s = inflight.State.base(scene)
        inflight._warm_up(c, s)
        inflight.plugged_step(c, s, 3, KINDS["write_random_mixed"], ("write_random_mixed", "overlap = 1"), mode=1)
    finally:
        c.close()
