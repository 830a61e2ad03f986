"""Frames that overflow the adaptive extent pool (include/rtr.h, option "pool_worst_case" = 0, the default), shared by
tests/test_gpu_pool_overflow.py and the child process that runs its sharded case (`python pool_overflow_scenes.py
sharded <colour>`).

A fresh cloud of n points gets max(n / 2, 2^20) pool entries; the whole cloud inside one 32 x 16 tile needs ~2 n.
- first-frame overflow: P_ONE (focal length 1 px, principal point (8, 8), camera 20 m back) is the first frame after
  the upload.
- late overflow: ORDINARY orbit frames size the pool first (8 x the most entries a frame had: ~1.8 M entries), then
  P_ONE, whose in-frustum count (all n) exceeds that; there are more of them than the split launch's grace period
  after an upload (8 frames), so the overflowing frame also runs after the split launch has been switched off."""
import os
import sys

import numpy as np

N, W, H = 2_000_000, 640, 480
SEED = 0xC0FFEE0B
ORDINARY = (0, 7, 100, 250, 600, 800, 0, 7, 100, 250)
WORST_MB = 16_000   # resident_millibytes_per_point once the pool holds 2 n entries (16 B per point)
JUMP_MB = 6_000     # the growth to that from an adaptive pool (4 B per point fresh, ~7.3 after ORDINARY)


def cloud(orc):
    return orc.generate("room_shell", SEED, 0, N, N)


def p_one(orc, cx=8.0):
    K = np.array([[1.0, 0, cx], [0, 1.0, 8.0], [0, 0, 1]])  # everything within a pixel of (cx, 8)
    E = np.eye(4)
    E[2, 3] = 20.0
    return orc.compose_projection(K, E), K, E


def check_poses(pkg, orc, xyzw):
    """The poses do what the scenarios need: P_ONE sees the whole cloud, more than the pool the ordinary frames size."""
    P = p_one(orc)[0]
    accepted = orc.envelope_points(xyzw, P, W, H, 0, 0)["accepted"]
    ordinary = max(orc.envelope_points(xyzw, pkg.orbit_projection(k, W, H), W, H, 0, 0)["accepted"] for k in ORDINARY)
    assert accepted == N and ordinary > 0
    assert accepted > 8 * ordinary and accepted > max(N // 2, 1 << 20), (accepted, ordinary)
    assert len(ORDINARY) > 8


def footprint(p):
    return p.get_option("resident_millibytes_per_point")


def prepare(pkg, orc, p, xyzw, rgba, scenario, options=(), sort=False):
    """Options, upload, resolution; for "late" the ordinary frames (checked against the oracle).  -> the footprint the
    overflowing frame starts from."""
    for k, v in dict(options).items():
        p.set_option(k, v)
    p.upload_points(xyzw, rgba)
    if sort:
        p.reorder_points()
        assert p.get_option("reordered") == 1
    p.set_resolution(W, H)
    assert p.get_option("pool_worst_case") == 0
    if scenario == "late":
        for k in ORDINARY:
            P = pkg.orbit_projection(k, W, H)
            img, depth = p.project(P)
            if k == ORDINARY[-1]:
                ref = orc.project(xyzw, rgba, P, W, H)
                assert np.array_equal(depth.view(np.uint32), ref["depth_bits"]) and np.array_equal(img, ref["img"])
        no_errors(p)
    else:
        assert scenario == "first"
    return footprint(p)


def no_errors(p):
    """frame_stats()["errors"] == 0 for a binned frame (the atomic form keeps no statistics)."""
    if p.get_option("mode") != 0:
        assert p.frame_stats()["errors"] == 0


def assert_overflowed(p, before, what=""):
    """The precondition of every test: the frame really overflowed the adaptive pool, which has grown to the worst case."""
    after = footprint(p)
    assert after >= WORST_MB and after - before >= JUMP_MB, ("the pool did not grow: no overflow", what, before, after)


def sharded_child(colour):
    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as entry
    pkg, orc = entry.load_package(), entry.load_oracle()
    orc.build()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29547")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        xyzw, rgba = cloud(orc)
        P = p_one(orc)[0]
        ref = orc.project(xyzw, rgba, P, W, H)
        rf = orc.filter(ref["depth_bits"], ref["img"])
        L = pkg._lib
        for scenario in ("first", "late"):
            p = pkg.Projector(0)
            try:
                before = prepare(pkg, orc, p, xyzw, rgba, scenario)
                loc = pkg.sharded.HipLocal(p)
                loc.bind_stream()
                sp = pkg.ShardedProjector(loc, colour=colour, force_exchange=True)
                sp.render(P, with_filter=True)
                torch.cuda.synchronize()
                assert_overflowed(p, before, (colour, scenario))
                assert np.array_equal(p.download(L.BUF_DEPTH), rf["depth"].view(np.uint32)), (colour, scenario, "depth")
                assert np.array_equal(p.download(L.BUF_IMAGE), rf["img"]), (colour, scenario, "image")
                assert np.array_equal(p.download(L.BUF_TENSOR).reshape(5, H, W), rf["tensor"]), (colour, scenario, "tensor")
                no_errors(p)
                # the next frame of the same cloud is exact too (the pool stays worst-case sized)
                P2 = pkg.orbit_projection(3, W, H)
                sp.render(P2, with_filter=False)
                torch.cuda.synchronize()
                r2 = orc.project(xyzw, rgba, P2, W, H)
                assert np.array_equal(p.download(L.BUF_DEPTH), r2["depth_bits"]), (colour, scenario, "next frame")
                assert np.array_equal(p.download(L.BUF_IMAGE), r2["img"]), (colour, scenario, "next frame")
            finally:
                p.close()
    finally:
        dist.destroy_process_group()
    print("sharded %s ok" % colour)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "sharded":
        sharded_child(sys.argv[2])
    else:
        sys.exit("usage: pool_overflow_scenes.py sharded <allreduce | reduce_scatter>")
