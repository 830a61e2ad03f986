"""Worker of test_gpu_point_keep.py (one rank of a torch.distributed.run job, both ranks on GPU 0): a point-sharded
cloud rendered with rtr_p2p_render / rtr_p2p_render_owned while each rank holds its own keep mask, in its own
rank-local indices, and a different one on each rank; the frames are checked against the oracle run on the subset of
the whole cloud that the two masks keep."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    form = sys.argv[1]
    W, H, n = 320, 240, 300_000
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    pkg, orc = entry.load_package(), entry.load_oracle()
    proj = pkg.Projector(0)
    lo, hi = pkg.shard_range(n, rank, world)
    proj.generate_synthetic("room_shell", 11, lo, hi - lo, n)
    proj.set_resolution(W, H)
    # rank 0 hides a random tenth of its points, rank 1 every fourth one and a contiguous stretch
    keep = np.ones(n, bool)
    keep[:n // 2] = np.random.default_rng(5).random(n // 2) >= 0.1
    i = np.arange(n // 2, n)
    keep[n // 2:] = (i % 4 != 1) & ((i < 200_000) | (i >= 250_000))
    assert pkg.shard_range(n, 0, world)[1] == n // 2
    proj.set_point_keep(keep[lo:hi])
    local = pkg.sharded.HipLocal(proj)
    local.bind_stream()
    xyzw, rgba = orc.generate("room_shell", 11, 0, n, n)
    xyzw, rgba = xyzw[keep], rgba[keep]
    ok, notes = True, []
    if form == "owned":
        local.p2p_setup(rank, world, None)
    else:
        sp = pkg.ShardedProjector(local, colour="reduce_scatter", exchange="p2p", check_every=16)
    for k in range(4):
        P = pkg.orbit_projection(130 * k, W, H)
        filt = k % 2 == 1
        owner = k % world
        if form == "owned":
            proj.p2p_render_owned(P, filt, owner)
            if rank != owner:
                proj.synchronize()
                continue
        else:
            sp.render(P, filt)
        ref = orc.project(xyzw, rgba, P, W, H)
        rd, ri = ref["depth_bits"], ref["img"]
        if filt:
            rf = orc.filter(rd, ri)
            rd, ri = rf["depth"].view(np.uint32), rf["img"]
        if not (np.array_equal(proj.download(pkg._lib.BUF_DEPTH), rd) and np.array_equal(proj.download(pkg._lib.BUF_IMAGE), ri)):
            ok = False
            notes.append("frame %d differs on rank %d" % (k, rank))
    out = {"rank": rank, "ok": ok, "notes": notes, "timeouts": proj.p2p_timeouts()}
    gathered = [None] * world
    dist.all_gather_object(gathered, out)
    if rank == 0:
        print(json.dumps(gathered), flush=True)
    dist.barrier()
    proj.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
