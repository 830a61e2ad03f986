"""Worker of test_gpu_transform.py (one rank of a torch.distributed.run job, both ranks on GPU 0): a point-sharded
cloud, the exchange opened (the "p2p" form opens and verifies it on its first frame, so one frame of the cloud as
generated comes first), then each rank moves part of its own shard by its rank-local indices -- a different transform
and selection on each rank.  The exchange stays open, and the rtr_p2p_render / rtr_p2p_render_owned frames after the
move are checked against the oracle run on the union of the moved shards."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def _moved(xyzw, M, sel):
    m = np.asarray(M, np.float64)[:3].astype(np.float32)
    out = xyzw.copy()
    x, y, z = out[sel, 0].copy(), out[sel, 1].copy(), out[sel, 2].copy()
    for r in range(3):
        out[sel, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    return out


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
    local = pkg.sharded.HipLocal(proj)
    local.bind_stream()
    if form == "owned":
        local.p2p_setup(rank, world, None)
    else:
        sp = pkg.ShardedProjector(local, colour="reduce_scatter", exchange="p2p", check_every=16)
    xyzw, rgba = orc.generate("room_shell", 11, 0, n, n)

    def frame(k, P, filt, xs):
        """Frame k through the exchange; -> None where this rank holds no frame, else whether it equals the oracle's
        frame of (xs, rgba)."""
        owner = k % world
        if form == "owned":
            proj.p2p_render_owned(P, filt, owner)
            if rank != owner:
                proj.synchronize()
                return None
        else:
            sp.render(P, filt)
        ref = orc.project(xs, rgba, P, W, H)
        rd, ri = ref["depth_bits"], ref["img"]
        if filt:
            rf = orc.filter(rd, ri)
            rd, ri = rf["depth"].view(np.uint32), rf["img"]
        return bool(np.array_equal(proj.download(pkg._lib.BUF_DEPTH), rd) and
                    np.array_equal(proj.download(pkg._lib.BUF_IMAGE), ri))

    # one frame of the cloud as generated: the "p2p" form opens (and verifies) the exchange on its first frame
    ok, notes = True, []
    if frame(0, pkg.orbit_projection(0, W, H), False, xyzw) is False:
        ok = False
        notes.append("frame before the move differs on rank %d" % rank)
    opened = proj.get_option("p2p_open")
    # rank 0 re-poses a contiguous scan of its shard, rank 1 a random fifth of its points
    c, s = np.cos(0.1), np.sin(0.1)
    Ms = [np.array([[c, -s, 0, 0.5], [s, c, 0, -0.3], [0, 0, 1, 0.2]]), np.array([[1, 0, 0, -0.7], [0, 1, 0, 0.4], [0, 0, 1, 0]])]
    sels = []
    for r in range(world):
        a, b = pkg.shard_range(n, r, world)
        if r == 0:
            sels.append((np.arange(b - a) >= 20_000) & (np.arange(b - a) < 90_000))
        else:
            sels.append(np.random.default_rng(7 + r).random(b - a) < 0.2)
    proj.transform_points(Ms[rank % 2], sels[rank])
    still_open = proj.get_option("p2p_open")
    for r in range(world):
        a, b = pkg.shard_range(n, r, world)
        xyzw[a:b] = _moved(xyzw[a:b], Ms[r % 2], sels[r])
    if not (opened == 1 and still_open == 1):
        ok = False
        notes.append("p2p_open %d -> %d" % (opened, still_open))
    for k in range(1, 5):
        if frame(k, pkg.orbit_projection(130 * k, W, H), k % 2 == 1, xyzw) is False:
            ok = False
            notes.append("frame %d differs on rank %d" % (k, rank))
    if form == "p2p" and sp.exchange != "p2p":  # (the frames after the move came through the exchange itself)
        ok = False
        notes.append("the exchange was dropped: %s" % sp.p2p_note)
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
