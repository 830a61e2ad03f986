"""Selecting resident points (include/rtr.h section 6f) on config C3 (room_shell, 1e8 points, the default packed upload,
1920x1080), every leg timed with a host clock around a call that ends in a synchronise, medians of --rounds:
  (a) the octant box (lo = min - 1, hi = centre + 0.013) with stats, against the only route without this call, timed in
      the same run: rtr_download_points of the cloud, camera.clip_keep in numpy, np.packbits, rtr_set_point_keep;
  (b) a selection that keeps everything / nothing (the box paths alone), the full-frame rectangle, every op other than
      REPLACE on the octant box, the same with pack = 0, the popcount pass on its own (a call with no region and op ADD |
      OUTSIDE changes nothing and counts), and ProjectCloud-style removeSelected of a 10 % slab against rtr_remove_points
      from host words.
  python tools/select_bench.py [--n N] [--rounds R] [--out FILE]
  python tools/select_bench.py --one box|rect|frame   one upload and ten calls (for rocprofv3 --kernel-trace --stats;
                                                      frame: ten frames with a point pass each, the kernel to compare with)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--one", choices=("box", "rect", "frame"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_select_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    L = pkg._lib
    W, H, N = 1920, 1080, args.n
    P = pkg.orbit_projection(3, W, H)

    def cloud(**options):
        p = pkg.Projector(0)
        for k, v in options.items():
            p.set_option(k, v)
        p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
        p.set_resolution(W, H)
        p.synchronize()
        return p

    p = cloud()
    # the octant box from the cloud's extent (100 slices spread over the generation order: every wall is hit)
    step = max(N // 100, 1)
    sample = np.concatenate([p.download_points(k * step, min(10_000, N - k * step))[0] for k in range(min(100, N))])
    lo = sample[:, :3].min(axis=0) - 1
    hi = (sample[:, :3].min(axis=0) + sample[:, :3].max(axis=0)) / 2 + np.float32(0.013)
    box = pkg.clip_box_planes(lo, hi)
    if args.one:
        for _ in range(10):
            if args.one == "box":
                p.select_points(planes=box)
            elif args.one == "rect":
                p.select_points(P=P, rect=(0, 0, W, H))
            else:
                p.render(P, True)
                p.point_pass(P, ids=False, visible=True)
                p.synchronize()
        p.close()
        return

    legs, stats = {}, {}

    def leg(name, fn):
        ms = []
        for _ in range(args.rounds):
            t, r = timed(fn)
            ms.append(t)
        legs[name] = ms
        if isinstance(r, tuple) and r[0] is not None:
            stats[name] = r

    p.select_points(planes=box)  # (allocates the buffer)
    leg("octant_box", lambda: p.select_points(planes=box))
    leg("octant_box_no_stats_then_sync", lambda: (p.select_points(planes=box, stats=False), p.synchronize()))
    leg("keep_all", lambda: p.select_points(planes=np.float32([[0, 0, 1, 100]])))
    leg("keep_none", lambda: p.select_points(planes=np.float32([[0, 0, 1, -100]])))
    leg("full_frame_rect", lambda: p.select_points(P=P, rect=(0, 0, W, H)))
    for op in ("add", "subtract", "intersect", "toggle"):
        leg("octant_box_" + op, lambda: p.select_points(planes=box, op=op))
    leg("popcount_only", lambda: p.select_points(op="add", outside=True))
    n_chunks = (N + 255) // 256

    def host_route():  # what a caller without this call has to do
        xyzw, _ = p.download_points()
        keep = pkg.clip_keep(box, xyzw)
        words = np.packbits(np.concatenate([keep, np.zeros(-keep.size % 32, bool)]), bitorder="little").view("<u4")
        p.set_point_keep(words)
        return int(keep.sum())

    ms, picked = timed(host_route)
    legs["host_route"] = [ms]
    p.set_point_keep(None)
    assert picked == p.select_points(planes=box)[0]

    # removeSelected of a slab of ~10 % against rtr_remove_points from host words
    x = np.sort(sample[:, 0])
    slab = np.float32([[1, 0, 0, -x[int(0.45 * x.size)]], [-1, 0, 0, x[int(0.55 * x.size)]]])
    rm_dev, rm_host = [], []
    for _ in range(args.rounds):
        def remove_selected():
            p.select_points(planes=slab, stats=False)
            p.select_points(op="toggle", stats=False)
            p.remove_points(p.selection())
        t, _ = timed(remove_selected)
        rm_dev.append(t)
        removed = N - p.num_points
        p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
        p.select_points(planes=slab, outside=True)
        words = p.download(L.BUF_SELECTION)
        t, _ = timed(lambda: p.remove_points(words))
        rm_host.append(t)
        p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
    legs["remove_selected_slab"], legs["remove_points_host_words_slab"] = rm_dev, rm_host
    p.close()

    q = cloud(pack=0)
    q.select_points(planes=box)
    ms = []
    for _ in range(args.rounds):
        t, r = timed(lambda: q.select_points(planes=box))
        ms.append(t)
    legs["octant_box_pack0"], stats["octant_box_pack0"] = ms, r
    q.close()

    med = {k: float(np.median(v)) for k, v in legs.items()}
    out = {"config": "C3 room_shell %d points %dx%d, %d rounds" % (N, W, H, args.rounds), "chunks": n_chunks,
           "legs_ms": med, "stats": {k: list(v) for k, v in stats.items()},
           "bars": {"octant_box_over_host_route": med["octant_box"] / med["host_route"]},
           "removed_slab_points": int(removed), "all": legs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("legs_ms", "stats", "bars", "removed_slab_points")}))


if __name__ == "__main__":
    main()
