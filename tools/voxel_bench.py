"""Thinning the resident cloud by a voxel grid (include/rtr.h section 6g) on config C3 (room_shell, 1e8 points, the
default packed upload), every leg timed with a host clock around the call -- which always ends in a synchronise --
after one warm-up call of the same shape, medians of --rounds; beside each median the device time of the call's key
kernel, sort and head kernel from the events the call records round them (rtr_get_option "voxel_keys_us" /
"voxel_sort_us" / "voxel_heads_us"), medians too; every round's figures and the slowest round are kept as well:
  (a) cells of 1 cm, 5 cm and 25 cm x min_count 1 and 3 on the packed cloud;
  (b) the 5 cm cell with pack = 0 (fp32 SoA) and on a cloud the library sorted, with point_ids = 1 (the keys scatter);
  (c) the only route without this call, timed once in the same run: rtr_extract_points of every point to the host, the
      numpy float32 statement of the contract (np.unique over the cell keys), np.packbits, rtr_set_point_keep of the
      words -- its count must equal the device's.
  python tools/voxel_bench.py [--n N] [--rounds R] [--out FILE] [--no-host-route]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

ORIGIN = (0.013, -0.4, 0.0)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def host_thin(xyz, cell, origin):
    """The contract in numpy float32 (min_count 1): bool [n], the first point in upload order of every cell, plus the
    points out of the grid."""
    f = np.float32
    inv = (f(1) / np.broadcast_to(np.asarray(cell, f), (3,))).astype(f)
    with np.errstate(all="ignore"):
        t = xyz - np.asarray(origin, f)[None, :]
        t *= inv[None, :]
        ok = (np.isfinite(t) & (t >= f(-2 ** 20)) & (t < f(2 ** 20))).all(axis=1)
        q = np.floor(t).astype(np.int64)
    q += 2 ** 20
    key = (q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2]
    idx = np.flatnonzero(ok)
    _, first = np.unique(key[idx], return_index=True)
    hit = ~ok
    hit[idx[first]] = True
    return hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    N = args.n

    def cloud(sort=False, **options):
        p = pkg.Projector(0)
        for k, v in options.items():
            p.set_option(k, v)
        p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
        if sort:
            p.reorder_points()
        p.synchronize()
        return p

    legs, stages, stats, all_ms, all_us = {}, {}, {}, {}, {}

    def leg(name, p, cell, min_count=1):
        call = lambda: p.select_voxel_grid(cell, ORIGIN, min_count)  # noqa: E731
        call()  # (warm-up: the first call allocates the selection, rocPRIM loads its code objects)
        ms, us = [], []
        for _ in range(args.rounds):
            t, r = timed(call)
            ms.append(t)
            us.append([p.get_option(k) for k in ("voxel_keys_us", "voxel_sort_us", "voxel_heads_us")])
        all_ms[name], all_us[name] = ms, us
        legs[name] = float(np.median(ms))
        stages[name] = dict(zip(("keys_ms", "sort_ms", "heads_ms"), (float(v) / 1e3 for v in np.median(np.array(us), axis=0))))
        stats[name] = list(r)
        print(name, legs[name], stages[name], stats[name], flush=True)

    p = cloud()
    info = {"packed": p.get_option("packed"), "reordered": p.get_option("reordered"),
            "packed_millibytes_per_point": p.get_option("packed_millibytes_per_point")}
    for cm in (1, 5, 25):
        for mc in (1, 3):
            leg("cell_%dcm_min%d" % (cm, mc), p, cm / 100.0, mc)
    host = None
    if not args.no_host_route:
        parts = {}

        def host_route():  # what a caller without this call has to do
            t0 = time.perf_counter()
            xyz = p.extract_points(rgb=False)[0]
            t1 = time.perf_counter()
            keep = host_thin(np.ascontiguousarray(xyz[:, :3]), 0.05, ORIGIN)
            words = np.packbits(np.concatenate([keep, np.zeros(-keep.size % 32, bool)]), bitorder="little").view("<u4")
            t2 = time.perf_counter()
            p.set_point_keep(words)
            p.synchronize()
            t3 = time.perf_counter()
            parts.update(extract_ms=(t1 - t0) * 1e3, numpy_ms=(t2 - t1) * 1e3, set_keep_ms=(t3 - t2) * 1e3)
            return int(keep.sum())

        ms, picked = timed(host_route)
        p.set_point_keep(None)
        assert picked == stats["cell_5cm_min1"][0], (picked, stats["cell_5cm_min1"])
        host = dict(parts, total_ms=ms, selected=picked)
        print("host_route", host, flush=True)
    p.close()

    q = cloud(pack=0)
    info["pack0_packed"] = q.get_option("packed")
    leg("cell_5cm_min1_pack0", q, 0.05)
    q.close()
    q = cloud(sort=True, point_ids=1)
    info["sorted_reordered"] = q.get_option("reordered")
    leg("cell_5cm_min1_sorted_point_ids", q, 0.05)
    q.close()
    assert stats["cell_5cm_min1_pack0"] == stats["cell_5cm_min1"] == stats["cell_5cm_min1_sorted_point_ids"]

    out = {"config": "C3 room_shell %d points, default packed upload, origin %s, %d rounds after one warm-up call" % (N, ORIGIN, args.rounds),
           "cloud": info, "legs_ms": legs, "stages_ms": stages, "stats": stats, "host_route": host,
           "bars": None if host is None else {"cell_5cm_min1_over_host_route": legs["cell_5cm_min1"] / host["total_ms"]},
           "worst_ms": {k: max(v) for k, v in all_ms.items()}, "all_ms": all_ms, "all_stage_us": all_us}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("legs_ms", "stages_ms", "stats", "host_route", "bars")}))


if __name__ == "__main__":
    main()
