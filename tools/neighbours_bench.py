"""Selecting the resident points by neighbour count (include/rtr.h section 6h) on room_shell and uniform_box at 1e8 points
(the default packed upload with point_ids = 1, since the library may sort the cloud): radius 0.05 m with min_neighbours 4 and radius 0.02 m with min_neighbours 2, each leg timed
with a host clock around the call -- which always ends in a synchronise -- after one warm-up call of the same shape,
medians of --rounds; beside each median the device time of the call's stages from the events the call records round them
(rtr_get_option "neighbours_keys_us" / "neighbours_sort_us" / "neighbours_count_us": key sweep; sort, with the wait for
the sweep's counters; gather + work list + count kernel), the call's statistics and its pair tests per point
("neighbours_pair_tests_k").
The same answer without the call, timed once: rtr_extract_points of every point to the host and a CPU neighbour count --
scipy's cKDTree (query_ball_point(..., return_length=True), all cores) where scipy is importable, else the numpy bucket
reference of tests/neighbours_ref.py.  The CPU leg runs on a cloud of --host-n points of the same scene (default: the
numpy route 1e6; cKDTree the whole cloud), in a context of its own whose device answer it must equal within the
tree's float64 distance test (the differing points, if any, are counted and recorded: the tree is not the contract).
  python tools/neighbours_bench.py [--n N] [--rounds R] [--host-n M] [--out FILE] [--no-host-route]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

CASES = ((0.05, 4), (0.02, 2))
KEYS = ("neighbours_keys_us", "neighbours_sort_us", "neighbours_count_us")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=0)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbours_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None

    def cloud(scene, n):
        p = pkg.Projector(0)
        p.set_option("point_ids", 1)  # (the library may sort a cloud on upload: the call then needs its upload order)
        p.generate_synthetic(scene, 0xC0FFEE03, 0, n, n)
        p.synchronize()
        return p

    legs, stages, stats, tests, all_ms, all_us, info, host = {}, {}, {}, {}, {}, {}, {}, {}
    for scene in ("room_shell", "uniform_box"):
        p = cloud(scene, args.n)
        info[scene] = {"packed": p.get_option("packed"), "reordered": p.get_option("reordered")}
        for radius, k in CASES:
            name = "%s_r%gcm_k%d" % (scene, radius * 100, k)
            call = lambda: p.select_neighbours(radius, k)  # noqa: E731
            call()  # (warm-up: the first call allocates the selection, rocPRIM loads its code objects)
            ms, us = [], []
            for _ in range(args.rounds):
                t, r = timed(call)
                ms.append(t)
                us.append([p.get_option(key) for key in KEYS])
            all_ms[name], all_us[name] = ms, us
            legs[name] = float(np.median(ms))
            stages[name] = dict(zip(("keys_ms", "sort_ms", "count_ms"), (float(v) / 1e3 for v in np.median(np.array(us), axis=0))))
            stats[name] = list(r)
            tests[name] = p.get_option("neighbours_pair_tests_k") * 1000.0 / args.n
            print(name, legs[name], stages[name], stats[name], tests[name], flush=True)
        p.close()
        if args.no_host_route:
            continue
        m = args.host_n or (args.n if cKDTree is not None else min(args.n, 1_000_000))
        q = cloud(scene, m)
        radius, k = CASES[0]
        dev_ms, dev = timed(lambda: q.select_neighbours(radius, k))
        dev_ms, dev = timed(lambda: q.select_neighbours(radius, k))
        dev_hit = np.unpackbits(q.download(pkg._lib.BUF_SELECTION).view(np.uint8), bitorder="little")[:m].astype(bool)
        t0 = time.perf_counter()
        xyz = np.ascontiguousarray(q.extract_points(rgb=False)[0][:, :3])
        t1 = time.perf_counter()
        if cKDTree is not None:
            tree = cKDTree(xyz)
            t2 = time.perf_counter()
            cnt = tree.query_ball_point(xyz, float(np.float32(radius)), workers=-1, return_length=True) - 1
            how = "scipy cKDTree (float64 distances), query_ball_point(return_length=True, workers=-1)"
        else:
            import neighbours_ref as nr
            t2 = time.perf_counter()
            cnt = nr.counts_bucket(xyz, radius)
            how = "scipy is absent: the numpy bucket reference of tests/neighbours_ref.py"
        t3 = time.perf_counter()
        hit = cnt >= k
        host[scene] = {"points": m, "method": how, "radius": radius, "min_neighbours": k, "extract_ms": (t1 - t0) * 1e3,
                       "build_ms": (t2 - t1) * 1e3, "count_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3,
                       "device_ms_same_cloud": dev_ms, "device_stats": list(dev), "host_hits": int(hit.sum()),
                       "points_where_host_and_device_differ": int((hit != dev_hit).sum()), "cpus": os.cpu_count()}
        print("host", scene, host[scene], flush=True)
        q.close()

    out = {"config": "%d points per scene, default packed upload, %d rounds after one warm-up call; cases (radius m, min_neighbours): %s"
                     % (args.n, args.rounds, list(CASES)),
           "cloud": info, "legs_ms": legs, "stages_ms": stages, "stats": stats, "pair_tests_per_point": tests,
           "host_route": host or None,
           "worst_ms": {k: max(v) for k, v in all_ms.items()}, "all_ms": all_ms, "all_stage_us": all_us}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("legs_ms", "stages_ms", "stats", "pair_tests_per_point", "host_route")}))


if __name__ == "__main__":
    main()
