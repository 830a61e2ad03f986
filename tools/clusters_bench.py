"""Selecting the resident points by connected cluster (include/rtr.h section 6i) on room_shell and uniform_box at 1e8
points (the default packed upload with point_ids = 1, since the library may sort the cloud): radius 0.05 m and 0.02 m with
min_points 50, each leg timed with a host clock around the call -- which always ends in a synchronise -- after one
warm-up call of the same shape, medians of --rounds; beside each median the device time of the call's stages from the
events the call records round them (rtr_get_option "clusters_keys_us" / "clusters_sort_us" / "clusters_label_us": key
sweep; sort, with the wait for the sweep's counters; gather + work list + union-find + flatten + hits), the call's
statistics and its pair tests per point ("clusters_pair_tests_k").
Beside every leg, on the same context, cloud and radius: rtr_select_neighbours with min_neighbours = 2^31 -- no early
exit, every candidate pair tested from both sides -- timed the same way; the difference between the two calls' third
stages is what the union-find costs over a count.
The same answer without the call, timed once ON A CLOUD OF --host-n POINTS (default 1e6; not the 1e8 of the legs):
rtr_extract_points of every point to the host, scipy's cKDTree.query_pairs and scipy.sparse.csgraph.connected_components
(skipped where scipy is not importable), against the device call in a context of its own on that cloud; the points whose
cluster differs are counted and recorded (the tree tests float64 distances: it is not the contract).
  python tools/clusters_bench.py [--n N] [--rounds R] [--host-n M] [--out FILE] [--no-host-route]"""
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

CASES = ((0.05, 50), (0.02, 50))
KEYS = ("clusters_keys_us", "clusters_sort_us", "clusters_label_us")
NB_KEYS = ("neighbours_keys_us", "neighbours_sort_us", "neighbours_count_us")
NO_EXIT = 2 ** 31


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=1_000_000)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clusters_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()

    def cloud(scene, n):
        p = pkg.Projector(0)
        p.set_option("point_ids", 1)  # (the library may sort a cloud on upload: the call then needs its upload order)
        p.generate_synthetic(scene, 0xC0FFEE03, 0, n, n)
        p.synchronize()
        return p

    def leg(p, call, keys, tests_key):
        call()  # (warm-up: the first call allocates the selection, rocPRIM loads its code objects)
        ms, us = [], []
        for _ in range(args.rounds):
            t, r = timed(call)
            ms.append(t)
            us.append([p.get_option(key) for key in keys])
        stage = dict(zip(("keys_ms", "sort_ms", "third_ms"), (float(v) / 1e3 for v in np.median(np.array(us), axis=0))))
        return {"ms": float(np.median(ms)), "stages_ms": stage, "stats": list(r),
                "pair_tests_per_point": p.get_option(tests_key) * 1000.0 / args.n, "all_ms": ms, "all_stage_us": us}

    legs, info, host = {}, {}, {}
    for scene in ("room_shell", "uniform_box"):
        p = cloud(scene, args.n)
        info[scene] = {"packed": p.get_option("packed"), "reordered": p.get_option("reordered")}
        for radius, k in CASES:
            name = "%s_r%gcm_min%d" % (scene, radius * 100, k)
            cl = leg(p, lambda: p.select_clusters(radius, k), KEYS, "clusters_pair_tests_k")
            nb = leg(p, lambda: p.select_neighbours(radius, NO_EXIT), NB_KEYS, "neighbours_pair_tests_k")
            legs[name] = {"clusters": cl, "neighbours_no_exit": nb, "ratio": cl["ms"] / nb["ms"],
                          "third_stage_difference_ms": cl["stages_ms"]["third_ms"] - nb["stages_ms"]["third_ms"]}
            print(name, json.dumps({k2: v for k2, v in legs[name].items()}), flush=True)
        p.close()
        if args.no_host_route:
            continue
        try:
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
            from scipy.spatial import cKDTree
        except ImportError:
            continue
        m = min(args.host_n, args.n)
        q = cloud(scene, m)
        radius, k = CASES[0]
        q.select_clusters(radius, k)
        dev_ms, (dev, dev_lab) = timed(lambda: q.select_clusters(radius, k, labels=True))
        t0 = time.perf_counter()
        xyz = np.ascontiguousarray(q.extract_points(rgb=False)[0][:, :3])
        t1 = time.perf_counter()
        tree = cKDTree(xyz)
        t2 = time.perf_counter()
        pairs = tree.query_pairs(float(np.float32(radius)), output_type="ndarray")
        t3 = time.perf_counter()
        ncomp, comp = connected_components(coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(m, m)),
                                           directed=False)
        size = np.bincount(comp)[comp]
        t4 = time.perf_counter()
        first = np.full(ncomp, m, np.int64)
        np.minimum.at(first, comp, np.arange(m))
        host[scene] = {"points": m, "method": "scipy cKDTree.query_pairs (float64 distances) + csgraph.connected_components, one process",
                       "radius": radius, "min_points": k, "extract_ms": (t1 - t0) * 1e3, "build_ms": (t2 - t1) * 1e3,
                       "pairs_ms": (t3 - t2) * 1e3, "components_ms": (t4 - t3) * 1e3, "total_ms": (t4 - t0) * 1e3,
                       "pairs": int(len(pairs)), "device_ms_same_cloud": dev_ms, "device_stats": list(dev),
                       "host_clusters": int(ncomp), "host_hits": int((size >= k).sum()),
                       "points_whose_label_differs": int((first[comp] != dev_lab).sum()), "cpus": os.cpu_count()}
        print("host", scene, host[scene], flush=True)
        q.close()

    out = {"config": "%d points per scene, default packed upload, %d rounds after one warm-up call; cases (radius m, min_points): %s; "
                     "neighbours_no_exit: rtr_select_neighbours with min_neighbours = 2^31 on the same context; host route on %d points only"
                     % (args.n, args.rounds, list(CASES), min(args.host_n, args.n)),
           "cloud": info, "legs": legs, "host_route": host or None}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({name: {"clusters_ms": v["clusters"]["ms"], "neighbours_no_exit_ms": v["neighbours_no_exit"]["ms"], "ratio": v["ratio"]}
                      for name, v in legs.items()}))


if __name__ == "__main__":
    main()
