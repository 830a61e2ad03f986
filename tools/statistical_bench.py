"""Selecting the resident points by mean neighbour distance (include/rtr_statistics.h section 6n) on room_shell and
uniform_box (the default packed upload with point_ids = 1, since the library may sort the cloud).  Two comparisons, both
timed with a host clock around the call -- every call here ends in a synchronise -- after one warm-up call of the same
shape:

1. THE PAIR TESTS, at --n points (default 1e8): radius 0.05 m and 0.02 m, k = 8, 16 and 64, medians of --rounds; beside
   each median the device time of the call's stages from its own events ("statistical_us0" .. "statistical_us2"), its
   statistics, its pair tests per point and the values written into rows per point.  Beside every radius, on the same
   context: rtr_select_neighbours with min_neighbours = 2^32 - 1 -- its early exit never fires, so it makes the same pair
   tests -- timed the same way.  ratio = statistical / neighbours: what the rows, the sort, the sums and the hits cost over
   a count.

2. THE FEATURE, at --route-n points (default 1e7), k = 8, radius 0.05 m: the route section 6m documents for the k nearest
   neighbours of the resident points themselves -- rtr_extract_points of every point into DEVICE memory, then
   rtr_nearest_k_points with k + 1 and its three outputs in device memory; the host pass that drops the own index and
   averages is NOT timed, in the route's favour -- against rtr_select_statistical with mean_dist and found in device
   memory, ALTERNATING route, call, route, call, ... for --route-rounds rounds on one context.  Per scene: the medians,
   route / call, and the run-to-run spread (max / min) of either side against itself.  The call has earned its place
   where route / call exceeds the larger of the two spreads.

  python tools/statistical_bench.py [--n N] [--rounds R] [--route-n M] [--route-rounds Q] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

RADII = (0.05, 0.02)
KS = (8, 16, 64)
KEYS = ("statistical_us0", "statistical_us1", "statistical_us2")
NB_KEYS = ("neighbours_keys_us", "neighbours_sort_us", "neighbours_count_us")
NO_EXIT = 2 ** 32 - 1


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--route-n", type=int, default=10_000_000)
    ap.add_argument("--route-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statistical_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    import torch

    def cloud(scene, n):
        p = pkg.Projector(0)
        p.set_option("point_ids", 1)  # (the library may sort a cloud on upload: the call then needs its upload order)
        p.generate_synthetic(scene, 0xC0FFEE03, 0, n, n)
        p.synchronize()
        return p

    def leg(p, n, call, keys, extra):
        call()  # (warm-up: the first call allocates the selection, rocPRIM loads its code objects)
        ms, us = [], []
        for _ in range(args.rounds):
            t, r = timed(call)
            ms.append(t)
            us.append([p.get_option(key) for key in keys])
        stage = dict(zip(("keys_ms", "sort_ms", "third_ms"), (float(v) / 1e3 for v in np.median(np.array(us), axis=0))))
        out = {"ms": float(np.median(ms)), "stages_ms": stage, "result": r, "all_ms": ms, "all_stage_us": us}
        out.update({name: p.get_option(key) * 1000.0 / n for name, key in extra.items()})
        return out

    legs, info, route = {}, {}, {}
    for scene in ("room_shell", "uniform_box"):
        p = cloud(scene, args.n)
        info[scene] = {"packed": p.get_option("packed"), "reordered": p.get_option("reordered")}
        for radius in RADII:
            nb = leg(p, args.n, lambda: list(p.select_neighbours(radius, NO_EXIT)), NB_KEYS, {"pair_tests_per_point": "neighbours_pair_tests_k"})
            for k in KS:
                name = "%s_r%gcm_k%d" % (scene, radius * 100, k)
                st = leg(p, args.n, lambda: [list(v) for v in p.select_statistical(k, radius)], KEYS,
                         {"pair_tests_per_point": "statistical_pair_tests_k", "row_updates_per_point": "statistical_row_updates_k"})
                legs[name] = {"statistical": st, "neighbours_no_exit": nb, "ratio": st["ms"] / nb["ms"],
                              "third_stage_ratio": st["stages_ms"]["third_ms"] / nb["stages_ms"]["third_ms"]}
                print(name, json.dumps(legs[name]), flush=True)
        p.close()

        # the feature against the documented route, alternating, on a cloud of --route-n points
        m, k, radius = args.route_n, 8, 0.05
        q = cloud(scene, m)
        lib, ctx = q._lib, q._ctx
        xyz = torch.empty((m, 4), dtype=torch.float32, device="cuda")
        idx = torch.empty((m, k + 1), dtype=torch.int32, device="cuda")
        d2 = torch.empty((m, k + 1), dtype=torch.float32, device="cuda")
        fnd = torch.empty(m, dtype=torch.int32, device="cuda")
        md = torch.empty(m, dtype=torch.float32, device="cuda")
        fd = torch.empty(m, dtype=torch.int32, device="cuda")
        mom, stats = np.zeros(3), np.zeros(4, np.uint64)
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

        def the_route():
            q.extract_points(out={"xyz": xyz})
            q._chk(lib.rtr_nearest_k_points(ctx, ptr(xyz), 16, m, radius, k + 1, 0, ptr(idx), ptr(d2), ptr(fnd), vp(stats)))
            return [int(v) for v in stats]

        def the_call():
            q._chk(lib.rtr_select_statistical(ctx, k, radius, 1.0, 0, 0, ptr(md), ptr(fd), vp(mom), vp(stats)))
            return [int(v) for v in stats]

        the_route(), the_call()
        r_ms, c_ms = [], []
        for _ in range(args.route_rounds):
            r_ms.append(timed(the_route)[0])
            c_ms.append(timed(the_call)[0])
        # the same rows from both: found of the call = min(k, found of the route - 1) wherever the route found the point itself
        same = bool(torch.equal(fd, torch.clamp(fnd - 1, min=0, max=k)))
        route[scene] = {"points": m, "k": k, "radius": radius, "route_ms": r_ms, "call_ms": c_ms,
                        "route_median_ms": float(np.median(r_ms)), "call_median_ms": float(np.median(c_ms)),
                        "route_over_call": float(np.median(r_ms) / np.median(c_ms)),
                        "route_spread_max_over_min": max(r_ms) / min(r_ms), "call_spread_max_over_min": max(c_ms) / min(c_ms),
                        "found_agree": same, "moments": list(mom), "stats": [int(v) for v in stats]}
        route[scene]["beats_the_route_by_more_than_the_spread"] = bool(
            route[scene]["route_over_call"] > max(route[scene]["route_spread_max_over_min"], route[scene]["call_spread_max_over_min"]))
        print("route", scene, json.dumps(route[scene]), flush=True)
        del xyz, idx, d2, fnd, md, fd
        q.close()

    out = {"config": "%d points per scene, default packed upload, point_ids = 1, %d rounds after one warm-up call; radii %s m; k %s; "
                     "neighbours_no_exit: rtr_select_neighbours with min_neighbours = 2^32 - 1 on the same context; route: "
                     "rtr_extract_points to device memory + rtr_nearest_k_points(k + 1) with device outputs against "
                     "rtr_select_statistical with device outputs, alternating for %d rounds on %d points, k = 8, radius 0.05 m"
                     % (args.n, args.rounds, list(RADII), list(KS), args.route_rounds, args.route_n),
           "cloud": info, "legs": legs, "route": route}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({"pair_tests_ratio": {name: v["ratio"] for name, v in legs.items()},
                      "route_over_call": {s: v["route_over_call"] for s, v in route.items()}}))


if __name__ == "__main__":
    main()
