"""Selecting the resident points by smooth segment (include/rtr_segments.h section 6q) against selecting them by
connected cluster (include/rtr.h section 6i) on room_shell and uniform_box at 1e8 points (the default packed upload with
point_ids = 1, since the library may sort the cloud): radius 0.05 m and 0.02 m with min_points 50.  Per leg the normals
are estimated once (rtr_estimate_normals, k = 16, the leg's radius, no viewpoint) into DEVICE memory and not timed; then
rtr_select_segments (cos_angle = cos 15 degrees as a float32, no curvature limit) and rtr_select_clusters ALTERNATE on
the same context with the same radius and window, each timed with a host clock around the call -- which always ends in a
synchronise -- after one warm-up call of either: medians of --rounds with the smallest and the largest round beside
them, the ratio of the medians, and both calls' statistics ([3]: the points of the largest segment / cluster).  The
cluster call is the yardstick: both run the same pair tests; the segment call adds one gather and 16 B per point, three
broadcasts and five fp32 operations per test, and makes different unions.  The segment call has no option keys, so
there are no stage times for it; the cluster call's are recorded.
  python tools/segments_bench.py [--n N] [--rounds R] [--out FILE]"""
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
K = 16
COS_ANGLE = np.float32(0.9659258)
KEYS = ("clusters_keys_us", "clusters_sort_us", "clusters_label_us")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    legs, info = {}, {}
    for scene in ("room_shell", "uniform_box"):
        p = pkg.Projector(0)
        p.set_option("point_ids", 1)  # (the library may sort a cloud on upload: the calls then need its upload order)
        p.generate_synthetic(scene, 0xC0FFEE03, 0, args.n, args.n)
        p.synchronize()
        info[scene] = {"packed": p.get_option("packed"), "reordered": p.get_option("reordered")}
        for radius, lo in CASES:
            name = "%s_r%gcm_min%d" % (scene, radius * 100, lo)
            normals_ms, (normals, est) = timed(lambda: p.estimate_normals(K, radius, curvature=False, device=True))

            def segments():
                return p.select_segments(radius, COS_ANGLE, normals, min_points=lo)

            def clusters():
                return p.select_clusters(radius, lo)

            segments(), clusters()  # (warm-up: the first call allocates the selection, rocPRIM loads its code objects)
            ms = {"segments": [], "clusters": []}
            stage_us = []
            for _ in range(args.rounds):
                t, sg_stats = timed(segments)
                ms["segments"].append(t)
                t, cl_stats = timed(clusters)
                ms["clusters"].append(t)
                stage_us.append([p.get_option(key) for key in KEYS])
            med = {k: float(np.median(v)) for k, v in ms.items()}
            legs[name] = {"segments_ms": med["segments"], "clusters_ms": med["clusters"], "ratio": med["segments"] / med["clusters"],
                          "segments_min_max_ms": [min(ms["segments"]), max(ms["segments"])],
                          "clusters_min_max_ms": [min(ms["clusters"]), max(ms["clusters"])],
                          "segments_stats": list(sg_stats), "clusters_stats": list(cl_stats),
                          "largest_segment": sg_stats[3], "largest_cluster": cl_stats[3],
                          "clusters_stages_ms": dict(zip(("keys_ms", "sort_ms", "third_ms"), (float(v) / 1e3 for v in np.median(np.array(stage_us), axis=0)))),
                          "pair_tests_per_point": p.get_option("clusters_pair_tests_k") * 1000.0 / args.n,
                          "normals_ms_not_in_the_ratio": normals_ms, "normals_stats": list(est), "all_ms": ms}
            print(name, json.dumps(legs[name]), flush=True)
            del normals
        p.close()
    out = {"config": "%d points per scene, default packed upload, point_ids = 1, %d rounds after one warm-up call of either, the two calls "
                     "alternating on one context; cases (radius m, min_points): %s; normals: rtr_estimate_normals k = %d at the leg's radius into "
                     "device memory, once per leg, not timed into the ratio; cos_angle %r, no curvature limit.  Not measured: a curvature limit, "
                     "host-memory inputs (they add two uploads of 16 B per point), ORIENTED, any CPU route."
                     % (args.n, args.rounds, list(CASES), K, float(COS_ANGLE)),
           "cloud": info, "legs": legs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({name: {k: v[k] for k in ("segments_ms", "clusters_ms", "ratio", "largest_segment", "largest_cluster")} for name, v in legs.items()}))


if __name__ == "__main__":
    main()
