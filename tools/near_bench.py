"""Selecting the resident points within a radius of GIVEN points (include/rtr.h section 6k) on room_shell and uniform_box
at 1e8 points (the default packed upload with point_ids = 1, since the library may sort the cloud).  The given sets come
from the same scene generated with another seed: the first 1e5 and the first 1e6 points of its generation order
("first1e5", "first1e6": what the scene's generator emits in a row, like a scan) and every 100th point ("every100th":
scattered over the whole map, the worst case for box rejection).  Radii 5 cm and 2 cm, each leg with and without the
near words, timed with a host clock around the call -- which always ends in a synchronise -- after one warm-up call of
the same shape, medians of --rounds; beside each median the device time of the call's two stages from the events it
records ("near_given_us": key, sort and gather of the given points; "near_sweep_us": the resident sweep, combine and
count), the chunks decided without their coordinates and decoded, the pair tests per given point and the statistics.
The yardstick in the same process: rtr_select_neighbours(radius, 1) on the same context, alternating with the call -- the
cost of gridding the WHOLE cloud, as the parent commit has it.  It is NOT the same answer; the ratio is recorded.
The same answer without the call, timed once at --host-n resident points (default 1e6) and 1e5 given ones:
rtr_extract_points of every point to the host and scipy's cKDTree over the given points (float64 distances: the points
where it differs from the device are counted and recorded, the tree is not the contract), else the numpy reference of
tests/near_ref.py, whose hits must be identical.  The CPU route at 1e8 points was not measured.
  python tools/near_bench.py [--n N] [--rounds R] [--host-n M] [--out FILE] [--no-host-route] [--scenes a,b]"""
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

RADII = (0.05, 0.02)
SEED, GIVEN_SEED = 0xC0FFEE03, 0xC0FFEE04
KEYS = ("near_given_us", "near_sweep_us", "near_chunks_skipped", "near_chunks_decoded", "near_pair_tests_k")


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
    ap.add_argument("--scenes", default="room_shell,uniform_box")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "near_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None

    def cloud(scene, seed, n, sorted_ok=True):
        p = pkg.Projector(0)
        p.set_option("point_ids", 1)  # (the library may sort a cloud on upload: the call then needs its upload order)
        if not sorted_ok:
            p.set_option("auto_reorder", 0)
        p.generate_synthetic(scene, seed, 0, n, n)
        p.synchronize()
        return p

    def given_sets(scene, n):
        """name -> float32 (m, 3): cut out of the scene generated with the other seed, in its generation order."""
        q = cloud(scene, GIVEN_SEED, n, sorted_ok=False)
        sets = {}
        for name, m in (("first1e5", min(100_000, n)), ("first1e6", min(1_000_000, n))):
            sets[name] = np.ascontiguousarray(q.extract_points(first=0, count=m, rgb=False)[0][:, :3])
        mask = np.zeros(n, bool)
        mask[::100] = True
        sets["every100th"] = np.ascontiguousarray(q.extract_points(select=mask, rgb=False)[0][:, :3])
        q.close()
        return sets

    legs, detail, yard, info, host, all_ms = {}, {}, {}, {}, {}, {}
    for scene in args.scenes.split(","):
        sets = given_sets(scene, args.n)
        p = cloud(scene, SEED, args.n)
        info[scene] = {"packed": p.get_option("packed"), "reordered": p.get_option("reordered"),
                       "given": {k: int(v.shape[0]) for k, v in sets.items()}}
        for radius in RADII:
            yard_ms = []
            for gname, G in sets.items():
                for near in (False, True):
                    name = "%s_%s_r%gcm_%s" % (scene, gname, radius * 100, "near" if near else "hits")
                    call = lambda: p.select_near(G, radius, near=near)  # noqa: E731
                    call()  # (warm-up: the first call allocates the selection, rocPRIM loads its code objects)
                    ms, opts = [], []
                    for _ in range(args.rounds):
                        t, r = timed(call)
                        ms.append(t)
                        opts.append([p.get_option(key) for key in KEYS])
                        if gname == "first1e5" and not near:  # the yardstick, alternating with the call
                            yard_ms.append(timed(lambda: p.select_neighbours(radius, 1))[0])
                    st = r[0] if near else r
                    med = np.median(np.array(opts), axis=0)
                    all_ms[name] = ms
                    legs[name] = float(np.median(ms))
                    detail[name] = {"given_ms": float(med[0]) / 1e3, "sweep_ms": float(med[1]) / 1e3, "chunks_skipped": int(med[2]),
                                    "chunks_decoded": int(med[3]), "pair_tests_per_given_point": float(med[4]) * 1000.0 / G.shape[0],
                                    "stats": list(st)}
                    print(name, legs[name], detail[name], flush=True)
            yname = "%s_r%gcm" % (scene, radius * 100)
            yard[yname] = {"select_neighbours_k1_ms": float(np.median(yard_ms)), "all_ms": yard_ms}
            for gname in sets:
                for kind in ("hits", "near"):
                    leg = "%s_%s_r%gcm_%s" % (scene, gname, radius * 100, kind)
                    detail[leg]["ratio_to_select_neighbours"] = legs[leg] / yard[yname]["select_neighbours_k1_ms"]
            print("yardstick", yname, yard[yname], flush=True)
        p.close()
        if args.no_host_route:
            continue
        m = min(args.host_n, args.n)
        q = cloud(scene, SEED, m)
        g = cloud(scene, GIVEN_SEED, m, sorted_ok=False)
        G = np.ascontiguousarray(g.extract_points(first=0, count=min(100_000, m), rgb=False)[0][:, :3])
        g.close()
        radius = RADII[0]
        dev_ms, dev = timed(lambda: q.select_near(G, radius, near=True))
        dev_ms, dev = timed(lambda: q.select_near(G, radius, near=True))
        dev_hit = np.unpackbits(q.download(pkg._lib.BUF_SELECTION).view(np.uint8), bitorder="little")[:m].astype(bool)
        t0 = time.perf_counter()
        xyz = np.ascontiguousarray(q.extract_points(rgb=False)[0][:, :3])
        t1 = time.perf_counter()
        if cKDTree is not None:
            tree = cKDTree(G)
            t2 = time.perf_counter()
            d, _ = tree.query(xyz, k=1, distance_upper_bound=float(np.float32(radius)) * (1 + 1e-6), workers=-1)
            hit = d <= float(np.float32(radius))
            how = "scipy cKDTree over the given points (float64 distances), query(k=1, workers=-1) of every resident point"
        else:
            import near_ref as nr
            t2 = time.perf_counter()
            hit, _ = nr.near_bucket(xyz, G, radius)
            how = "scipy is absent: the numpy bucket reference of tests/near_ref.py"
        t3 = time.perf_counter()
        import near_ref as nr
        exact, _ = nr.near_bucket(xyz, G, radius)
        host[scene] = {"resident_points": m, "given_points": int(G.shape[0]), "method": how, "radius": radius,
                       "extract_ms": (t1 - t0) * 1e3, "build_ms": (t2 - t1) * 1e3, "query_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3,
                       "device_ms_same_cloud": dev_ms, "device_stats": list(dev[0]), "host_hits": int(hit.sum()),
                       "points_where_host_and_device_differ": int((hit != dev_hit).sum()),
                       "points_where_the_numpy_reference_and_device_differ": int((exact != dev_hit).sum()), "cpus": os.cpu_count()}
        print("host", scene, host[scene], flush=True)
        q.close()

    out = {"config": "%d resident points per scene, default packed upload, point_ids = 1, %d rounds after one warm-up call; given sets of "
                     "the same scene with another seed; radii %s m" % (args.n, args.rounds, list(RADII)),
           "cloud": info, "legs_ms": legs, "legs": detail, "yardstick": yard, "host_route": host or None,
           "cpu_route_at_1e8_points": "not measured",
           "worst_ms": {k: max(v) for k, v in all_ms.items()}, "all_ms": all_ms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("legs_ms", "yardstick", "host_route")}))


if __name__ == "__main__":
    main()
