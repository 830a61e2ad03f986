"""The nearest resident point to each GIVEN point (include/rtr.h section 6l) on room_shell and uniform_box at 1e8 points
(the default packed upload with point_ids = 1, since the library may sort the cloud).  tools/near_bench.py's scenes,
given sets -- the first 1e5 and the first 1e6 points of the same scene generated with another seed ("first1e5",
"first1e6": what the generator emits in a row, like a scan) and every 100th point ("every100th": scattered over the whole
map) -- and radii, 5 cm and 2 cm.  Each leg three times: the given side only ("given") and both sides ("both") with the
given points and every output in host memory -- the call then copies its arrays to the host, 8 B per given point and,
with both sides, 8 B per RESIDENT point, which the yardstick does not --, and both sides with the given points and the
outputs in device memory ("both_device": torch tensors, nothing of size n crosses the bus).  Timed with a host clock
around the call, which always ends in a synchronise, after one warm-up call of the same shape, medians of --rounds;
beside each median the device time of the call's two stages from the events it records ("nearest_given_us": key, sort and
gather of the given points; "nearest_sweep_us": the sweep and the unpacking), the chunks decided without their
coordinates and decoded, the pair tests per given point and the statistics.
The yardstick in the same process: rtr_select_near with near words on the same context and inputs, alternating with the
call -- the parent commit's closest call, with the same pair tests and no early exit; both times, their ratio, and the
ratio of the two sweeps' device times are recorded.
The same answer without the call, timed once at --host-n resident points (default 1e6) and 1e5 given ones:
rtr_extract_points of every point to the host and scipy's cKDTree over the resident points, query(k=1,
distance_upper_bound=radius) of the given ones (float64 distances: the given points where index or distance bits differ
from the device are counted and recorded, the tree is not the contract), else the numpy reference of
tests/nearest_ref.py.  The CPU route at 1e8 points was not measured.
  python tools/nearest_bench.py [--n N] [--rounds R] [--host-n M] [--out FILE] [--no-host-route] [--scenes a,b]"""
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
SEED, GIVEN_SEED = 0xC0FFEE03, 0xC0FFEE04  # (near_bench.py's)
KEYS = ("nearest_given_us", "nearest_sweep_us", "nearest_chunks_skipped", "nearest_chunks_decoded", "nearest_pair_tests_k")
YARD_KEYS = ("near_given_us", "near_sweep_us", "near_chunks_skipped", "near_chunks_decoded", "near_pair_tests_k")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_bench.json"))
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

    import torch
    legs, detail, info, host, all_ms = {}, {}, {}, {}, {}
    for scene in args.scenes.split(","):
        sets = given_sets(scene, args.n)
        p = cloud(scene, SEED, args.n)
        info[scene] = {"packed": p.get_option("packed"), "reordered": p.get_option("reordered"),
                       "given": {k: int(v.shape[0]) for k, v in sets.items()}}
        for radius in RADII:
            for gname, G in sets.items():
                Gd = torch.from_numpy(G).cuda()
                for kind in ("given", "both", "both_device"):
                    name = "%s_%s_r%gcm_%s" % (scene, gname, radius * 100, kind)
                    both, rows = kind != "given", Gd if kind == "both_device" else G
                    call = lambda: p.nearest_points(rows, radius, resident=both)  # noqa: E731
                    yard = lambda: p.select_near(rows, radius, near=True)  # noqa: E731
                    call(), yard()  # (warm-up: the first call allocates the selection, rocPRIM loads its code objects)
                    ms, opts, yms, yopts = [], [], [], []
                    for _ in range(args.rounds):  # the call and its yardstick, alternating
                        t, r = timed(call)
                        ms.append(t)
                        opts.append([p.get_option(key) for key in KEYS])
                        t, y = timed(yard)
                        yms.append(t)
                        yopts.append([p.get_option(key) for key in YARD_KEYS])
                    med, ymed = np.median(np.array(opts), axis=0), np.median(np.array(yopts), axis=0)
                    all_ms[name] = {"call": ms, "select_near": yms}
                    legs[name] = float(np.median(ms))
                    m = G.shape[0]
                    detail[name] = {
                        "select_near_ms": float(np.median(yms)), "ratio_to_select_near": legs[name] / float(np.median(yms)),
                        "given_ms": float(med[0]) / 1e3, "sweep_ms": float(med[1]) / 1e3,
                        "select_near_given_ms": float(ymed[0]) / 1e3, "select_near_sweep_ms": float(ymed[1]) / 1e3,
                        "sweep_ratio": float(med[1]) / max(float(ymed[1]), 1.0),
                        "outside_the_stages_ms": legs[name] - float(med[0] + med[1]) / 1e3,
                        "select_near_outside_the_stages_ms": float(np.median(yms)) - float(ymed[0] + ymed[1]) / 1e3,
                        "chunks_skipped": int(med[2]), "chunks_decoded": int(med[3]),
                        "pair_tests_per_given_point": float(med[4]) * 1000.0 / m,
                        "select_near_pair_tests_per_given_point": float(ymed[4]) * 1000.0 / m,
                        "bytes_copied_to_the_host": 0 if kind == "both_device" else 8 * m + (8 * args.n if both else 0),
                        "stats": list(r[-1]), "select_near_stats": list(y[0])}
                    assert r[-1][0] == y[0][2] and r[-1][1] == y[0][1], (name, r[-1], y[0])  # (section 6l: the counts agree)
                    print(name, legs[name], detail[name], flush=True)
        p.close()
        if args.no_host_route:
            continue
        m = min(args.host_n, args.n)
        q = cloud(scene, SEED, m)
        g = cloud(scene, GIVEN_SEED, m, sorted_ok=False)
        G = np.ascontiguousarray(g.extract_points(first=0, count=min(100_000, m), rgb=False)[0][:, :3])
        g.close()
        radius = RADII[0]
        dev_ms, dev = timed(lambda: q.nearest_points(G, radius))
        dev_ms, dev = timed(lambda: q.nearest_points(G, radius))
        t0 = time.perf_counter()
        xyz = np.ascontiguousarray(q.extract_points(rgb=False)[0][:, :3])
        t1 = time.perf_counter()
        import nearest_ref as nf
        if cKDTree is not None:
            tree = cKDTree(xyz)
            t2 = time.perf_counter()
            d, i = tree.query(G, k=1, distance_upper_bound=float(np.float32(radius)), workers=-1)
            idx = np.where(np.isfinite(d), i, nf.NONE).astype(np.uint32)
            d2 = (d * d).astype(np.float32)
            how = ("scipy cKDTree over the resident points (float64 distances), query(k=1, distance_upper_bound=radius, workers=-1) of "
                   "every given point")
        else:
            t2 = time.perf_counter()
            idx, d2 = nf.nearest_bucket(xyz, G, radius)[:2]
            how = "scipy is absent: the numpy bucket reference of tests/nearest_ref.py"
        t3 = time.perf_counter()
        exact = nf.nearest_bucket(xyz, G, radius)
        host[scene] = {"resident_points": m, "given_points": int(G.shape[0]), "method": how, "radius": radius,
                       "extract_ms": (t1 - t0) * 1e3, "build_ms": (t2 - t1) * 1e3, "query_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3,
                       "device_ms_same_cloud": dev_ms, "device_stats": list(dev[2]),
                       "given_points_where_host_and_device_indices_differ": int((idx != dev[0]).sum()),
                       "given_points_where_host_and_device_distance_bits_differ": int((nf.bits(d2) != nf.bits(dev[1])).sum()),
                       "given_points_where_the_numpy_reference_and_device_differ":
                           int(((exact[0] != dev[0]) | (nf.bits(exact[1]) != nf.bits(dev[1]))).sum()), "cpus": os.cpu_count()}
        print("host", scene, host[scene], flush=True)
        q.close()

    out = {"config": "%d resident points per scene, default packed upload, point_ids = 1, %d rounds after one warm-up call, each round the "
                     "call and then its yardstick (rtr_select_near with near words, same context and inputs); given sets of the same scene "
                     "with another seed; radii %s m" % (args.n, args.rounds, list(RADII)),
           "cloud": info, "legs_ms": legs, "legs": detail, "host_route": host or None, "cpu_route_at_1e8_points": "not measured",
           "worst_ms": {k: max(v["call"]) for k, v in all_ms.items()}, "all_ms": all_ms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("legs_ms", "host_route")}))


if __name__ == "__main__":
    main()
