"""The k nearest resident points to each GIVEN point (include/rtr.h section 6m) on room_shell and uniform_box at 1e8 points
(the default packed upload with point_ids = 1, since the library may sort the cloud).  tools/nearest_bench.py's scenes,
given sets ("first1e5", "first1e6", "every100th") and radii, 5 cm and 2 cm.  Each leg with k = 1, 8, 16 and 64, with the
given points and the three outputs in host memory ("host": the call copies 8 k + 4 B per given point back) and in device
memory ("device": torch tensors).  Timed with a host clock around the call, which always ends in a synchronise, after one
warm-up call of the same shape, medians of --rounds; beside each median the device time of the call's two stages
("nearest_k_given_us", "nearest_k_sweep_us": the sweep and the unpacking), the chunks skipped and decoded, the pair tests
per given point, the cascades started ("nearest_k_cascades_k": it depends on timing) and the statistics.
The yardstick in the same process: rtr_nearest_points, given side only, on the same context and inputs, alternating with
the call -- the parent commit's closest call, with the same pair tests; both times, their ratio, and the ratio of the two
sweeps' device times are recorded, and per leg the cost of k over k = 1.  The cascades are also given per ACCEPTED pair
where that number is known: the k = 64 leg of the same inputs when none of its rows is full (the sum of found is then
every accepted pair), else null; per entry found they are always given.
The same answer without the call, timed once at --host-n resident points (default 1e6), 1e5 given ones and k = 8:
rtr_extract_points of every point to the host and scipy's cKDTree, query(k, distance_upper_bound=radius) (float64
distances: the rows that differ from the device are counted, the tree is not the contract), else the numpy reference of
tests/nearest_k_ref.py.  The CPU route at 1e8 points was not measured.
  python tools/nearest_k_bench.py [--n N] [--rounds R] [--host-n M] [--out FILE] [--no-host-route] [--scenes a,b] [--ks 1,8,16,64]"""
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
KEYS = ("nearest_k_given_us", "nearest_k_sweep_us", "nearest_k_chunks_skipped", "nearest_k_chunks_decoded", "nearest_k_pair_tests_k",
        "nearest_k_cascades_k")
YARD_KEYS = ("nearest_given_us", "nearest_sweep_us", "nearest_chunks_skipped", "nearest_chunks_decoded", "nearest_pair_tests_k")


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
    ap.add_argument("--ks", default="1,8,16,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_k_bench.json"))
    args = ap.parse_args()
    ks = [int(v) for v in args.ks.split(",")]
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
                m = G.shape[0]
                for kind in ("host", "device"):
                    rows = Gd if kind == "device" else G
                    group = {}
                    for k in ks:
                        name = "%s_%s_r%gcm_k%d_%s" % (scene, gname, radius * 100, k, kind)
                        call = lambda: p.nearest_k_points(rows, k, radius)  # noqa: E731
                        yard = lambda: p.nearest_points(rows, radius)  # noqa: E731
                        call(), yard()  # (warm-up)
                        ms, opts, yms, yopts = [], [], [], []
                        for _ in range(args.rounds):  # the call and its yardstick, alternating
                            t, r = timed(call)
                            ms.append(t)
                            opts.append([p.get_option(key) for key in KEYS])
                            t, y = timed(yard)
                            yms.append(t)
                            yopts.append([p.get_option(key) for key in YARD_KEYS])
                        med, ymed = np.median(np.array(opts), axis=0), np.median(np.array(yopts), axis=0)
                        all_ms[name] = {"call": ms, "nearest_points": yms}
                        legs[name] = float(np.median(ms))
                        st = list(r[3])
                        detail[name] = group[k] = {
                            "nearest_points_ms": float(np.median(yms)), "ratio_to_nearest_points": legs[name] / float(np.median(yms)),
                            "given_ms": float(med[0]) / 1e3, "sweep_ms": float(med[1]) / 1e3,
                            "nearest_points_given_ms": float(ymed[0]) / 1e3, "nearest_points_sweep_ms": float(ymed[1]) / 1e3,
                            "sweep_ratio": float(med[1]) / max(float(ymed[1]), 1.0),
                            "outside_the_stages_ms": legs[name] - float(med[0] + med[1]) / 1e3,
                            "chunks_skipped": int(med[2]), "chunks_decoded": int(med[3]),
                            "pair_tests_per_given_point": float(med[4]) * 1000.0 / m,
                            "nearest_points_pair_tests_per_given_point": float(ymed[4]) * 1000.0 / m,
                            "cascades_k": float(med[5]), "cascades_per_entry_found": float(med[5]) * 1000.0 / max(st[1], 1),
                            "bytes_copied_to_the_host": 0 if kind == "device" else (8 * k + 4) * m,
                            "stats": st, "nearest_points_stats": list(y[2])}
                        assert st[0] == y[2][0] and st[2] == y[2][2], (name, st, y[2])  # (section 6m: the counts agree)
                        del r, y
                    big = group.get(64)
                    pairs = big["stats"][1] if big and big["stats"][3] == 0 else None  # (no row full: every accepted pair was found)
                    for k, d in group.items():
                        d["accepted_pairs"] = pairs
                        d["cascades_per_accepted_pair"] = d["cascades_k"] * 1000.0 / pairs if pairs else None
                        if 1 in group:
                            d["ms_over_k1"] = legs["%s_%s_r%gcm_k%d_%s" % (scene, gname, radius * 100, k, kind)] / \
                                legs["%s_%s_r%gcm_k1_%s" % (scene, gname, radius * 100, kind)]
                            d["sweep_over_k1"] = d["sweep_ms"] / max(group[1]["sweep_ms"], 1e-3)
                        print("%s_%s_r%gcm_k%d_%s" % (scene, gname, radius * 100, k, kind), d, flush=True)
                del Gd
        p.close()
        if args.no_host_route:
            continue
        m = min(args.host_n, args.n)
        q = cloud(scene, SEED, m)
        g = cloud(scene, GIVEN_SEED, m, sorted_ok=False)
        G = np.ascontiguousarray(g.extract_points(first=0, count=min(100_000, m), rgb=False)[0][:, :3])
        g.close()
        radius, k = RADII[0], 8
        dev_ms, dev = timed(lambda: q.nearest_k_points(G, k, radius))
        dev_ms, dev = timed(lambda: q.nearest_k_points(G, k, radius))
        t0 = time.perf_counter()
        xyz = np.ascontiguousarray(q.extract_points(rgb=False)[0][:, :3])
        t1 = time.perf_counter()
        import nearest_k_ref as kf
        if cKDTree is not None:
            tree = cKDTree(xyz)
            t2 = time.perf_counter()
            d, i = tree.query(G, k=k, distance_upper_bound=float(np.float32(radius)), workers=-1)
            d, i = d.reshape(-1, k), i.reshape(-1, k)
            idx = np.where(np.isfinite(d), i, kf.NONE).astype(np.uint32)
            d2 = (d * d).astype(np.float32)
            how = ("scipy cKDTree over the resident points (float64 distances), query(k=%d, distance_upper_bound=radius, workers=-1) of "
                   "every given point" % k)
        else:
            t2 = time.perf_counter()
            idx, d2 = kf.nearest_k_bucket(xyz, G, radius, k)[:2]
            how = "scipy is absent: the numpy bucket reference of tests/nearest_k_ref.py"
        t3 = time.perf_counter()
        exact = kf.nearest_k_bucket(xyz, G, radius, k)
        host[scene] = {"resident_points": m, "given_points": int(G.shape[0]), "k": k, "method": how, "radius": radius,
                       "extract_ms": (t1 - t0) * 1e3, "build_ms": (t2 - t1) * 1e3, "query_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3,
                       "device_ms_same_cloud": dev_ms, "device_stats": list(dev[3]),
                       "rows_where_host_and_device_indices_differ": int((idx != dev[0]).any(axis=1).sum()),
                       "rows_where_host_and_device_distance_bits_differ": int((kf.bits(d2) != kf.bits(dev[1])).any(axis=1).sum()),
                       "rows_where_the_numpy_reference_and_device_differ":
                           int(((exact[0] != dev[0]) | (kf.bits(exact[1]) != kf.bits(dev[1]))).any(axis=1).sum()), "cpus": os.cpu_count()}
        print("host", scene, host[scene], flush=True)
        q.close()

    out = {"config": "%d resident points per scene, default packed upload, point_ids = 1, %d rounds after one warm-up call, each round the "
                     "call and then its yardstick (rtr_nearest_points, given side only, same context and inputs); given sets of the same "
                     "scene with another seed; radii %s m; k %s" % (args.n, args.rounds, list(RADII), ks),
           "cloud": info, "legs_ms": legs, "legs": detail, "host_route": host or None, "cpu_route_at_1e8_points": "not measured",
           "worst_ms": {k: max(v["call"]) for k, v in all_ms.items()}, "all_ms": all_ms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("legs_ms", "host_route")}))


if __name__ == "__main__":
    main()
