"""Estimating the normals and the curvature of the resident points (include/rtr_normals.h section 6o) on room_shell and
uniform_box (the default packed upload with point_ids = 1, since the library may sort the cloud).  Two comparisons, both
timed with a host clock around the call -- every call here ends in a synchronise -- after one warm-up call of the same
shape, with every output in DEVICE memory:

1. THE YARDSTICK, at --n points (default 1e8): radius 0.05 m and 0.02 m, k = 8, 16 and 64, medians of --rounds; beside
   each median the device time of the call's stages from its own events ("normals_us0" .. "normals_us2"), its
   statistics, its pair tests per point and the entries written into rows per point.  Beside every (radius, k), on the
   same context: rtr_select_statistical with the same k and radius -- the same pair tests and a row of one plane --
   timed the same way.  ratio = normals / statistical: what the second plane, the order by index, the second read of the
   neighbours, the fp64 sums and the 24 rotations cost over a mean distance.

2. THE FEATURE, at --route-n points (default 1e7), k = 16, radius 0.05 m: the route that exists for normals -- every
   point extracted into DEVICE memory (rtr_extract_points), rtr_nearest_k_points with k + 1 and its three outputs in
   device memory, then on the device with torch: the own index dropped, the neighbours gathered, the covariances formed
   in float64 and torch.linalg.eigh batched over the points -- against rtr_estimate_normals with normals and curvature
   in device memory, ALTERNATING route, call, route, call, ... for --route-rounds rounds on one context.  Per scene: the
   medians (the route's also split into extract + nearest_k and the torch part), route / call, the run-to-run spread
   (max / min) of either side against itself, and how far the two sets of normals agree (the largest angle between them,
   from the cross product in float64, over the points whose two smallest eigenvalues are well separated).

--parts legs | route | legs,route: which of the two to run; a part that is not run is kept from an existing --out file.

  python tools/normals_bench.py [--n N] [--rounds R] [--route-n M] [--route-rounds Q] [--parts P] [--out FILE]"""
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
KEYS = ("normals_us0", "normals_us1", "normals_us2")
ST_KEYS = ("statistical_us0", "statistical_us1", "statistical_us2")


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
    ap.add_argument("--parts", default="legs,route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    import torch
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def cloud(scene, n):
        p = pkg.Projector(0)
        p.set_option("point_ids", 1)  # (the library may sort a cloud on upload: the call then needs its upload order)
        p.generate_synthetic(scene, 0xC0FFEE03, 0, n, n)
        p.synchronize()
        return p

    def leg(p, n, call, keys, extra):
        call()  # (warm-up: rocPRIM loads its code objects, the kernel's code object is loaded)
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
    parts = set(args.parts.split(","))
    if parts != {"legs", "route"} and os.path.exists(args.out):
        with open(args.out) as fh:
            old = json.load(fh)
        legs, info, route = ({} if "legs" in parts else old["legs"]), old["cloud"], ({} if "route" in parts else old["route"])

    def save():  # (after every piece: a run that is cut short leaves what it measured)
        out = {"config": "%d points per scene, default packed upload, point_ids = 1, %d rounds after one warm-up call, outputs in device memory; "
                         "radii %s m; k %s; statistical: rtr_select_statistical with the same k and radius on the same context; route: "
                         "rtr_extract_points to device memory + rtr_nearest_k_points(k + 1) with device outputs + covariances and "
                         "torch.linalg.eigh in float64 on the device against rtr_estimate_normals with device outputs, alternating for %d "
                         "rounds on %d points, k = 16, radius 0.05 m.  Not measured: any CPU route."
                         % (args.n, args.rounds, list(RADII), list(KS), args.route_rounds, args.route_n),
               "cloud": info, "legs": legs, "route": route}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh)
            fh.write("\n")

    for scene in ("room_shell", "uniform_box") if "legs" in parts else ():
        n = args.n
        p = cloud(scene, n)
        lib, ctx = p._lib, p._ctx
        info[scene] = {"packed": p.get_option("packed"), "reordered": p.get_option("reordered")}
        nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        curv = torch.empty(n, dtype=torch.float32, device="cuda")
        fd = torch.empty(n, dtype=torch.int32, device="cuda")
        md = torch.empty(n, dtype=torch.float32, device="cuda")
        mom, stats = np.zeros(3), np.zeros(4, np.uint64)

        def normals_call(k, radius):
            p._chk(lib.rtr_estimate_normals(ctx, k, radius, 0, None, ptr(nrm), ptr(curv), ptr(fd), vp(stats)))
            return [int(v) for v in stats]

        def statistical_call(k, radius):
            p._chk(lib.rtr_select_statistical(ctx, k, radius, 1.0, 0, 0, ptr(md), ptr(fd), vp(mom), vp(stats)))
            return [int(v) for v in stats]

        for radius in RADII:
            for k in KS:
                name = "%s_r%gcm_k%d" % (scene, radius * 100, k)
                st = leg(p, n, lambda: statistical_call(k, radius), ST_KEYS,
                         {"pair_tests_per_point": "statistical_pair_tests_k", "row_updates_per_point": "statistical_row_updates_k"})
                nm = leg(p, n, lambda: normals_call(k, radius), KEYS,
                         {"pair_tests_per_point": "normals_pair_tests_k", "row_updates_per_point": "normals_row_updates_k"})
                legs[name] = {"normals": nm, "statistical": st, "ratio": nm["ms"] / st["ms"],
                              "third_stage_ratio": nm["stages_ms"]["third_ms"] / st["stages_ms"]["third_ms"]}
                print(name, json.dumps(legs[name]), flush=True)
        del nrm, curv, fd, md
        p.close()
        save()

    # the feature against the route that exists, alternating, on a cloud of --route-n points
    for scene in ("room_shell", "uniform_box") if "route" in parts else ():
        m, k, radius = args.route_n, 16, 0.05
        q = cloud(scene, m)
        lib, ctx = q._lib, q._ctx
        xyz = torch.empty((m, 4), dtype=torch.float32, device="cuda")
        idx = torch.empty((m, k + 1), dtype=torch.int32, device="cuda")
        d2 = torch.empty((m, k + 1), dtype=torch.float32, device="cuda")
        fnd = torch.empty(m, dtype=torch.int32, device="cuda")
        nrm = torch.empty((m, 3), dtype=torch.float32, device="cuda")
        curv = torch.empty(m, dtype=torch.float32, device="cuda")
        stats = np.zeros(4, np.uint64)
        me = torch.arange(m, dtype=torch.int32, device="cuda")[:, None]
        split = []

        def the_route(block=2_000_000):
            t0 = time.perf_counter()
            q.extract_points(out={"xyz": xyz})
            q._chk(lib.rtr_nearest_k_points(ctx, ptr(xyz), 16, m, radius, k + 1, 0, ptr(idx), ptr(d2), ptr(fnd), vp(stats)))
            t1 = time.perf_counter()
            out = torch.zeros((m, 3), dtype=torch.float32, device="cuda")
            lam = torch.zeros((m, 3), dtype=torch.float64, device="cuda")
            for s in range(0, m, block):  # (in blocks: the gathered neighbours of 1e7 points in float64 would take 4 GB)
                e = min(s + block, m)
                ix = idx[s:e]
                real = (torch.arange(k + 1, device="cuda")[None, :] < fnd[s:e, None]) & (ix != me[s:e])  # (the row without the own index)
                pts = xyz[s:e, :3].double()
                nb = xyz[ix.clamp(min=0).long().clamp(max=m - 1)][:, :, :3].double() - pts[:, None, :]
                nb = nb * real[:, :, None]
                cnt = real.sum(dim=1).double() + 1.0
                mean = nb.sum(dim=1) / cnt[:, None]
                cov = torch.einsum("nka,nkb->nab", nb, nb) / cnt[:, None, None] - mean[:, :, None] * mean[:, None, :]
                w, v = torch.linalg.eigh(cov)
                out[s:e] = v[:, :, 0].float()
                lam[s:e] = w
            torch.cuda.synchronize()
            split.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
            return out, lam

        def the_call():
            q._chk(lib.rtr_estimate_normals(ctx, k, radius, 0, None, ptr(nrm), ptr(curv), None, vp(stats)))
            return [int(v) for v in stats]

        the_route(), the_call()
        split.clear()
        r_ms, c_ms = [], []
        for _ in range(args.route_rounds):
            t, (route_n, lam) = timed(the_route)
            r_ms.append(t)
            c_ms.append(timed(the_call)[0])
        # agreement: the angle between the two normals where the fit is well conditioned and the point has a normal
        tr = lam.sum(dim=1)
        good = ((lam[:, 1] - lam[:, 0]) > 1e-3 * tr) & (nrm.abs().sum(dim=1) > 0)
        sine = torch.linalg.cross(route_n.double(), nrm.double()).norm(dim=1).clamp(max=1.0)  # (the two are unit vectors up to fp32 rounding)
        worst = float(torch.asin(sine[good]).max()) if bool(good.any()) else None
        same_bits = int((route_n.view(torch.int32) == nrm.view(torch.int32)).all(dim=1).sum())
        route[scene] = {"points": m, "k": k, "radius": radius, "route_ms": r_ms, "call_ms": c_ms,
                        "route_median_ms": float(np.median(r_ms)), "call_median_ms": float(np.median(c_ms)),
                        "route_extract_nearest_k_median_ms": float(np.median([a for a, _ in split])),
                        "route_torch_median_ms": float(np.median([b for _, b in split])),
                        "route_over_call": float(np.median(r_ms) / np.median(c_ms)),
                        "route_spread_max_over_min": max(r_ms) / min(r_ms), "call_spread_max_over_min": max(c_ms) / min(c_ms),
                        "well_conditioned_points": int(good.sum()), "largest_angle_rad": worst, "normals_with_the_same_bits": same_bits, "stats": [int(v) for v in stats]}
        route[scene]["beats_the_route_by_more_than_the_spread"] = bool(
            route[scene]["route_over_call"] > max(route[scene]["route_spread_max_over_min"], route[scene]["call_spread_max_over_min"]))
        print("route", scene, json.dumps(route[scene]), flush=True)
        del xyz, idx, d2, fnd, nrm, curv, route_n, lam
        q.close()
        save()

    print(json.dumps({"ratio_to_statistical": {name: v["ratio"] for name, v in legs.items()},
                      "route_over_call": {s: v["route_over_call"] for s, v in route.items()}}))


if __name__ == "__main__":
    main()
