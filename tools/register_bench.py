"""Registering a scan against the resident points (include/rtr_register.h section 6p) on room_shell and uniform_box (the
default packed upload with point_ids = 1, since the library may sort the cloud).  The scan is the first m points of a
SECOND cloud of the same scene (another seed), in device memory.  Two comparisons, both timed with a host clock around the
call -- every call here ends in a synchronise -- after one warm-up call of the same shape:

1. ONE STEP against rtr_nearest_points, given side, at --n resident points (default 1e8): m = 1e5 and 1e6, radius 0.05 m
   and 0.02 m; the same context, the same inputs in device memory, ALTERNATING nearest, point-to-point, point-to-plane for
   --rounds rounds.  rtr_nearest_points is the parent's closest call and makes the same pair tests.  Per leg: the medians,
   the ratios register / nearest, the run-to-run spread (max / min) of every side, the device time of the search's two
   stages from its own events ("nearest_given_us", "nearest_sweep_us": the registration call keeps no timers), what a
   step costs beyond the search (the difference of the medians) and the statistics.  The normals of the plane mode come from one rtr_estimate_normals(16, 0.05) into device memory (not timed).

2. THE LOOP against the route INTEGRATION.md documented until now, at --n resident points and m = 1e6: ten iterations of
   ProjectCloud.registerPoints (point-to-point, scan in device memory) against ten iterations of matchPoints + a numpy
   Kabsch in float64 with the scan re-posed on the host, ALTERNATING for --loop-rounds rounds.  The scan is the second
   cloud moved by a known small motion (register_cases.MOTION's: 2 degrees, 3 cm).  Per scene: both medians, their ratio,
   the spreads, and the difference of the two final poses (rotation angle and translation).

--parts step | loop | step,loop: which of the two to run; a part that is not run is kept from an existing --out file.

  python tools/register_bench.py [--n N] [--rounds R] [--loop-rounds Q] [--parts P] [--scenes S] [--out FILE]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

RADII = (0.05, 0.02)
GIVEN = (100_000, 1_000_000)
NN_KEYS = ("nearest_given_us", "nearest_sweep_us")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def rigid(deg, axis, shift):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    M[:3, 3] = shift
    return M


def kabsch(p, q):
    pb, qb = p.mean(axis=0), q.mean(axis=0)
    U, _, Vt = np.linalg.svd((p - pb).T @ (q - qb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, qb - R @ pb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop-rounds", type=int, default=3)
    ap.add_argument("--parts", default="step,loop")
    ap.add_argument("--scenes", default="room_shell,uniform_box")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    import torch
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    parts, scenes = set(args.parts.split(",")), args.scenes.split(",")
    step, loop, info = {}, {}, {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            old = json.load(fh)
        step, loop, info = old.get("step", {}), old.get("loop", {}), old.get("cloud", {})

    def save():  # (after every piece: a run that is cut short leaves what it measured)
        out = {"config": "%d resident points per scene, default packed upload, point_ids = 1; the scan: the first m points of a second cloud "
                         "of the scene, device memory; step: %d rounds alternating rtr_nearest_points (given side, device outputs), "
                         "rtr_register_points point-to-point and point-to-plane after one warm-up call each, radii %s m, m %s; loop: %d rounds "
                         "alternating 10 iterations of registerPoints against 10 of matchPoints + numpy Kabsch with the scan re-posed on the "
                         "host, m = %d, radius 0.05 m.  Not measured: point-to-plane in the loop, host-memory scans, any CPU route."
                         % (args.n, args.rounds, list(RADII), list(GIVEN), args.loop_rounds, GIVEN[-1]),
               "cloud": info, "step": step, "loop": loop}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh)
            fh.write("\n")

    def second_cloud(scene, m):
        q = pkg.Projector(0)
        q.set_option("point_ids", 1)
        q.generate_synthetic(scene, 0xC0FFEE04, 0, m, m)
        xyz = torch.empty((m, 4), dtype=torch.float32, device="cuda")
        q.extract_points(out={"xyz": xyz})
        q.close()
        return xyz

    for scene in scenes:
        n = args.n
        p = pkg.Projector(0)
        p.set_option("point_ids", 1)  # (the library may sort a cloud on upload: the call then needs its upload order)
        p.generate_synthetic(scene, 0xC0FFEE03, 0, n, n)
        p.synchronize()
        lib, ctx = p._lib, p._ctx
        info[scene] = {"packed": p.get_option("packed"), "reordered": p.get_option("reordered")}
        scan = second_cloud(scene, GIVEN[-1])
        if "step" in parts:
            nrm = p.estimate_normals(16, 0.05, curvature=False, device=True)[0]
            gi = torch.empty(GIVEN[-1], dtype=torch.int32, device="cuda")
            gd = torch.empty(GIVEN[-1], dtype=torch.float32, device="cuda")
            mom, stp, st = np.zeros(32), np.zeros(12), np.zeros(4, np.uint64)
            for m in GIVEN:
                for radius in RADII:
                    def nearest():
                        p._chk(lib.rtr_nearest_points(ctx, ptr(scan), 16, m, radius, 0, ptr(gi), ptr(gd), None, None, vp(st)))
                        return [int(v) for v in st], [p.get_option(k) for k in NN_KEYS]

                    def register(flags):
                        p._chk(lib.rtr_register_points(ctx, ptr(scan), 16, m, radius, flags, None, ptr(nrm) if flags else None, vp(mom), vp(stp), vp(st)))
                        return [int(v) for v in st], None

                    calls = {"nearest": nearest, "point": lambda: register(0), "plane": lambda: register(1)}
                    for fn in calls.values():
                        fn()
                    ms, res = {k: [] for k in calls}, {}
                    for _ in range(args.rounds):
                        for k, fn in calls.items():
                            t, res[k] = timed(fn)
                            ms[k].append(t)
                    med = {k: float(np.median(v)) for k, v in ms.items()}
                    name = "%s_m%d_r%gcm" % (scene, m, radius * 100)
                    step[name] = {"median_ms": med, "all_ms": ms, "spread_max_over_min": {k: max(v) / min(v) for k, v in ms.items()},
                                  "point_over_nearest": med["point"] / med["nearest"], "plane_over_nearest": med["plane"] / med["nearest"],
                                  "stats": {k: r[0] for k, r in res.items()}, "nearest_stage_us": res["nearest"][1],
                                  "beyond_nearest_ms": {"point": med["point"] - med["nearest"], "plane": med["plane"] - med["nearest"]},
                                  "nearest_pair_tests_k": p.get_option("nearest_pair_tests_k")}
                    print(name, json.dumps(step[name]), flush=True)
                    save()
            del nrm, gi, gd
        if "loop" in parts:
            m, radius, its = GIVEN[-1], 0.05, 10
            M = rigid(2.0, (1, 2, 3), (0.02, -0.02, 0.01))
            Mi = np.linalg.inv(M)
            host = scan.cpu().numpy()[:, :3].astype(np.float64)
            c = host.mean(axis=0)
            moved = ((host - c) @ Mi[:3, :3].T + c + Mi[:3, 3]).astype(np.float32)  # (about the scan's middle: a small motion everywhere)
            dev = torch.from_numpy(moved).cuda()
            cloud = pkg.ProjectCloud.__new__(pkg.ProjectCloud)
            cloud._p = p

            def the_call():
                return cloud.registerPoints(dev, radius, iterations=its)

            def the_route():
                pose = np.eye(4)
                for _ in range(its):
                    cur = (moved.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)
                    index, _, xyz, _ = cloud.matchPoints(cur, radius)
                    ok = index != pkg._lib.NEAREST_NONE
                    if ok.sum() < 3:
                        break
                    R, t = kabsch(cur[ok].astype(np.float64), xyz[ok].astype(np.float64))
                    S = np.eye(4)
                    S[:3, :3], S[:3, 3] = R, t
                    pose = S @ pose
                return pose

            the_call(), the_route()
            c_ms, r_ms = [], []
            for _ in range(args.loop_rounds):
                t, (pose_c, rms, st) = timed(the_call)
                c_ms.append(t)
                t, pose_r = timed(the_route)
                r_ms.append(t)
            dR = pose_c[:3, :3].T @ pose_r[:3, :3]
            loop[scene] = {"points": m, "radius": radius, "iterations": its, "calls_made": len(rms), "call_ms": c_ms, "route_ms": r_ms,
                           "call_median_ms": float(np.median(c_ms)), "route_median_ms": float(np.median(r_ms)),
                           "route_over_call": float(np.median(r_ms) / np.median(c_ms)),
                           "call_spread_max_over_min": max(c_ms) / min(c_ms), "route_spread_max_over_min": max(r_ms) / min(r_ms),
                           "rms": [float(v) for v in rms], "stats": list(st),
                           "pose_difference_angle_rad": float(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2)))),
                           "pose_difference_translation_m": float(np.linalg.norm(pose_c[:3, 3] - pose_r[:3, 3]))}
            print("loop", scene, json.dumps(loop[scene]), flush=True)
            del dev
            save()
        del scan
        p.close()
    print(json.dumps({"point_over_nearest": {k: v["point_over_nearest"] for k, v in step.items()},
                      "plane_over_nearest": {k: v["plane_over_nearest"] for k, v in step.items()},
                      "route_over_call": {k: v["route_over_call"] for k, v in loop.items()}}))


if __name__ == "__main__":
    main()
