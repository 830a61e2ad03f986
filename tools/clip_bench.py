"""Clip planes on config C3 (room_shell, 1e8 points, 1920x1080 + prefilter, bench.py's orbit poses): ms per frame of
six legs measured in ONE process, each clipped leg alternated with the no-planes leg (a) so that drift hits both.
  (a) no planes; (b) one plane that keeps the whole cloud; (c) an axis box enclosing the whole cloud (6 planes);
  (d) a plane that cuts the in-frustum part about in half; (e) a crop box keeping ~1/8 of the room; (f) an overview
  from above with the ceiling clipped away.
T1's own time: run under `rocprofv3 --kernel-trace --stats` (k_project_bin<...> vs k_project_bin<..., rtr::Clip> rows).
  python tools/clip_bench.py [--steps K] [--rounds R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def overview_from_above(pkg, W, H):
    """A camera 9 m above the room centre looking straight down (world y is 'down' for the orbit camera: it looks along
    +y from y = -9)."""
    cal = pkg.benchmark_calibration(W, H)
    R = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])  # camera z = world +y, camera y = world -z
    c = np.array([0.0, -9.0, 0.0])
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ c
    return pkg.compose_projection(cal.getIntrinsicsMatrix(), E)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_clip_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    W, H, N = 1920, 1080, args.n
    p = pkg.Projector(0)
    p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
    p.set_resolution(W, H)
    poses = [pkg.orbit_projection(k, W, H) for k in range(args.steps)]
    f = np.float32
    legs = {
        "b_keep_all_plane": (f([[0, 0, 1, 100]]), poses),
        "c_enclosing_box": (pkg.clip_box_planes([-4.5, -2.0, -4.5], [4.5, 2.0, 4.5]), poses),
        "d_half_plane": (f([[1, 0, 0, 0]]), poses),
        "e_crop_eighth": (pkg.clip_box_planes([0.0, -1.5, 0.0], [4.0, 0.0, 4.0]), poses),
        "f_overview_no_ceiling": (f([[0, 1, 0, 1.2]]), [overview_from_above(pkg, W, H)] * args.steps),
    }

    def run(planes, ps):
        p.set_clip_planes(planes)
        for P in ps[:5]:
            p.render(P, True)
        p.synchronize()
        t0 = time.perf_counter()
        for P in ps:
            p.render(P, True)
        p.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(ps)

    res = {k: {"ms": [], "base_ms": []} for k in legs}
    for _ in range(args.rounds):
        for name, (planes, ps) in legs.items():
            base_ps = ps
            res[name]["base_ms"].append(run(None, base_ps))
            res[name]["ms"].append(run(planes, ps))
    stats = {}
    for name, (planes, ps) in legs.items():
        p.set_clip_planes(planes)
        p.project(ps[0])
        st = p.frame_stats()
        p.set_clip_planes(None)
        p.project(ps[0])
        st0 = p.frame_stats()
        r = res[name]
        stats[name] = {"planes": int(len(planes)), "ms_per_frame": float(np.median(r["ms"])),
                       "no_planes_ms_per_frame": float(np.median(r["base_ms"])),
                       "ratio": float(np.median(r["ms"]) / np.median(r["base_ms"])),
                       "ms_all": r["ms"], "no_planes_ms_all": r["base_ms"],
                       "entries": int(st["entries"]), "no_planes_entries": int(st0["entries"]),
                       "colour_chunks": int(st["colour_chunks"]), "no_planes_colour_chunks": int(st0["colour_chunks"])}
    out = {"config": "C3 room_shell %d points %dx%d prefilter, %d poses x %d rounds" % (N, W, H, args.steps, args.rounds),
           "legs": stats}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: (round(v["ms_per_frame"], 4), round(v["no_planes_ms_per_frame"], 4), round(v["ratio"], 3))
                      for k, v in stats.items()}))
    p.close()


if __name__ == "__main__":
    main()
