"""Times rtr_point_pass on config C3 (1e8-point room_shell, 1920x1080, filtered frames) for a rocprofv3 kernel trace:
   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/point_pass_profile.py [--reordered]
--reordered: the cloud is Morton-sorted with option point_ids = 1 first (the permutation form of the pass).
Prints the pass's own device time (hipEvents around --steps passes) as one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reordered", action="store_true")
    a = ap.parse_args()
    pkg = entry.load_package()
    W, H = 1920, 1080
    p = pkg.Projector(0)
    if a.reordered:
        p.set_option("point_ids", 1)
    p.generate_synthetic("room_shell", 0xC0FFEE03, 0, a.points, a.points)  # (bench.py's C3 cloud)
    if a.reordered:
        p.reorder_points()
    p.set_resolution(W, H)
    P = pkg.orbit_projection(0, W, H)
    for _ in range(3):
        p.render(P, True)
        p.point_pass(P)
    p.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        p.render(P, True)
        p.point_pass(P)
    p.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    ids = p.download(pkg._lib.BUF_POINT_ID)
    lit = int((ids != pkg._lib.NO_POINT).sum())
    print(json.dumps({"points": a.points, "reordered": bool(p.get_option("reordered")), "packed": p.get_option("packed"),
                      "ms_per_frame_plus_pass": round(ms, 4), "pixels_with_id": lit}))
    p.close()


if __name__ == "__main__":
    main()
