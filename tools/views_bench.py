"""Several views in one pass (rtr_render_views, include/rtr.h section 6c) against the same frames rendered by K
sequential rtr_render calls, on the BASELINE C3 cloud (1e8 points, 1920x1080, prefiltered).  Prints one JSON line:
per pose set (stereo pairs, neighbouring orbit poses, disjoint directions) and K = 1, 2, 4, 8 the milliseconds per
batch both ways, their ratio, and the point kernel's (T1) device time per batch / per sequential frame set.
  python tools/views_bench.py [--points N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402  (loads the package from the repository tree)

SEED_C3 = 0xC0FFEE03


def pose_sets(pkg, K, W, H):
    cal = pkg.benchmark_calibration(W, H)
    Kc = cal.getIntrinsicsMatrix()
    out = {}
    # stereo: pairs 6.4 cm apart along the camera's x axis, neighbouring pairs for K > 2
    st = []
    for i in range((K + 1) // 2):
        E = pkg.orbit_pose(100 + i)
        E2 = E.copy()
        E2[0, 3] -= 0.064
        st += [pkg.compose_projection(Kc, E), pkg.compose_projection(Kc, E2)]
    out["stereo"] = st[:K]
    out["orbit"] = [pkg.orbit_projection(100 + i, W, H) for i in range(K)]  # neighbouring poses of the trajectory
    out["disjoint"] = [pkg.orbit_projection(100 + i * 1000 // 8, W, H) for i in range(K)]  # 45 degrees apart
    return {k: np.stack([np.asarray(P, np.float32).reshape(16) for P in v]) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = __graft_entry__.load_package()
    W, H = args.width, args.height
    p = pkg.Projector(0)
    p.generate_synthetic("room_shell", SEED_C3, 0, args.points, args.points)
    p.set_resolution(W, H)

    def t1_us(fn):
        p.synchronize()
        p.timing_enable(2)
        p.timing_reset()
        fn()
        t = p.timing()["min_depth"]
        p.timing_enable(0)
        return 1e3 * t[0], t[1]

    def timed(fn):
        p.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        p.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.reps

    res = {}
    for name in ("stereo", "orbit", "disjoint"):
        for K in (1, 2, 4, 8):
            Ps = pose_sets(pkg, K, W, H)[name]
            batch = lambda: p.render_views(Ps, True)  # noqa: E731

            def seq():
                for P in Ps:
                    p.render(P, True)
            for _ in range(3):  # warm-up: allocation, pools, lean parity, split cool-down
                batch()
                seq()
            b, s = [], []
            for r in range(args.rounds):  # alternating rounds
                if r % 2 == 0:
                    b.append(timed(batch)); s.append(timed(seq))
                else:
                    s.append(timed(seq)); b.append(timed(batch))
            tb, nb = t1_us(batch)
            ts, ns = t1_us(seq)
            res["%s_K%d" % (name, K)] = {
                "ms_per_batch": round(min(b), 4), "ms_sequential": round(min(s), 4),
                "ratio": round(min(b) / min(s), 4),
                "t1_us_batch": round(tb / max(nb, 1), 2), "t1_us_sequential": round(ts / max(ns, 1) * K, 2),
                "t1_launches": [nb, ns]}
    line = json.dumps({"tool": "views_bench", "points": args.points, "W": W, "H": H, "filtered": True,
                       "reps": args.reps, "rounds": args.rounds, "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    p.close()


if __name__ == "__main__":
    main()
