"""Moving points (include/rtr.h section 2d) on config C3 (room_shell, 1920x1080 + prefilter, bench.py's orbit poses),
every leg timed with a host clock around a call that ends in a synchronise, medians of --rounds:
  (a) rtr_transform_points of the whole 1e8 cloud by a small rigid motion, against rtr_upload_points of the moved cloud
      from host arrays in the same run;
  (b) the last appended 1e7 of 1e8 + 1e7 moved, against the append of that block;
  (c) 1e6 contiguous points at index 1e7 of 1e8 (the packed tail behind them moves, undecoded);
  (d) 10 % at random (every chunk touched);
  (e) ms per frame after the whole-cloud and the 1e6 moves, against the moved cloud uploaded in the same resident order,
      alternated in one process (so that drift hits both), and the resident / packed footprints.
  Selections are passed as upload-order words precomputed in host memory (packing a bool array of 1e8 in numpy costs
  more than the move itself).
  python tools/transform_bench.py [--steps K] [--rounds R] [--out FILE]
  python tools/transform_bench.py --one whole|range   one upload and one move (for rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def rigid(k=1):
    a = 0.01 * k
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0, 0.05 * k], [s, c, 0, -0.03 * k], [0, 0, 1, 0.01 * k]], np.float64)


def moved(xyzw, M, sel=None):
    """numpy float32, every product and sum rounded on its own (the library's arithmetic)."""
    m = M.astype(np.float32)
    out = xyzw.copy()
    idx = slice(None) if sel is None else sel
    x, y, z = out[idx, 0].copy(), out[idx, 1].copy(), out[idx, 2].copy()
    for r in range(3):
        out[idx, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    return out


def words_of(sel):
    return np.packbits(np.concatenate([sel, np.zeros(-sel.size % 32, bool)]), bitorder="little").view("<u4").copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--one", choices=("whole", "range"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_transform_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    W, H, N = 1920, 1080, args.n
    tail = N // 10
    total = N + tail
    g = pkg.Projector(0)  # (host arrays: the scene generated on the device, read back in generation order)
    g.set_option("auto_reorder", 0)
    g.generate_synthetic("room_shell", 0xC0FFEE03, 0, total, total)
    xyzw, rgba = g.download_points()
    g.close()
    X, Cc = xyzw[:N], rgba[:N]
    idx = np.arange(N)
    rng_sel = (idx >= N // 10) & (idx < N // 10 + 1_000_000)
    if args.one:
        p = pkg.Projector(0)
        p.upload_points(X, Cc)
        p.synchronize()
        p.transform_points(rigid(), None if args.one == "whole" else rng_sel)
        p.close()
        return

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    legs = {"whole": [], "upload_moved": [], "last_append": [], "append": [], "range_1e6_at_1e7": [], "random_10pct": []}
    # (selection words precomputed in host memory, as tools/remove_bench.py does for its keep words)
    w10 = words_of(np.random.default_rng(10).random(N) < 0.10)
    w_rng = words_of(rng_sel)
    Xw = moved(X, rigid())
    p = pkg.Projector(0)
    p.upload_points(X, Cc)
    for k in range(args.rounds):  # (a) -- the same small motion again each round: the cloud drifts by centimetres
        legs["whole"].append(timed(lambda: p.transform_points(rigid())))
        legs["upload_moved"].append(timed(lambda: p.upload_points(Xw, Cc)))
    p.upload_points(X, Cc)
    for k in range(args.rounds):  # (c), (d)
        legs["range_1e6_at_1e7"].append(timed(lambda: p.transform_points(rigid(), w_rng)))
        legs["random_10pct"].append(timed(lambda: p.transform_points(rigid(), w10)))
    w_tail = words_of(np.arange(total) >= N)
    for k in range(args.rounds):  # (b)
        p.upload_points(X, Cc)
        legs["append"].append(timed(lambda: p.append_points(xyzw[N:], rgba[N:])))
        legs["last_append"].append(timed(lambda: p.transform_points(rigid(), w_tail)))
    p.close()
    del w10, w_tail

    # (e): frames after a move vs the moved cloud uploaded in the same resident order
    ctx = {}
    for name, sel in (("whole", None), ("range", rng_sel)):
        a, b = pkg.Projector(0), pkg.Projector(0)
        for q in (a, b):
            q.set_option("auto_reorder", 0)
            q.set_resolution(W, H)
        a.upload_points(X, Cc)
        a.transform_points(rigid(), sel)
        b.upload_points(Xw if sel is None else moved(X, rigid(), sel), Cc)
        ctx[name] = (a, b)
    poses = [pkg.orbit_projection(k, W, H) for k in range(args.steps)]

    def run(q):
        for P in poses[:5]:
            q.render(P, True)
        q.synchronize()
        t0 = time.perf_counter()
        for P in poses:
            q.render(P, True)
        q.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(poses)

    frame = {"%s_%s" % (name, w): [] for name in ctx for w in ("moved", "uploaded")}
    for _ in range(args.rounds):
        for name, (a, b) in ctx.items():
            frame[name + "_uploaded"].append(run(b))
            frame[name + "_moved"].append(run(a))
    same = all(np.array_equal(a.project(P, filtered=True)[1], b.project(P, filtered=True)[1])
               for a, b in ctx.values() for P in poses[::10])
    mem = {name + "_" + w: {o: q.get_option(o) for o in ("resident_millibytes_per_point", "packed_millibytes_per_point",
                                                          "order_ratio_ppm")}
           for name, (a, b) in ctx.items() for w, q in (("moved", a), ("uploaded", b))}
    for a, b in ctx.values():
        a.close(); b.close()
    med = lambda v: float(np.median(v))  # noqa: E731
    m = {k: med(v) for k, v in legs.items()}
    out = {"config": "C3 room_shell %d points %dx%d prefilter, %d poses x %d rounds" % (N, W, H, args.steps, args.rounds),
           "legs_ms": m,
           "bars": {"whole_over_upload": m["whole"] / m["upload_moved"],
                    "last_append_over_append": m["last_append"] / m["append"],
                    "range_over_whole": m["range_1e6_at_1e7"] / m["whole"],
                    "random_10pct_over_whole": m["random_10pct"] / m["whole"]},
           "ms_per_frame": {k: med(v) for k, v in frame.items()},
           "frame_moved_over_uploaded": {name: med(frame[name + "_moved"]) / med(frame[name + "_uploaded"]) for name in ctx},
           "depth_equal": bool(same), "footprint": mem,
           "all": {"legs_ms": legs, "frame_ms": frame}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("legs_ms", "bars", "ms_per_frame", "frame_moved_over_uploaded", "depth_equal",
                                          "footprint")}))


if __name__ == "__main__":
    main()
