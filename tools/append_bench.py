"""Appending points (include/rtr.h section 2b) on config C3 (room_shell, 1920x1080 + prefilter, bench.py's orbit poses):
  (a) wall time of rtr_upload_points of 1e8 + m points from host arrays, for m in {1e5, 1e6, 1e7};
  (b) wall time of rtr_append_points of m points onto a resident 1e8;
  (c) ms per frame of a 1e8 cloud built as 1e7 + nine appends of 1e7, alternated with the one-shot cloud in one
      process (so that drift hits both);
  (d) resident_millibytes_per_point of both.
  python tools/append_bench.py [--steps K] [--rounds R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_append_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    W, H, N = 1920, 1080, args.n
    ms = (100_000, 1_000_000, 10_000_000)
    total = N + max(ms)
    g = pkg.Projector(0)  # (host arrays: the scene generated on the device, read back in generation order)
    g.set_option("auto_reorder", 0)
    g.generate_synthetic("room_shell", 0xC0FFEE03, 0, total, total)
    xyzw, rgba = g.download_points()
    g.close()

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    upload_ms, append_ms = {}, {}
    p = pkg.Projector(0)
    for m in ms:
        upload_ms[m] = [timed(lambda: p.upload_points(xyzw[:N + m], rgba[:N + m])) for _ in range(args.rounds)]
        append_ms[m] = []
        for _ in range(args.rounds):
            p.upload_points(xyzw[:N], rgba[:N])
            append_ms[m].append(timed(lambda: p.append_points(xyzw[N:N + m], rgba[N:N + m])))
    p.close()

    step = N // 10
    a = pkg.Projector(0)
    a.upload_points(xyzw[:step], rgba[:step])
    for lo in range(step, N, step):
        a.append_points(xyzw[lo:lo + step], rgba[lo:lo + step])
    b = pkg.Projector(0)
    b.upload_points(xyzw[:N], rgba[:N])
    poses = [pkg.orbit_projection(k, W, H) for k in range(args.steps)]
    for q in (a, b):
        q.set_resolution(W, H)

    def run(q):
        for P in poses[:5]:
            q.render(P, True)
        q.synchronize()
        t0 = time.perf_counter()
        for P in poses:
            q.render(P, True)
        q.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(poses)

    frame = {"appended": [], "one_shot": []}
    for _ in range(args.rounds):
        frame["one_shot"].append(run(b))
        frame["appended"].append(run(a))
    same = all(np.array_equal(a.project(P, filtered=True)[1], b.project(P, filtered=True)[1]) for P in poses[::10])
    mem = {k: q.get_option("resident_millibytes_per_point") for k, q in (("appended", a), ("one_shot", b))}
    opts = {k: {o: q.get_option(o) for o in ("reordered", "packed", "packed_millibytes_per_point")}
            for k, q in (("appended", a), ("one_shot", b))}
    a.close()
    b.close()
    med = lambda v: float(np.median(v))  # noqa: E731
    out = {"config": "C3 room_shell %d points %dx%d prefilter, %d poses x %d rounds" % (N, W, H, args.steps, args.rounds),
           "a_upload_ms": {str(m): med(v) for m, v in upload_ms.items()},
           "b_append_ms": {str(m): med(v) for m, v in append_ms.items()},
           "b_over_a_at_1e6": med(append_ms[1_000_000]) / med(upload_ms[1_000_000]),
           "c_ms_per_frame": {k: med(v) for k, v in frame.items()},
           "c_ratio": med(frame["appended"]) / med(frame["one_shot"]),
           "c_depth_equal": bool(same),
           "d_resident_millibytes_per_point": mem, "options": opts,
           "all": {"upload_ms": {str(m): v for m, v in upload_ms.items()},
                   "append_ms": {str(m): v for m, v in append_ms.items()}, "frame_ms": frame}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("a_upload_ms", "b_append_ms", "b_over_a_at_1e6", "c_ms_per_frame", "c_ratio",
                                          "c_depth_equal", "d_resident_millibytes_per_point")}))


if __name__ == "__main__":
    main()
