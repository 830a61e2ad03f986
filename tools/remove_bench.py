"""Removing points (include/rtr.h section 2c) on config C3 (room_shell, 1920x1080 + prefilter, bench.py's orbit poses):
  (a) wall time of rtr_remove_points (keep words precomputed in host memory) for random 1 %, 10 % and 50 % removals of
      a resident 1e8 and for the last appended 1e7 of 1e8 + 1e7, against rtr_upload_points of the survivors from host
      arrays (and, for the tail, rtr_append_points of it); a keep-all call times the count and chunk scan alone;
  (b) ms per frame after removing 50 % at random, against the same points hidden by a keep mask and a one-shot upload
      of the survivors, alternated in one process (so that drift hits all three);
  (c) resident_millibytes_per_point of each.
  python tools/remove_bench.py [--steps K] [--rounds R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def words_of(keep):
    return np.packbits(np.concatenate([keep, np.zeros(-keep.size % 32, bool)]), bitorder="little").view("<u4").copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_remove_bench.json"))
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

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    rng = np.random.default_rng(11)
    remove_ms, upload_ms, kept = {}, {}, {}
    p = pkg.Projector(0)
    for frac in (0.01, 0.10, 0.50):
        keep = rng.random(N) >= frac
        w = words_of(keep)
        xs, cs = X[keep], Cc[keep]
        key = "random_%g" % frac
        kept[key] = int(keep.sum())
        remove_ms[key], upload_ms[key] = [], []
        for _ in range(args.rounds):
            p.upload_points(X, Cc)
            remove_ms[key].append(timed(lambda: p.remove_points(w)))
            assert p.num_points == kept[key]
            upload_ms[key].append(timed(lambda: p.upload_points(xs, cs)))
        del xs, cs
    # the last appended block
    keep = np.arange(total) < N
    w = words_of(keep)
    remove_ms["last_append"], upload_ms["last_append"], append_ms = [], [], []
    kept["last_append"] = N
    for _ in range(args.rounds):
        p.upload_points(X, Cc)
        append_ms.append(timed(lambda: p.append_points(xyzw[N:], rgba[N:])))
        remove_ms["last_append"].append(timed(lambda: p.remove_points(w)))
        assert p.num_points == N
        tail_pk = {"removed": p.get_option("packed_millibytes_per_point")}
        upload_ms["last_append"].append(timed(lambda: p.upload_points(X, Cc)))
        tail_pk["one_shot"] = p.get_option("packed_millibytes_per_point")
    # keep-all: the count pass and the chunk scan, nothing else changes
    w_all = words_of(np.ones(N, bool))
    scan_ms = [timed(lambda: p.remove_points(w_all)) for _ in range(args.rounds)]
    p.close()

    # (b), (c): 50 % removed vs hidden vs one-shot
    keep = np.random.default_rng(50).random(N) >= 0.5
    a, m, b = pkg.Projector(0), pkg.Projector(0), pkg.Projector(0)
    a.upload_points(X, Cc)
    a.remove_points(keep)
    m.upload_points(X, Cc)
    m.set_point_keep(keep)
    b.upload_points(X[keep], Cc[keep])
    poses = [pkg.orbit_projection(k, W, H) for k in range(args.steps)]
    for q in (a, m, b):
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

    frame = {"removed": [], "masked": [], "one_shot": []}
    for _ in range(args.rounds):
        frame["one_shot"].append(run(b))
        frame["removed"].append(run(a))
        frame["masked"].append(run(m))
    same = all(np.array_equal(a.project(P, filtered=True)[1], b.project(P, filtered=True)[1]) and
               np.array_equal(a.project(P, filtered=True)[1], m.project(P, filtered=True)[1]) for P in poses[::10])
    mem = {k: q.get_option("resident_millibytes_per_point") for k, q in (("removed", a), ("masked", m), ("one_shot", b))}
    opts = {k: {o: q.get_option(o) for o in ("reordered", "packed", "packed_millibytes_per_point")}
            for k, q in (("removed", a), ("masked", m), ("one_shot", b))}
    for q in (a, m, b):
        q.close()
    med = lambda v: float(np.median(v))  # noqa: E731
    out = {"config": "C3 room_shell %d points %dx%d prefilter, %d poses x %d rounds" % (N, W, H, args.steps, args.rounds),
           "a_remove_ms": {k: med(v) for k, v in remove_ms.items()},
           "a_upload_survivors_ms": {k: med(v) for k, v in upload_ms.items()},
           "a_remove_over_upload": {k: med(remove_ms[k]) / med(upload_ms[k]) for k in remove_ms},
           "a_append_tail_ms": med(append_ms),
           "a_keep_all_count_scan_ms": med(scan_ms),
           "a_survivors": kept,
           "a_last_append_packed_millibytes_per_point": tail_pk,
           "b_ms_per_frame": {k: med(v) for k, v in frame.items()},
           "b_removed_over_one_shot": med(frame["removed"]) / med(frame["one_shot"]),
           "b_masked_over_removed": med(frame["masked"]) / med(frame["removed"]),
           "b_depth_equal": bool(same),
           "c_resident_millibytes_per_point": mem, "options": opts,
           "all": {"remove_ms": remove_ms, "upload_ms": upload_ms, "append_ms": append_ms, "scan_ms": scan_ms,
                   "frame_ms": frame}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("a_remove_ms", "a_upload_survivors_ms", "a_remove_over_upload",
                                          "a_append_tail_ms", "a_keep_all_count_scan_ms",
                                          "a_last_append_packed_millibytes_per_point", "b_ms_per_frame",
                                          "b_removed_over_one_shot", "b_masked_over_removed", "b_depth_equal",
                                          "c_resident_millibytes_per_point")}))


if __name__ == "__main__":
    main()
