"""Keep mask on config C3 (room_shell, 1e8 points, 1920x1080 + prefilter, bench.py's orbit poses): ms per frame of
six legs measured in ONE process, each masked leg alternated with the unmasked leg (a) so that drift hits both.
  (a) no mask; (b) an all-kept mask; (c) 10 % of the points hidden at random; (d) 50 % hidden at random; (e) a
  contiguous half of the RESIDENT order hidden (whole chunks rejected on their summary); (f) the mask fed back from
  RTR_BUF_VISIBLE of another pose (device memory).
T1's own time: run under `rocprofv3 --kernel-trace --stats` (k_project_bin<...> vs k_project_bin<..., rtr::Clip, rtr::Keep> rows).
  python tools/mask_bench.py [--steps K] [--rounds R] [--out FILE]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_mask_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    L = pkg._lib
    W, H, N = 1920, 1080, args.n
    p = pkg.Projector(0)
    p.set_option("point_ids", 1)  # (a sorted cloud keeps its upload order; room_shell is not sorted: see "reordered")
    p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
    p.set_resolution(W, H)
    reordered = p.get_option("reordered")
    poses = [pkg.orbit_projection(k, W, H) for k in range(args.steps)]
    rng = np.random.default_rng(9)
    half = np.ones(N, bool)
    half[N // 2:] = False  # (upload order = resident order unless "reordered")
    Pf = pkg.orbit_projection(args.steps // 2 + 7, W, H)
    p.render(Pf, True)
    p.point_pass(Pf, ids=False, visible=True)
    p.synchronize()
    vis_words = p.download(L.BUF_VISIBLE)
    legs = {
        "b_all_kept": np.ones(N, bool),
        "c_hide10_random": rng.random(N) >= 0.10,
        "d_hide50_random": rng.random(N) >= 0.50,
        "e_hide_resident_half": half,
        "f_visible_fed_back": "visible",
    }

    def install(mask):
        if isinstance(mask, str):  # RTR_BUF_VISIBLE of pose Pf, straight from device memory
            p.render(Pf, True)
            p.point_pass(Pf, ids=False, visible=True)
            p.set_point_keep(p.device_buffer(L.BUF_VISIBLE))
        else:
            p.set_point_keep(mask)

    def run(mask):
        if mask is None:
            p.set_point_keep(None)
        else:
            install(mask)
        for P in poses[:5]:
            p.render(P, True)
        p.synchronize()
        t0 = time.perf_counter()
        for P in poses:
            p.render(P, True)
        p.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(poses)

    res = {k: {"ms": [], "base_ms": []} for k in legs}
    for _ in range(args.rounds):
        for name, mask in legs.items():
            res[name]["base_ms"].append(run(None))
            res[name]["ms"].append(run(mask))
    stats = {}
    for name, mask in legs.items():
        install(mask)
        kept = int(np.unpackbits(p.download(L.BUF_POINT_KEEP).view(np.uint8), bitorder="little")[:N].sum())
        p.project(poses[0])
        st = p.frame_stats()
        p.set_point_keep(None)
        p.project(poses[0])
        st0 = p.frame_stats()
        r = res[name]
        stats[name] = {"kept_points": kept, "ms_per_frame": float(np.median(r["ms"])),
                       "no_mask_ms_per_frame": float(np.median(r["base_ms"])),
                       "ratio": float(np.median(r["ms"]) / np.median(r["base_ms"])),
                       "ms_all": r["ms"], "no_mask_ms_all": r["base_ms"],
                       "entries": int(st["entries"]), "no_mask_entries": int(st0["entries"]),
                       "colour_chunks": int(st["colour_chunks"]), "no_mask_colour_chunks": int(st0["colour_chunks"])}
    a = [x for r in res.values() for x in r["base_ms"]]
    out = {"config": "C3 room_shell %d points %dx%d prefilter, %d poses x %d rounds" % (N, W, H, args.steps, args.rounds),
           "reordered": int(reordered), "visible_pose_kept_points": int(np.unpackbits(vis_words.view(np.uint8))[:N].sum()),
           "a_no_mask_ms_per_frame": {"median": float(np.median(a)), "min": float(np.min(a)), "max": float(np.max(a))},
           "legs": stats}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: (round(v["ms_per_frame"], 4), round(v["no_mask_ms_per_frame"], 4), round(v["ratio"], 3))
                      for k, v in stats.items()}))
    p.close()


if __name__ == "__main__":
    main()
