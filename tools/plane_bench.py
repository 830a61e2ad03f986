"""Fitting the dominant plane of the resident cloud (include/rtr.h section 6j) at 1e8 points on room_shell and
uniform_box (both with point_ids = 1: the sampler draws by upload index, and the library sorts uniform_box), 256
iterations at dist 2 cm and 5 cm, every leg timed with a host clock around the call -- which always ends in a
synchronise -- after one warm-up call of the same shape, medians of --rounds:
  (a) rtr_fit_plane, with the split the call itself reports (rtr_get_option "plane_sample_us": drawing the sample and
      extracting it, "plane_count_us": counting the candidates);
  (b) rtr_count_in_bands alone on the same bands (rebuilt here from the sample with tests/planes_ref.py), whose three
      statistics sums -- (chunk, band) pairs decided outside / inside on the box / tested point by point -- are reported;
  (c) the yardstick, the only route on the device without these calls, in the same process on the same bands: one
      rtr_select_points with two planes and stats per band, a median of --rounds like the other legs.  Its counts must
      equal (b)'s, and the winner (a)'s.
      yardstick_over_fit = (c) / (a) is the bar: the fit must beat the route that existed before it.
On 1e6-point clouds only (--host-n), numpy float32 on the host for the same bands is timed as well; the CPU route at 1e8
points was not measured.
  python tools/plane_bench.py [--n N] [--host-n M] [--rounds R] [--iterations K] [--out FILE]"""
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
import planes_ref as pr  # noqa: E402

SEED = 0xC0FFEE03


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def candidates(p, n, iterations, seed, dist):
    """The fit's own candidates, rebuilt on the host: (candidate numbers, planes, bands)."""
    ranks = pr.ranks(seed, iterations, n)
    idx = np.array([[int(v) for v in row] for row in ranks], np.int64)
    mask = np.zeros(n, bool)
    mask[idx.reshape(-1)] = True
    xyz, got = p.extract_points(mask, rgb=False, indices=True)
    at = np.searchsorted(got, idx)
    who, planes, bands = [], [], []
    for c in range(iterations):
        pl = pr.candidate(xyz[at[c, 0], :3], xyz[at[c, 1], :3], xyz[at[c, 2], :3], idx[c])
        if pl is not None and np.isfinite(pr.band_of(pl, dist)).all():
            who.append(c), planes.append(pl), bands.append(pr.band_of(pl, dist))
    return who, np.array(planes, np.float32), np.array(bands, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--host-n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_bench.json"))
    args = ap.parse_args()
    pkg = entry.load_package()
    K = args.iterations
    cases, host_cases = {}, {}

    def cloud(scene, n):
        p = pkg.Projector(0)
        p.set_option("point_ids", 1)
        p.generate_synthetic(scene, SEED, 0, n, n)
        p.synchronize()
        return p

    def case(p, scene, n, cm, host):
        dist = np.float32(cm / 100.0)
        fit = lambda: p.fit_plane(dist, K, 0)  # noqa: E731
        fit()  # (warm-up)
        ms, split = [], []
        for _ in range(args.rounds):
            t, (plane, inliers, st) = timed(fit)
            ms.append(t)
            split.append([p.get_option("plane_sample_us") / 1e3, p.get_option("plane_count_us") / 1e3])
        who, planes, bands = candidates(p, n, K, 0, dist)
        assert len(who) == st[1] and np.array_equal(planes[who.index(st[2])].view(np.uint32), plane.view(np.uint32))
        count = lambda: p.count_in_bands(bands)  # noqa: E731
        count()
        cms = []
        for _ in range(args.rounds):
            t, (counts, cst) = timed(count)
            cms.append(t)
        assert int(counts.max()) == inliers and int(np.argmax(counts)) == who.index(st[2])

        def yardstick():
            return [p.select_points(planes=pr.two_planes(b))[0] for b in bands]
        for b in bands[:8]:
            p.select_points(planes=pr.two_planes(b))  # (warm-up: the first call allocates the selection)
        yall = []
        for _ in range(args.rounds):
            t, ycounts = timed(yardstick)
            yall.append(t)
        yms = float(np.median(yall))
        p.clear_selection()
        assert ycounts == [int(v) for v in counts]
        pairs = ((n + 255) // 256) * len(bands)
        out = {"n": n, "dist_m": float(dist), "iterations": K, "candidates": len(who), "plane": [float(v) for v in plane],
               "inliers": inliers, "winner": st[2], "fit_ms": float(np.median(ms)), "fit_all_ms": ms,
               "fit_sample_ms": float(np.median([s[0] for s in split])), "fit_count_ms": float(np.median([s[1] for s in split])),
               "count_in_bands_ms": float(np.median(cms)), "count_all_ms": cms,
               "pairs": pairs, "pairs_outside": cst[1], "pairs_inside": cst[2], "pairs_tested": cst[3],
               "yardstick_select_points_ms": yms, "yardstick_all_ms": yall, "fit_beats_yardstick": bool(yms > float(np.median(ms))),
               "yardstick_over_fit": yms / float(np.median(ms)),
               "yardstick_over_count": yms / float(np.median(cms)),
               "cloud": {"packed": p.get_option("packed"), "reordered": p.get_option("reordered")}}
        if host:  # numpy float32 on the host, the coordinates already there
            xyz = np.ascontiguousarray(p.extract_points(rgb=False)[0][:, :3])
            hms, hcounts = timed(lambda: pr.counts(xyz, bands))
            assert np.array_equal(hcounts, counts)
            out["numpy_host_ms"] = hms
        print(scene, cm, json.dumps({k: v for k, v in out.items() if not k.endswith("all_ms")}), flush=True)
        if not out["fit_beats_yardstick"]:
            print("WARNING: %s %d cm: rtr_fit_plane does not beat the yardstick (ratio %.2f)" % (scene, cm, out["yardstick_over_fit"]), flush=True)
        return out

    for scene in ("room_shell", "uniform_box"):
        p = cloud(scene, args.n)
        for cm in (2, 5):
            cases["%s_%dcm" % (scene, cm)] = case(p, scene, args.n, cm, False)
        p.close()
    if args.host_n:
        for scene in ("room_shell", "uniform_box"):
            p = cloud(scene, args.host_n)
            host_cases["%s_5cm" % scene] = case(p, scene, args.host_n, 5, True)
            p.close()
    out = {"config": "%d points (host legs: %d), %d iterations, seed 0, point_ids = 1, pass width 64, %d rounds after one warm-up call"
                     % (args.n, args.host_n, K, args.rounds),
           "cases": cases, "host_cases": host_cases,
           "fit_beats_yardstick_everywhere": all(c["fit_beats_yardstick"] for c in list(cases.values()) + list(host_cases.values())),
           "note": "the numpy route was timed on the host-n clouds only; the CPU route at the full size was not measured"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
