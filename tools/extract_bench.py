"""Reading resident points back out (include/rtr.h section 2e) on config C3 (room_shell, 1e8 points, the default packed
upload, 1920x1080), every leg timed with a host clock around a call that waits for its work, medians of --rounds:
  (a) every point into device buffers (torch tensors: float4 / uchar4 records, and tight 12 / 3 ones);
  (b) every point into host arrays, beside rtr_download_points(0, n) in the same run (that call's code is the parent
      commit's: this change does not touch it);
  (c) a box selection of about 1 % of the cloud (a corner box whose size is bisected on the device's count) and a screen-rectangle
      selection, each from the device selection into host arrays, indices included;
  (d) the cloud Morton-sorted with point_ids = 1, every point into device buffers in upload order (scattered stores).
The one relation expected: each leg of (c) takes less time than (b).
  python tools/extract_bench.py [--n N] [--rounds R] [--out FILE]
  python tools/extract_bench.py --one all|box|sorted   one upload and ten calls (for rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--one", choices=("all", "box", "sorted"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_extract_bench.json"))
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    W, H, N = 1920, 1080, args.n
    P = pkg.orbit_projection(3, W, H)

    def cloud(sort=False, **options):
        p = pkg.Projector(0)
        for k, v in options.items():
            p.set_option(k, v)
        p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
        if sort:
            p.reorder_points()
        p.set_resolution(W, H)
        p.synchronize()
        return p

    def device_out(tight=False, indices=False):
        cols = 3 if tight else 4
        out = {"xyz": torch.empty((N, cols), dtype=torch.float32, device="cuda"),
               "rgb": torch.empty((N, cols), dtype=torch.uint8, device="cuda")}
        if indices:
            out["indices"] = torch.empty(N, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return out

    legs, counts = {}, {}

    def leg(name, fn):
        ms = []
        for _ in range(args.rounds):
            t, r = timed(fn)
            ms.append(t)
        legs[name] = ms
        return r

    if args.one in ("sorted",):
        q = cloud(sort=True, point_ids=1)
        out = device_out()
        for _ in range(10):
            q.extract_points(out=out)
        q.close()
        return

    p = cloud()
    # a corner box holding about 1 % of the points: its extent from a sample, its size bisected with the device's own count
    step = max(N // 100, 1)
    sample = np.concatenate([p.download_points(k * step, min(10_000, N - k * step))[0] for k in range(min(100, N))])[:, :3]
    lo, low, top = sample.min(axis=0) - 1, sample.min(axis=0), sample.max(axis=0) + 1
    f_lo, f_hi = 0.0, 1.0
    for _ in range(24):
        f = (f_lo + f_hi) / 2
        hi = (low + f * (top - low)).astype(np.float32)
        if p.select_points(planes=pkg.clip_box_planes(lo, hi))[0] < N // 100:
            f_lo = f
        else:
            f_hi = f
    hi = (low + f_hi * (top - low)).astype(np.float32)
    box = pkg.clip_box_planes(lo, hi)
    rect = (W // 4, H // 4, 3 * W // 4, 3 * H // 4)
    if args.one:
        out = device_out()
        if args.one == "box":
            p.select_points(planes=box)
        for _ in range(10):
            if args.one == "all":
                p.extract_points(out=out)
            else:
                p.extract_points(p.selection(), indices=True)
        p.close()
        return

    # (a) every point into device buffers
    out = device_out()
    p.extract_points(out=out)  # (warm: the kernel's code object, torch's allocations)
    leg("all_to_device", lambda: p.extract_points(out=out))
    del out
    out = device_out(tight=True, indices=True)
    leg("all_to_device_tight_with_indices", lambda: p.extract_points(out=out))
    del out
    torch.cuda.empty_cache()
    # (b) every point into host arrays, beside rtr_download_points
    leg("all_to_host", lambda: p.extract_points())
    leg("download_points", lambda: p.download_points())
    # (c) selections of the device into host arrays
    counts["box"] = p.select_points(planes=box)[0]
    leg("box_to_host", lambda: p.extract_points(p.selection(), indices=True))
    leg("box_count_only", lambda: p.count_selected(p.selection()))
    counts["rect"] = p.select_points(P=P, rect=rect)[0]
    leg("rect_to_host", lambda: p.extract_points(p.selection(), indices=True))
    packed_mb = p.get_option("packed_millibytes_per_point")
    p.close()
    # (d) sorted, every point in upload order into device buffers
    q = cloud(sort=True, point_ids=1)
    out = device_out()
    q.extract_points(out=out)
    leg("sorted_all_to_device", lambda: q.extract_points(out=out))
    del out
    q.close()

    med = {k: float(np.median(v)) for k, v in legs.items()}
    rate = lambda pts, ms: pts / (ms * 1e-3) / 1e9  # noqa: E731  (points per nanosecond = 1e9 points / s)
    out = {"config": "C3 room_shell %d points, default packed upload (%d millibytes per point), %d rounds" % (N, packed_mb, args.rounds),
           "legs_ms": med, "selected": counts,
           "gpoints_per_s": {"all_to_device": rate(N, med["all_to_device"]), "all_to_host": rate(N, med["all_to_host"]),
                             "download_points": rate(N, med["download_points"]),
                             "sorted_all_to_device": rate(N, med["sorted_all_to_device"])},
           "bars": {"box_to_host_under_all_to_host": med["box_to_host"] < med["all_to_host"],
                    "rect_to_host_under_all_to_host": med["rect_to_host"] < med["all_to_host"]},
           "note": "download_points is rtr_download_points(0, n) as the parent commit has it: the call is unchanged",
           "all": legs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("legs_ms", "selected", "gpoints_per_s", "bars")}))


if __name__ == "__main__":
    main()
