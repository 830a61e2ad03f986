"""Writing points back (include/rtr.h section 2f) on config C3 (room_shell, 1e8 points, the default packed upload), every
leg timed with a host clock around a call that waits for its work, medians of --rounds (at least 5), each beside its
alternatives as the parent commit has them -- rtr_upload_points of the whole cloud, rtr_transform_points over the same
selection -- in the same run:
  (a) every point: xyz only, rgb only, both, from device buffers (torch tensors, float4 / uchar4 records) and from host
      arrays;
  (b) the last 1e7 points (device records);
  (c) a random 1 % selection (device words, device records);
  (d) one broadcast colour onto half the cloud (every other point).
The records written are the resident ones (extracted first), so every round starts from the same cloud and the packed
form keeps its size.  No time target: nobody has measured any of this before.
  python tools/write_bench.py [--n N] [--rounds R] [--out FILE]"""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_bench.json"))
    args = ap.parse_args()
    assert args.rounds >= 5, "medians over at least 5 repetitions"
    import torch
    pkg = entry.load_package()
    N = args.n
    p = pkg.Projector(0)
    p.generate_synthetic("room_shell", 0xC0FFEE03, 0, N, N)
    p.set_resolution(1920, 1080)
    p.synchronize()
    packed_mb = p.get_option("packed_millibytes_per_point")
    legs = {}

    def leg(name, fn):
        fn()  # (warm: code objects, the allocator)
        legs[name] = [timed(fn)[0] for _ in range(args.rounds)]

    dev = torch.device("cuda", 0)
    words = lambda bits: np.packbits(np.concatenate([bits, np.zeros(-bits.size % 32, bool)]), bitorder="little").view("<u4")  # noqa: E731
    dwords = lambda w: torch.from_numpy(w.view(np.int32).copy()).to(dev)  # noqa: E731
    M = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)  # (the identity costs what any matrix costs)

    # (a) every point, device records
    dx = torch.empty((N, 4), dtype=torch.float32, device=dev)
    dc = torch.empty((N, 4), dtype=torch.uint8, device=dev)
    p.extract_points(out={"xyz": dx, "rgb": dc})
    torch.cuda.synchronize()
    leg("all_xyz_device", lambda: p.write_points(dx, None))
    leg("all_rgb_device", lambda: p.write_points(None, dc))
    leg("all_both_device", lambda: p.write_points(dx, dc))
    leg("transform_all", lambda: p.transform_points(M))
    # (b) the last 1e7 points
    m = min(N, 10_000_000)
    tail = dwords(words(np.arange(N) >= N - m))
    leg("tail_both_device", lambda: p.write_points(dx[N - m:], dc[N - m:], tail))
    leg("tail_xyz_device", lambda: p.write_points(dx[N - m:], None, tail))
    leg("tail_rgb_device", lambda: p.write_points(None, dc[N - m:], tail))
    leg("transform_tail", lambda: p.transform_points(M, tail))
    # (c) a random 1 % selection
    bits = np.random.default_rng(3).random(N) < 0.01
    k = int(bits.sum())
    some = dwords(words(bits))
    del bits
    sx = torch.empty((k, 4), dtype=torch.float32, device=dev)
    scol = torch.empty((k, 4), dtype=torch.uint8, device=dev)
    p.extract_points(some, out={"xyz": sx, "rgb": scol})
    torch.cuda.synchronize()
    leg("random_both_device", lambda: p.write_points(sx, scol, some))
    leg("random_xyz_device", lambda: p.write_points(sx, None, some))
    leg("random_rgb_device", lambda: p.write_points(None, scol, some))
    leg("transform_random", lambda: p.transform_points(M, some))
    # (d) one colour onto half the cloud: read what is there first, so that the colours can go back afterwards
    half = dwords(np.full((N + 31) // 32, 0x55555555, np.uint32))
    leg("half_broadcast_colour", lambda: p.write_points(None, np.uint8([255, 64, 0]), half, broadcast=True))
    leg("transform_half", lambda: p.transform_points(M, half))
    p.write_points(None, dc)  # (the colours as they were)
    # (a) again from host arrays, then the alternative: one upload of the whole cloud
    hx, hc = dx.cpu().numpy(), dc.cpu().numpy()
    del dx, dc, sx, scol
    torch.cuda.empty_cache()
    leg("all_xyz_host", lambda: p.write_points(hx, None))
    leg("all_rgb_host", lambda: p.write_points(None, hc))
    leg("all_both_host", lambda: p.write_points(hx, hc))
    p.set_option("auto_reorder", 0)  # (the upload as the parent commit has it, without a sort of its own)
    leg("upload_all", lambda: (p.upload_points(hx, hc), p.synchronize()))
    p.close()

    med = {name: float(np.median(v)) for name, v in legs.items()}
    ratio = lambda a, b: med[a] / med[b]  # noqa: E731
    out = {"config": "C3 room_shell %d points, default packed upload (%d millibytes per point), %d rounds, medians" % (N, packed_mb, args.rounds),
           "legs_ms": med, "selected": {"tail": m, "random": k, "half": (N + 1) // 2},
           "write_over_transform": {"all_xyz_device": ratio("all_xyz_device", "transform_all"),
                                    "tail_xyz_device": ratio("tail_xyz_device", "transform_tail"),
                                    "random_xyz_device": ratio("random_xyz_device", "transform_random"),
                                    "all_rgb_device": ratio("all_rgb_device", "transform_all"),
                                    "tail_rgb_device": ratio("tail_rgb_device", "transform_tail"),
                                    "random_rgb_device": ratio("random_rgb_device", "transform_random"),
                                    "half_broadcast_colour": ratio("half_broadcast_colour", "transform_half")},
           "write_over_upload": {name: ratio(name, "upload_all") for name in legs if name not in ("upload_all",) and not name.startswith("transform")},
           "all": legs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps({key: out[key] for key in ("legs_ms", "selected", "write_over_transform", "write_over_upload")}))


if __name__ == "__main__":
    main()
