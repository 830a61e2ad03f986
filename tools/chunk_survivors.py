#!/usr/bin/env python3
"""How many chunks of C3's cloud survive the point kernel's chunk test, counted on the CPU (no GPU, no library).

The cloud is the bench's (room_shell, seed 0xC0FFEE03, 1e8 points, generator order), made by the oracle's generator in
slabs of 1e7 points.  The packer's width rule (k_pack_measure), both forms of chunk_box, wide_box_word and box_outside
(csrc/rtr_chunk_box.h) are restated in numpy float32.  Per sampled bench pose it prints the chunks the test keeps with
  header boxes           the six-argument chunk_box: a wide chunk has no box and is kept
  header + wide box      the seven-argument chunk_box: a wide chunk's first wide axis from its box word
  exact boxes            every chunk's exact min / max box (what a side array would give)
and, of the wide chunks, how many the wide box keeps, how many their exact box would keep and how many hold a point
inside the frustum.

    python tools/chunk_survivors.py [--points N] [--poses 10,20,...] [--json OUT]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

WIDE_FLAG_BITS = 25  # kPackMaxBits: more differing bits than this make an axis wide
FLT_MAX = np.float32(3.4028234663852886e38)


def order_key(bits):
    return bits ^ np.where(bits >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def order_bits(key):
    return key ^ np.where(key >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


def wide_box_word(mn, mx):
    """rtr::wide_box_word on arrays of patterns."""
    lo16 = (mn >> 16) + (((mn >> 31) != 0) & ((mn & 0xFFFF) != 0)).astype(np.uint32)
    hi16 = (mx >> 16) + (((mx >> 31) == 0) & ((mx & 0xFFFF) != 0)).astype(np.uint32)
    ok = ((lo16 & 0x7F80) != 0x7F80) & ((hi16 & 0x7F80) != 0x7F80)
    return np.where(ok, lo16 | (hi16 << 16), 0).astype(np.uint32)


def chunk_headers(bits):
    """bits: uint32 [nch, 256, 3] -> per chunk: widths [nch, 3] (0..25 or 32), base [nch, 3], box word [nch]."""
    diff = np.bitwise_or.reduce(bits ^ bits[:, :1, :], axis=1)
    nb = np.where(diff == 0, 0, np.floor(np.log2(np.maximum(diff, 1).astype(np.float64))).astype(np.int64) + 1)
    w = np.where(nb > WIDE_FLAG_BITS, 32, nb).astype(np.uint32)
    base = np.where(w == 32, 0, (bits[:, 0, :] >> np.minimum(w, 31)) << np.minimum(w, 31)).astype(np.uint32)
    wide = w == 32
    first = np.argmax(wide, axis=1)  # (0 when none is wide: masked below)
    vals = np.take_along_axis(bits, first[:, None, None], axis=2)[:, :, 0]
    keys = order_key(vals)
    finite = ((bits & 0x7F800000) != 0x7F800000).all(axis=(1, 2))
    word = wide_box_word(order_bits(keys.min(axis=1)), order_bits(keys.max(axis=1)))
    word = np.where(wide.any(axis=1) & finite, word, 0).astype(np.uint32)
    return w, base, word


def chunk_box(w, base, word=None):
    """Both forms of rtr::chunk_box: word None = the six-argument one.  -> ok [nch], lo, hi float32 [nch, 3]."""
    wide = w == 32
    any_wide = wide.any(axis=1)
    top = base | ((np.uint32(1) << (w & 31)) - np.uint32(1))
    p0, p1 = base.copy(), top.copy()
    if word is None:
        ok = ~any_wide
    else:
        ok = ~any_wide | (word != 0)
        first = wide & (np.cumsum(wide, axis=1) == 1)
        later = wide & ~first
        p0 = np.where(first, (word << 16)[:, None], np.where(later, np.uint32(0xFF7FFFFF), p0)).astype(np.uint32)
        p1 = np.where(first, (word & np.uint32(0xFFFF0000))[:, None], np.where(later, np.uint32(0x7F7FFFFF), p1)).astype(np.uint32)
    ok = ok & ((p0 & 0x7F800000) != 0x7F800000).all(axis=1) & ((p1 & 0x7F800000) != 0x7F800000).all(axis=1)
    f0, f1 = p0.view(np.float32), p1.view(np.float32)
    neg = ~wide & ((base >> 31) != 0)
    return ok, np.where(neg, f1, f0), np.where(neg, f0, f1)


def frustum_planes(m, fW, fH):
    f = np.float32
    comb = np.array([[0, 0, 1], [1, 0, 1], [-1, 0, fW], [0, 1, 1], [0, -1, fH]], f)
    m = np.asarray(m, f).reshape(-1)[:12].reshape(3, 4)
    pl = (comb[:, 0:1] * m[0] + comb[:, 1:2] * m[1]) + comb[:, 2:3] * m[2]
    a = np.abs(comb[:, 0:1] * m[0]) + np.abs(comb[:, 1:2] * m[1]) + np.abs(comb[:, 2:3] * m[2])
    return pl.astype(f), a[:, :3].astype(f), a[:, 3].astype(f)


def box_outside(planes, lo, hi):
    pl, plm, pld = planes
    culled = np.zeros(len(lo), bool)
    mag = np.maximum(np.abs(lo), np.abs(hi))
    with np.errstate(over="ignore", invalid="ignore"):
        for q in range(5):
            v = np.full(len(lo), pl[q, 3], np.float32)
            m = np.full(len(lo), pld[q], np.float32)
            for k in range(3):
                v = v + np.maximum(pl[q, k] * lo[:, k], pl[q, k] * hi[:, k])
                m = m + plm[q, k] * mag[:, k]
            culled |= v < np.float32(-2e-6) * m
    return culled


def in_frustum(P, xyz, W, H):
    """A point lands on a pixel (numpy restatement of the projection, for counting only)."""
    m = np.asarray(P, np.float32).reshape(4, 4)
    with np.errstate(all="ignore"):
        r = [((m[i, 0] * xyz[..., 0] + m[i, 1] * xyz[..., 1]) + m[i, 2] * xyz[..., 2]) + m[i, 3] for i in range(3)]
        px, py = np.rint(r[0] / r[2]), np.rint(r[1] / r[2])
        return (r[2] > 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--poses", default="10,20,30,40,50,60,70,80,90,100,109")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    pkg, orc = entry.load_package(), entry.load_oracle()
    orc.build()
    n, W, H = args.points, args.width, args.height
    poses = [int(k) for k in args.poses.split(",")]
    boxes = {k: [] for k in ("ok6", "lo6", "hi6", "ok7", "lo7", "hi7", "lo_x", "hi_x", "wide", "nwide")}
    wide_pts = []
    carry = np.zeros((0, 3), np.float32)
    slab = 10_000_000
    for first in range(0, n, slab):
        xyzw, _ = orc.generate("room_shell", 0xC0FFEE03, first, min(slab, n - first), n)
        xyz = np.concatenate([carry, xyzw[:, :3]])
        last = first + slab >= n
        whole = len(xyz) // 256 * 256
        if last and whole < len(xyz):  # the cloud's last chunk: lanes past the end repeat its last quad (NaN padding)
            pad = np.full((-len(xyz) % 4, 3), np.nan, np.float32)
            xyz = np.concatenate([xyz, pad])
            xyz = np.concatenate([xyz] + [xyz[-4:]] * ((-len(xyz) % 256) // 4))
            whole = len(xyz)
        carry = xyz[whole:]
        pts = np.ascontiguousarray(xyz[:whole]).reshape(-1, 256, 3)
        w, base, word = chunk_headers(pts.view(np.uint32))
        ok6, lo6, hi6 = chunk_box(w, base)
        ok7, lo7, hi7 = chunk_box(w, base, word)
        wide = (w == 32).any(axis=1)
        with np.errstate(invalid="ignore"):
            for key, val in (("ok6", ok6), ("lo6", lo6), ("hi6", hi6), ("ok7", ok7), ("lo7", lo7), ("hi7", hi7),
                             ("lo_x", np.nanmin(pts, axis=1)), ("hi_x", np.nanmax(pts, axis=1)), ("wide", wide),
                             ("nwide", (w == 32).sum(axis=1))):
                boxes[key].append(val)
        wide_pts.append(pts[wide])
        print("slab at %d: %d chunks, %d wide" % (first, len(pts), int(wide.sum())), file=sys.stderr, flush=True)
    b = {k: np.concatenate(v) for k, v in boxes.items()}
    wide_pts = np.concatenate(wide_pts)
    wide = b["wide"]
    out = {"points": n, "chunks": int(len(wide)), "wide": int(wide.sum()),
           "wide_axes": {str(k): int((b["nwide"] == k).sum()) for k in (1, 2, 3)},
           "wide_boxed": int((wide & b["ok7"]).sum()), "poses": {}}
    print("chunks %d, wide %d (one axis %d, two %d, three %d), wide with a box word %d" %
          (out["chunks"], out["wide"], out["wide_axes"]["1"], out["wide_axes"]["2"], out["wide_axes"]["3"], out["wide_boxed"]))
    print("pose  header  header+wide  exact | wide: kept  exact-kept  in-frustum")
    for k in poses:
        P = pkg.orbit_projection(k, W, H)
        pl = frustum_planes(P, np.float32(W), np.float32(H))
        keep6 = ~(b["ok6"] & box_outside(pl, b["lo6"], b["hi6"]))
        keep7 = ~(b["ok7"] & box_outside(pl, b["lo7"], b["hi7"]))
        keepx = ~box_outside(pl, b["lo_x"], b["hi_x"])
        inside = in_frustum(P, wide_pts, W, H).any(axis=1)
        assert not (inside & ~keep7[wide]).any(), "the wide box rejected a chunk with a point in the frustum"
        row = {"header": int(keep6.sum()), "header_wide": int(keep7.sum()), "exact": int(keepx.sum()),
               "wide_kept": int(keep7[wide].sum()), "wide_exact_kept": int(keepx[wide].sum()), "wide_in_frustum": int(inside.sum())}
        out["poses"][str(k)] = row
        print("%4d  %6d  %11d  %5d | %10d  %10d  %10d" % (k, row["header"], row["header_wide"], row["exact"], row["wide_kept"],
                                                         row["wide_exact_kept"], row["wide_in_frustum"]), flush=True)
    rows = list(out["poses"].values())
    out["mean"] = {key: float(np.mean([r[key] for r in rows])) for key in rows[0]}
    print("mean  %6.0f  %11.0f  %5.0f | %10.0f  %10.0f  %10.0f" % tuple(out["mean"][key] for key in rows[0]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
