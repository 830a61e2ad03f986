#!/usr/bin/env python3
"""Idle time on the tail stream's chain, from a rocprofv3 kernel trace of tools/overlap_bench.py:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/overlap_bench.py --settings=-1:0,0:0
    python tools/chain_edges.py DIR [--label NAME]        -> one JSON line

Kernel trace only (no counters, no other tracing beside it).  Every whole frame with the prefilter is one k_project_bin
(T1), one k_tile<0> and one k_filter4, so the k-th of each in start order make frame k.  A frame is OVERLAPPED when its
T1 started before the previous frame's k_filter4 ended, else SERIAL.  A synchronising call of the bench shows as a gap
of more than --gap us in front of a tile launch and splits the frames into runs; only runs of at least --min-run frames
count (the 100 measured frames of a setting; not its warm-up, its two checksum frames and its 20 bracketed frames),
without their first --skip frames and their last one.  Per class, median / p10 / p90 / min / max in us of

  edge_a   k_tile<0>(k) end   -> k_filter4(k) start
  edge_b   k_filter4(k) end   -> k_tile<0>(k+1) start
  t1_lead  T1(k+1) end        -> k_filter4(k) end   (positive: T1 had ended before the tail did, so the tile launch's
                                                      wait for `binned` is a packet and not a wait)
  hand_in  k_filter4(k) end   -> T1(k+1) start   } the serial chain's other two hand-overs (edge_b of a serial frame holds
  hand_out T1(k) end          -> k_tile<0>(k) start }  both and T1 between them); negative where the kernels overlap
  period   k_tile<0>(k) start -> k_tile<0>(k+1) start
  and the three kernels' durations.

Not part of the product; fills profiles/r17_chain_edges.json and DESIGN.md section 4."""
import argparse
import csv
import glob
import json
import os


def load(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"].replace("void ", "").replace("rtr::", "")
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    return rows


def stats(v):
    if not v:
        return None
    s = sorted(v)
    q = lambda p: s[min(len(s) - 1, int(p * len(s)))]
    return {"median": round(q(0.5), 2), "p10": round(q(0.1), 2), "p90": round(q(0.9), 2), "min": round(s[0], 2),
            "max": round(s[-1], 2), "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--label", default="")
    ap.add_argument("--gap", type=float, default=150.0)
    ap.add_argument("--min-run", type=int, default=60)
    ap.add_argument("--skip", type=int, default=5)
    a = ap.parse_args()
    rows = load(a.dir)
    t1 = [r for r in rows if "k_project_bin<" in r[2]]
    tile = [r for r in rows if "k_tile<0>" in r[2]]
    flt = [r for r in rows if "k_filter4" in r[2]]
    assert len(t1) == len(tile) == len(flt) and tile, ("one T1, one k_tile<0>, one k_filter4 per frame", len(t1), len(tile), len(flt))
    n = len(tile)
    us = 1e-3
    runs, first = [], 0
    for k in range(1, n + 1):
        if k == n or (tile[k][0] - flt[k - 1][1]) * us > a.gap:
            runs.append((first, k))
            first = k
    out = {"label": a.label, "frames": n, "runs": [b - f for f, b in runs], "overlapped": None, "serial": None}
    acc = {"overlapped": {}, "serial": {}}
    for f, b in runs:
        if b - f < a.min_run:
            continue
        for k in range(f + a.skip, b - 1):
            cls = "overlapped" if t1[k][0] < flt[k - 1][1] else "serial"
            nxt = "overlapped" if t1[k + 1][0] < flt[k][1] else "serial"
            if cls != nxt:
                continue
            m = acc[cls]
            m.setdefault("edge_a", []).append((flt[k][0] - tile[k][1]) * us)
            m.setdefault("edge_b", []).append((tile[k + 1][0] - flt[k][1]) * us)
            m.setdefault("t1_lead", []).append((flt[k][1] - t1[k + 1][1]) * us)
            m.setdefault("hand_in", []).append((t1[k + 1][0] - flt[k][1]) * us)
            m.setdefault("hand_out", []).append((tile[k][0] - t1[k][1]) * us)
            m.setdefault("period", []).append((tile[k + 1][0] - tile[k][0]) * us)
            m.setdefault("t1", []).append((t1[k][1] - t1[k][0]) * us)
            m.setdefault("tile", []).append((tile[k][1] - tile[k][0]) * us)
            m.setdefault("filter4", []).append((flt[k][1] - flt[k][0]) * us)
    for cls, m in acc.items():
        if m:
            out[cls] = {name: stats(v) for name, v in m.items()}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
