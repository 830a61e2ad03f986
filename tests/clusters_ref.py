"""The reference model of rtr_select_clusters (include/rtr.h section 6i), in numpy only.

Clusters are the connected components of section 6h's neighbour relation (neighbours_ref.py: float32, the contract's
order, inclusive, never a point with itself, a non-finite point has no neighbours); a cluster's label is the smallest
upload index among its members.

pairs: every ordered pair (i, j) of neighbours, by neighbours_ref's bucket expansion (cells of edge 2 * radius anchored
at BUCKET_ORIGIN: not the library's grid).
labels: min-label propagation over those pairs with pointer jumping until nothing changes.  lab[i] always names a
member of i's component with lab[i] <= i; at the fixed point lab is constant over every edge, hence over every
component, and lab[lab] == lab, so the constant is a member c with lab[c] == c -- and the component's smallest index s
has lab[s] <= s within the component, so c == s: the label rule falls out.
labels_brute: every pair as a matrix, components by a graph search from each unlabelled index in ascending order (good
to about 4k points); shares only the distance arithmetic with `labels`.
"""
import numpy as np

import neighbours_ref as nr

f32 = np.float32


def pairs(xyz, radius, max_pairs=8_000_000):
    """(i, j): upload indices of every ordered pair of neighbours, each unordered pair in both directions."""
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    r2 = nr.r2_of(radius)
    at = np.flatnonzero(nr.finite(p))
    none = np.zeros(0, np.int64)
    if at.size == 0:
        return none, none
    q = np.floor((p[at].astype(np.float64) - np.float64(nr.BUCKET_ORIGIN)) / (2.0 * float(f32(radius))))
    if np.abs(q).max() >= 2 ** 20:
        raise ValueError("pairs: the cloud spans more than 2^20 cells")
    q = q.astype(np.int64) + 2 ** 20 + 1
    key = (q[:, 0] << 44) | (q[:, 1] << 22) | q[:, 2]
    order = np.argsort(key, kind="stable")
    key, at = key[order], at[order]
    ps = p[at]
    m = at.size
    out_i, out_j = [none], [none]
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            lo_key = key + (dx << 44) + (dy << 22) - 1
            start = np.searchsorted(key, lo_key, "left")
            cnt = np.searchsorted(key, lo_key + 2, "right") - start
            cum = np.cumsum(cnt)
            s = 0
            while s < m:
                e = int(np.searchsorted(cum, (cum[s - 1] if s else 0) + max_pairs, "right"))
                e = min(max(e, s + 1), m)
                c = cnt[s:e]
                total = int(c.sum())
                if total:
                    qi = np.repeat(np.arange(s, e), c)
                    first = np.cumsum(c) - c
                    cj = np.repeat(start[s:e] - first, c) + np.arange(total)
                    nb = (nr._d2(ps[qi], ps[cj]) <= r2) & (at[qi] != at[cj])
                    out_i.append(at[qi[nb]])
                    out_j.append(at[cj[nb]])
                s = e
    return np.concatenate(out_i), np.concatenate(out_j)


def labels_of_pairs(n, i, j):
    lab = np.arange(n, dtype=np.int64)
    while True:
        new = lab.copy()
        np.minimum.at(new, i, lab[j])
        while True:  # pointer jumping: new[v] <= v names a member of v's component
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            return lab.astype(np.uint32)
        lab = new


def labels(xyz, radius):
    """labels[i]: the smallest upload index of point i's cluster (uint32, upload order)."""
    i, j = pairs(xyz, radius)
    return labels_of_pairs(np.asarray(xyz).shape[0], i, j)


def labels_brute(xyz, radius):
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    n = p.shape[0]
    ok = nr.finite(p)
    adj = (nr._d2(p[:, None, :], p[None, :, :]) <= nr.r2_of(radius)) & ok[None, :] & ok[:, None]
    adj[np.arange(n), np.arange(n)] = False
    lab = np.full(n, -1, np.int64)
    for s in range(n):  # (ascending: the first index to reach a component is its smallest)
        if lab[s] >= 0:
            continue
        lab[s] = s
        front = np.array([s])
        while front.size:
            reach = adj[front].any(axis=0) & (lab < 0)
            lab[reach] = s
            front = np.flatnonzero(reach)
    return lab.astype(np.uint32)


def sizes(lab):
    """size[i]: the member count of point i's cluster."""
    return np.bincount(lab, minlength=lab.size)[lab]


def hits(lab, min_points=1, max_points=0, seeds=None):
    """hit[i] before OUTSIDE; seeds: None (not seeded) or the bool selection as it was before the call."""
    sz = sizes(lab)
    hit = sz >= int(min_points)
    if max_points:
        hit &= sz <= int(max_points)
    if seeds is not None:
        touched = np.zeros(lab.size, bool)
        touched[lab[np.asarray(seeds, bool)]] = True
        hit &= touched[lab]
    return hit


def stats(lab, hit):
    """(stats[1], stats[2], stats[3]): clusters, clusters that hit (hit: before OUTSIDE), points of the largest cluster."""
    n = lab.size
    if n == 0:
        return 0, 0, 0
    roots = lab == np.arange(n)
    return int(roots.sum()), int((roots & hit).sum()), int(np.bincount(lab).max())


words = nr.words
