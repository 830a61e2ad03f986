"""The reference model of rtr_nearest_points (include/rtr.h section 6l), in numpy only.

Relation: near_ref's, between a resident point i of A and a given point j of G: with r2 = float32(radius) *
float32(radius) the pair is a candidate iff d2 = ((dx*dx + dy*dy) + dz*dz) <= r2, every operation in float32 on its own;
a point with a NaN or infinite coordinate on either side is nobody's candidate.  Given point j gets the resident index
with the smallest d2 among its candidates -- of equal d2 bits the smallest index -- and that d2; resident point i the
same over the given points.  No candidate: NONE and +inf.  d2 is never negative, so the order of the float32 values is
the order of their bits, and numpy's argmin, which returns the FIRST occurrence of the minimum, is the tie rule.

nearest_brute: every pair, in blocks.
nearest_bucket: the given points sorted by neighbours_ref's foreign grid (near_ref.near_bucket's: it shares no cell face
and no arithmetic with the library's grid), each resident point tested against the 27 cells around its own.
Both return (given_index uint32[m], given_dist2 float32[m], resident_index uint32[n], resident_dist2 float32[n], stats).
"""
import numpy as np

from near_ref import _cells, _xyz
from neighbours_ref import _d2, f32, finite, r2_of

NONE = 0xFFFFFFFF
INF_BITS = 0x7F800000


def _empty(n, m):
    return np.full(m, NONE, np.uint32), np.full(m, np.inf, f32), np.full(n, NONE, np.uint32), np.full(n, np.inf, f32)


def stats(gi, ri, G):
    """rtr_nearest_points' four statistics."""
    return (int((gi != NONE).sum()), int((ri != NONE).sum()), int((~finite(_xyz(G))).sum()) if np.asarray(G).size else 0, 0)


def bits(d2):
    return np.ascontiguousarray(d2, f32).view(np.uint32)


def nearest_brute(A, G, radius, block=512):
    a, g = _xyz(A), _xyz(G)
    n, m = a.shape[0], g.shape[0]
    gi, gd, ri, rd = _empty(n, m)
    if m == 0 or n == 0:
        return gi, gd, ri, rd, stats(gi, ri, g)
    oka, okg = finite(a), finite(g)
    r2 = r2_of(radius)
    for s in range(0, n, block):
        d2 = _d2(a[s:s + block, None, :], g[None, :, :])
        with np.errstate(invalid="ignore"):
            ok = (d2 <= r2) & okg[None, :] & oka[s:s + block, None]
        d2 = np.where(ok, d2, f32(np.inf))  # (an accepted d2 is <= r2 < inf: the mask never ties with a candidate)
        # resident side: this block's rows are complete
        j = d2.argmin(axis=1)  # (first occurrence: the smallest given index)
        best = d2[np.arange(d2.shape[0]), j]
        has = ok.any(axis=1)
        ri[s:s + block] = np.where(has, j, NONE)
        rd[s:s + block] = np.where(has, best, f32(np.inf))
        # given side: the block's minimum against the minimum so far; a tie stays with the earlier block (smaller index)
        i = d2.argmin(axis=0)  # (first occurrence: the smallest resident index of the block)
        best = d2[i, np.arange(m)]
        take = ok.any(axis=0) & (best < gd)
        gi[take] = (i[take] + s).astype(np.uint32)
        gd[take] = best[take]
    return gi, gd, ri, rd, stats(gi, ri, g)


def nearest_bucket(A, G, radius, max_pairs=8_000_000):
    a, g = _xyz(A), _xyz(G)
    n, m = a.shape[0], g.shape[0]
    gi, gd, ri, rd = _empty(n, m)
    r2 = r2_of(radius)
    ga, aa = np.flatnonzero(finite(g)), np.flatnonzero(finite(a))
    if ga.size == 0 or aa.size == 0:
        return gi, gd, ri, rd, stats(gi, ri, g)
    qg = _cells(g[ga], radius)
    if np.abs(qg).max() >= 2 ** 20:
        raise ValueError("nearest_bucket: the given points span more than 2^20 cells")
    qa = _cells(a[aa], radius)
    inr = (np.abs(qa) <= 2 ** 20).all(axis=1)  # (a resident point further out has no given point in its 27 cells)
    aa, qa = aa[inr], qa[inr]
    if aa.size == 0:
        return gi, gd, ri, rd, stats(gi, ri, g)
    off = 2 ** 20 + 2
    qg, qa = qg.astype(np.int64) + off, qa.astype(np.int64) + off
    key = (qg[:, 0] << 44) | (qg[:, 1] << 22) | qg[:, 2]
    order = np.argsort(key, kind="stable")
    key, ga = key[order], ga[order]
    gs, ps = g[ga], a[aa]
    akey = (qa[:, 0] << 44) | (qa[:, 1] << 22) | qa[:, 2]
    pairs = []  # (resident index, given index, d2 bits) of every candidate pair
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):  # (z is the lowest field: the cells z - 1 .. z + 1 are one key range)
            lo_key = akey + (dx << 44) + (dy << 22) - 1
            start = np.searchsorted(key, lo_key, "left")
            cnt = np.searchsorted(key, lo_key + 2, "right") - start
            cum = np.cumsum(cnt)
            s = 0
            while s < aa.size:
                e = int(np.searchsorted(cum, (cum[s - 1] if s else 0) + max_pairs, "right"))
                e = min(max(e, s + 1), aa.size)
                c = cnt[s:e]
                total = int(c.sum())
                if total:
                    qi = np.repeat(np.arange(s, e), c)
                    first = np.cumsum(c) - c
                    cj = np.repeat(start[s:e] - first, c) + np.arange(total)
                    d2 = _d2(ps[qi], gs[cj])
                    nb = d2 <= r2
                    pairs.append((aa[qi[nb]], ga[cj[nb]], bits(d2[nb])))
                s = e
    if pairs:
        pi, pj, pb = (np.concatenate(x) for x in zip(*pairs))
        # the smallest (d2 bits, other side's index) per point: sort by that pair, keep the first of every run
        for mine, other, idx, dist in ((pj, pi, gi, gd), (pi, pj, ri, rd)):
            o = np.lexsort((other, pb, mine))
            head = np.r_[True, mine[o][1:] != mine[o][:-1]]
            at = o[head]
            idx[mine[at]] = other[at].astype(np.uint32)
            dist[mine[at]] = pb[at].view(f32)
    return gi, gd, ri, rd, stats(gi, ri, g)


def nearest(A, G, radius):
    big = np.asarray(A).shape[0] * max(np.asarray(G).shape[0], 1) > 3e8
    return nearest_bucket(A, G, radius) if big else nearest_brute(A, G, radius)


def same(got, want):
    """index arrays equal, distance arrays equal as bits"""
    return all(np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32)) for g, w in zip(got, want))
