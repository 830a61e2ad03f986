"""The reference model of rtr_nearest_k_points (include/rtr.h section 6m), in numpy only.

Relation: nearest_ref's.  Row j holds the candidates of given point j in ascending order of (d2 bits, resident index),
the first min(k, candidates) of them, NONE and +inf behind them; found[j] counts the real entries.  d2 is never negative,
so the order of the float32 values is the order of their bits.

nearest_k_brute: every pair; per given point a STABLE sort of the candidates' d2 bits, the candidates in index order.
nearest_k_bucket: the candidate pairs through near_ref's foreign grid (as nearest_ref.nearest_bucket finds them), one
lexsort on (given, bits, index), the first k of every run.
Both return (index uint32[m, k], dist2 float32[m, k], found uint32[m], stats).
"""
import numpy as np

from near_ref import _cells, _xyz
from neighbours_ref import _d2, f32, finite, r2_of

NONE = 0xFFFFFFFF
INF_BITS = 0x7F800000
MAX_K = 64


def _empty(m, k):
    return np.full((m, k), NONE, np.uint32), np.full((m, k), np.inf, f32), np.zeros(m, np.uint32)


def stats(found, G, k):
    """rtr_nearest_k_points' four statistics."""
    g = np.asarray(G)
    return (int((found > 0).sum()), int(found.sum(dtype=np.uint64)), int((~finite(_xyz(g))).sum()) if g.size else 0, int((found == k).sum()))


def bits(d2):
    return np.ascontiguousarray(d2, f32).view(np.uint32)


def nearest_k_brute(A, G, radius, k):
    assert 1 <= k <= MAX_K
    a, g = _xyz(A), _xyz(G)
    n, m = a.shape[0], g.shape[0]
    idx, d2, found = _empty(m, k)
    if m == 0 or n == 0:
        return idx, d2, found, stats(found, g, k)
    oka, okg = finite(a), finite(g)
    r2 = r2_of(radius)
    for j in np.flatnonzero(okg):
        col = _d2(a, g[j][None, :])
        with np.errstate(invalid="ignore"):
            cand = np.flatnonzero((col <= r2) & oka)  # (in index order)
        take = cand[np.argsort(bits(col[cand]), kind="stable")[:k]]
        found[j] = take.size
        idx[j, :take.size] = take
        d2[j, :take.size] = col[take]
    return idx, d2, found, stats(found, g, k)


def candidate_pairs(A, G, radius, max_pairs=8_000_000):
    """(resident index, given index, d2 bits) of every candidate pair, through the grid"""
    a, g = _xyz(A), _xyz(G)
    none = (np.zeros(0, np.int64),) * 2 + (np.zeros(0, np.uint32),)
    r2 = r2_of(radius)
    ga, aa = np.flatnonzero(finite(g)), np.flatnonzero(finite(a))
    if ga.size == 0 or aa.size == 0:
        return none
    qg = _cells(g[ga], radius)
    if np.abs(qg).max() >= 2 ** 20:
        raise ValueError("candidate_pairs: the given points span more than 2^20 cells")
    qa = _cells(a[aa], radius)
    inr = (np.abs(qa) <= 2 ** 20).all(axis=1)  # (a resident point further out has no given point in its 27 cells)
    aa, qa = aa[inr], qa[inr]
    if aa.size == 0:
        return none
    off = 2 ** 20 + 2
    qg, qa = qg.astype(np.int64) + off, qa.astype(np.int64) + off
    key = (qg[:, 0] << 44) | (qg[:, 1] << 22) | qg[:, 2]
    order = np.argsort(key, kind="stable")
    key, ga = key[order], ga[order]
    gs, ps = g[ga], a[aa]
    akey = (qa[:, 0] << 44) | (qa[:, 1] << 22) | qa[:, 2]
    pairs = []
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
    if not pairs:
        return none
    return tuple(np.concatenate(x) for x in zip(*pairs))


def rows_of_pairs(pairs, m, k, G):
    """the three arrays and the stats from the candidate pairs; several k can share one set of pairs"""
    pi, pj, pb = pairs
    idx, d2, found = _empty(m, k)
    if pi.size:
        o = np.lexsort((pi, pb, pj))
        pi, pj, pb = pi[o], pj[o], pb[o]
        head = np.flatnonzero(np.r_[True, pj[1:] != pj[:-1]])
        rank = np.arange(pj.size) - np.repeat(head, np.diff(np.r_[head, pj.size]))
        keep = rank < k
        idx[pj[keep], rank[keep]] = pi[keep].astype(np.uint32)
        d2.view(np.uint32)[pj[keep], rank[keep]] = pb[keep]
        np.add.at(found, pj[keep], 1)
    return idx, d2, found, stats(found, _xyz(G), k)


def nearest_k_bucket(A, G, radius, k):
    assert 1 <= k <= MAX_K
    return rows_of_pairs(candidate_pairs(A, G, radius), _xyz(G).shape[0], k, G)


def nearest_k(A, G, radius, k):
    big = np.asarray(A).shape[0] * max(np.asarray(G).shape[0], 1) > 2e6
    return nearest_k_bucket(A, G, radius, k) if big else nearest_k_brute(A, G, radius, k)


def same(got, want):
    """index and found arrays equal, distance arrays equal as bits"""
    return all(np.asarray(g).shape == np.asarray(w).shape and
               np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)) for g, w in zip(got, want))
