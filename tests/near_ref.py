"""The reference model of rtr_select_near (include/rtr.h section 6k), in numpy only.

Relation: neighbours_ref's, between a resident point i of A and a given point j of G: with r2 = float32(radius) *
float32(radius) the pair is near iff ((dx*dx + dy*dy) + dz*dz) <= r2, dx = A[i].x - G[j].x ..., every operation in float32
on its own.  There is no self-exclusion: the two sets are distinct.  A point with a NaN or infinite coordinate on either
side is near nothing; a difference that overflows fails the comparison by itself.

near_brute: every pair, in blocks.
near_bucket: the given points sorted by neighbours_ref's foreign grid (edge 2 * radius anchored at BUCKET_ORIGIN: it
shares no cell face and no arithmetic with the library's grid), each resident point tested against the 27 cells around
its own.  |d| <= radius * (1 + 2^-22) on an axis for every accepted pair, half a cell, so the 27 cells hold every given
point near it.
Both return (hit_resident bool[n], near_given bool[m]).
"""
import numpy as np

from neighbours_ref import BUCKET_ORIGIN, _d2, f32, finite, r2_of, words  # noqa: F401  (words: re-exported)


def _xyz(a):
    a = np.asarray(a, f32)
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1] if a.ndim == 2 else 3)[:, :3])


def near_brute(A, G, radius, block=512):
    a, g = _xyz(A), _xyz(G)
    oka, okg = finite(a), finite(g)
    r2 = r2_of(radius)
    hit, near = np.zeros(a.shape[0], bool), np.zeros(g.shape[0], bool)
    if g.shape[0] == 0:
        return hit, near
    for s in range(0, a.shape[0], block):
        nb = (_d2(a[s:s + block, None, :], g[None, :, :]) <= r2) & okg[None, :] & oka[s:s + block, None]
        hit[s:s + block] = nb.any(axis=1)
        near |= nb.any(axis=0)
    return hit, near


def _cells(p, radius):
    q = np.floor((p.astype(np.float64) - np.float64(BUCKET_ORIGIN)) / (2.0 * float(f32(radius))))
    return q


def near_bucket(A, G, radius, max_pairs=8_000_000):
    a, g = _xyz(A), _xyz(G)
    r2 = r2_of(radius)
    hit, near = np.zeros(a.shape[0], bool), np.zeros(g.shape[0], bool)
    ga, aa = np.flatnonzero(finite(g)), np.flatnonzero(finite(a))
    if ga.size == 0 or aa.size == 0:
        return hit, near
    qg = _cells(g[ga], radius)
    if np.abs(qg).max() >= 2 ** 20:
        raise ValueError("near_bucket: the given points span more than 2^20 cells")
    qa = _cells(a[aa], radius)
    inr = (np.abs(qa) <= 2 ** 20).all(axis=1)  # (a resident point further out has no given point in its 27 cells)
    aa, qa = aa[inr], qa[inr]
    if aa.size == 0:
        return hit, near
    off = 2 ** 20 + 2
    qg, qa = qg.astype(np.int64) + off, qa.astype(np.int64) + off
    key = (qg[:, 0] << 44) | (qg[:, 1] << 22) | qg[:, 2]
    order = np.argsort(key, kind="stable")
    key, ga = key[order], ga[order]
    gs, ps = g[ga], a[aa]
    akey = (qa[:, 0] << 44) | (qa[:, 1] << 22) | qa[:, 2]
    m = aa.size
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):  # (z is the lowest field: the cells z - 1 .. z + 1 are one key range)
            lo_key = akey + (dx << 44) + (dy << 22) - 1
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
                    nb = _d2(ps[qi], gs[cj]) <= r2
                    hit[aa[qi[nb]]] = True
                    near[ga[cj[nb]]] = True
                s = e
    return hit, near


def near(A, G, radius):
    return near_brute(A, G, radius) if np.asarray(A).shape[0] * max(np.asarray(G).shape[0], 1) <= 3e8 else near_bucket(A, G, radius)


def stats(hit, near_bits, G, sel_after):
    """rtr_select_near's four statistics for hits `hit`, near bits `near_bits` (None: not asked for) and the selection
    after op `sel_after`."""
    return (int(np.count_nonzero(sel_after)), int(hit.sum()), 0 if near_bits is None else int(near_bits.sum()),
            int((~finite(_xyz(G))).sum()) if np.asarray(G).size else 0)
