"""The reference model of rtr_select_neighbours (include/rtr.h section 6h), in numpy only.

Neighbour relation: with r2 = float32(radius) * float32(radius), points i != j are neighbours iff
((dx*dx + dy*dy) + dz*dz) <= r2, dx = x[i] - x[j] ..., every operation in float32 on its own.  A point with a NaN or
infinite coordinate has no neighbours and is nobody's; a difference that overflows fails the comparison by itself.

counts_brute: every pair, in blocks (good to about 8k points).
counts_bucket: the points sorted by a cell of edge 2 * radius anchored at BUCKET_ORIGIN (not the library's grid: its cells
are of edge radius * (1 + 2^-10) and anchored at 0, so the two share no cell face and no arithmetic), each point tested
against the 27 cells around its own.  |d| <= radius * (1 + 2^-22) on an axis for every accepted pair, half a cell, so
the 27 cells hold every neighbour.
"""
import numpy as np

f32 = np.float32
BUCKET_ORIGIN = (0.37, -1.21, 0.083)


def r2_of(radius):
    return f32(radius) * f32(radius)


def finite(xyz):
    return np.isfinite(np.asarray(xyz, f32)[:, :3]).all(axis=1)


def _d2(a, b):
    """float32 in the contract's order; a, b broadcastable (.., 3)."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def counts_brute(xyz, radius, block=512):
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    n = p.shape[0]
    ok = finite(p)
    r2 = r2_of(radius)
    out = np.zeros(n, np.int64)
    idx = np.arange(n)
    for s in range(0, n, block):
        d2 = _d2(p[s:s + block, None, :], p[None, :, :])
        nb = (d2 <= r2) & ok[None, :] & ok[s:s + block, None] & (idx[s:s + block, None] != idx[None, :])
        out[s:s + block] = nb.sum(axis=1)
    return out


def counts_bucket(xyz, radius, max_pairs=8_000_000):
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    n = p.shape[0]
    ok = finite(p)
    r2 = r2_of(radius)
    out = np.zeros(n, np.int64)
    at = np.flatnonzero(ok)
    if at.size == 0:
        return out
    q = np.floor((p[at].astype(np.float64) - np.float64(BUCKET_ORIGIN)) / (2.0 * float(f32(radius))))
    if np.abs(q).max() >= 2 ** 20:
        raise ValueError("counts_bucket: the cloud spans more than 2^20 cells")
    q = q.astype(np.int64) + 2 ** 20 + 1  # (1 .. 2^21: a neighbouring cell's field stays within 22 bits)
    key = (q[:, 0] << 44) | (q[:, 1] << 22) | q[:, 2]
    order = np.argsort(key, kind="stable")
    key, at = key[order], at[order]  # at: upload index of sorted position
    ps = p[at]
    m = at.size
    got = np.zeros(m, np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):  # (z is the lowest field: the cells z - 1 .. z + 1 are one key range)
            lo_key = key + (dx << 44) + (dy << 22) - 1
            start = np.searchsorted(key, lo_key, "left")
            cnt = np.searchsorted(key, lo_key + 2, "right") - start
            cum = np.cumsum(cnt)
            s = 0
            while s < m:  # (query points s .. e - 1: at most max_pairs pairs at a time, at least one point)
                e = int(np.searchsorted(cum, (cum[s - 1] if s else 0) + max_pairs, "right"))
                e = min(max(e, s + 1), m)
                c = cnt[s:e]
                total = int(c.sum())
                if total:
                    qi = np.repeat(np.arange(s, e), c)
                    first = np.cumsum(c) - c
                    cj = np.repeat(start[s:e] - first, c) + np.arange(total)
                    nb = (_d2(ps[qi], ps[cj]) <= r2) & (at[qi] != at[cj])
                    got[s:e] += np.bincount(qi[nb] - s, minlength=e - s)
                s = e
    out[at] = got
    return out


def counts(xyz, radius):
    return counts_brute(xyz, radius) if np.asarray(xyz).shape[0] <= 6000 else counts_bucket(xyz, radius)


def select(xyz, radius, min_neighbours, cnt=None):
    """(hit, (stats[1], stats[2], stats[3])): hit[i] iff point i has at least min_neighbours neighbours; the points with
    that many, the finite points with none at all, the non-finite points.  cnt: counts(xyz, radius), to share."""
    if cnt is None:
        cnt = counts(xyz, radius)
    ok = finite(xyz)
    hit = cnt >= int(min_neighbours)
    return hit, (int(hit.sum()), int((ok & (cnt == 0)).sum()), int((~ok).sum()))


def words(hit):
    """RTR_BUF_SELECTION's download of a selection: (n + 31) / 32 little-endian words."""
    n = hit.size
    bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
    bits[:n] = hit
    return np.packbits(bits, bitorder="little").view(np.uint32)
