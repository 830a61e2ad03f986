"""The reference model of rtr_select_statistical (include/rtr_statistics.h section 6n), in numpy only.

Candidates: neighbours_ref's relation -- points i != j with ((dx*dx + dy*dy) + dz*dz) <= r2 in float32, inclusive; a
non-finite point has none and is nobody's.  Row i: the k smallest d2 of i's candidates in ascending order of their bits
(d2 >= +0, so of their values), padded with +inf; found[i] = min(k, candidates).  mean[i] = the float32 sequential sum of
np.sqrt(row) over the real entries (np.cumsum in float32) divided by float32(found[i]); +inf where found is 0.

rows_brute: every pair, in blocks (good to about 8k points).
rows_bucket: neighbours_ref's bucket grid (cells of edge 2 * radius anchored at BUCKET_ORIGIN: not the library's grid),
every accepted pair listed, sorted by (query, d2), the first k of each query kept.

Moments in float64 over the points with found > 0: mu = sum / c, sigma = sqrt(sum((mean - mu)^2) / (c - 1)) (0 for c < 2,
both 0 for c = 0), t = mu + std_mul * sigma.  numpy's sums run in its own order: the library's differ by at most
moments_tolerance(c) relative.  hit = found > 0 and float64(mean) <= t.
"""
import numpy as np

import neighbours_ref as nr

f32 = np.float32
INF = f32(np.inf)


def _rows_from_pairs(n, k, qi, d2):
    """(rows (n, k) float32 padded with +inf, found (n,) uint32) from the accepted pairs' query indices and d2."""
    rows = np.full((n, k), INF, f32)
    found = np.zeros(n, np.uint32)
    if qi.size:
        order = np.lexsort((d2.view(np.uint32), qi))
        qi, d2 = qi[order], d2[order]
        first = np.searchsorted(qi, qi, "left")
        rank = np.arange(qi.size) - first
        keep = rank < k
        rows[qi[keep], rank[keep]] = d2[keep]
        found = np.minimum(np.bincount(qi, minlength=n), k).astype(np.uint32)
    return rows, found


def rows_brute(xyz, radius, k, block=512):
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    n = p.shape[0]
    ok = nr.finite(p)
    r2 = nr.r2_of(radius)
    idx = np.arange(n)
    qs, ds = [], []
    for s in range(0, n, block):
        d2 = nr._d2(p[s:s + block, None, :], p[None, :, :])
        nb = (d2 <= r2) & ok[None, :] & ok[s:s + block, None] & (idx[s:s + block, None] != idx[None, :])
        a, b = np.nonzero(nb)
        qs.append(a + s)
        ds.append(d2[a, b])
    return _rows_from_pairs(n, k, np.concatenate(qs) if qs else np.zeros(0, np.int64), np.concatenate(ds) if ds else np.zeros(0, f32))


def rows_bucket(xyz, radius, k, max_pairs=8_000_000):
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    n = p.shape[0]
    ok = nr.finite(p)
    r2 = nr.r2_of(radius)
    at = np.flatnonzero(ok)
    if at.size == 0:
        return _rows_from_pairs(n, k, np.zeros(0, np.int64), np.zeros(0, f32))
    q = np.floor((p[at].astype(np.float64) - np.float64(nr.BUCKET_ORIGIN)) / (2.0 * float(f32(radius))))
    if np.abs(q).max() >= 2 ** 20:
        raise ValueError("rows_bucket: the cloud spans more than 2^20 cells")
    q = q.astype(np.int64) + 2 ** 20 + 1
    key = (q[:, 0] << 44) | (q[:, 1] << 22) | q[:, 2]
    order = np.argsort(key, kind="stable")
    key, at = key[order], at[order]
    ps = p[at]
    m = at.size
    qs, ds = [], []
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
                    d2 = nr._d2(ps[qi], ps[cj])
                    nb = (d2 <= r2) & (at[qi] != at[cj])
                    qs.append(at[qi[nb]])
                    ds.append(d2[nb])
                s = e
    return _rows_from_pairs(n, k, np.concatenate(qs), np.concatenate(ds))


def rows(xyz, radius, k):
    return rows_brute(xyz, radius, k) if np.asarray(xyz).shape[0] <= 6000 else rows_bucket(xyz, radius, k)


def cut(rows_k, found_k, k):
    """The rows and found of a smaller k from those of a larger one."""
    return np.ascontiguousarray(rows_k[:, :k]), np.minimum(found_k, k).astype(np.uint32)


def means(rows_k, found_k):
    """float32, upload order: the contract's sequential sum of square roots and its division; +inf where found is 0."""
    n, k = rows_k.shape
    with np.errstate(invalid="ignore", over="ignore"):
        cum = np.cumsum(np.sqrt(rows_k), axis=1, dtype=f32)
    out = np.full(n, INF, f32)
    has = found_k > 0
    out[has] = cum[has, found_k[has].astype(np.int64) - 1] / found_k[has].astype(f32)
    return out


def moments(mean, found, std_mul):
    """(mu, sigma, t) in numpy float64."""
    md = mean[found > 0].astype(np.float64)
    c = md.size
    mu = float(md.sum() / c) if c else 0.0
    sigma = float(np.sqrt(((md - mu) ** 2).sum() / (c - 1))) if c >= 2 else 0.0
    return mu, sigma, mu + float(std_mul) * sigma


def moments_tolerance(c):
    """Relative: the order of a sum of c non-negative doubles moves it by at most (c - 1) 2^-53; 64 c 2^-53 leaves a
    cushion for the square root, the division and the mean's own error inside the squares."""
    return 64.0 * max(int(c), 1) * 2.0 ** -53


def hits(mean, found, t):
    with np.errstate(invalid="ignore"):
        return (found > 0) & (mean.astype(np.float64) <= float(t))


def stats(xyz, found, hit):
    """(stats[1], stats[2], stats[3]): hits before `outside`, finite points with found == 0, non-finite points."""
    ok = nr.finite(xyz)
    return int(hit.sum()), int((ok & (found == 0)).sum()), int((~ok).sum())


def select(xyz, radius, k, std_mul=1.0, threshold=None, rows_found=None):
    """Everything at once: dict(rows, found, mean, moments, hit, stats).  rows_found: rows(xyz, radius, K) of some
    K >= k, to share."""
    rk, fk = rows_found if rows_found is not None else rows(xyz, radius, k)
    rk, fk = cut(rk, fk, k)
    mean = means(rk, fk)
    mu, sigma, t = moments(mean, fk, std_mul)
    if threshold is not None:
        t = float(threshold)
    hit = hits(mean, fk, t)
    return {"rows": rk, "found": fk, "mean": mean, "moments": (mu, sigma, t), "hit": hit, "stats": stats(xyz, fk, hit)}
