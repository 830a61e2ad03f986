"""The reference model of rtr_estimate_normals (include/rtr_normals.h section 6o), in numpy only.

Candidates: neighbours_ref's relation -- points i != j with ((dx*dx + dy*dy) + dz*dz) <= r2 in float32, inclusive; a
non-finite point has none and is nobody's.  Row i: the candidates of i in ascending order of (d2 bits, upload index),
the first k of them: index NONE and d2 +inf behind them; found[i] = min(k, candidates).  This is nearest_k_ref's row of
the point itself for k + 1 with its own index dropped (rows_from_nearest_k states it that way).

rows_brute: every pair, in blocks (good to about 8k points).
rows_bucket: neighbours_ref's bucket grid (cells of edge 2 * radius anchored at BUCKET_ORIGIN: not the library's grid).

sums: the nine float64 sums over the row, slot by slot in row order from +0.0 -- an explicit loop over the slots,
vectorised over the points, never np.sum.  covariance: C = S_ab / m - mean_a mean_b with m = found + 1.
jacobi: the contract's 8 cyclic sweeps with + - * / and np.sqrt only, vectorised with masks.  fit: the eigenvector of
the smallest diagonal entry (the first on ties), normalised, signed, rounded to float32, and the curvature.
eigh_of: np.linalg.eigh of the same C -- a second path that shares nothing with the Jacobi.
"""
import numpy as np

import neighbours_ref as nr

f32, f64 = np.float32, np.float64
INF = f32(np.inf)
NONE = 0xFFFFFFFF
MAX_K = 64
MIN_FOUND = 2
SWEEPS = 8
ROTATIONS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))  # (p, q, the third index r)


def _rows_from_pairs(n, k, qi, cj, d2):
    """(index (n, k) uint32 padded with NONE, d2 (n, k) float32 padded with +inf, found (n,) uint32)"""
    idx = np.full((n, k), NONE, np.uint32)
    rows = np.full((n, k), INF, f32)
    found = np.zeros(n, np.uint32)
    if qi.size:
        order = np.lexsort((cj, d2.view(np.uint32), qi))
        qi, cj, d2 = qi[order], cj[order], d2[order]
        first = np.searchsorted(qi, qi, "left")
        rank = np.arange(qi.size) - first
        keep = rank < k
        idx[qi[keep], rank[keep]] = cj[keep].astype(np.uint32)
        rows[qi[keep], rank[keep]] = d2[keep]
        found = np.minimum(np.bincount(qi, minlength=n), k).astype(np.uint32)
    return idx, rows, found


def _cat(parts, dtype):
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def rows_brute(xyz, radius, k, block=512):
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    n = p.shape[0]
    ok = nr.finite(p)
    r2 = nr.r2_of(radius)
    ar = np.arange(n)
    qs, cs, ds = [], [], []
    for s in range(0, n, block):
        d2 = nr._d2(p[s:s + block, None, :], p[None, :, :])
        nb = (d2 <= r2) & ok[None, :] & ok[s:s + block, None] & (ar[s:s + block, None] != ar[None, :])
        a, b = np.nonzero(nb)
        qs.append(a + s)
        cs.append(b)
        ds.append(d2[a, b])
    return _rows_from_pairs(n, k, _cat(qs, np.int64), _cat(cs, np.int64), _cat(ds, f32))


def rows_bucket(xyz, radius, k, max_pairs=8_000_000):
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    n = p.shape[0]
    ok = nr.finite(p)
    r2 = nr.r2_of(radius)
    at = np.flatnonzero(ok)
    qs, cs, ds = [], [], []
    if at.size:
        q = np.floor((p[at].astype(f64) - f64(nr.BUCKET_ORIGIN)) / (2.0 * float(f32(radius))))
        if np.abs(q).max() >= 2 ** 20:
            raise ValueError("rows_bucket: the cloud spans more than 2^20 cells")
        q = q.astype(np.int64) + 2 ** 20 + 1
        key = (q[:, 0] << 44) | (q[:, 1] << 22) | q[:, 2]
        order = np.argsort(key, kind="stable")
        key, at = key[order], at[order]
        ps = p[at]
        m = at.size
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
                        cs.append(at[cj[nb]])
                        ds.append(d2[nb])
                    s = e
    return _rows_from_pairs(n, k, _cat(qs, np.int64), _cat(cs, np.int64), _cat(ds, f32))


def rows(xyz, radius, k):
    return rows_brute(xyz, radius, k) if np.asarray(xyz).shape[0] <= 6000 else rows_bucket(xyz, radius, k)


def cut(rows_k, k):
    """The rows of a smaller k from those of a larger one."""
    idx, d2, found = rows_k
    return np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(d2[:, :k]), np.minimum(found, k).astype(np.uint32)


def rows_from_nearest_k(index, dist2, found, k):
    """nearest_k_ref's rows of the cloud against itself for k + 1 -> this model's rows for k: the own index dropped (it
    is there whenever the point is finite: d2 == +0 at the smallest index of its coincident pile or later), the row cut
    to k."""
    n = index.shape[0]
    idx = np.full((n, k), NONE, np.uint32)
    d2 = np.full((n, k), INF, f32)
    fd = np.zeros(n, np.uint32)
    for i in range(n):
        real = index[i, :found[i]]
        keep = np.flatnonzero(real != i)[:k]
        idx[i, :keep.size] = real[keep]
        d2[i, :keep.size] = dist2[i, keep]
        fd[i] = keep.size
    return idx, d2, fd


def sums(xyz, idx, found):
    """(S (n, 3), Q (n, 6)) float64: the sums of dx, dy, dz and of dx dx, dx dy, dx dz, dy dy, dy dz, dz dz over each
    row, slot by slot."""
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    n, k = idx.shape
    S = np.zeros((n, 3), f64)
    Q = np.zeros((n, 6), f64)
    for t in range(k):
        has = found > t
        if not has.any():
            break
        j = np.where(has, idx[:, t], 0).astype(np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            e = (p - p[j]).astype(f64)  # (float32 differences, as the pair test forms them, then widened: exact)
        c = 0
        for a in range(3):
            S[:, a] = np.where(has, S[:, a] + e[:, a], S[:, a])
        for a in range(3):
            for b in range(a, 3):
                Q[:, c] = np.where(has, Q[:, c] + e[:, a] * e[:, b], Q[:, c])
                c += 1
    return S, Q


def covariance(S, Q, found):
    """C (n, 3, 3) float64, symmetric by construction; rows with found < MIN_FOUND are computed all the same."""
    m = found.astype(f64) + 1.0
    mean = S / m[:, None]
    C = np.zeros((S.shape[0], 3, 3), f64)
    c = 0
    for a in range(3):
        for b in range(a, 3):
            C[:, a, b] = C[:, b, a] = Q[:, c] / m - mean[:, a] * mean[:, b]
            c += 1
    return C


def jacobi(C, sweeps=SWEEPS):
    """(A, V): the contract's cyclic Jacobi on every C at once; A's diagonal holds the eigenvalues, V's columns the
    vectors.  Every operation is a numpy float64 ufunc on its own: no FMA, no dot product."""
    A = np.array(C, f64)
    n = A.shape[0]
    V = np.zeros((n, 3, 3), f64)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    for _ in range(sweeps):
        for p, q, r in ROTATIONS:
            apq = A[:, p, q].copy()
            on = apq != 0.0
            with np.errstate(all="ignore"):
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                app, aqq = A[:, p, p] - h, A[:, q, q] + h
                arp, arq = c * A[:, r, p] - s * A[:, r, q], s * A[:, r, p] + c * A[:, r, q]
                vp, vq = c[:, None] * V[:, :, p] - s[:, None] * V[:, :, q], s[:, None] * V[:, :, p] + c[:, None] * V[:, :, q]
            A[:, p, p] = np.where(on, app, A[:, p, p])
            A[:, q, q] = np.where(on, aqq, A[:, q, q])
            A[:, p, q] = A[:, q, p] = np.where(on, 0.0, apq)
            A[:, r, p] = A[:, p, r] = np.where(on, arp, A[:, r, p])
            A[:, r, q] = A[:, q, r] = np.where(on, arq, A[:, r, q])
            V[:, :, p] = np.where(on[:, None], vp, V[:, :, p])
            V[:, :, q] = np.where(on[:, None], vq, V[:, :, q])
    return A, V


def fit(xyz, C, found, viewpoint=None):
    """(normals (n, 3) float32, curvature (n,) float32, flipped (n,) bool) from the covariances."""
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    n = p.shape[0]
    have = found >= MIN_FOUND
    A, V = jacobi(np.where(have[:, None, None], C, 0.0))
    lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1)
    a = np.zeros(n, np.int64)
    la = lam[:, 0].copy()
    for b in (1, 2):
        less = lam[:, b] < la
        a = np.where(less, b, a)
        la = np.where(less, lam[:, b], la)
    ar = np.arange(n)
    w = V[ar, :, a]
    L = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    nv = w / L[:, None]
    mag = np.abs(nv)
    big = np.zeros(n, np.int64)
    top = mag[:, 0].copy()
    for b in (1, 2):
        more = mag[:, b] > top
        big = np.where(more, b, big)
        top = np.where(more, mag[:, b], top)
    nv = np.where((nv[ar, big] < 0.0)[:, None], -nv, nv)
    flipped = np.zeros(n, bool)
    if viewpoint is not None:
        vp = np.asarray(viewpoint, f32).astype(f64)
        with np.errstate(invalid="ignore", over="ignore"):
            d = vp[None, :] - p.astype(f64)
            g = (nv[:, 0] * d[:, 0] + nv[:, 1] * d[:, 1]) + nv[:, 2] * d[:, 2]
            flipped = have & (g < 0.0)
        nv = np.where(flipped[:, None], -nv, nv)
    lp = np.where(lam > 0.0, lam, 0.0)
    tot = (lp[:, 0] + lp[:, 1]) + lp[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.where(tot == 0.0, 0.0, lp[ar, a] / tot).astype(f32)
    normals = np.where(have[:, None], nv, 0.0).astype(f32)
    curv = np.where(have, curv, INF).astype(f32)
    return normals, curv, flipped


def eigh_of(C):
    """np.linalg.eigh of every C: (eigenvalues ascending (n, 3), vectors (n, 3, 3) in columns)."""
    return np.linalg.eigh(np.asarray(C, f64))


def stats(xyz, found, flipped):
    """rtr_estimate_normals' four statistics."""
    ok = nr.finite(xyz)
    have = found >= MIN_FOUND
    return int(have.sum()), int((ok & ~have).sum()), int((~ok).sum()), int(flipped.sum())


def estimate(xyz, radius, k, viewpoint=None, rows_k=None):
    """Everything at once: dict(index, d2, found, C, normals, curvature, flipped, stats).  rows_k: rows(xyz, radius, K) of
    some K >= k, to share."""
    idx, d2, found = cut(rows_k if rows_k is not None else rows(xyz, radius, k), k)
    S, Q = sums(xyz, idx, found)
    C = covariance(S, Q, found)
    normals, curv, flipped = fit(xyz, C, found, viewpoint)
    return {"index": idx, "d2": d2, "found": found, "S": S, "Q": Q, "C": C, "normals": normals, "curvature": curv, "flipped": flipped,
            "stats": stats(xyz, found, flipped)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
