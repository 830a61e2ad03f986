"""The reference model of rtr_register_points (include/rtr_register.h section 6p), in numpy only.

posed:      p' = ((T_a0 x + T_a1 y) + T_a2 z) + T_a3 in float64, every operation on its own, rounded to float32.
pairs:      nearest_ref's given side on the p' (q = the winner's coordinates, n = its normal); in plane mode a pair
            whose normal has a non-finite component or is exactly (0, 0, 0) is dropped.
fold:       the summation shape, as explicit loops: blocks of 1024 given indices, thread t adding j = 1024 c + t, + 256,
            + 512, + 768 in that order from +0.0, the 64 lanes folded by a butterfly, the four waves added in order, the
            blocks' sums folded the same way.  No np.sum anywhere.
terms:      the terms of both passes as explicit float64 ufunc steps.
fit_point / fit_plane / compose: csrc/rtr_register_fit.h in Python floats (IEEE doubles: + - * / and math.sqrt are
            correctly rounded and never fused).
register:   one call: (moments[32], step[12], stats).   loop: ProjectCloud.registerPoints.
kabsch / plane_solve: the two independent paths, np.linalg.svd and np.linalg.solve on the same pairs.
"""
import math

import numpy as np

import nearest_ref as nr
from near_ref import _xyz

f32, f64 = np.float32, np.float64
MOMENTS = 32
POINT_TO_PLANE = 1
SWEEPS = 12
POINT_RESIDUAL, PLANE_RESIDUAL = 16, 31
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def bits64(a):
    return np.ascontiguousarray(a, f64).view(np.uint64)


def posed(G, pose):
    g = np.ascontiguousarray(_xyz(G), f32)
    if pose is None:
        return g.copy()
    T = np.asarray(pose, f64).reshape(3, 4)
    x, y, z = (g[:, k].astype(f64) for k in range(3))
    out = np.empty_like(g)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for a in range(3):
            out[:, a] = (((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]).astype(f32)
    return out


def pairs(A, P, radius, normals=None, finder=None):
    """(winner index uint32[m] with NONE, used bool[m]) of the posed points P."""
    gi = (finder or nr.nearest)(A, P, radius)[0]
    used = gi != nr.NONE
    if normals is not None and used.any():
        nrm = np.asarray(normals, f32).reshape(-1, 3)[gi[used]]
        ok = np.isfinite(nrm).all(axis=1) & (nrm != 0).any(axis=1)
        used[np.flatnonzero(used)[~ok]] = False
    return gi, used


def _block(v):
    """(blocks, 256) thread values -> (blocks,): the butterfly over each wave's 64 lanes, then the four waves in order"""
    w = v.reshape(-1, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ off]
    w = w[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def fold(terms, count):
    """terms: (count, k) float64, rows without a pair all +0.0 -> the k sums in the fixed shape"""
    k = terms.shape[1]
    nb = (count + 1023) // 1024
    out = np.zeros(k, f64)
    if nb == 0:
        return out
    pad = np.zeros((nb * 1024, k), f64)
    pad[:count] = terms
    pad = pad.reshape(nb, 4, 256, k)
    for s in range(k):
        v = np.zeros((nb, 256), f64)
        for j in range(4):  # (thread t: 1024 c + t, + 256, + 512, + 768)
            v = v + pad[:, j, :, s]
        part = _block(v)
        t = np.zeros(256, f64)
        for c0 in range(0, nb, 256):  # (thread t: partial[t], [t + 256], ...)
            row = np.zeros(256, f64)
            row[:min(256, nb - c0)] = part[c0:c0 + 256]
            t = t + row
        out[s] = _block(t[None, :])[0]
    return out


def _masked(cols, used):
    t = np.stack(cols, axis=1)
    return np.where(used[:, None], t, 0.0)


def terms0(p, q, used):
    one = np.ones(p.shape[0], f64)
    return _masked([one] + [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)], used)


def terms_point(p, q, used, pbar, qbar):
    u = [p[:, a] - pbar[a] for a in range(3)]
    v = [q[:, a] - qbar[a] for a in range(3)]
    d = [p[:, a] - q[:, a] for a in range(3)]
    e = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return _masked([u[a] * v[b] for a in range(3) for b in range(3)] + [e], used)


def terms_plane(p, q, n, used, pbar):
    u = [p[:, a] - pbar[a] for a in range(3)]
    a = [u[1] * n[:, 2] - u[2] * n[:, 1], u[2] * n[:, 0] - u[0] * n[:, 2], u[0] * n[:, 1] - u[1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]]
    b = (n[:, 0] * (q[:, 0] - p[:, 0]) + n[:, 1] * (q[:, 1] - p[:, 1])) + n[:, 2] * (q[:, 2] - p[:, 2])
    return _masked([a[r] * a[s] for r in range(6) for s in range(r, 6)] + [a[r] * b for r in range(6)] + [b * b], used)


def moments_of(A, P, gi, used, normals=None):
    """moments[32] of the posed points P (float32) and their pairs"""
    a = np.ascontiguousarray(_xyz(A), f32)
    m = P.shape[0]
    p = P.astype(f64)
    q = np.zeros((m, 3), f64)
    q[used] = a[gi[used]].astype(f64)
    p = np.where(used[:, None], p, 0.0)  # (rows without a pair never reach a sum: NaN and inf stay out of the products)
    mom = np.zeros(MOMENTS, f64)
    s0 = fold(terms0(p, q, used), m)
    c = s0[0]
    mom[0] = c
    if not c > 0:
        return mom
    mom[1:7] = s0[1:7] / c
    if normals is None:
        mom[7:17] = fold(terms_point(p, q, used, mom[1:4], mom[4:7]), m)
    else:
        n = np.zeros((m, 3), f64)
        n[used] = np.asarray(normals, f32).reshape(-1, 3)[gi[used]].astype(f64)
        mom[4:32] = fold(terms_plane(p, q, n, used, mom[1:4]), m)  # (qbar is not returned in plane mode)
    return mom


# ---- the step: csrc/rtr_register_fit.h ------------------------------------------------------------------------------
def _rotate(A, V, p, q):
    apq = A[p][q]
    if apq == 0.0:
        return
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    tt = theta * theta + 1.0
    t = 1.0 / (abs(theta) + (math.sqrt(tt) if tt < math.inf else math.inf))
    if theta < 0.0:
        t = -t
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    A[p][p] = A[p][p] - h
    A[q][q] = A[q][q] + h
    A[p][q] = A[q][p] = 0.0
    for r in range(4):
        if r in (p, q):
            continue
        A[r][p], A[r][q] = c * A[r][p] - s * A[r][q], s * A[r][p] + c * A[r][q]
        A[p][r], A[q][r] = A[r][p], A[r][q]
    for r in range(4):
        V[r][p], V[r][q] = c * V[r][p] - s * V[r][q], s * V[r][p] + c * V[r][q]


def horn(S, sweeps=SWEEPS):
    """(A, V) after the sweeps: Horn's N from the row-major cross sums"""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (float(v) for v in S)
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0], A[0][1], A[0][2], A[0][3] = (xx + yy) + zz, yz - zy, zx - xz, xy - yx
    A[1][1], A[1][2], A[1][3] = (xx - yy) - zz, xy + yx, zx + xz
    A[2][2], A[2][3] = (yy - xx) - zz, yz + zy
    A[3][3] = (zz - xx) - yy
    for i in range(4):
        for j in range(i):
            A[i][j] = A[j][i]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(sweeps):
        for p in range(3):
            for q in range(p + 1, 4):
                _rotate(A, V, p, q)
    return A, V


def _put(R, base, p, add):
    step = [0.0] * 12
    for a in range(3):
        rp = (R[3 * a] * p[0] + R[3 * a + 1] * p[1]) + R[3 * a + 2] * p[2]
        step[4 * a:4 * a + 3] = R[3 * a:3 * a + 3]
        step[4 * a + 3] = (base[a] - rp) + add[a] if add is not None else base[a] - rp
    return step


def fit_point(mom):
    """(step[12], degenerate)"""
    mom = [float(v) for v in mom]
    if not mom[0] >= 3.0:
        return list(IDENTITY), True
    A, V = horn(mom[7:16])
    k = 0
    for i in range(1, 4):
        if A[i][i] > A[k][k]:
            k = i
    w, x, y, z = V[0][k], V[1][k], V[2][k], V[3][k]
    L = math.sqrt(((w * w + x * x) + y * y) + z * z)
    if not (L > 0.0 and L < math.inf):
        return list(IDENTITY), True
    w, x, y, z = w / L, x / L, y / L, z / L
    if w < 0.0 or (w == 0.0 and (x < 0.0 or (x == 0.0 and (y < 0.0 or (y == 0.0 and z < 0.0))))):
        w, x, y, z = -w, -x, -y, -z
    R = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
         2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]
    return _put(R, mom[4:7], mom[1:4], None), False


def fit_plane(mom):
    mom = [float(v) for v in mom]
    if not mom[0] >= 6.0:
        return list(IDENTITY), True
    A = [[0.0] * 6 for _ in range(6)]
    at = 4
    for r in range(6):
        for s in range(r, 6):
            A[r][s] = A[s][r] = mom[at]
            at += 1
    Lm = [[0.0] * 6 for _ in range(6)]
    W = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    for j in range(6):
        v = A[j][j]
        for k in range(j):
            W[j][k] = Lm[j][k] * d[k]
            v = v - Lm[j][k] * W[j][k]
        if not (v > 0.0 and v < math.inf):
            return list(IDENTITY), True
        d[j] = v
        for i in range(j + 1, 6):
            u = A[i][j]
            for k in range(j):
                u = u - Lm[i][k] * W[j][k]
            Lm[i][j] = u / v
    x = [0.0] * 6
    for i in range(6):
        v = mom[25 + i]
        for k in range(i):
            v = v - Lm[i][k] * x[k]
        x[i] = v
    for i in range(6):
        x[i] = x[i] / d[i]
    for i in range(5, -1, -1):
        v = x[i]
        for k in range(i + 1, 6):
            v = v - Lm[k][i] * x[k]
        x[i] = v
    if not all(math.isfinite(v) for v in x):
        return list(IDENTITY), True
    w0, w1, w2 = x[0] / 2.0, x[1] / 2.0, x[2] / 2.0
    m = (w0 * w0 + w1 * w1) + w2 * w2
    k = 2.0 / (1.0 + m)
    R = [1.0 + k * (w0 * w0 - m), k * (w0 * w1 - w2), k * (w0 * w2 + w1),
         k * (w1 * w0 + w2), 1.0 + k * (w1 * w1 - m), k * (w1 * w2 - w0),
         k * (w2 * w0 - w1), k * (w2 * w1 + w0), 1.0 + k * (w2 * w2 - m)]
    return _put(R, mom[1:4], mom[1:4], x[3:6]), False


def compose(step, pose):
    s, p = [float(v) for v in np.asarray(step).reshape(-1)], [float(v) for v in np.asarray(pose).reshape(-1)]
    out = [0.0] * 12
    for a in range(3):
        for b in range(4):
            v = (s[4 * a] * p[b] + s[4 * a + 1] * p[4 + b]) + s[4 * a + 2] * p[8 + b]
            if b == 3:
                v = v + s[4 * a + 3]
            out[4 * a + b] = v
    return out


def rms_of(mom, plane):
    c = float(mom[0])
    return math.sqrt(float(mom[PLANE_RESIDUAL if plane else POINT_RESIDUAL]) / c) if c > 0 else math.inf


def register(A, G, radius, flags=0, pose=None, normals=None, finder=None):
    """One call: (moments float64[32], step float64[12], stats (4 ints))."""
    plane = bool(flags & POINT_TO_PLANE)
    P = posed(G, pose)
    gi, used = pairs(A, P, radius, normals if plane else None, finder)
    mom = moments_of(A, P, gi, used, normals if plane else None)
    step, deg = (fit_plane if plane else fit_point)(mom)
    fin = np.isfinite(P).all(axis=1) if P.shape[0] else np.zeros(0, bool)
    stats = (int(used.sum()), int(fin.sum() - used.sum()), int((~fin).sum()), int(deg))
    return mom, np.array(step, f64), stats


def loop(A, G, radius, iterations=20, plane=False, normals=None, pose=None, finder=None):
    """ProjectCloud.registerPoints: (pose 4x4 float64, [rms per iteration], last stats)."""
    cur = list(IDENTITY) if pose is None else [float(v) for v in np.asarray(pose, f64).reshape(-1)[:12]]
    rms, stats, prev = [], (0, 0, 0, 0), None
    for _ in range(iterations):
        mom, step, stats = register(A, G, radius, POINT_TO_PLANE if plane else 0, cur, normals, finder)
        r = rms_of(mom, plane)
        rms.append(r)
        if stats[3]:
            break
        if prev is not None and stats[0] == prev[0] and not r < prev[1]:
            break
        prev = (stats[0], r)
        cur = compose(step, cur)
    out = np.eye(4)
    out[:3] = np.array(cur, f64).reshape(3, 4)
    return out, rms, stats


# ---- the independent paths --------------------------------------------------------------------------------------------
def kabsch(p, q):
    """np.linalg.svd on the pairs p -> q (float64 (k, 3)): (R, t)"""
    pb, qb = p.mean(axis=0), q.mean(axis=0)
    H = (p - pb).T @ (q - qb)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, qb - R @ pb


def plane_solve(p, q, n):
    """np.linalg.solve of the linearised point-to-plane system about the mean of p: (omega, tau, pbar)"""
    pb = p.mean(axis=0)
    a = np.concatenate([np.cross(p - pb, n), n], axis=1)
    b = np.einsum("ij,ij->i", n, q - p)
    x = np.linalg.solve(a.T @ a, a.T @ b)
    return x[:3], x[3:], pb


def rotation_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return math.acos(max(-1.0, min(1.0, c))) if abs(c) < 1 - 1e-12 else float(np.linalg.norm(Ra - Rb) / math.sqrt(2.0))
