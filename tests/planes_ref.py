"""Reference answers of rtr_count_in_bands and rtr_fit_plane (include/rtr.h section 6j): the band test in numpy float32 in
the contract's order, the sampler in Python integers modulo 2^64, the candidate plane in numpy float64 in the order of
csrc/rtr_plane_fit.h, and the RANSAC loop over them.  Nothing here has a tolerance."""
import numpy as np

MASK = (1 << 64) - 1
MAX_BANDS = 4096


def in_band(xyz, band):
    """bool [n]: u + d_lo >= 0 and (-u) + d_hi >= 0, u = (a*x + b*y) + c*z, every operation rounded to float32."""
    f = np.float32
    p = np.asarray(xyz, np.float32)
    a, b, c, lo, hi = (f(v) for v in np.asarray(band, np.float32).reshape(5))
    with np.errstate(all="ignore"):
        u = (a * p[:, 0] + b * p[:, 1]) + c * p[:, 2]
        return ((u + lo) >= 0) & (((-u) + hi) >= 0)


def two_planes(band):
    """The band's two section 6d planes, as rtr_select_points takes them."""
    a, b, c, lo, hi = np.asarray(band, np.float32).reshape(5)
    return np.array([[a, b, c, lo], [-a, -b, -c, hi]], np.float32)


def counts(xyz, bands, population=None):
    """uint64 [k]: the points of the population (bool [n]; None: every point) in each band."""
    bands = np.asarray(bands, np.float32).reshape(-1, 5)
    pop = np.ones(len(xyz), bool) if population is None else np.asarray(population, bool)
    pts = np.asarray(xyz, np.float32)[pop]
    return np.array([int(in_band(pts, b).sum()) for b in bands], np.uint64)


def draw(seed, t):
    """Draw t of the stream `seed`: splitmix64's output over the state seed + (t + 1) * golden."""
    z = (seed + (t + 1) * 0x9E3779B97F4A7C15) & MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def ranks(seed, iterations, m):
    """int [iterations, 3]: the ranks of every candidate's three draws in a population of m > 0."""
    return np.array([[draw(seed, 3 * c + j) % m for j in range(3)] for c in range(iterations)], dtype=object)


def candidate(p0, p1, p2, r):
    """float32 [4] plane of the sample, or None when it is DEGENERATE."""
    if r[0] == r[1] or r[0] == r[2] or r[1] == r[2]:
        return None
    p = np.asarray([p0, p1, p2], np.float32)[:, :3].astype(np.float64)
    if not np.isfinite(p).all():
        return None
    with np.errstate(all="ignore"):
        x0, y0, z0 = p[0]
        e1, e2 = p[1] - p[0], p[2] - p[0]
        nx = e1[1] * e2[2] - e1[2] * e2[1]
        ny = e1[2] * e2[0] - e1[0] * e2[2]
        nz = e1[0] * e2[1] - e1[1] * e2[0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        if not (np.isfinite(ln) and ln > 0):
            return None
        A = [nx / ln, ny / ln, nz / ln]
        if A[2] < 0 or (A[2] == 0 and (A[1] < 0 or (A[1] == 0 and A[0] < 0))):
            A = [-A[0], -A[1], -A[2]]
        D = -((A[0] * x0 + A[1] * y0) + A[2] * z0)
        plane = np.array([A[0], A[1], A[2], D], np.float64).astype(np.float32)
    return plane if np.isfinite(plane[3]) else None


def band_of(plane, dist):
    """float32 [5]: {a, b, c, d + dist, dist - d}, each sum one float32 operation."""
    p = np.asarray(plane, np.float32).reshape(4)
    d = np.float32(dist)
    with np.errstate(all="ignore"):
        return np.array([p[0], p[1], p[2], p[3] + d, d - p[3]], np.float32)


def fit(xyz, dist, iterations, seed=0, population=None):
    """-> (plane float32 [4], stats (count, non-degenerate candidates, the winner's c, population size)); the plane is
    all zeros when every candidate is degenerate."""
    xyz = np.asarray(xyz, np.float32)[:, :3]
    idx = np.arange(len(xyz)) if population is None else np.flatnonzero(np.asarray(population, bool))
    m = len(idx)
    planes, who = [], []
    if m >= 3:
        for c, r in enumerate(ranks(seed & MASK, iterations, m)):
            pl = candidate(xyz[idx[int(r[0])]], xyz[idx[int(r[1])]], xyz[idx[int(r[2])]], r)
            if pl is not None and np.isfinite(band_of(pl, dist)).all():
                planes.append(pl), who.append(c)
    if not planes:
        return np.zeros(4, np.float32), (0, 0, 0, m)
    cnt = counts(xyz, [band_of(pl, dist) for pl in planes], None if population is None else population)
    best = int(np.argmax(cnt))  # (the first of the largest: the smallest c)
    return planes[best], (int(cnt[best]), len(planes), who[best], m)
