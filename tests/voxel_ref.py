"""Reference answers of rtr_select_voxel_grid (include/rtr.h section 6g) in numpy float32: the contract is exact, so the
words compare with np.array_equal.  words / unpack / combine are select_ref's."""
import numpy as np

from select_ref import combine, unpack, words  # noqa: F401  (re-exported)

SPAN = 2 ** 20
OUT = np.uint64(1) << np.uint64(63)


def cells(xyz, cell, origin=(0, 0, 0)):
    """(in_grid bool [n], key int64 [n]): key = q0 << 42 | q1 << 21 | q2 with q = floor(t) + 2^20 for the points in the
    grid (0 elsewhere); t = (p - origin) * (1 / cell), every operation rounded to float32 on its own."""
    f = np.float32
    xyz = np.asarray(xyz, f)[:, :3]
    cell3 = np.broadcast_to(np.asarray(cell, f), (3,))
    origin3 = np.asarray(origin, f).reshape(3)
    with np.errstate(all="ignore"):
        inv = (f(1) / cell3).astype(f)
        t = ((xyz - origin3[None, :]).astype(f) * inv[None, :]).astype(f)
        ok = (np.isfinite(t) & (t >= f(-SPAN)) & (t < f(SPAN))).all(axis=1)
        q = np.where(ok[:, None], np.floor(t), 0).astype(np.int64) + SPAN
    key = np.where(ok, (q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2], 0)
    return ok, key


def keys_u64(xyz, cell, origin=(0, 0, 0)):
    """rtr::voxel_key of every point: the 63-bit key, or 1 << 63 for a point out of the grid."""
    ok, key = cells(xyz, cell, origin)
    return np.where(ok, key.astype(np.uint64), OUT)


def runs(xyz, cell, origin=(0, 0, 0)):
    """(in_grid bool [n], the first point in upload order of every occupied cell, the cells' populations): what select
    derives every min_count from -- compute it once per cloud and grid."""
    ok, key = cells(xyz, cell, origin)
    idx = np.flatnonzero(ok)
    _, first, counts = np.unique(key[idx], return_index=True, return_counts=True)
    return ok, idx[first], counts


def select(xyz, cell, origin=(0, 0, 0), min_count=1, of=None):
    """(hit bool [n], (occupied in-grid cells, those with >= min_count points, out-of-grid points)): hit = the first
    point in upload order of every cell that holds at least min_count points, plus, at min_count 1, the points out of
    the grid.  of: runs(xyz, cell, origin), when the caller has it."""
    ok, first, counts = of if of is not None else runs(xyz, cell, origin)
    full = counts >= min_count
    hit = np.zeros(ok.size, bool)
    hit[first[full]] = True
    if min_count == 1:
        hit |= ~ok
    return hit, (int(counts.size), int(full.sum()), int((~ok).sum()))


def select_loop(xyz, cell, origin=(0, 0, 0), min_count=1):
    """The same, point by point with a dictionary (what voxel_ref.select is checked against)."""
    f = np.float32
    xyz = np.asarray(xyz, f)[:, :3]
    cell3 = np.broadcast_to(np.asarray(cell, f), (3,))
    origin3 = np.asarray(origin, f).reshape(3)
    seen, out = {}, []
    with np.errstate(all="ignore"):
        inv = [f(1) / cell3[k] for k in range(3)]
        for i in range(xyz.shape[0]):
            t = [f(f(xyz[i, k] - origin3[k]) * inv[k]) for k in range(3)]
            if all(np.isfinite(v) and -SPAN <= v < SPAN for v in t):
                seen.setdefault(tuple(int(np.floor(v)) for v in t), []).append(i)
            else:
                out.append(i)
    hit = np.zeros(xyz.shape[0], bool)
    for members in seen.values():
        if len(members) >= min_count:
            hit[min(members)] = True
    if min_count == 1:
        hit[out] = True
    return hit, (len(seen), sum(len(m) >= min_count for m in seen.values()), len(out))
