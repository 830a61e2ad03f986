"""The reference model of rtr_select_segments (include/rtr_segments.h section 6q), in numpy only.

Segments are the connected components of: section 6h's neighbour relation (clusters_ref.pairs), AND both points usable
(curvature None, or curvature[i] <= max_curvature in float32: NaN fails, +inf fails any finite limit), AND
|dot| >= cos_angle -- oriented: dot >= cos_angle -- with dot = (nx nx' + ny ny') + nz nz' in float32, every product and
sum a float32 ufunc of its own (numpy never contracts them).  A NaN dot fails.  A segment's label is the smallest
upload index among its members (clusters_ref.labels_of_pairs).

edges: clusters_ref.pairs filtered by that rule.
labels: labels_of_pairs over the edges.
labels_brute: every pair as a matrix, components by a graph search (good to about 4k points); shares only the distance
arithmetic (neighbours_ref._d2) with `labels`: the dot is formed from columns of a matrix, not from gathered pairs.
gathered: the library's substitution -- the normal of a point that is not usable replaced by (0, 0, 0) -- after which
the rule WITHOUT the usable test gives the same edges, because cos_angle > 0 (test_segments_host.py checks it).
hits, sizes, stats, words: clusters_ref's.
"""
import numpy as np

import clusters_ref as cr
import neighbours_ref as nr

f32 = np.float32

hits, sizes, stats, words = cr.hits, cr.sizes, cr.stats, cr.words


def _f32(a, cols=None):
    a = np.ascontiguousarray(np.asarray(a, f32))
    return a if cols is None else a.reshape(-1, cols)


def usable(n, curvature=None, max_curvature=np.inf):
    if curvature is None:
        return np.ones(n, bool)
    with np.errstate(invalid="ignore"):
        return _f32(curvature).reshape(n) <= f32(max_curvature)


def dot(a, b):
    """float32 in the contract's order; a, b broadcastable (.., 3)."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def passes(d, cos_angle, oriented=False):
    with np.errstate(invalid="ignore"):
        return (d if oriented else np.abs(d)) >= f32(cos_angle)


def gathered(normals, curvature=None, max_curvature=np.inf):
    nrm = _f32(normals, 3).copy()
    nrm[~usable(nrm.shape[0], curvature, max_curvature)] = 0
    return nrm


def edges(xyz, radius, cos_angle, normals, curvature=None, max_curvature=np.inf, oriented=False, near=None):
    """(i, j): upload indices of every ordered pair of JOINED points.  near: clusters_ref.pairs(xyz, radius), to share."""
    nrm = _f32(normals, 3)
    i, j = cr.pairs(xyz, radius) if near is None else near
    ok = usable(nrm.shape[0], curvature, max_curvature)
    keep = ok[i] & ok[j] & passes(dot(nrm[i], nrm[j]), cos_angle, oriented)
    return i[keep], j[keep]


def labels(xyz, radius, cos_angle, normals, curvature=None, max_curvature=np.inf, oriented=False, near=None):
    """labels[i]: the smallest upload index of point i's segment (uint32, upload order)."""
    i, j = edges(xyz, radius, cos_angle, normals, curvature, max_curvature, oriented, near)
    return cr.labels_of_pairs(np.asarray(xyz).shape[0], i, j)


def adjacency_brute(xyz, radius, cos_angle, normals, curvature=None, max_curvature=np.inf, oriented=False):
    p = np.ascontiguousarray(np.asarray(xyz, f32)[:, :3])
    nrm = _f32(normals, 3)
    n = p.shape[0]
    ok = nr.finite(p) & usable(n, curvature, max_curvature)
    adj = (nr._d2(p[:, None, :], p[None, :, :]) <= nr.r2_of(radius)) & ok[None, :] & ok[:, None]
    adj &= passes(dot(nrm[:, None, :], nrm[None, :, :]), cos_angle, oriented)
    adj[np.arange(n), np.arange(n)] = False
    return adj


def labels_brute(xyz, radius, cos_angle, normals, curvature=None, max_curvature=np.inf, oriented=False):
    adj = adjacency_brute(xyz, radius, cos_angle, normals, curvature, max_curvature, oriented)
    n = adj.shape[0]
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
