"""The host statement of rtr_write_points (include/rtr.h section 2f), shared by the write tests and the edit model."""
import numpy as np


def window(n, sel, first, count):
    """The upload indices s_first .. of the points a write touches: of the selected points (sel: bool (n,), None =
    every point) in ascending order, the ranks [first, first + count)."""
    s = np.arange(n) if sel is None else np.flatnonzero(np.asarray(sel, bool))
    first = int(first)
    return s[first:first + int(count)] if first < s.size else s[:0]


def written(xyz, rgb, sel, first, X, C):
    """-> (xyz', rgb', idx): the cloud (xyz (n, >= 3) float32, rgb (n, >= 3) uint8; further columns stay) after record j
    of X and / or C went into point idx[j] = s_{first + j}.  X: float32 rows (>= 3 columns) or None; C: uint8 rows
    (>= 3 columns), ONE colour of shape (3,) for every written point, or None.  The rows give the count; a lone
    broadcast colour reaches to the last selected point.  Coordinates are copied as bit patterns."""
    xyz, rgb = np.array(xyz, np.float32), np.array(rgb, np.uint8)
    n = xyz.shape[0]
    one = C is not None and np.ndim(C) == 1
    if X is not None:
        count = np.shape(X)[0]
    elif C is not None and not one:
        count = np.shape(C)[0]
    else:
        assert one
        count = n
    idx = window(n, sel, first, count)
    m = idx.size
    if X is not None:
        xyz.view(np.uint32)[idx, :3] =np.ascontiguousarray(np.asarray(X, np.float32)[:m, :3]).view(np.uint32)
    if C is not None:
        rgb[idx, :3] = np.asarray(C, np.uint8)[:3] if one else np.asarray(C, np.uint8)[:m, :3]
    return xyz, rgb, idx
