"""Inputs that the nearest tests share (test_nearest_host.py pins the reference on them without a GPU,
test_gpu_nearest.py runs the library on them).

tie_lattice: every coordinate is a multiple of 1/256 inside +-16, so every difference, square and sum of the pair test is
exact in float32.  Given point c sits at the centre of a cell of eight resident points, its corners at (+-4, +-4, +-4) /
256 from it: all eight d2 are 48 / 65536, bitwise equal, and the winner is the smallest UPLOAD index among them.  Centres
are 16 / 256 apart and the radius is 8 / 256, so a corner of a neighbouring cell (d2 >= 176 / 65536 > r2 = 64 / 65536) is
no candidate.  On top: three resident points coincident with one more given point (d2 = +0 three times), and three
coincident given points beside two more, coincident, resident points (the resident side's tie: the smallest given index
wins).  So EVERY given point has at least two resident points at its bitwise-minimal d2.
`order` decides where the eight of a cell lie in the upload order:
  "beside"   consecutively: the other components of the winner's lane and the next lane
  "lanes"    16 apart: eight lanes of one chunk (of one or two where a cell crosses a chunk's end)
  "chunks"   corner k of every cell in block k of 256 + ... points: eight chunks, i.e. eight waves' atomics
  "random"   anywhere (the sorted form: the smallest upload index is not the smallest resident index)
"""
import numpy as np

f32 = np.float32
TIE_RADIUS = f32(8 / 256)
TIE_ORDERS = ("beside", "lanes", "chunks", "random")
TIE_CELLS = (8, 6, 6)  # cells per axis: 288 cells (a multiple of 16), 2304 corners, nine chunks


def tie_lattice(order):
    """(resident (n, 3), given (m, 3)) in float32."""
    c = np.stack(np.meshgrid(*[np.arange(k) for k in TIE_CELLS], indexing="ij"), -1).reshape(-1, 3)
    centres = (c * 16 - 40) / 256.0
    corners = np.stack(np.meshgrid(*[[-4, 4]] * 3, indexing="ij"), -1).reshape(-1, 3) / 256.0
    cells = centres.shape[0]
    pts = (centres[:, None, :] + corners[None, :, :]).reshape(-1, 3)  # (cell-major: cell c's corners at 8 c .. 8 c + 7)
    pile = np.repeat([[5.0, 5.0, 5.0]], 3, axis=0)    # three coincident resident points ...
    lone = np.repeat([[-5.0, 5.0, 0.25]], 2, axis=0)  # ... and two beside three coincident given points
    n8 = pts.shape[0]
    k, cell = np.arange(n8) % 8, np.arange(n8) // 8
    if order == "beside":
        at = np.arange(n8)
    elif order == "lanes":  # groups of 16 cells = 128 points = 32 lanes: corner k of the group's cell j at lane 4 k + j / 4
        at = (cell // 16) * 128 + k * 16 + cell % 16
    elif order == "chunks":
        at = k * cells + cell
    else:
        at = np.random.default_rng(8).permutation(n8)
    res = np.empty_like(pts)
    res[at] = pts
    # the specials go where they cross chunks too: the pile's members far apart, in the middle of the cloud
    res = np.concatenate([res[:300], pile[:1], res[300:900], pile[1:2], lone[:1], res[900:], pile[2:], lone[1:]])
    given = np.concatenate([centres, pile[:1], lone[:1] + [[1 / 256.0, 0, 0]] * 3])
    return res.astype(f32), given.astype(f32)


def tie_counts(res, given):
    """per given point: how many resident points lie at its bitwise-minimal d2 (0: no candidate)"""
    a, g = res.astype(f32), given.astype(f32)
    d = a[:, None, :] - g[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    ok = d2 <= TIE_RADIUS * TIE_RADIUS
    d2 = np.where(ok, d2, f32(np.inf))
    return ((d2 == d2.min(axis=0)[None, :]) & ok).sum(axis=0), ((d2 == d2.min(axis=1)[:, None]) & ok).sum(axis=1)
