"""Frame-covering clouds for the prefilter's shape tests (inputs only; no reference or product logic).

The orbit poses of the other tests leave frames of extreme aspect ratio (16x131104, 65552x40) almost empty, so the
cloud is built FROM the frame: one point per pixel, un-projected from the pixel centre (the projection rounds to the
nearest integer, so pixel (u, v) has its centre at (u, v)) with +-0.3 px of jitter, through the camera
P = K * I, fx = fy = max(W, H), cx = W / 2, cy = H / 2.  Everything is drawn from default_rng(7 * W + H).

  pixels  each kept with probability 0.85; whole 8x8 pixel blocks emptied with probability 0.12
  depth   background 4 + 0.001 (u % 97) + 0.002 (v % 89); 5x5 pixel blocks with probability 0.15 are foreground at
          2 + 0.003 (u % 7); 2 % of the points are pushed 0.05 .. 1 m behind (the filter's candidates for dropping)
  second  a fifth of the kept pixels get a second point on the same ray at 1.001, 1.004 or 1.02 times the depth:
          inside and outside the 2 cm accumulation window
  colour  random; the point order is a random permutation

`SHAPES4` / `LEVEL_SHAPES` are the frame sizes of tests/test_gpu_filter_shapes.py and tests/test_filter_shapes_host.py,
`coverage` the conditions both assert on the ORACLE's frames so that no case can go vacuous."""
import numpy as np

from helpers import cloud

# levels = 4.  What each size pins is told in tests/test_gpu_filter_shapes.py.
SMALL4 = [(16, 16), (16, 17), (16, 31), (32, 33), (48, 47), (80, 63), (112, 65), (144, 97), (176, 49), (208, 111)]
LARGE4 = [(4112, 1047), (65552, 40), (16, 131104)]
SHAPES4 = SMALL4 + LARGE4
# every other level count at the narrowest widths check_prefilter lets through
LEVEL_SHAPES = {1: [(2, 2), (6, 5), (10, 7), (14, 33)], 2: [(12, 9), (20, 6)], 3: [(24, 19), (40, 8)],
                5: [(32, 32), (96, 70)], 6: [(64, 65)], 7: [(128, 129)], 8: [(256, 300)]}


def camera(orc, W, H, dcx=0.0):
    f = float(max(W, H))
    K = np.array([[f, 0, W / 2 + dcx], [0, f, H / 2], [0, 0, 1.0]])
    return orc.compose_projection(K, np.eye(4))


def frame_cloud(orc, W, H):
    """-> (P float32[16], xyzw float32 [n,4], rgba uint8 [n,4])"""
    rng = np.random.default_rng(7 * W + H)
    f, cx, cy = float(max(W, H)), W / 2, H / 2
    v, u = np.divmod(np.arange(W * H, dtype=np.int64), W)
    keep = rng.random(W * H) < 0.85
    hole = rng.random(((H + 7) // 8, (W + 7) // 8)) < 0.12
    keep &= ~hole[v // 8, u // 8]
    fg = rng.random(((H + 4) // 5, (W + 4) // 5)) < 0.15
    z = np.where(fg[v // 5, u // 5], 2 + 0.003 * (u % 7), 4 + 0.001 * (u % 97) + 0.002 * (v % 89))
    z = z + np.where(rng.random(W * H) < 0.02, rng.uniform(0.05, 1.0, W * H), 0.0)
    second = keep & (rng.random(W * H) < 0.2)
    scale = rng.choice(np.array([1.001, 1.004, 1.02]), W * H)

    def unproject(sel, depth):
        ju, jv = rng.uniform(-0.3, 0.3, sel.sum()), rng.uniform(-0.3, 0.3, sel.sum())
        return np.stack([(u[sel] + ju - cx) * depth / f, (v[sel] + jv - cy) * depth / f, depth], axis=1)

    xyz = np.concatenate([unproject(keep, z[keep]), unproject(second, (z * scale)[second])]).astype(np.float32)
    rgb = rng.integers(0, 256, size=(len(xyz), 3), dtype=np.uint8)
    perm = rng.permutation(len(xyz))
    xyzw, rgba = cloud(xyz[perm], rgb[perm])
    return camera(orc, W, H), xyzw, rgba


def coverage(depth_bits, mask, levels):
    """What the oracle's frame (unfiltered depth bits, filter mask) shows of the edges: -> dict of
    (kept, dropped, filtered) pixel counts -- mask set, mask clear, and mask clear although the pixel was FILLED, i.e.
    taken out by the pyramid test -- for the last 16 columns, the rows [h_eff - 16, h_eff), the tail rows [h_eff, H)
    (None when H == h_eff; the pyramid never tests them, so `filtered` is 0 there) and the whole frame."""
    H, W = depth_bits.shape
    h_eff = (H >> levels) << levels
    filled = depth_bits != 0x7F7FFFFF
    kept, dropped = (mask > 0), (mask == 0)

    def both(sl):
        return int(kept[sl].sum()), int(dropped[sl].sum()), int((dropped & filled)[sl].sum())
    return {"columns": both((slice(0, h_eff), slice(max(W - 16, 0), W))),
            "rows": both((slice(max(h_eff - 16, 0), h_eff), slice(None))),
            "tail": both((slice(h_eff, H), slice(None))) if H > h_eff else None,
            "all": both((slice(None), slice(None)))}
