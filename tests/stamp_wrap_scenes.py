"""Inputs of the frame-stamp wrap tests (tests/test_gpu_stamp_wrap.py, the sharded wrap runs of tests/p2p_worker.py),
and the oracle's own entry counts per 32x16 storage tile for them, pinned without a GPU by test_stamp_wrap_host.py.

The extent directory -- the one thing a tile store's 24-bit frame stamp protects -- only matters for tile streams longer
than the 4096-entry static extent: stream positions 4096 .. 8191 live in dynamic extent 1, 8192 .. 16383 in extent 2.
So every pose here puts more than 8192 entries into at least two storage tiles of a 64x48 frame (2 x 3 storage tiles,
the smallest frame with more than one of them in each direction), and consecutive poses put them into DIFFERENT tiles:
a directory word left by the previous frame then names an extent the current frame must not read.

uniform_box (hash order: every shard of it is a uniform sample) seen whole from outside; 60 000 points per context."""
import numpy as np

W, H = 64, 48
N = 60_000
SEED = 0xC0FFEE21
STAMP_MAX = 0xFFFFFF
DYN2 = 8192  # a stream longer than this uses dynamic extents 1 AND 2

# focal length, principal point, distance along the optical axis, yaw about the y axis (degrees)
POSE_SPECS = ((60.0, 32.0, 24.0, 12.0, 0.0),     # A: the box across the middle row of storage tiles
              (60.0, 32.0, 16.0, 12.0, 0.0),     # B: across the upper two rows
              (45.0, 20.0, 32.0, 10.0, 30.0),    # C: the left column of the lower two rows
              (70.0, 44.0, 30.0, 14.0, -40.0),   # D: the right column of the lower two rows
              (60.0, 32.0, 32.0, 12.0, 90.0))    # E: across the lower two rows, seen from the side
# entries per storage tile, row-major over (3 rows, 2 columns), of the N-point cloud under each pose (the oracle's)
PINNED = {0: (576, 618, 27533, 28763, 1194, 1316),
          1: (13608, 14262, 15695, 16435, 0, 0),
          2: (0, 0, 21742, 4980, 25467, 5798),
          3: (0, 0, 5815, 28143, 4022, 18687),
          4: (0, 0, 13664, 14216, 15579, 16541)}

# the edits of the "edits across the wrap" case: points appended behind the cloud, then points removed from the result
APPEND_N, APPEND_SEED = 9_000, 0xC0FFEE22
REMOVE_SEED, REMOVE_KEEP = 5, 0.85
PINNED_EDITED = {0: (583, 597, 26728, 28206, 1194, 1264),
                 1: (13170, 13997, 15335, 16070, 0, 0)}

# the pool-overflow case: pool_overflow_scenes' one-pixel camera with its principal point on the border between the
# storage tiles (0, 0) and (0, 1) of a 640x480 frame -- half of the 2 000 000 points in each
OVERFLOW_CX = 31.5

# the sharded wrap runs (p2p_worker.py): world -> total points; every rank's shard is one context's cloud
P2P_SEED = 11
P2P_N = {2: 120_000, 3: 180_000}


def pose(orc, i):
    f, cx, cy, tz, yaw = POSE_SPECS[i]
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    a = np.deg2rad(yaw)
    E = np.eye(4)
    E[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    E[2, 3] = tz
    return orc.compose_projection(K, E)


def cloud(orc):
    return orc.generate("uniform_box", SEED, 0, N, N)


def edited_cloud(orc):
    """-> (the appended points, the keep mask over base + appended, the cloud after both edits)."""
    xyzw, rgba = cloud(orc)
    ax, ac = orc.generate("uniform_box", APPEND_SEED, 0, APPEND_N, APPEND_N)
    keep = np.random.default_rng(REMOVE_SEED).random(N + APPEND_N) < REMOVE_KEEP
    return (ax, ac), keep, (np.concatenate([xyzw, ax])[keep], np.concatenate([rgba, ac])[keep])


def shard(pkg, orc, rank, world):
    n = P2P_N[world]
    lo, hi = pkg.shard_range(n, rank, world)
    return orc.generate("uniform_box", P2P_SEED, lo, hi - lo, n)


def tile_counts(orc, xyzw, rgba, P, w=W, h=H):
    """The oracle's in-frustum entries per 32x16 storage tile, int64 [h / 16, w / 32]: its accumulate pass with a window
    that takes every point of a pixel, summed over the tile's pixels."""
    assert w % 32 == 0 and h % 16 == 0
    depth, acc = orc.clear(w, h)
    orc.min_depth_pass(xyzw, P, w, h, depth)
    orc.accumulate_pass(xyzw, rgba, P, w, h, depth, acc, window=3e38)
    per_pixel = acc.reshape(h, w, 4)[..., 3].astype(np.int64)
    return per_pixel.reshape(h // 16, 16, w // 32, 32).sum(axis=(1, 3))


def heaviest_tile(counts):
    """Entries of the heaviest 32x32 PROCESSING tile (two storage tiles, one above the other; the last row of a frame
    whose height is no multiple of 32 has one): what frame_stats()["heaviest_tile"] reports."""
    c = np.asarray(counts)
    if c.shape[0] % 2:
        c = np.concatenate([c, np.zeros((1, c.shape[1]), c.dtype)])
    return int(c.reshape(c.shape[0] // 2, 2, c.shape[1]).sum(axis=1).max())


def uses_dynamic_extents(counts):
    """At least two storage tiles hold more than 8192 entries: extents 1 and 2 are in use in both."""
    return int((np.asarray(counts) > DYN2).sum()) >= 2
