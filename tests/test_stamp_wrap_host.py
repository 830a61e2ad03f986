"""The inputs of the frame-stamp wrap tests are what those tests need, shown without a GPU: for exactly the clouds and
poses of tests/stamp_wrap_scenes.py (test_gpu_stamp_wrap.py, the sharded wrap runs of p2p_worker.py) the oracle's
entries per 32x16 storage tile are pinned, at least two tiles of every frame hold more than 8192 entries (dynamic
extents 1 and 2 in use), and consecutive poses load different tiles."""
import numpy as np
import pytest

import pool_overflow_scenes as po
import stamp_wrap_scenes as sw


@pytest.fixture(scope="module")
def base(orc):
    return sw.cloud(orc)


def test_every_pose_uses_dynamic_extents_in_two_tiles(orc, base):
    xyzw, rgba = base
    assert len(sw.PINNED) == len(sw.POSE_SPECS)
    for i in range(len(sw.POSE_SPECS)):
        c = sw.tile_counts(orc, xyzw, rgba, sw.pose(orc, i))
        assert c.shape == (3, 2)
        assert tuple(c.ravel().tolist()) == sw.PINNED[i], (i, c.ravel().tolist())
        assert sw.uses_dynamic_extents(c), (i, c)


def test_tile_counts_are_the_frames_entries(orc, base):
    """The counting itself: the tiles of a frame sum to the points the oracle accepts for it, and a pixel's count is
    what its accumulator holds when the blending window takes every point."""
    xyzw, rgba = base
    for i in range(len(sw.POSE_SPECS)):
        P = sw.pose(orc, i)
        c = sw.tile_counts(orc, xyzw, rgba, P)
        assert int(c.sum()) == orc.envelope_points(xyzw, P, sw.W, sw.H, 0, 0)["accepted"], i
    assert sw.heaviest_tile(np.array([[1, 2], [3, 4], [50, 6]])) == 50
    assert sw.heaviest_tile(np.array([[1, 2], [3, 40], [5, 6]])) == 42


def test_consecutive_poses_load_different_tiles(orc, base):
    """Alternating two poses (and walking through all of them) never repeats the set of tiles that use dynamic extents,
    so the directory words of one frame are stale in the next."""
    heavy = [frozenset(np.flatnonzero(np.array(sw.PINNED[i]) > sw.DYN2).tolist()) for i in range(len(sw.POSE_SPECS))]
    for i in range(len(heavy)):
        assert heavy[i] != heavy[(i + 1) % len(heavy)], (i, heavy)
    assert heavy[0] != heavy[1] and heavy[0] != heavy[2] and heavy[1] != heavy[2]


def test_edited_cloud(orc, base):
    (ax, ac), keep, (xyzw, rgba) = sw.edited_cloud(orc)
    assert len(ax) == sw.APPEND_N and keep.shape == (sw.N + sw.APPEND_N,) and 0 < keep.sum() < keep.size
    assert len(xyzw) == int(keep.sum())
    for i, want in sw.PINNED_EDITED.items():
        c = sw.tile_counts(orc, xyzw, rgba, sw.pose(orc, i))
        assert tuple(c.ravel().tolist()) == want, (i, c.ravel().tolist())
        assert sw.uses_dynamic_extents(c)
    # and after the append alone (the frame between the two edits is not rendered, but the pool is re-sized for it)
    both = np.concatenate([base[0], ax]), np.concatenate([base[1], ac])
    assert sw.uses_dynamic_extents(sw.tile_counts(orc, both[0], both[1], sw.pose(orc, 0)))


def test_every_shard_uses_dynamic_extents(pkg, orc):
    """The sharded wrap runs: every rank's own store -- the one its peers map -- has two tiles above 8192 entries."""
    for world in sorted(sw.P2P_N):
        for rank in range(world):
            xyzw, rgba = sw.shard(pkg, orc, rank, world)
            assert len(xyzw) == sw.N
            for i in (0, 1):
                c = sw.tile_counts(orc, xyzw, rgba, sw.pose(orc, i))
                assert sw.uses_dynamic_extents(c), (world, rank, i, c)
    c = sw.tile_counts(orc, *sw.shard(pkg, orc, 0, 2), sw.pose(orc, 0))
    assert tuple(c.ravel().tolist()) == (531, 606, 27436, 28857, 1268, 1302)
    c = sw.tile_counts(orc, *sw.shard(pkg, orc, 2, 3), sw.pose(orc, 1))
    assert tuple(c.ravel().tolist()) == (13575, 14503, 15644, 16278, 0, 0)


def test_overflow_pose_straddles_two_tiles(orc):
    """The pool-overflow case: pool_overflow_scenes' cloud under its one-pixel camera moved onto the border between two
    storage tiles -- every point is an entry, about half of them in each tile."""
    xyzw, rgba = po.cloud(orc)
    P = po.p_one(orc, sw.OVERFLOW_CX)[0]
    c = sw.tile_counts(orc, xyzw, rgba, P, po.W, po.H)
    assert int(c.sum()) == po.N and c[0, 0] == 999_990 and c[0, 1] == 1_000_010
    assert sw.uses_dynamic_extents(c) and sw.heaviest_tile(c) == 1_000_010
