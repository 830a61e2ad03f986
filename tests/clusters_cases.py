"""The inputs that the cluster tests share (test_clusters_host.py pins the reference on them without a GPU,
test_gpu_clusters.py runs the library on them): neighbours_cases' two generators at its point counts and seed.

The radii were chosen on the CPU with clusters_ref.  room_shell (points on surfaces): 0.06 is well below and 0.08 just
below the radius at which the walls fuse (at 0.10 one cluster holds 89 % of the points).  uniform_box (points in a
volume) percolates between 0.14 and 0.16 (at 0.16 one cluster holds 85 %): 0.12 lies below, 0.14 near it -- the largest
cluster there has 573 points, ten times that at 0.12."""
SEED = 41
# (min_points, max_points) of rtr_select_clusters
WINDOWS = ((1, 0), (2, 0), (50, 0), (2, 49))
# scene -> (points, the two radii)
SCENES = {"room_shell": (40_001, (0.06, 0.08)), "uniform_box": (41_003, (0.12, 0.14))}
# (scene, radius) -> (clusters, clusters of two or more points, points of the largest cluster, the points hit for each
# of WINDOWS), as clusters_ref gives them.
PINS = {("room_shell", 0.06): (16_425, 9_387, 28, (40_001, 32_963, 0, 32_963)),
        ("room_shell", 0.08): (5_066, 3_846, 170, (40_001, 38_781, 6_039, 32_742)),
        ("uniform_box", 0.12): (16_924, 7_481, 53, (41_003, 31_560, 106, 31_454)),
        ("uniform_box", 0.14): (8_274, 4_137, 573, (41_003, 36_866, 13_619, 23_247))}
# Every one of these four is a "spread" case: at least 20 clusters of two or more points, a largest cluster of at most
# 90 % of the points, and for each window named here between 5 % and 95 % of the points hit -- a kernel that answers all,
# nothing or one cluster cannot pass.  The other windows: (1, 0) hits every point; the rest as pinned.
SPREAD = {("room_shell", 0.06): ((2, 0), (2, 49)), ("room_shell", 0.08): ((50, 0), (2, 49)),
          ("uniform_box", 0.12): ((2, 0), (2, 49)), ("uniform_box", 0.14): ((2, 0), (50, 0), (2, 49))}
# the two named cases: (scene, radius, min_points, max_points) -> (clusters, largest, points hit)
EVERYTHING = ("room_shell", 0.3, 1, 0)  # one cluster of all 40 001 points
NOTHING = ("room_shell", 0.06, 40_002, 0)  # min_points > n
NAMED_PINS = {EVERYTHING: (1, 40_001, 40_001), NOTHING: (16_425, 28, 0)}


def spread_holds(clusters2, largest, hits, n):
    return clusters2 >= 20 and largest <= 0.9 * n and 0.05 * n <= hits <= 0.95 * n
