"""The inputs that the statistical-filter tests share (test_statistical_host.py pins the reference on them without a GPU,
test_gpu_statistical.py runs the library on them): the scenes, seed and radii of neighbours_cases.py, and a dense cloud
in which every row of 64 overflows."""
import numpy as np

import neighbours_cases as nc

SEED = nc.SEED
SCENES = nc.SCENES
KS = (1, 8, 16, 64)
STD_MULS = (0.5, 1, 2)
# (scene, radius) -> the hits (stats[1]) as statistical_ref gives them, k-major: (k, std_mul) for k in KS, std_mul in STD_MULS
PINS = {("room_shell", 0.07): (24465, 29985, 36871, 24501, 31034, 36871, 24501, 31034, 36871, 24501, 31034, 36871),
        ("room_shell", 0.18): (27791, 33366, 38783, 27957, 33816, 38997, 27378, 34006, 39400, 27318, 33739, 39343),
        ("uniform_box", 0.12): (20227, 25671, 31560, 20568, 26555, 31560, 20567, 26555, 31560, 20567, 26555, 31560),
        ("uniform_box", 0.25): (28507, 34317, 39900, 28270, 34331, 40049, 28011, 34634, 40334, 28133, 34823, 40337)}
# the points with a full row at k = 8: rows are mostly short at the small radii and mostly full at the large ones
FULL_AT_8 = {("room_shell", 0.07): 7, ("room_shell", 0.18): 39970, ("uniform_box", 0.12): 6, ("uniform_box", 0.25): 37900}

# the dense cloud: 4099 points uniform in the unit cube at radius 0.4, about 670 candidates a point on average, so that
# every row of k = 64 overflows and the replacement path of the row runs
DENSE_N, DENSE_RADIUS, DENSE_KS = 4099, 0.4, (1, 8, 64)
DENSE_PINS = {(1, 0.5): 2879, (1, 1): 3434, (1, 2): 3979, (8, 0.5): 2986, (8, 1): 3458, (8, 2): 3951,
              (64, 0.5): 3125, (64, 1): 3460, (64, 2): 3916}


def dense_cloud():
    return np.random.default_rng(77).uniform(0, 1, (DENSE_N, 3)).astype(np.float32)


def pin(key, k, std_mul):
    return PINS[key][KS.index(k) * len(STD_MULS) + STD_MULS.index(std_mul)]
