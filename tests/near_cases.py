"""The inputs that the near tests share (test_near_host.py pins the reference on them without a GPU, test_gpu_near.py
runs the library on them).  The resident cloud is the oracle's generate(scene, SEED, 0, n, n), the given set is taken
from generate(scene, GIVEN_SEED, 0, n, n)."""
SEED = 41
GIVEN_SEED = 43
SCENES = {"room_shell": 40_001, "uniform_box": 41_003}
# how the given set is cut out of the second cloud
TAKES = {"first5003": lambda g: g[:5003], "every8th": lambda g: g[::8], "every8th5003": lambda g: g[::8][:5003],
         "first257": lambda g: g[:257]}
# (scene, take, radius, given count, resident hits, given near): the two counts as near_ref.near_brute gives them
CASES = (
    ("room_shell", "first5003", 0.05, 5003, 3_820, 3_792),
    ("room_shell", "first5003", 0.18, 5003, 5_939, 5_003),
    ("room_shell", "every8th", 0.05, 5001, 6_311, 3_855),
    ("room_shell", "every8th", 0.07, 5001, 11_876, 4_779),
    ("room_shell", "first257", 0.07, 257, 276, 242),
    ("uniform_box", "first5003", 0.09, 5003, 3_070, 2_350),
    ("uniform_box", "first5003", 0.12, 5003, 6_919, 3_902),
    ("uniform_box", "first5003", 0.25, 5003, 32_646, 5_002),
    ("uniform_box", "every8th5003", 0.09, 5003, 3_084, 2_373),
    ("uniform_box", "first257", 0.12, 257, 387, 190),
)


def given(case, second_cloud):
    return TAKES[case[1]](second_cloud)


def spread(part, whole):
    return 0.05 * whole <= part <= 0.95 * whole
