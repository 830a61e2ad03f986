"""The inputs that the neighbour tests share (test_neighbours_host.py pins the reference on them without a GPU,
test_gpu_neighbours.py runs the library on them)."""
SEED = 41
KS = (1, 2, 4, 16)
# scene -> (points, the two radii)
SCENES = {"room_shell": (40_001, (0.07, 0.18)), "uniform_box": (41_003, (0.12, 0.25))}
# (scene, radius) -> the points with at least k neighbours, k in KS, as neighbours_ref gives them.  "spread": between
# 5 % and 95 % of the points hit, so that a kernel answering all or nothing cannot pass; the two named kinds are
# "nothing" (no point at all) and "everything" (at least 99 %).
PINS = {("room_shell", 0.07): (36_871, 26_314, 4_506, 0), ("room_shell", 0.18): (40_001, 40_001, 40_001, 20_847),
        ("uniform_box", 0.12): (31_560, 18_022, 2_683, 0), ("uniform_box", 0.25): (41_002, 40_988, 40_808, 11_637)}
KINDS = {("room_shell", 0.07): ("spread", "spread", "spread", "nothing"),
         ("room_shell", 0.18): ("everything", "everything", "everything", "spread"),
         ("uniform_box", 0.12): ("spread", "spread", "spread", "nothing"),
         ("uniform_box", 0.25): ("everything", "everything", "everything", "spread")}


def kind_holds(kind, hits, n):
    if kind == "nothing":
        return hits == 0
    if kind == "everything":
        return hits >= 0.99 * n
    return 0.05 * n <= hits <= 0.95 * n
