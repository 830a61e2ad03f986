"""The inputs that the segment tests share (test_segments_host.py pins the reference on them without a GPU,
test_gpu_segments.py runs the library on them): clusters_cases' generators, seed and windows, normals and curvature from
normals_ref.estimate at K neighbours within the case's own radius, without a viewpoint.

room_shell at radius 0.10 is the case the call exists for: plain clustering (clusters_ref.labels) gives 214 clusters, one
of them with 35 719 of the 40 001 points -- walls, floor and ceiling touch.  With normals within 15 degrees 94.7 % of the
neighbour edges survive and the six largest segments hold 9 735, 9 731, 3 575, 3 551, 3 494 and 3 458 points: the six
faces of the room.  The second case adds the curvature limit 0.02 (38 123 points are usable), which takes the edges'
rounded rims off the faces.  uniform_box (points in a volume, no surfaces) falls apart: no segment above 11 points."""
import numpy as np

from clusters_cases import SEED, WINDOWS, spread_holds  # noqa: F401  (re-exported)

K = 16
COS_ANGLE = np.float32(0.9659258)  # cos 15 degrees, as a float32
# name -> (scene, points, radius, max_curvature or None)
CASES = {"room": ("room_shell", 40_001, 0.10, None),
         "room_smooth": ("room_shell", 40_001, 0.10, 0.02),
         "box": ("uniform_box", 41_003, 0.14, None)}
# name -> (segments, segments of two or more points, points of the largest segment, the points hit for each of WINDOWS),
# as segments_ref gives them
PINS = {"room": (1_892, 390, 9_735, (40_001, 38_499, 36_971, 1_528)),
        "room_smooth": (2_432, 223, 9_707, (40_001, 37_792, 36_755, 1_037)),
        "box": (33_110, 5_094, 11, (41_003, 12_987, 0, 12_987))}
# the six largest segments of the two room cases: the faces
FACES = {"room": (9_735, 9_731, 3_575, 3_551, 3_494, 3_458), "room_smooth": (9_707, 9_690, 3_538, 3_521, 3_465, 3_416)}
USABLE = {"room_smooth": 38_123}
# plain clustering of room_shell at the same radius: (clusters, points of the largest)
PLAIN_ROOM = (214, 35_719)
# the windows of each case for which clusters_cases.spread_holds: at least 20 segments of two or more points, a largest
# segment of at most 90 % of the points, between 5 % and 95 % of the points hit
SPREAD = {"room": ((50, 0),), "room_smooth": ((50, 0),), "box": ((2, 0), (2, 49))}


f32 = np.float32
R = f32(0.125)  # the radius of the special clouds: exact in fp32, as are its square and the steps below
C08 = f32(0.8)  # (0, 0.6f, 0.8f) . (0, 0, 1) = (0 + 0.6f * 0) + 0.8f * 1 = 0.8f exactly


def _line(n, step=0.75, z=0.0, y=0.0):
    return np.stack([np.arange(n) * (f32(step) * R), np.full(n, f32(y)), np.full(n, f32(z))], 1).astype(f32)


def special_clouds():
    """name -> dict(xyz, normals, curvature (or None), max_curvature, cos_angle, oriented, labels): small clouds at radius
    R whose segments are known by construction (`labels`: what the contract gives, written down by hand)."""
    up, down, tilt = f32([0, 0, 1]), f32([0, 0, -1]), f32([0, f32(0.6), C08])
    out = {}

    def add(name, xyz, normals, labels, curvature=None, max_curvature=np.inf, cos_angle=COS_ANGLE, oriented=False):
        out[name] = dict(xyz=np.ascontiguousarray(xyz, f32), normals=np.ascontiguousarray(normals, f32),
                         curvature=None if curvature is None else np.ascontiguousarray(curvature, f32),
                         max_curvature=f32(max_curvature), cos_angle=f32(cos_angle), oriented=oriented,
                         labels=np.asarray(labels, np.uint32))

    # two parallel sheets of 6 x 6 points half a radius apart, normals opposite: one segment by |dot|, two by dot
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 2) * (f32(0.75) * R)
    sheet = np.concatenate([np.c_[g, np.zeros(36)], np.c_[g, np.full(36, f32(0.5) * R)]]).astype(f32)
    nrm = np.concatenate([np.tile(up, (36, 1)), np.tile(down, (36, 1))])
    add("sheets", sheet, nrm, np.zeros(72))
    add("sheets_oriented", sheet, nrm, np.repeat([0, 36], 36), oriented=True)
    # a fold: ten points in a line, the last five tilted so that the dot across the fold is exactly cos_angle
    fold = np.concatenate([np.tile(up, (5, 1)), np.tile(tilt, (5, 1))])
    add("fold_at_threshold", _line(10), fold, np.zeros(10), cos_angle=C08)
    below = fold.copy()
    below[5:, 2] = np.nextafter(C08, f32(0))  # (the dot across the fold is one ulp below cos_angle; within a side it is about 1)
    add("fold_one_ulp_below", _line(10), below, np.repeat([0, 5], 5), cos_angle=C08)
    add("fold_oriented", _line(10), fold * f32([1, 1, -1]), np.zeros(10), cos_angle=C08, oriented=True)  # (dot(-up, tilt') = 0.8f too)
    # a chain of five; the middle point's curvature is exactly the limit (usable) or the next float (not)
    lim = f32(0.02)
    curv = np.full(5, f32(0.01))
    curv[2] = lim
    add("curvature_at_limit", _line(5), np.tile(up, (5, 1)), np.zeros(5), curvature=curv, max_curvature=lim)
    over = curv.copy()
    over[2] = np.nextafter(lim, f32(1))
    add("curvature_next_float", _line(5), np.tile(up, (5, 1)), [0, 0, 2, 3, 3], curvature=over, max_curvature=lim)
    # twelve points within a quarter radius of each other; bad normals or curvatures make singletons of their own index
    rng = np.random.default_rng(9)
    pile = (rng.uniform(-1, 1, (12, 3)) * (f32(0.125) * R)).astype(f32)
    nrm = np.tile(up, (12, 1))
    # (an infinite component meets a zero one in every product here: inf * 0 = NaN, and a NaN dot fails)
    nrm[1], nrm[3], nrm[5], nrm[6] = 0, f32([np.nan, 0, 1]), f32([np.inf, 0, 1]), f32([0, -np.inf, 1])
    curv = np.full(12, f32(0.01))
    curv[8], curv[9], curv[10] = np.nan, np.inf, -np.inf  # (-inf <= limit: usable)
    add("bad_normals_and_curvature", pile, nrm, [0, 1, 0, 3, 0, 5, 6, 0, 8, 9, 0, 0], curvature=curv, max_curvature=lim)
    inf_lab = [0, 1, 0, 3, 0, 5, 6, 0, 8, 0, 0, 0]  # (max_curvature = +inf admits the +inf curvature, still not NaN)
    add("infinite_limit", pile, nrm, inf_lab, curvature=curv, max_curvature=np.inf)
    # non-finite coordinates with good normals: nobody's neighbour
    bad = _line(8, 0.5)
    bad[2, 0], bad[4, 1], bad[5, 2] = np.nan, np.inf, -np.inf
    add("non_finite_coordinates", bad, np.tile(up, (8, 1)), [0, 0, 2, 0, 4, 5, 6, 6])
    return out


def make(orc, nref, name):
    """(xyzw, rgba, normals, curvature or None, max_curvature) of a case; orc: the oracle, nref: normals_ref"""
    scene, n, radius, max_curvature = CASES[name]
    xyzw, rgba = orc.generate(scene, SEED, 0, n, n)
    est = nref.estimate(xyzw, radius, K)
    if max_curvature is None:
        return xyzw, rgba, est["normals"], None, np.inf
    return xyzw, rgba, est["normals"], est["curvature"], max_curvature
