"""The inputs that the normal-estimation tests share (test_normals_host.py pins the reference on them without a GPU,
test_cpp_normals.py runs csrc/rtr_normal_fit.h on them with g++, test_gpu_normals.py the library): the scenes, seed and
radii of neighbours_cases.py at k = 8 and 16, the dense cloud of statistical_cases.py at k = 64, and the special clouds
below.  Every special cloud is small: a case is (name, xyz float32 (n, 3), radius, ks, viewpoint or None)."""
import numpy as np

import neighbours_cases as nc
import statistical_cases as sc

f32 = np.float32
SEED = nc.SEED
SCENES = nc.SCENES
KS = (8, 16)
SCENE_VIEWPOINT = (0.25, -0.5, 1.5)
DENSE_N, DENSE_RADIUS, DENSE_K = sc.DENSE_N, sc.DENSE_RADIUS, 64
dense_cloud = sc.dense_cloud

# (a) / (b): a lattice plane z = const whose spacing IS the radius (a power of two: every d2 is exact), so that the four
# neighbours of an inner point tie and k = 3 cuts the tie by index; upload index = row-major.  (k = 2 would take the
# left and right neighbours of a point of the first row alone: a collinear neighbourhood, whose normal is not the plane's.)
LATTICE_W, LATTICE_H, LATTICE_STEP, LATTICE_Z = 19, 13, 0.25, 1.5
LATTICE_KS = (3, 8)
BELOW = (0.5, 0.25, -3.0)  # a viewpoint below the plane
# (c): the rotation of the tilted plane, by Rodrigues about (1, 2, 3) / sqrt(14) through 1 radian: irrational entries
TILT_AXIS, TILT_ANGLE = (1.0, 2.0, 3.0), 1.0


def lattice_plane():
    ix, iy = np.meshgrid(np.arange(LATTICE_W), np.arange(LATTICE_H))
    return np.stack([ix.ravel() * LATTICE_STEP - 2.0, iy.ravel() * LATTICE_STEP - 1.0, np.full(ix.size, LATTICE_Z)], 1).astype(f32)


def tilt_rotation():
    a = np.float64(TILT_AXIS) / np.sqrt(np.dot(TILT_AXIS, TILT_AXIS))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(TILT_ANGLE) * K + (1 - np.cos(TILT_ANGLE)) * (K @ K)


def tilted_plane():
    """(xyz, the analytic normal): 1500 random points of the plane through the origin, rotated; in float64 the points
    lie on the plane exactly, rounding to float32 moves each by at most 2^-24 of its coordinates."""
    rng = np.random.default_rng(31)
    uv = rng.uniform(-1, 1, (1500, 2))
    R = tilt_rotation()
    return (np.c_[uv, np.zeros(1500)] @ R.T).astype(f32), R[:, 2]


def sphere_shell():
    rng = np.random.default_rng(32)
    v = rng.normal(size=(3001, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * 0.5 + [3.0, -2.0, 1.0]).astype(f32)


def line():
    t = np.arange(257, dtype=np.float64)
    return (t[:, None] * np.float64([0.03125, 0.0625, -0.03125]) + [1.0, 0.0, 2.0]).astype(f32)


def piles():
    """65 and 3000 coincident points and 200 sparse ones, shuffled."""
    rng = np.random.default_rng(33)
    xyz = np.empty((3265, 3), f32)
    at = rng.permutation(3265)
    xyz[at[:3000]] = f32([0.7, -0.3, 1.9])
    xyz[at[3000:3065]] = f32([-2.5, 0.25, -0.004])
    xyz[at[3065:]] = (rng.uniform(-1, 1, (200, 3)) * 50 + [100, 0, 0]).astype(f32)
    return xyz, at[:3000], at[3000:3065], at[3065:]


def specials(flt_max=False):
    """pairs and triples 1e-20 apart (subnormal d2), an isolated point, a coincident pair and NaN / +-inf coordinates
    among ordinary points.  flt_max: +-FLT_MAX coordinates too -- finite points whose every difference overflows, so they
    have no candidates; they lie beyond the span of the library's grid at any legal radius, so the library refuses such
    a cloud (RTR_ERR_UNSUPPORTED) and only the reference's brute route runs on it."""
    rng = np.random.default_rng(34)
    xyz = rng.uniform(-1, 1, (1200, 3)).astype(f32)
    at = rng.choice(np.arange(100, 1100), 30, replace=False)
    big = np.finfo(f32).max
    for j, v in enumerate((np.nan, np.inf, -np.inf)):
        xyz[at[j], j % 3] = v
        xyz[at[5 + j], :] = v
    if flt_max:
        xyz[at[3], 0], xyz[at[4], 1], xyz[at[8], :], xyz[at[9], :] = big, -big, big, -big
    for j in range(4):
        xyz[at[10 + 3 * j]] = f32([40 + j, 0, 0])
        xyz[at[11 + 3 * j]] = f32([40 + j, 1e-20 * (j + 1), 0])
        xyz[at[12 + 3 * j]] = f32([40 + j, 0, 2e-20]) if j % 2 else f32([70 + j, 0, 0])
    xyz[at[22]] = f32([80, -80, 80])  # isolated
    xyz[at[23]] = xyz[at[24]] = f32([60, 60, 60])  # a coincident pair: found = 1, no normal
    return xyz, at


def far_cloud():
    rng = np.random.default_rng(35)
    uv = rng.uniform(-2, 2, (2500, 2))
    z = 0.1 * np.sin(uv[:, 0]) + 0.02 * rng.normal(size=2500)
    return (np.c_[uv, z] + [7000.0, -7000.0, 120.0]).astype(f32)


def duplicated_blocks():
    """a block of 700 random points four times over, the copies interleaved: every d2 occurs four times and k = 3, 5, 8
    cut each tie by index"""
    rng = np.random.default_rng(36)
    b = rng.uniform(0, 1, (700, 3)).astype(f32)
    xyz = np.concatenate([b, b[::-1], b, b[rng.permutation(700)]])
    return xyz[rng.permutation(xyz.shape[0])]


def special_cases():
    return [("lattice", lattice_plane(), LATTICE_STEP, LATTICE_KS, None),
            ("lattice_from_below", lattice_plane(), LATTICE_STEP, LATTICE_KS, BELOW),
            ("tilted_plane", tilted_plane()[0], 0.2, (8, 16), None),
            ("sphere_shell", sphere_shell(), 0.08, (8, 16), (3.0, -2.0, 1.0)),
            ("line", line(), 0.2, (2, 8), None),
            ("piles", piles()[0], 0.01, (2, 8, 64), None),
            ("specials", specials()[0], 0.15, (1, 2, 8), (0.0, 0.0, 0.0)),
            ("far_cloud", far_cloud(), 0.25, (8, 16), (7000.0, -7000.0, 1000.0)),
            ("duplicated_blocks", duplicated_blocks(), 0.12, (3, 5, 8), None)]
