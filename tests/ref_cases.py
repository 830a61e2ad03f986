"""The inputs of tests/test_oracle_vs_reference.py, tests/test_gpu_reference_filter.py and
tests/golden/make_ref_golden.py (inputs only; no reference or product logic).

`scene_cases()`   both scenes x 64x48, 160x120, 320x240 x three (pose, point count) pairs, 1 000 ... 50 000 points
`adversarial()`   the inputs tests/test_gpu_parity.py and tests/test_oracle_vs_pymodel.py already use against the oracle
`frame_cases()`   16x16, 16x31 and 48x47 of frame_cloud.py (set and clear mask bytes in tail rows, a dropped pixel at
                  every level)
Every case is (name, xyzw float32 [n,4], rgba uint8 [n,4], P float32[16], W, H)."""
import numpy as np

import frame_cloud
from helpers import cloud, kat_P

SIZES = [(64, 48), (160, 120), (320, 240)]
POSES = [(3, 1000), (137, 12000), (500, 50000)]  # (orbit pose, points)
SCENES = ["uniform_box", "room_shell"]
SEED = 0xC0FFEE01
GPU_CASES = [("room_shell", 64, 48, 500, 50000), ("room_shell", 160, 120, 500, 50000), ("room_shell", 320, 240, 137, 12000)]
GOLDEN_CASES = [("ref_room_64x48", "room_shell", 64, 48, 500, 50000), ("ref_box_160x120", "uniform_box", 160, 120, 137, 12000)]


def scene_case(orc, pkg, scene, W, H, pose, n):
    xyzw, rgba = orc.generate(scene, SEED + pose, 0, n, n)
    return ("%s_%dx%d_pose%d_n%d" % (scene, W, H, pose, n), xyzw, rgba, pkg.orbit_projection(pose, W, H), W, H)


def scene_cases(orc, pkg):
    return [scene_case(orc, pkg, s, W, H, pose, n) for s in SCENES for (W, H) in SIZES for (pose, n) in POSES]


def frame_cases(orc):
    out = []
    for (W, H) in ((16, 16), (16, 31), (48, 47)):
        P, xyzw, rgba = frame_cloud.frame_cloud(orc, W, H)
        out.append(("frame_cloud_%dx%d" % (W, H), xyzw, rgba, P, W, H))
    return out


def _colours(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3), dtype=np.uint8)


def boundary_points(pkg, W, H, pose, count, seed):
    """Points within +-2 ulp of a half-pixel boundary in u (the construction of tests/test_oracle_vs_pymodel.py)."""
    E = pkg.orbit_pose(pose)
    K = pkg.benchmark_calibration(W, H).getIntrinsicsMatrix()
    Rinv, t = E[:3, :3].T, E[:3, 3]
    rng = np.random.default_rng(seed)
    pts = []
    for _ in range(count):
        u = rng.integers(0, W) + 0.5
        v = rng.integers(0, H) + rng.uniform(-0.4, 0.4)
        z = rng.uniform(0.5, 6.0)
        cam = np.array([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z])
        base = (Rinv @ (cam - t)).astype(np.float32)
        for d in (-2, -1, 0, 1, 2):
            p = base.copy()
            p[0] = np.float32(p[0]) + d * np.spacing(np.float32(p[0]))
            pts.append(p)
    return np.array(pts, np.float32)


def oblique_camera(orc, W, H):
    """The orbit poses keep the camera level: P[1] = P[9] = 0, a product of rows x and z of matmul (render.cu:33-40)
    vanishes and its contraction variants mostly coincide.  Here no entry is zero.  -> (P, K, E)"""
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + np.sin(0.7) * Kx + (1 - np.cos(0.7)) * (Kx @ Kx)
    E[:3, 3] = (0.3, -0.2, 5.0)
    K = np.array([[W * 0.875, 0, W / 2 + 0.5], [0, W * 0.88125, H / 2 - 0.75], [0, 0, 1]])
    return orc.compose_projection(K, E), K, E


def oblique_boundary_points(K, E, W, H, count, seed):
    Rinv, t = E[:3, :3].T, E[:3, 3]
    rng = np.random.default_rng(seed)
    pts = []
    for _ in range(count):
        in_u = rng.random() < 0.5
        u = rng.integers(0, W) + (0.5 if in_u else rng.uniform(-0.4, 0.4))
        v = rng.integers(0, H) + (rng.uniform(-0.4, 0.4) if in_u else 0.5)
        z = rng.uniform(3.0, 8.0)
        cam = np.array([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z])
        base = (Rinv @ (cam - t)).astype(np.float32)
        for d in (-2, -1, 0, 1, 2):
            p = base.copy()
            p[0] = np.float32(p[0]) + d * np.spacing(np.float32(p[0]))
            pts.append(p)
    return np.array(pts, np.float32)


def adversarial(orc, pkg):
    out = []
    P = kat_P(orc)
    # the KAT points (test_gpu_parity.test_kat_points) and the ties of test_oracle_kat.test_kat3
    pts = [(0, 0, 2), (0, 0, 0), (0, 0, -1), (0, 0, 1e-30), (-0.32, 0, 1.0), (-0.325, 0, 1.0), (0.315, 0, 1.0),
           (0.0, 0.0, 1.0), (0.0, 0.0, 1.01), (0.0, 0.0, 1.03)]
    pts += [(x, 0.0, 25.0) for x in (-7.875, -7.625, -7.375, -8.125, 7.875)]
    out.append(("kat_points",) + cloud(pts, [(10 * i, 20, 255 - i) for i in range(len(pts))]) + (P, 64, 48))
    # r.z <= 0, -0, NaN, +-inf, denormals, huge values (test_oracle_vs_pymodel's specials among them)
    nan, inf = float("nan"), float("inf")
    pts = [(0, 0, 0.0), (0, 0, -0.0), (0.1, 0.1, -0.0), (0, 0, -1e-45), (0, 0, 1e-45), (0.3, -0.2, 1e-45), (0, 0, nan),
           (nan, 0, 1), (0, nan, 1), (nan, nan, nan), (0, 0, inf), (0, 0, -inf), (inf, 0, 1), (-inf, 0, 1), (0, inf, 2),
           (inf, inf, inf), (1e30, 0, 1e30), (1e-38, 0, 1e-38), (0, 0, 3e38), (3e38, 0, 1), (-3e38, 3e38, 1),
           (0, 0, 1.17549435e-38), (-0.32, 0.0, 1.0), (0.05, 0.05, 1.5), (0.05, 0.05, 1.51)]
    out.append(("special_values",) + cloud(pts, _colours(len(pts), 1)) + (P, 64, 48))
    # raw bit patterns mixed with an ordinary cloud (test_gpu_parity.test_adversarial_floats), two cameras
    rng = np.random.default_rng(123)
    n, W, H = 20000, 160, 120
    wild = rng.integers(0, 2 ** 32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    tame, _ = orc.generate("room_shell", 3, 0, n, n)
    xyz = np.where(rng.random((n, 1)) < 0.5, wild, tame[:, :3]).astype(np.float32)
    xyz[::7, 2] = np.float32(1e-41)
    xyz[::11, 0] = np.float32(3e38)
    xyzw, rgba = cloud(xyz, _colours(n, 2))
    out.append(("wild_bits_orbit", xyzw, rgba, pkg.orbit_projection(444, W, H), W, H))
    K = np.array([[125.0, 0, 80], [0, 125.0, 60], [0, 0, 1]])
    out.append(("wild_bits_identity", xyzw, rgba, orc.compose_projection(K, np.eye(4)), W, H))
    # a camera whose rotation has no zero entry: a scene, and points +-2 ulp round half-pixel boundaries in u and in v
    Po, Ko, Eo = oblique_camera(orc, 160, 120)
    xyzw, rgba = orc.generate("room_shell", 9, 0, 20000, 20000)
    out.append(("oblique_camera", xyzw, rgba, Po, 160, 120))
    ob = oblique_boundary_points(Ko, Eo, 160, 120, 4000, 4)
    out.append(("oblique_boundaries",) + cloud(ob, _colours(len(ob), 4)) + (Po, 160, 120))
    # within +-2 ulp of half-pixel boundaries
    W, H = 640, 480
    bp = boundary_points(pkg, W, H, 40, 400, 3)
    out.append(("half_pixel_boundaries",) + cloud(bp, _colours(len(bp), 3)) + (pkg.orbit_projection(40, W, H), W, H))
    # one pixel with 255 ... 5000 points (test_gpu_parity.test_packed_accumulator_boundary)
    for n_same in (255, 256, 257, 258, 600, 5000):
        rng = np.random.default_rng(n_same)
        pts = [(0.0, 0.0, 2.0)] * n_same + [(float(x), float(y), 2.0) for x, y in rng.uniform(-0.3, 0.3, size=(400, 2))]
        cols = np.concatenate([np.full((n_same, 3), 255, np.uint8), _colours(400, n_same)])
        out.append(("hot_pixel_%d" % n_same,) + cloud(pts, cols) + (P, 64, 48))
    # two points exactly 0.02f apart, and one ulp either side (render.cu:106), each pair in a pixel of its own
    edge = np.float32(1.0) + np.float32(0.02)
    pts, cols = [], []
    for k, z in enumerate((np.nextafter(edge, np.float32(0), dtype=np.float32), edge,
                           np.nextafter(edge, np.float32(np.inf), dtype=np.float32))):
        for zz in (np.float32(1.0), z):  # x = 0.05 k z / ... keeps both on the ray of pixel (32 + 5 k, 24)
            pts.append((0.05 * k * float(zz), 0.0, float(zz)))
            cols.append((50 * k, 100, 200) if zz == 1.0 else (255, 255, 255))
    out.append(("window_edge",) + cloud(pts, cols) + (P, 64, 48))
    return out
