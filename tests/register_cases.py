"""The inputs that the registration tests share (test_register_host.py pins the reference on them without a GPU,
test_gpu_register.py runs the library on them, test_cpp_register.py dumps their moments for the C++ fit).

A case is a dict: res (n, 3) float32 resident points, scan (m, 3) float32 given points, radius, normals (n, 3) float32 of
the resident points, pose (3x4 float64 or None: the pose the single-step tests pass), well (the modes in which the fit is
well posed: "point", "plane"), motion (4x4: scan -> res where the scan is a moved subset, else None).
"""
import math

import numpy as np

import neighbours_cases as nbc

f32, f64 = np.float32, np.float64
RADIUS = 0.1
SCENE_STRIDE = 16   # the scan of a scene: every 16th point
LOOP_N = 6001       # the clouds of the loop tests: the first points of a scene's stream ...
LOOP_STRIDE = 5     # ... and every 5th of them as the scan


def rigid(deg, axis, shift):
    """4x4 float64: a rotation by `deg` degrees about `axis` through the origin, then a translation by `shift`"""
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    t = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    M[:3, 3] = shift
    return M


MOTION = rigid(2.0, (1, 2, 3), (0.02, -0.02, 0.01))                      # 2 degrees about (1, 2, 3) and 3 cm
GENERAL_POSE = rigid(0.7, (3, -1, 2), (0.004, 0.003, -0.005))[:3].copy()  # a pose for the single-step tests


def unmoved(points, M):
    """the scan whose image under M is `points`: M^-1 in float64, rounded to float32"""
    Mi = np.linalg.inv(M)
    return (points.astype(f64) @ Mi[:3, :3].T + Mi[:3, 3]).astype(f32)


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def _case(res, scan, normals, well, motion=None, pose=None, radius=RADIUS):
    return dict(res=np.ascontiguousarray(res, f32), scan=np.ascontiguousarray(scan, f32), radius=radius,
                normals=np.ascontiguousarray(normals, f32), pose=pose, well=well, motion=motion)


def lattice_plane():
    g = np.stack(np.meshgrid(np.arange(48), np.arange(48), indexing="ij"), -1).reshape(-1, 2) / 64.0
    res = np.concatenate([g, np.zeros((g.shape[0], 1))], axis=1).astype(f32)
    M = rigid(1.0, (0, 0, 1), (0.003, -0.002, 0.004))
    nrm = np.tile(f32([0, 0, 1]), (res.shape[0], 1))
    return _case(res, unmoved(res[::3], M), nrm, ("point",), M, radius=0.05)


def corner():
    """three faces of a room corner, jittered in their planes: well posed in both modes"""
    rng = np.random.default_rng(11)
    g = (np.stack(np.meshgrid(np.arange(24), np.arange(24), indexing="ij"), -1).reshape(-1, 2) + rng.uniform(0.1, 0.9, (576, 2))) / 24.0
    z = np.zeros((576, 1))
    res = np.concatenate([np.c_[g, z], np.c_[g[:, :1], z, g[:, 1:]], np.c_[z, g]], axis=0).astype(f32)
    nrm = np.repeat(f32([[0, 0, 1], [0, 1, 0], [1, 0, 0]]), 576, axis=0)
    M = rigid(2.0, (1, 2, 3), (0.012, -0.008, 0.01))
    return _case(res, unmoved(res[1::2], M), nrm, ("point", "plane"), M)


def line():
    t = np.arange(400)[:, None] / 400.0
    res = (t * f64([[0.5, 1.0, -0.5]])).astype(f32)
    M = rigid(0.5, (0, 0, 1), (0.002, 0.001, -0.001))
    nrm = _unit(np.tile(f64([[1.0, 0.0, 1.0]]), (400, 1)))
    return _case(res, unmoved(res[::2], M), nrm, (), M, radius=0.05)


def piles():
    """nearest_cases.tie_lattice("chunks"): every given point has eight resident points at its bitwise-minimal d2, plus
    coincident piles on both sides"""
    import nearest_cases as ncs
    res, given = ncs.tie_lattice("chunks")
    rng = np.random.default_rng(5)
    return _case(res, given, _unit(rng.normal(size=res.shape)), ("point", "plane"), radius=float(ncs.TIE_RADIUS))


def subnormal():
    """d2 below 2^-126: the pairs are kept and their terms are not flushed"""
    base = np.array([[41, 0, 0], [41.5, 0.25, 0], [42, 0, 0.5], [41, 1, 1], [42.5, 1, 0], [41.25, 0.5, 0.75], [43, 0.5, 0.25]], f64)
    scan = base + f64([[0, 2e-20, 0], [0, 0, 2e-20], [1e-20, 0, 0], [0, 1e-20, 1e-20], [2e-21, 0, 0], [0, 0, 0], [0, 3e-20, 0]])
    rng = np.random.default_rng(6)
    return _case(base, scan, _unit(rng.normal(size=base.shape)), ("point", "plane"), radius=0.01)


def nonfinite():
    c = corner()
    scan = c["scan"].copy()
    scan[3, 0], scan[40, 1], scan[41, 2], scan[500] = np.nan, np.inf, -np.inf, (np.nan, np.inf, 0)
    return _case(c["res"], scan, c["normals"], ("point", "plane"), c["motion"])


def nothing_near():
    c = corner()
    return _case(c["res"], c["scan"] + f32([10, 0, 0]), c["normals"], ())


def far_surface():
    """a wavy patch 7 km from the origin: the sums must be centred before they are multiplied"""
    rng = np.random.default_rng(9)
    g = rng.uniform(0, 2, (3000, 2))
    res = np.c_[7000.0 + g[:, 0], -7000.0 + g[:, 1], 0.2 * np.sin(3 * g[:, 0]) * np.cos(2 * g[:, 1]) + 100.0].astype(f32)
    gx, gy = 0.6 * np.cos(3 * g[:, 0]) * np.cos(2 * g[:, 1]), -0.4 * np.sin(3 * g[:, 0]) * np.sin(2 * g[:, 1])
    nrm = _unit(np.c_[-gx, -gy, np.ones(3000)])
    c = f64([7001.0, -6999.0, 100.0])
    M = rigid(0.5, (1, 2, 3), (0, 0, 0))
    M[:3, 3] = c - M[:3, :3] @ c + f64([0.004, -0.003, 0.005])  # (about the patch's middle)
    return _case(res, unmoved(res[::2], M), nrm, ("point", "plane"), M)


def zero_normals():
    """normals as section 6o leaves them where a point has too few neighbours, and a NaN one: those pairs are dropped"""
    c = corner()
    nrm = c["normals"].copy()
    nrm[::7] = 0
    nrm[5] = (-0.0, 0.0, -0.0)
    nrm[9, 1] = np.nan
    nrm[13, 0] = np.inf
    return _case(c["res"], c["scan"], nrm, ("point", "plane"), c["motion"])


def few_pairs(k):
    """k pairs: the thresholds 3 (point) and 6 (plane)"""
    c = corner()
    return _case(c["res"], c["scan"][np.arange(k) * 97 % c["scan"].shape[0]], c["normals"], ())


SPECIALS = {"lattice_plane": lattice_plane, "corner": corner, "line": line, "piles": piles, "subnormal": subnormal,
            "nonfinite": nonfinite, "nothing_near": nothing_near, "far_surface": far_surface, "zero_normals": zero_normals,
            "pairs2": lambda: few_pairs(2), "pairs3": lambda: few_pairs(3), "pairs5": lambda: few_pairs(5), "pairs6": lambda: few_pairs(6)}


def special_cases():
    out = {}
    for name, make in SPECIALS.items():
        c = make()
        if c["pose"] is None and c["motion"] is not None and name != "far_surface":
            c["pose"] = GENERAL_POSE
        out[name] = c
    return out


def scene_case(orc, scene, n=None, stride=SCENE_STRIDE, normals=None):
    """a scene of neighbours_cases.py with the scan a moved subset; normals: (n, 3), or None for fixed pseudo-normals"""
    n = n or nbc.SCENES[scene][0]
    res = np.ascontiguousarray(orc.generate(scene, nbc.SEED, 0, n, n)[0][:, :3])
    if normals is None:
        normals = _unit(np.random.default_rng(n).normal(size=res.shape) + f64([0, 0, 2.0]))
    return _case(res, unmoved(res[::stride], MOTION), normals, ("point",), MOTION)
