"""The projection matrices and the clouds that the general-camera tests share (test_camera_cases_host.py pins with the
oracle alone that they do what their names say, test_frustum_general.py runs the conservative rejections on them on the
host, test_gpu_general_cameras.py the library).  Pure numpy, every seed fixed.

matrices(pkg, W, H) is the table: name -> [P of pose 0, P of pose 1], float32[16] each.  Where an intrinsic matrix K and
a pose E exist it is pkg.compose_projection(K, E); rows_general and the three rescalings are composed in float64 and
rounded once (a power of two: not rounded at all).

  centre        the control: the benchmark calibration on the orbit, as every other test uses it
  offaxis_near  cx = -2.5 W, cy = 0.5 H: a sub-window left of the optical axis
  offaxis_far   cx = 6 W, cy = -4 H
  roll_pitch    37 deg of roll about the optical axis on a pose pitched 80 deg down
  aniso         fx = 40 fy
  skew          K[0,1] = 0.3 fx
  tele          fx = fy = 200 W, the camera 50 scene units from the cloud
  wide          fx = fy = W / 64: the side planes almost coincide with the camera plane
  mirror_x      fx < 0
  mirror_xy     fx < 0 and fy < 0
  lefthanded    det E[:3,:3] = -1
  rows_general  P = A [R | t], A a full upper-triangular 3 x 3 with A[2,2] = 0.01: r.z is not in scene units
  scale_up      centre x 2^40: the same pixels, the depth scaled
  scale_down    centre x 2^-40
  scale_tiny    centre x 2^-104: every accepted r.z lies below 1e-30
  scale_guard   centre x 2^-100: the accepted r.z lie on both sides of 1e-30, the guard of the per-point test
  grid_km       centre, cloud and camera translated by (8192.5, -16384.25, 1024)
  grid_far      the same by (1.2e6, -2.4e6, 300): the cloud is quantised to 0.125 .. 0.25

clouds(pkg, orc, name, pose, W, H) gives the three clouds of a matrix, placed through the float64 inverse of P[:3,:3]:
"straddle", "lanes" and "scene", each a dict with xyzw, rgba and the generator's own notes (which half-space a chunk
is aimed at).  Half-spaces are numbered as csrc/rtr_chunk_box.h numbers them: 0 r.z >= 0, 1 left, 2 right, 3 top,
4 bottom."""
import numpy as np

from helpers import cloud
from test_gpu_chunk_test import _camera, _chunks

W0, H0 = 160, 128
POSES = (17, 523)
NAMES = ("centre", "offaxis_near", "offaxis_far", "roll_pitch", "aniso", "skew", "tele", "wide", "mirror_x", "mirror_xy",
         "lefthanded", "rows_general", "scale_up", "scale_down", "scale_tiny", "scale_guard", "grid_km", "grid_far")
CLOUDS = ("straddle", "lanes", "scene")
SHIFTS = {"grid_km": (8192.5, -16384.25, 1024.0), "grid_far": (1.2e6, -2.4e6, 300.0)}
SCALES = {"scale_up": 40, "scale_down": -40, "scale_tiny": -104, "scale_guard": -100}
SPREADS = ((1e-4, 0), (1e-6, 0), (0.0, 4), (0.02, 0))  # (of the scene scale, then ulps of the stored coordinates)
SCENE_N = 60_001
_cache = {}


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _pose(R, t):
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, t
    return E


def _facing(pkg, k, K, W, H, dist):
    """The orbit's rotation with the scene's centre `dist` units away along the ray of the frame's centre pixel: what a
    frame far off the optical axis needs to see the scene at all."""
    ray = np.linalg.solve(np.asarray(K, np.float64), np.array([W / 2.0, H / 2.0, 1.0]))
    return _pose(pkg.orbit_pose(k)[:3, :3], dist * ray / np.linalg.norm(ray))


def scene_scale(name):
    """The extent of what the camera looks at, in scene units: depths and spreads are multiples of it."""
    return {"tele": 50.0, "scale_tiny": 1.0}.get(name, 4.0)  # (scale_tiny: r.z up to 10 x 2^-104 < 1e-30)


def scene_map(name):
    """(factor, shift): the room of the `scene` cloud is scaled about the origin, then translated."""
    return (0.2 if name == "tele" else 1.0), np.asarray(SHIFTS.get(name, (0.0, 0.0, 0.0)), np.float64)


def _intrinsics(name, W, H):
    f, cx, cy = 0.8 * W, W / 2.0, H / 2.0
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float64)
    if name == "offaxis_near":
        K[0, 2], K[1, 2] = -2.5 * W, 0.5 * H
    elif name == "offaxis_far":
        K[0, 2], K[1, 2] = 6.0 * W, -4.0 * H
    elif name == "aniso":
        K[0, 0], K[1, 1] = 4.0 * W, 0.1 * W
    elif name == "skew":
        K[0, 1] = 0.3 * f
    elif name == "tele":
        K[0, 0] = K[1, 1] = 200.0 * W
    elif name == "wide":
        K[0, 0] = K[1, 1] = W / 64.0
    elif name == "mirror_x":
        K[0, 0] = -f
    elif name == "mirror_xy":
        K[0, 0], K[1, 1] = -f, -f
    return K


def _matrix(pkg, name, k, W, H):
    if name in SCALES:  # (a power of two: exact, and far from the ends of the exponent range)
        P = _matrix(pkg, "centre", k, W, H).reshape(4, 4).copy()
        P[:3] *= np.float32(2.0) ** SCALES[name]
        return P.reshape(16)
    K, E = _intrinsics(name, W, H), pkg.orbit_pose(k)
    if name == "offaxis_near":
        E = _facing(pkg, k, K, W, H, 40.0)
    elif name == "offaxis_far":
        E = _facing(pkg, k, K, W, H, 120.0)
    elif name == "tele":
        E = _facing(pkg, k, K, W, H, 50.0)
    elif name == "roll_pitch":
        E = _pose(_rot("z", 37.0) @ _rot("x", -80.0) @ E[:3, :3], (_rot("z", 37.0) @ _rot("x", -80.0)) @ E[:3, 3])
    elif name == "lefthanded":
        E = _pose(E[:3, :3] @ np.diag([1.0, -1.0, 1.0]), E[:3, 3])
    elif name in SHIFTS:
        E = _pose(E[:3, :3], E[:3, 3] - E[:3, :3] @ np.asarray(SHIFTS[name]))
    if name == "rows_general":
        A = np.array([[0.008 * W, 0.3, 0.005 * W], [0, 0.0088 * W, 0.005 * H], [0, 0, 0.01]], np.float64)
        P = np.zeros((4, 4), np.float64)
        P[:3] = A @ E[:3]
        P[3, 3] = 1.0
        return P.astype(np.float32).reshape(16)
    return pkg.compose_projection(K, E)


def intrinsics_and_pose(pkg, name, pose, W=W0, H=H0):
    """(K, E) of a matrix that is the two composed on the plain orbit (`skew`: the host test composes them with the
    oracle as well)."""
    assert name in ("centre", "aniso", "skew", "wide", "mirror_x", "mirror_xy")
    return _intrinsics(name, W, H), pkg.orbit_pose(POSES[pose])


def matrices(pkg, W=W0, H=H0):
    key = ("P", W, H)
    if key not in _cache:
        _cache[key] = {name: [_matrix(pkg, name, k, W, H) for k in POSES] for name in NAMES}
    return _cache[key]


def _frame(P):
    """Camera centre, inverse of the 3 x 3 part, the three rows and the length of the r.z row, all float64."""
    c, Minv = _camera(P)
    M = np.asarray(P, np.float64).reshape(4, 4)[:3, :3]
    return c, Minv, M, float(np.linalg.norm(M[2]))


def depths(name, P):
    """Four values of r.z spanning three decades of what the matrix gives the scene."""
    return scene_scale(name) * _frame(P)[3] * np.array([0.01, 0.1, 1.0, 10.0])


def _straddle(name, P, W, H, rng):
    c, Minv, M, zunit = _frame(P)
    D = scene_scale(name)
    pts, aim = [], []
    for spread, ulps in SPREADS:
        centres, cam = [], []
        for di, d in enumerate(depths(name, P)):
            fx, fy = (lambda: rng.uniform(0.1, 0.9) * W), (lambda: rng.uniform(0.1, 0.9) * H)
            targets = [(-0.5, fy(), 2), (W - 0.5, fy(), 4), (fx(), -0.5, 8), (fx(), H - 0.5, 16),  # the side planes
                       (-0.5, -0.5, 2 | 8), (W - 0.5, -0.5, 4 | 8), (-0.5, H - 0.5, 2 | 16), (W - 0.5, H - 0.5, 4 | 16),  # corners
                       (-1.0, fy(), 2), (float(W), fy(), 4), (fx(), -1.0, 8), (fx(), float(H), 16)]  # one pixel outside
            if di % 2:  # the margins of the per-point conservative test
                targets += [(-0.75, fy(), 2), (W + 0.25, fy(), 4), (fx(), -0.75, 8), (fx(), H + 0.25, 16)]
            for u, v, a in targets:
                centres.append(c + d * (Minv @ np.array([u, v, 1.0])))
                aim.append(a)
            cam.append(d)
        pts.append(_chunks(centres, rng, spread * D, ulps))
        for d in cam:  # across the camera plane: r.z within +-d x spread / 0.02, the pixel anywhere around the frame
            for _ in range(2):
                z = rng.uniform(-1.0, 1.0, 256) * d * (spread / 0.02)
                u, v = rng.uniform(-0.1, 1.1, 256) * W, rng.uniform(-0.1, 1.1, 256) * H
                q = c + (Minv @ np.stack([u * z, v * z, z])).T
                pts.append(_chunks(q[:1], rng, 0.0, ulps) if ulps else q.astype(np.float32))
                aim.append(1)
    return np.concatenate(pts), np.asarray(aim, np.int32)


def _lanes(name, P, W, H, rng):
    """Per lane: point 4 l outside, one of 4 l + 1 .. 4 l + 3 inside, the step between them along the sign vector of the
    margin's coefficients -- the direction in which the lane test's L1 bound is attained."""
    c, Minv, M, zunit = _frame(P)
    pts, kind = [], []
    sides = {1: (0, -0.5, 1.0, M[0] + 0.75 * M[2]), 2: (0, W - 0.5, -1.0, (W + 0.25) * M[2] - M[0]),
             3: (1, -0.5, 1.0, M[1] + 0.75 * M[2]), 4: (1, H - 0.5, -1.0, (H + 0.25) * M[2] - M[1])}
    lanes = np.arange(64)
    for d in depths(name, P):
        for q in (1, 2, 3, 4, 0):
            for rep in range(8):
                # (the point kernel lets a chunk go only when EVERY lane is rejected: in three chunks of eight all lanes
                # are far outside and barely inside by about the same step, so that a bound half as large would lose them)
                tight = rep >= 5
                uv = np.stack([rng.uniform(0.05, 0.95, 64) * W, rng.uniform(0.05, 0.95, 64) * H])
                if q == 0:  # across the camera plane
                    z1 = d * (rng.uniform(0.05, 0.1, 64) if tight else rng.uniform(0.05, 1.0, 64))
                    z0 = -d * (rng.uniform(0.9, 1.0, 64) if tight else rng.uniform(0.05, 1.0, 64))
                    inner = c + (Minv @ np.stack([uv[0] * z1, uv[1] * z1, z1])).T
                    outer = inner - np.sign(M[2]) * ((z1 - z0) / np.abs(M[2]).sum())[:, None]
                    tau = 0.04
                else:
                    axis, edge, inward, g = sides[q]
                    t_out = edge - inward * (rng.uniform(1.9, 2.0, 64) if tight else rng.uniform(0.3, 2.0, 64))
                    uv[axis] = edge + inward * (rng.uniform(0.02, 0.08, 64) if tight else rng.uniform(0.02, 0.98, 64))
                    inner = c + d * (Minv @ np.stack([uv[0], uv[1], np.ones(64)])).T
                    e = np.sign(g)
                    ra, rz = (inner - c) @ M[axis], (inner - c) @ M[2]
                    ga, gz = M[axis] @ e, M[2] @ e
                    den = ga - t_out * gz
                    with np.errstate(all="ignore"):
                        t = np.where(den != 0, (ra - t_out * rz) / den, -1.0)
                    uv[axis] = t_out  # (where there is no such step: along the image axis alone)
                    along = c + d * (Minv @ np.stack([uv[0], uv[1], np.ones(64)])).T
                    good = (t > 0) & (rz - t * gz > 0.25 * rz)
                    outer = np.where(good[:, None], inner - t[:, None] * e, along)
                    tau = 0.1
                chunk = outer[:, None, :] + rng.uniform(0.0, tau, (64, 4, 1)) * (inner - outer)[:, None, :]
                chunk[:, 0] = outer
                chunk[lanes, rng.integers(1, 4, 64)] = inner
                pts.append(chunk.reshape(256, 3).astype(np.float32))
                kind.append(q)
    return np.concatenate(pts), np.asarray(kind, np.int32)


def clouds(pkg, orc, name, pose, W=W0, H=H0):
    """-> {"straddle": ..., "lanes": ..., "scene": ...}: dicts of xyzw, rgba and `aim` (per chunk: straddle a bit mask of
    the half-spaces the chunk is aimed at, lanes the half-space's number); shared, never written to."""
    key = (name, pose, W, H)
    if key in _cache:
        return _cache[key]
    P = matrices(pkg, W, H)[name][pose]
    seed = 1000 * NAMES.index(name) + 10 * pose + (W * 7 + H) % 7
    out = {}
    for ci, (cname, make) in enumerate((("straddle", _straddle), ("lanes", _lanes))):
        rng = np.random.default_rng(seed + ci)
        pts, aim = make(name, P, W, H, rng)
        xyzw, rgba = cloud(pts, rng.integers(0, 256, size=(len(pts), 3), dtype=np.uint8))
        out[cname] = {"xyzw": xyzw, "rgba": rgba, "aim": aim}
    key_s = ("room", SCENE_N)
    if key_s not in _cache:
        _cache[key_s] = orc.generate("room_shell", 61, 0, SCENE_N, SCENE_N)
    xyzw, rgba = _cache[key_s]
    factor, shift = scene_map(name)
    moved = xyzw.copy()
    moved[:, :3] = (xyzw[:, :3].astype(np.float64) * factor + shift).astype(np.float32)
    out["scene"] = {"xyzw": moved, "rgba": rgba, "aim": None}
    for v in out.values():
        v["xyzw"].setflags(write=False)
        v["rgba"].setflags(write=False)
    _cache[key] = out
    return out


def half_space_values(P, xyz, W, H):
    """float64 [5, n]: the five half-space functions at the points (>= 0 inside, up to the exact test's rounding)."""
    M = np.asarray(P, np.float64).reshape(4, 4)
    r = M[:3, :3] @ np.asarray(xyz, np.float64)[:, :3].T + M[:3, 3:4]
    return np.stack([r[2], r[0] + 0.5 * r[2], (W - 0.5) * r[2] - r[0], r[1] + 0.5 * r[2], (H - 0.5) * r[2] - r[1]])
