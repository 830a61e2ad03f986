"""The inputs of the general-camera tests do what their names say (tests/camera_cases.py), checked with the oracle
alone: these are conditions on the inputs, not measurements of the library.  CPU only."""
import numpy as np
import pytest

import camera_cases as cc
import select_ref as sr

W, H = cc.W0, cc.H0
CASES = [(name, pose) for name in cc.NAMES for pose in range(len(cc.POSES))]


def _kept(orc, P, xyzw):
    pix = sr.pixels(orc, xyzw, P, W, H)
    return pix >= 0, pix


def test_table_is_what_it_says(pkg, orc):
    Ps = cc.matrices(pkg)
    assert tuple(Ps) == cc.NAMES and all(len(v) >= 2 and all(P.dtype == np.float32 and P.shape == (16,) for P in v) for v in Ps.values())
    for pose, k in enumerate(cc.POSES):
        assert np.array_equal(Ps["centre"][pose], pkg.orbit_projection(k, W, H))
        for name, e in cc.SCALES.items():  # the same pixels: an exact power of two on the three rows
            assert np.array_equal(Ps[name][pose].reshape(4, 4)[:3], Ps["centre"][pose].reshape(4, 4)[:3] * np.float32(2.0) ** e)
        K, E = cc.intrinsics_and_pose(pkg, "skew", pose)
        assert K[0, 1] == 0.3 * K[0, 0]
        assert np.array_equal(Ps["skew"][pose], orc.compose_projection(K, E))  # (three non-zero terms per sum)
        M = lambda n: Ps[n][pose].astype(np.float64).reshape(4, 4)[:3, :3]  # noqa: E731
        assert np.linalg.det(M("centre")) > 0 and np.linalg.det(M("lefthanded")) < 0 and np.linalg.det(M("mirror_x")) < 0
        assert np.linalg.det(M("mirror_xy")) > 0 and M("mirror_xy")[1, 1] < 0
        assert abs(np.linalg.norm(M("rows_general")[2]) - 0.01) < 1e-6
        Ka = cc._intrinsics("aniso", W, H)
        assert Ka[0, 0] == 40 * Ka[1, 1]


@pytest.mark.parametrize("name,pose", CASES)
def test_clouds_reach_what_they_aim_at(pkg, orc, name, pose):
    P = cc.matrices(pkg)[name][pose]
    cl = cc.clouds(pkg, orc, name, pose)
    zmin, zmax = np.inf, 0.0
    for cname in cc.CLOUDS:
        xyzw = cl[cname]["xyzw"]
        assert 150 * 256 <= len(xyzw) <= 260 * 256, (cname, len(xyzw))
        kept, pix = _kept(orc, P, xyzw)
        assert len(np.unique(pix[kept])) >= 64, (cname, "filled pixels", len(np.unique(pix[kept])))
        if kept.any():
            r = P.astype(np.float64).reshape(4, 4)[2]
            z = xyzw[kept, :3].astype(np.float64) @ r[:3] + r[3]
            zmin, zmax = min(zmin, float(z.min())), max(zmax, float(z.max()))
    # straddle: every half-space has points on both sides among the chunks aimed at it
    s = cl["straddle"]
    kept, _ = _kept(orc, P, s["xyzw"])
    hv = cc.half_space_values(P, s["xyzw"], W, H)
    aim = np.repeat(s["aim"], 256)
    for q in range(5):
        at = (aim & (1 << q)) != 0
        assert (kept & at).sum() >= 32, ("straddle kept", q, int((kept & at).sum()))
        assert (~kept & at & (hv[q] < 0)).sum() >= 32, ("straddle dropped", q, int((~kept & at & (hv[q] < 0)).sum()))
    # lanes: the lane's first point dropped, a later one kept
    kept, _ = _kept(orc, P, cl["lanes"]["xyzw"])
    k4 = kept.reshape(-1, 4)
    assert (~k4[:, 0] & k4[:, 1:].any(axis=1)).sum() >= 16, ("lanes", int((~k4[:, 0] & k4[:, 1:].any(axis=1)).sum()))
    kept, _ = _kept(orc, P, cl["scene"]["xyzw"])
    assert 0.01 * cc.SCENE_N <= kept.sum() <= 0.95 * cc.SCENE_N, ("scene", int(kept.sum()))
    if name == "scale_tiny":
        assert 0 < zmax < 1e-30
    if name == "scale_guard":
        assert zmin < 1e-30 < zmax
    if name == "grid_far":  # quantised: many points coincide
        assert len(np.unique(cl["scene"]["xyzw"], axis=0)) <= cc.SCENE_N - 5000
