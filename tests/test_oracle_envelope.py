"""How far the oracle's arithmetic contract can be from a CUDA build of the reference:
render.cu:33-40 (`matmul` under nvcc's unspecified FMA contraction) and render.cu:65-66 (`__fdividef`, x
times an approximate reciprocal) cannot be reproduced off an NVIDIA toolchain, and the reference ships no golden frame.
Everything else is pinned by tests/test_oracle_vs_reference.py (the reference's kernels compiled for the host); for
these two, the tests here BOUND the gap: every evaluation a CUDA build
could plausibly produce (oracle/rtr_oracle.c "ENVELOPE": other contractions / associations of matmul, IEEE division,
the reciprocal perturbed by +-1 / +-2 ulp) against the contract, on BASELINE C3's cloud and poses (a sample: the full
table in DESIGN.md is tools/oracle_envelope.py at 1e7 points x 100 poses).  CPU only."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_envelope as env  # noqa: E402

W, H = 1920, 1080
N, POSES, FRAME_POSES = 1_000_000, [0, 11, 22, 33, 44, 55, 66, 77, 88, 99], [7, 93]


@pytest.fixture(scope="module")
def rows(pkg, orc):
    xyzw, rgba = orc.generate("room_shell", 0xC0FFEE03, 0, N, N)
    return {(r["mm"], r["dv"]): r for r in env.measure(orc, pkg, xyzw, rgba, W, H, POSES, FRAME_POSES, 8)}


def test_the_contract_is_variant_zero(pkg, orc):
    xyzw, rgba = orc.generate("room_shell", 0xC0FFEE03, 0, 50_000, 50_000)
    P = pkg.orbit_projection(17, 640, 480)
    e = orc.envelope_points(xyzw, P, 640, 480, 0, 0, 2)
    assert e["flips"] == 0 and e["max_depth_ulp"] == 0 and e["accepted"] > 0
    a, b = orc.project(xyzw, rgba, P, 640, 480), orc.project_variant(xyzw, rgba, P, 640, 480, 0, 0)
    assert np.array_equal(a["depth_bits"], b["depth_bits"]) and np.array_equal(a["img"], b["img"])


def test_depth_stays_within_two_ulp(rows):
    """Depth = bits of r.z: only the matmul variants can move it, by at most 2 ulp (measured: <= 1) -- far inside
    north_star's 1e-5 tolerance on float depth (1 ulp of a 3 m depth is 2.4e-7 m)."""
    for r in rows.values():
        assert r["max_depth_ulp"] <= 2, r
    assert all(rows[(0, dv)]["max_depth_ulp"] == 0 for dv in range(1, 6))  # the quotient never touches the depth


def test_pixel_index_flip_rate_is_bounded(rows):
    """A point's pixel index changes only when its quotient sits within the perturbation of a half-pixel boundary:
    <= 1e-4 of the accepted points for the matmul variants and IEEE division, <= 1e-3 with the reciprocal off by
    up to 2 ulp (__fdividef's documented bound; measured 1.3e-4 ... 3.3e-4)."""
    for (mm, dv), r in rows.items():
        bound = 1e-4 if dv <= 1 else 1e-3
        assert r["index_flip_rate"] <= bound, r
    assert rows[(0, 5)]["index_flips"] > 0  # (the measurement does see the effect it bounds)


def test_frames_and_prefilter_masks_barely_move(rows):
    """Whole frames: colour differs on <= 2e-4 of the pixels and the prefilter's keep mask flips on <= 2e-4 of them;
    depth pixels differ by 1 ulp on up to a few 1e-3 of the pixels under the matmul variants (the same surface point,
    rounded differently) and on <= 1e-4 of them under the quotient variants."""
    for (mm, dv), r in rows.items():
        px = r["pixels"]
        assert r["colour_pixels_differ"] <= 2e-4 * px, r
        assert r["mask_flips"] <= 2e-4 * px, r
        assert r["depth_pixels_differ"] <= (5e-3 if mm in (2, 3) else 1e-4) * px, r
        assert r["depth_pixels_beyond_2ulp"] <= 2e-4 * px, r  # (another point wins the pixel: an index flip's consequence)
