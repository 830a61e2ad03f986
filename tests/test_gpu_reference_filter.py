"""-m gpu: the HIP prefilter against the REFERENCE'S OWN filter kernels, compiled for the host (oracle/_ref, built by
oracle/ref_build.py where the reference tree is; the built libraries travel, and nothing here reads the tree).

At 64x48, 160x120 and 320x240 the unfiltered frame is rendered on the GPU and downloaded, the reference's
applyDepthFilter (ref_filter) runs on exactly that frame, and all five filtered outputs -- depth bits, image, mask, the
five fp16 tensor planes, min/max -- are compared with the HIP prefilter's, bit for bit.  No oracle in between.

The cases (tests/ref_cases.py GPU_CASES) are ones whose reference outputs do not depend on how the host compiler
contracts the bilinear blend: the contraction-off and the fused build of the reference agree on them, checked on the
CPU by tests/test_oracle_vs_reference.py (its filter cases include these three) and asserted again below.  Where the
project's layout differs from the reference's on purpose (160x120 has eight rows behind the
filter domain) the documented relation is asserted, as in the CPU file."""
import numpy as np
import pytest

import ref_cases

pytestmark = pytest.mark.gpu
EMPTY = 0x7F7FFFFF


@pytest.fixture(scope="module")
def ref(orc):
    if not orc.ref_available():
        pytest.skip("neither the reference tree nor a built oracle/_ref")
    return {v: orc.ref(v) for v in ("off_recip", "fast_recip")}


@pytest.mark.parametrize("scene,W,H,pose,n", ref_cases.GPU_CASES, ids=["%dx%d" % (c[1], c[2]) for c in ref_cases.GPU_CASES])
def test_hip_prefilter_is_the_reference_filter(pkg, orc, projector, ref, scene, W, H, pose, n):
    name, xyzw, rgba, P, W, H = ref_cases.scene_case(orc, pkg, scene, W, H, pose, n)
    projector.upload_points(xyzw, rgba)
    projector.set_resolution(W, H)
    img, depth = projector.project(P)
    depth_bits = depth.view(np.uint32).reshape(H, W).copy()
    img = img.reshape(H, W, 3).copy()
    assert (depth_bits != EMPTY).sum() > 1000

    r = ref["off_recip"].filter(depth_bits, img)
    f = ref["fast_recip"].filter(depth_bits, img)
    assert all(np.array_equal(r[k], f[k]) for k in ("img", "mask", "minmax", "tensor_raw"))
    assert np.array_equal(r["depth"].view(np.uint32), f["depth"].view(np.uint32))

    img_f, depth_f = projector.project(P, filtered=True)
    depth_f, img_f = depth_f.view(np.uint32).reshape(H, W), img_f.reshape(H, W, 3)
    mask = projector.download(pkg._lib.BUF_MASK).reshape(H, W)
    tensor = projector.download(pkg._lib.BUF_TENSOR).reshape(5, H, W)
    h_eff = (H >> 4) << 4
    assert r["mask"].shape == (h_eff, W) and (h_eff < H) == (H == 120)
    assert np.array_equal(depth_f[:h_eff], r["depth"][:h_eff].view(np.uint32))
    assert np.array_equal(img_f[:h_eff], r["img"][:h_eff])
    assert np.array_equal(mask[:h_eff], r["mask"])
    assert np.array_equal(tensor[:, :h_eff], r["tensor"])  # the same halves; plane stride W * H here, W * H_eff there
    assert np.array_equal(projector.download(pkg._lib.BUF_MINMAX), r["minmax"])
    assert (r["mask"] > 0).sum() > 100 and ((r["mask"] == 0) & (depth_bits[:h_eff] != EMPTY)).sum() > 100
    # rows behind the filter domain: the reference leaves them alone; the project takes them through removeMask
    filled = depth_bits[h_eff:] != EMPTY
    assert np.array_equal(r["depth"][h_eff:].view(np.uint32), depth_bits[h_eff:]) and np.array_equal(r["img"][h_eff:], img[h_eff:])
    assert np.array_equal(mask[h_eff:], np.where(filled, 255, 0))
    assert np.array_equal(depth_f[h_eff:], np.where(filled, depth_bits[h_eff:], 0xBF800000))
    assert np.array_equal(img_f[h_eff:], np.where(filled[..., None], img[h_eff:], 0))
