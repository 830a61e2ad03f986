"""CPU: the checker of tests/test_gpu_filter_shapes.py at the very shapes it is used at.  For every frame size of
frame_cloud.SHAPES4 (levels 4) and frame_cloud.LEVEL_SHAPES (levels 1, 2, 3, 5, 6, 7, 8) the C oracle's prefilter equals
the independent numpy statement (tests/npfilter.py) on all five outputs, and the oracle's frame of the frame-covering
cloud meets the coverage conditions the GPU tests rely on: kept and filtered-out pixels in the last 16 columns and in
the last 16 rows of the pyramid's domain, set and clear mask bytes in the tail rows below it, and for every level count
a filled pixel that the filter drops.

Left out of the numpy comparison: none.  The three large shapes (4112x1047, 65552x40, 16x131104) take about 2 s each in
numpy and are compared too."""
import numpy as np
import pytest

import frame_cloud as fc
import npfilter

CASES = [(4, W, H) for W, H in fc.SHAPES4] + [(lv, W, H) for lv, shapes in sorted(fc.LEVEL_SHAPES.items())
                                             for W, H in shapes]


def _frames(orc, levels, W, H):
    P, xyzw, rgba = fc.frame_cloud(orc, W, H)
    prm = orc.default_params()
    prm.levels = levels
    r = orc.project(xyzw, rgba, P, W, H, params=prm)
    return r, orc.filter(r["depth_bits"], r["img"], params=prm)


@pytest.mark.parametrize("levels,W,H", CASES, ids=["L%d-%dx%d" % c for c in CASES])
def test_oracle_matches_numpy_model_and_covers_the_edges(orc, levels, W, H):
    r, a = _frames(orc, levels, W, H)
    b = npfilter.apply_filter(r["depth_bits"], r["img"], levels=levels)
    assert np.array_equal(a["mask"], b["mask"])
    assert np.array_equal(a["minmax"], b["minmax"])
    assert np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))
    assert np.array_equal(a["img"], b["img"])
    assert np.array_equal(a["tensor"], b["tensor"])
    if levels == 4:
        cov = fc.coverage(r["depth_bits"], a["mask"], levels)
        assert cov["columns"][0] > 0 and cov["columns"][2] > 0, cov
        assert cov["rows"][0] > 0 and cov["rows"][2] > 0, cov
        if cov["tail"] is not None:
            assert cov["tail"][0] > 0 and cov["tail"][1] > 0, cov


@pytest.mark.parametrize("levels", sorted(fc.LEVEL_SHAPES))
def test_every_level_count_drops_a_filled_pixel(orc, levels):
    dropped = 0
    for W, H in fc.LEVEL_SHAPES[levels]:
        r, a = _frames(orc, levels, W, H)
        dropped += fc.coverage(r["depth_bits"], a["mask"], levels)["all"][2]
    assert dropped > 0
