"""-m gpu: the depth-heuristic prefilter at RAGGED frame sizes and at every level count, bit for bit against the oracle
(tests/test_filter_shapes_host.py pins the oracle against the numpy model at the same shapes).  The other GPU tests
filter round frames only (W a multiple of 32, H % 16 in {0, 8}, nothing below 64x48, levels != 4 at 640x480 alone); the
kernels' shape arithmetic -- tile_pyramid in the tile kernel, k_pyramid, k_filter4's 64x16 blocks with their halo
windows and "doubled truncated" level heights, the k_reduce / k_up / k_final chain -- is exercised here where it can go
wrong.  Clouds cover the frame (tests/frame_cloud.py); the coverage conditions are asserted on the oracle's frames.

levels = 4 (frame_cloud.SHAPES4), what each size pins:
  16x16               one level-4 pixel; every pixel of every level is a border pixel; one tile and one filter block,
                      mostly outside the frame
  16x17, 16x31        1 and 15 tail rows; level 1 has 8 and 15 rows in memory while 8 are used
  32x33               a second tile row holding one (tail) pixel row
  48x47               W < 64, W % 32 = 16, H % 16 = 15
  80x63               W % 64 = 16
  112x65              W % 64 = 48, H % 32 = 1
  144x97, 176x49, 208x111   mixed residues over several tiles and blocks
  4112x1047           64-wide tiles (129x33 > 4096 tiles of 32) with 16 stray columns, odd H
  65552x40            64-wide tiles, 1025 filter blocks per row, last tile 16 wide
  16x131104           more than 4096 tiles even at 64 wide: the atomic fallback at W = 16
levels 1, 2, 3, 5, 6, 7, 8 (frame_cloud.LEVEL_SHAPES): the narrowest widths rtr_set_params lets through, among them
W % 4 == 2 at levels 1 (6x5, 10x7, 14x33: W*H % 4 == 2, where a four-pixel final step would leave the frame and the
tensor planes -- k_final_px) and a single pixel at the coarsest level.

Compared every time: the unfiltered depth, image and accumulators, then the filtered depth, image, mask, min / max and
all five tensor planes."""
import numpy as np
import pytest

import frame_cloud as fc
from streak_ctx import Ctx

pytestmark = pytest.mark.gpu

_refs = {}


class Ref:
    """A frame-covering cloud, its camera(s) and the oracle's frames; computed once and never changed."""

    def __init__(self, orc, W, H, levels=4, filtered=True):
        self.W, self.H, self.levels = W, H, levels
        self.P, self.xyzw, self.rgba = fc.frame_cloud(orc, W, H)
        self.prm = orc.default_params()
        self.prm.levels = levels
        self.r, self.f = self.frames(orc, self.P, filtered)
        if filtered:
            self.cov = fc.coverage(self.r["depth_bits"], self.f["mask"], levels)

    def frames(self, orc, P, filtered=True):
        r = orc.project(self.xyzw, self.rgba, P, self.W, self.H, params=self.prm)
        return r, (orc.filter(r["depth_bits"], r["img"], params=self.prm) if filtered else None)

    def shifted(self, orc, k):
        """Pose k of a consumer test: the camera with cx moved by k pixels; -> (P, unfiltered, filtered)"""
        if not hasattr(self, "_shifted"):
            self._shifted = {}
        if k not in self._shifted:
            P = fc.camera(orc, self.W, self.H, dcx=float(k))
            self._shifted[k] = (P,) + self.frames(orc, P)
        return self._shifted[k]


def ref_of(orc, W, H, levels=4, keep=True, filtered=True):
    key = (W, H, levels, filtered)
    if key in _refs:
        return _refs[key]
    ref = Ref(orc, W, H, levels, filtered)
    if keep:  # (the three large clouds are used by one test each and not kept)
        _refs[key] = ref
    return ref


def assert_covers_edges(ref):
    """levels 4: kept pixels and filled pixels the filter drops in the last 16 columns and in rows [h_eff - 16, h_eff);
    set and clear mask bytes in the tail rows (which the pyramid never tests)."""
    cov = ref.cov
    assert cov["columns"][0] > 0 and cov["columns"][2] > 0, cov
    assert cov["rows"][0] > 0 and cov["rows"][2] > 0, cov
    if cov["tail"] is not None:
        assert cov["tail"][0] > 0 and cov["tail"][1] > 0, cov


def check_unfiltered(pkg, p, r, what):
    L = pkg._lib
    assert np.array_equal(p.download(L.BUF_DEPTH), r["depth_bits"]), ("depth", what)
    assert np.array_equal(p.download(L.BUF_IMAGE), r["img"]), ("image", what)
    assert np.array_equal(p.download(L.BUF_ACCUM), r["acc"]), ("accumulators", what)


def _where(got, want):
    bad = np.argwhere(got != want)
    return len(bad), bad[:6].tolist()


def check_filtered(pkg, p, f, what):
    L = pkg._lib
    H, W = f["mask"].shape
    got = {"mask": p.download(L.BUF_MASK), "depth": p.download(L.BUF_DEPTH), "img": p.download(L.BUF_IMAGE),
           "minmax": p.download(L.BUF_MINMAX), "tensor": p.download(L.BUF_TENSOR).reshape(5, H, W)}
    want = dict(f, depth=f["depth"].view(np.uint32))
    for name in ("minmax", "mask", "depth", "img", "tensor"):
        assert np.array_equal(got[name], want[name]), (name, what) + _where(got[name], want[name])


def phases(p, P):
    p.clear()
    p.min_depth_pass(P)
    p.accumulate_pass(P)
    p.resolve()


MODES = {"tile": 1, "tile-split": 2, "two-pass": 0}


def set_mode(p, m):
    p.set_option("mode", 1 if m else 0)
    p.set_option("split_threshold", 64 if m == 2 else 32768)
    p.set_option("split_slice", 48 if m == 2 else 16384)


@pytest.fixture
def ctx(projector):
    """The shared context with the accumulators kept; every option and parameter a test changes is put back."""
    projector.set_option("keep_accum", 1)
    yield projector
    set_mode(projector, 1)
    projector.set_option("lean", 1)
    projector.set_option("keep_accum", 0)
    projector.set_params(depth_window=0.02, filter_strength=1.025, gradient_threshold=0.03, levels=4)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("W,H", fc.SMALL4, ids=["%dx%d" % s for s in fc.SMALL4])
def test_small_ragged_frames(pkg, orc, ctx, W, H, mode):
    """rtr_render with and without the prefilter, lean frames and the epilogue form.  (A context renders its first
    eight frames of a resolution with the split launch, which a lean frame does not have: ten filtered frames in a
    row, the first and the last compared.  With the split threshold at 64 every frame keeps the split launch.)"""
    ref = ref_of(orc, W, H)
    assert_covers_edges(ref)
    set_mode(ctx, MODES[mode])
    ctx.upload_points(ref.xyzw, ref.rgba)
    ctx.set_resolution(W, H)
    for lean in (1, 0):
        ctx.set_option("lean", lean)
        ctx.render(ref.P, False)
        check_unfiltered(pkg, ctx, ref.r, (mode, lean))
        for k in range(10):
            ctx.render(ref.P, True)
            if k in (0, 9):
                check_filtered(pkg, ctx, ref.f, (mode, lean, k))
        if mode != "two-pass":  # (the tile store's statistics)
            assert ctx.frame_stats()["errors"] == 0


@pytest.mark.parametrize("W,H", fc.SMALL4, ids=["%dx%d" % s for s in fc.SMALL4])
def test_small_ragged_frames_by_phase_calls(pkg, orc, ctx, W, H):
    """clear ... resolve, filter: the pyramid comes from k_pyramid, not from the tile kernel"""
    ref = ref_of(orc, W, H)
    assert_covers_edges(ref)
    ctx.upload_points(ref.xyzw, ref.rgba)
    ctx.set_resolution(W, H)
    for mode in ("tile", "two-pass"):
        set_mode(ctx, MODES[mode])
        phases(ctx, ref.P)
        check_unfiltered(pkg, ctx, ref.r, mode)
        ctx.filter()
        check_filtered(pkg, ctx, ref.f, mode)


@pytest.mark.parametrize("W,H", fc.LARGE4, ids=["%dx%d" % s for s in fc.LARGE4])
def test_large_ragged_frames(pkg, orc, ctx, W, H):
    """The default mode and the phase calls where the tiles are 64 wide, and where even those are too many."""
    ref = ref_of(orc, W, H, keep=False)
    assert_covers_edges(ref)
    ctx.upload_points(ref.xyzw, ref.rgba)
    ctx.set_resolution(W, H)
    ctx.render(ref.P, False)
    check_unfiltered(pkg, ctx, ref.r, "render")
    ctx.render(ref.P, True)
    check_filtered(pkg, ctx, ref.f, "render")
    phases(ctx, ref.P)
    check_unfiltered(pkg, ctx, ref.r, "phases")
    ctx.filter()
    check_filtered(pkg, ctx, ref.f, "phases")
    if -(-W // 64) * -(-H // 32) <= 4096:
        assert ctx.frame_stats()["errors"] == 0
    else:  # (the atomic form bins nothing: a new resolution with no tile store shows that these frames took it)
        with pytest.raises(pkg.RtrError, match="no binned frame"):
            ctx.frame_stats()


LEVEL_CASES = [(lv, W, H) for lv, shapes in sorted(fc.LEVEL_SHAPES.items()) for W, H in shapes]


@pytest.mark.parametrize("mode", ["tile", "two-pass"])
@pytest.mark.parametrize("levels,W,H", LEVEL_CASES, ids=["L%d-%dx%d" % c for c in LEVEL_CASES])
def test_every_level_count_at_the_narrowest_widths(pkg, orc, ctx, levels, W, H, mode):
    """The whole-frame call and the phase calls with levels != 4: k_pyramid, k_reduce (levels 5..8), k_up and
    k_final, or k_final_px where W % 4 == 2."""
    ref = ref_of(orc, W, H, levels)
    set_mode(ctx, MODES[mode])
    ctx.upload_points(ref.xyzw, ref.rgba)
    ctx.set_resolution(W, H)
    ctx.set_params(levels=levels)
    for by_phases in (False, True):
        if by_phases:
            phases(ctx, ref.P)
        else:
            ctx.render(ref.P, False)
        check_unfiltered(pkg, ctx, ref.r, (mode, by_phases))
        if by_phases:
            ctx.filter()
        else:
            ctx.render(ref.P, True)
        check_filtered(pkg, ctx, ref.f, (mode, by_phases))


@pytest.mark.parametrize("levels", sorted(fc.LEVEL_SHAPES))
def test_every_level_count_drops_a_filled_pixel(orc, levels):
    """The cases above are not vacuous: at every level count the filter takes out a filled pixel of some shape."""
    assert sum(ref_of(orc, W, H, levels).cov["all"][2] for W, H in fc.LEVEL_SHAPES[levels]) > 0


@pytest.mark.parametrize("W,H", [(24, 20), (16, 15)], ids=["W24", "H15"])
def test_unsupported_sizes_leave_the_frame_alone(pkg, orc, ctx, W, H):
    """levels 4 needs W % 16 == 0 and H >= 16: RTR_ERR_UNSUPPORTED from the whole-frame calls and from rtr_filter, and
    the last unfiltered frame is still in the buffers."""
    ref = ref_of(orc, W, H, filtered=False)
    ctx.upload_points(ref.xyzw, ref.rgba)
    ctx.set_resolution(W, H)
    ctx.render(ref.P, False)
    check_unfiltered(pkg, ctx, ref.r, "before")
    assert (ref.r["depth_bits"] != orc.EMPTY_DEPTH).any()
    for call in (lambda: ctx.render(ref.P, True), lambda: ctx.project(ref.P, filtered=True), ctx.filter):
        with pytest.raises(pkg.RtrError) as e:
            call()
        assert e.value.code == pkg._lib.RTR_ERR_UNSUPPORTED
        check_unfiltered(pkg, ctx, ref.r, "after")


@pytest.mark.parametrize("W,H", [(112, 65), (48, 47)], ids=["112x65", "48x47"])
def test_render_views_at_ragged_sizes(pkg, orc, W, H):
    ref = ref_of(orc, W, H)
    assert_covers_edges(ref)
    L = pkg._lib
    p = pkg.Projector(0)
    try:
        p.upload_points(ref.xyzw, ref.rgba)
        p.set_resolution(W, H)
        poses = [ref.shifted(orc, k) for k in range(3)]
        p.render_views(np.stack([np.asarray(P, np.float32).reshape(4, 4) for P, _, _ in poses]), True)
        depth, img = p.download(L.BUF_VIEW_DEPTH), p.download(L.BUF_VIEW_IMAGE)
        tensor, minmax = p.download(L.BUF_VIEW_TENSOR), p.download(L.BUF_VIEW_MINMAX)
        for v, (_, _, f) in enumerate(poses):
            assert np.array_equal(minmax[v], f["minmax"]), ("minmax", v)
            assert np.array_equal(depth[v], f["depth"].view(np.uint32)), ("depth", v) + _where(depth[v], f["depth"].view(np.uint32))
            assert np.array_equal(img[v], f["img"]), ("image", v)
            assert np.array_equal(tensor[v], f["tensor"]), ("tensor", v)
    finally:
        p.close()


@pytest.mark.parametrize("W,H", [(112, 65), (32, 33)], ids=["112x65", "32x33"])
def test_overlapped_frames_at_ragged_sizes(pkg, orc, W, H):
    """Six filtered frames back to back with option "overlap" = 1, the camera moved by a pixel each time; every frame
    is cloned on the context's stream between the renders and compared."""
    import torch
    ref = ref_of(orc, W, H)
    assert_covers_edges(ref)
    poses = [ref.shifted(orc, k) for k in range(6)]
    c = Ctx(pkg, ref, {"overlap": 1})
    try:
        c.bufs["mask"] = torch.as_tensor(c.p.device_buffer(pkg._lib.BUF_MASK), device=torch.device("cuda", 0))
        for run in range(2):  # (the second run's frames are lean)
            active, snaps = [], []
            for P, _, _ in poses:
                c.p.render(P, True)
                active.append(c.p.get_option("overlap_active"))
                with torch.cuda.stream(c.st):
                    snaps.append({k: v.clone() for k, v in c.bufs.items()})
            c.st.synchronize()
            assert active[-1] == 1, active
            for k, (s, (_, _, f)) in enumerate(zip(snaps, poses)):
                got = {name: t.cpu().numpy() for name, t in s.items()}
                assert np.array_equal(got["minmax"].view(np.uint32), f["minmax"]), ("minmax", run, k)
                assert np.array_equal(got["mask"], f["mask"]), ("mask", run, k) + _where(got["mask"], f["mask"])
                assert np.array_equal(got["depth"].view(np.uint32), f["depth"].view(np.uint32)), ("depth", run, k)
                assert np.array_equal(got["img"], f["img"]), ("image", run, k)
                assert np.array_equal(got["tensor"].view(np.uint16).reshape(5, H, W), f["tensor"]), ("tensor", run, k)
            assert c.p.frame_stats()["errors"] == 0
    finally:
        c.close()


def test_project_async_at_ragged_sizes(pkg, orc, ctx):
    """Both pinned output slots: filtered at 112x65, unfiltered at 333x131, where neither the depth's nor the image's
    byte count is a multiple of 16."""
    for W, H, filtered in ((112, 65, True), (333, 131, False)):
        ref = ref_of(orc, W, H, filtered=filtered)
        if filtered:
            assert_covers_edges(ref)
            want = [(f["depth"].view(np.uint32), f["img"]) for _, _, f in (ref.shifted(orc, k) for k in range(2))]
            poses = [ref.shifted(orc, k)[0] for k in range(2)]
        else:
            assert (W * H * 4) % 16 and (W * H * 3) % 16
            poses = [fc.camera(orc, W, H, dcx=float(k)) for k in range(2)]
            want = [(r["depth_bits"], r["img"]) for r in (ref.frames(orc, P, False)[0] for P in poses)]
        ctx.upload_points(ref.xyzw, ref.rgba)
        ctx.set_resolution(W, H)
        bufs = [ctx.host_output_buffers(s) for s in range(2)]
        for s in range(2):
            ctx.project_async(poses[s], s, filtered)
        for s in range(2):
            ctx.wait_outputs(s)
            img, depth = bufs[s]
            assert np.array_equal(depth.view(np.uint32), want[s][0]), (W, H, s)
            assert np.array_equal(img, want[s][1]), (W, H, s)
