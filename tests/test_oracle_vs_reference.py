"""CPU: the oracle against the REFERENCE'S OWN KERNELS, compiled for the host (oracle/ref_build.py -> oracle/_ref/).

The four builds are {contraction off | the host compiler's own} x {__fdividef = x * RN(1/z) | IEEE x / z}.  What a host
build decides it decides exactly, so every comparison below is an equality of bits:

  projection   contraction off  ==  oracle.project_variant(mm=2, dv=0 | 1)       depth bits, four accumulators, image
               compiler's own   ==  one form of matmul PER ROW (x, y: mm 0, z: mm 1), which is the contract itself
                                    (oracle.project) under every level camera and differs from it by <= 1 ulp of depth
                                    under an oblique one
  prefilter    contraction off  ==  tests/npfilter.py with blend="unfused"        all five outputs and min/max
               compiler's own   ==  oracle.filter; its blend is fma(1 - w, a, RN(w b)) -- the OTHER product fused than in
                                    the contract's fma(w, b, RN((1 - w) a)) -- shown on resizeKernel's own output
  end to end   ref_frame == ref_project followed by ref_filter

Only the pixels the reference's launch geometry writes are compared (quirks Q1/Q2 of DESIGN.md section 2), and where
the project's layout differs on purpose (Q3) the documented relation is asserted instead of equality.

With the reference tree present these tests FAIL when oracle/_ref cannot be built; they skip only when neither the tree
nor a built oracle/_ref is there.  The last two tests need neither: they check the oracle against reference-made
fixtures (tests/golden/ref_*.npz, written by tests/golden/make_ref_golden.py from the contraction-off builds)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import npfilter
import ref_cases

EMPTY = 0x7F7FFFFF
LEVELS = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref(orc):
    if not orc.ref_available():
        pytest.skip("neither the reference tree nor a built oracle/_ref")
    libs = {v: orc.ref(v) for v in orc.REF_VARIANTS}  # builds; an error here is a failure, not a skip
    return libs


@pytest.fixture(scope="module")
def clouds(orc, pkg):
    return ref_cases.scene_cases(orc, pkg) + ref_cases.adversarial(orc, pkg)


@pytest.fixture(scope="module")
def filter_inputs(orc, pkg):
    """The ORACLE's unfiltered frame of every filter case: (name, depth_bits, img)."""
    out = []
    for name, xyzw, rgba, P, W, H in ref_cases.scene_cases(orc, pkg) + ref_cases.frame_cases(orc):
        u = orc.project(xyzw, rgba, P, W, H)
        out.append((name, u["depth_bits"], u["img"]))
    return out


def written(W, H):
    """How many pixels, in linear order, the grids of fillBuffer and resolvePass cover (project_cloud.cu:293-294,
    316, 325): (W / 16) * (H / 16) blocks of 256 threads, each thread its linear index."""
    return (W // 16) * (H // 16) * 256


def assert_same_frame(a, b, W, H, what):
    n = written(W, H)
    for k in ("depth_bits", "acc", "img"):
        x, y = a[k].reshape(W * H, -1)[:n], b[k].reshape(W * H, -1)[:n]
        assert np.array_equal(x, y), (what, k, int((x != y).any(axis=1).sum()))


def differs(a, b, W, H):
    n = written(W, H)
    return any(not np.array_equal(a[k].reshape(W * H, -1)[:n], b[k].reshape(W * H, -1)[:n]) for k in ("depth_bits", "acc", "img"))


def test_builds_are_what_their_names_say(ref):
    assert [(ref[v].contracted, ref[v].ieee_quotient) for v in ("off_recip", "off_ieee", "fast_recip", "fast_ieee")] == \
        [(False, False), (False, True), (True, False), (True, True)]


def test_inputs_do_what_they_are_for(orc, clouds):
    """The adversarial clouds reach what they are named after (asserted on the oracle's frames)."""
    byname = {c[0]: c for c in clouds}
    assert len(clouds) == 18 + 14
    _, xyzw, rgba, P, W, H = byname["window_edge"]
    acc = orc.project(xyzw, rgba, P, W, H)["acc"]
    assert [int(acc[24, 32 + 5 * k, 3]) for k in range(3)] == [2, 2, 1]  # one ulp below, exactly 0.02f, one ulp above
    for n_same in (255, 256, 257, 258, 600, 5000):
        _, xyzw, rgba, P, W, H = byname["hot_pixel_%d" % n_same]
        assert orc.project(xyzw, rgba, P, W, H)["acc"][24, 32, 3] >= n_same
    _, xyzw, rgba, P, W, H = byname["half_pixel_boundaries"]
    pix = [orc.project_point(P, float(x), float(y), float(z), W, H)[0] for x, y, z in xyzw[:, :3]]
    groups = np.array(pix).reshape(-1, 5)
    assert ((groups.min(axis=1) != groups.max(axis=1)) & (groups.min(axis=1) >= 0)).sum() > 100  # the 5 ulp steps straddle a boundary
    for name in ("wild_bits_orbit", "wild_bits_identity", "special_values"):
        _, xyzw, rgba, P, W, H = byname[name]
        assert not np.isfinite(xyzw[:, :3]).all()
        assert (orc.project(xyzw, rgba, P, W, H)["depth_bits"] != EMPTY).sum() >= (3 if name == "special_values" else 500)


@pytest.mark.parametrize("quotient,dv", [("recip", 0), ("ieee", 1)])
def test_projection_without_contraction_is_variant_mm2(orc, ref, clouds, quotient, dv):
    """No compiler freedom left: the reference's text with every operation rounded on its own IS mm 2."""
    lib = ref["off_" + quotient]
    for name, xyzw, rgba, P, W, H in clouds:
        assert_same_frame(lib.project(xyzw, rgba, P, W, H), orc.project_variant(xyzw, rgba, P, W, H, 2, dv), W, H, name)


FUSED_ROWS = (0, 0, 1)  # the forms (oracle MM_VARIANTS) this host compiler gives rows x, y, z of matmul; DESIGN.md section 2


@pytest.mark.parametrize("quotient,dv", [("recip", 0), ("ieee", 1)])
def test_projection_fused_by_the_host_compiler(orc, ref, clouds, quotient, dv):
    """matmul (render.cu:33-40) as the host compiler contracts it.  FINDING: it is none of the five forms mm 0..4 applied
    to all rows -- gcc picks a form PER ROW: rows x and y as the contract (mm 0: t = m0 x; fma(m1, y, t); fma(m2, z, t);
    + m3), row z with the first add fused with the LEFT product (mm 1: t = m1 y; fma(m0, x, t); ...).  Both are
    legal contractions of the same text, and nvcc is as free.  What is asserted, all of it exact:
      * of the 125 per-row assignments exactly one reproduces the fused build on the two oblique-camera clouds, and
        it is FUSED_ROWS; that assignment then reproduces the fused build on EVERY cloud
      * on every cloud whose camera has P[1] == P[9] == 0 (all but the oblique ones: a level camera or K * I) the
        two forms cannot differ in rows x and z, so the fused build IS the contract, oracle.project, bit for bit
      * on the oblique boundary cloud it is none of mm 0..4 (on the oblique scene only mm 1: no point there is near
        enough to a pixel boundary for rows x and y to matter), and against the contract it stays inside the envelope that
        tests/test_oracle_envelope.py asserts: depth <= 2 ulp wherever the same point wins, another point wins (or
        colour differs) on <= 2e-4 of the pixels of the scene frame."""
    lib = ref["fast_" + quotient]
    byname = {c[0]: c for c in clouds}
    oblique = ("oblique_camera", "oblique_boundaries")
    got = {name: lib.project(*byname[name][1:]) for name in oblique}
    matches = []
    for mz in range(5):
        for my in range(5):
            for mx in range(5):
                if not any(differs(got[name], orc.project_variant(*byname[name][1:], orc.mm_rows(mx, my, mz), dv),
                                   *byname[name][4:]) for name in oblique):
                    matches.append((mx, my, mz))
    assert matches == [FUSED_ROWS], "the host compiler contracts matmul differently now: %s (update DESIGN.md section 2)" % matches
    contract_clouds = 0
    for name, xyzw, rgba, P, W, H in clouds:
        f = lib.project(xyzw, rgba, P, W, H)
        assert_same_frame(f, orc.project_variant(xyzw, rgba, P, W, H, orc.mm_rows(*FUSED_ROWS), dv), W, H, name)
        contract = orc.project(xyzw, rgba, P, W, H) if dv == 0 else orc.project_variant(xyzw, rgba, P, W, H, 0, dv)
        if name in oblique:
            assert P[1] != 0 and P[9] != 0
            same = [mm for mm in range(5) if not differs(f, orc.project_variant(xyzw, rgba, P, W, H, mm, dv), W, H)]
            # (the scene's points are not near enough to a boundary for rows x and y to tell mm 0 from mm 1)
            assert same == ([] if name == "oblique_boundaries" else [1]), (name, same)
        else:
            assert P[1] == 0 and P[9] == 0, name
            assert_same_frame(f, contract, W, H, name)
            contract_clouds += 1
        if name == "oblique_camera":
            n = written(W, H)
            a, b = f["depth_bits"].reshape(-1)[:n].astype(np.int64), contract["depth_bits"].reshape(-1)[:n].astype(np.int64)
            ulp = np.abs(a - b)
            colour = (f["img"].reshape(-1, 3)[:n] != contract["img"].reshape(-1, 3)[:n]).any(axis=1).sum()
            counts = (f["acc"].reshape(-1, 4)[:n] != contract["acc"].reshape(-1, 4)[:n]).any(axis=1).sum()
            print("fused build vs contract, %s (%d pixels, %d filled): depth differs on %d (max %d ulp), beyond 2 ulp on %d, "
                  "colour on %d, accumulators on %d" % (name, n, (a != EMPTY).sum(), (ulp > 0).sum(), ulp[ulp <= 2].max(),
                                                       (ulp > 2).sum(), colour, counts))
            assert (ulp > 0).sum() > 50                      # (the two do differ: this case sees what it bounds)
            assert (ulp > 2).sum() <= 2e-4 * n and colour <= 2e-4 * n and counts <= 2e-4 * n
    assert contract_clouds == len(clouds) - 2 == 30


@pytest.mark.parametrize("W,H", [(64, 48), (160, 120), (320, 240), (100, 75), (16, 31)])
def test_unwritten_pixels_are_the_ones_design_names(orc, pkg, ref, W, H):
    """Q1/Q2: fillBuffer and resolvePass run on a grid of (W / 16) x (H / 16) blocks of 16 x 16 threads, each thread
    its LINEAR index, so exactly the first (W/16)(H/16)256 pixels are written -- for W % 16 == 0 that is every row
    below H - H % 16 (rows 112..119 at 160x120; 1072..1079 at 1080p).  Undefined memory is played by two different
    poison bytes.  The oracle clears and resolves every pixel."""
    xyzw, rgba = orc.generate("uniform_box", 77, 0, 30000, 30000)
    P = pkg.orbit_projection(137, W, H)
    lib = ref["off_recip"]
    lo, hi = lib.project(xyzw, rgba, P, W, H, poison=0x00), lib.project(xyzw, rgba, P, W, H, poison=0xFF)
    n = written(W, H)
    # fillBuffer: with poison 0 the depth of an unwritten pixel stays 0 (atomicMin cannot lower it); written pixels
    # hold positive float bits or the sentinel
    unwritten_depth = lo["depth_bits"].reshape(-1) == 0
    # resolvePass: an unwritten image pixel shows either poison; a written one is the same in both runs
    unwritten_img = (lo["img"].reshape(-1, 3) == 0x00).all(axis=1) & (hi["img"].reshape(-1, 3) == 0xFF).all(axis=1)
    expect = np.arange(W * H) >= n
    assert np.array_equal(unwritten_depth, expect) and np.array_equal(unwritten_img, expect)
    if W % 16 == 0:
        assert np.array_equal(expect.reshape(H, W), np.broadcast_to((np.arange(H) >= H - H % 16)[:, None], (H, W)))
    assert expect.sum() == {(64, 48): 0, (160, 120): 8 * 160, (320, 240): 0, (100, 75): 7500 - 6144, (16, 31): 15 * 16}[(W, H)]
    assert_same_frame(lo, hi, W, H, "poison must not reach a written pixel")
    o = orc.project_variant(xyzw, rgba, P, W, H, 2, 0)
    assert_same_frame(lo, o, W, H, "oracle")
    # the oracle on the pixels the reference leaves undefined: cleared (the sentinel, or a point's depth), and resolved
    d, acc, img = o["depth_bits"].reshape(-1)[n:], o["acc"].reshape(-1, 4)[n:].astype(np.int64), o["img"].reshape(-1, 3)[n:]
    assert ((d == EMPTY) == (acc[:, 3] == 0)).all() and ((d > 0) & (d <= EMPTY)).all()
    cnt = np.maximum(acc[:, 3:4], 1)
    assert np.array_equal(img, np.where(acc[:, 3:4] > 0, acc[:, :3] // cnt, 0).astype(np.uint8))
    if expect.any() and (W, H) != (16, 31):
        assert (acc[:, 3] > 0).any()  # (the case is not vacuous: the camera sees points down there)


def test_block_size_does_not_change_a_result(orc, pkg, ref):
    """project_cloud.cu:216 takes block_size from the occupancy API of the GPU at hand; it must not matter."""
    name, xyzw, rgba, P, W, H = ref_cases.scene_case(orc, pkg, "room_shell", 160, 120, 500, 50000)
    lib = ref["off_recip"]
    u0, f0 = lib.frame(xyzw, rgba, P, W, H, block_size=1024)
    for bs in (768, 96):
        u, f = lib.frame(xyzw, rgba, P, W, H, block_size=bs)
        assert all(np.array_equal(u[k], u0[k]) for k in u)
        assert all(np.array_equal(f[k], f0[k]) for k in ("img", "mask", "minmax", "tensor_raw"))
        assert np.array_equal(f["depth"].view(np.uint32), f0["depth"].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# prefilter

def same_filter_outputs(r, o, W, H):
    """Reference outputs `r` (RefLib.filter) against a statement `o` in the PROJECT's layout (oracle.filter /
    npfilter.apply_filter).  Inside the reference's filter domain -- rows < H_eff, the truncated dims doubled back
    (project_cloud.cu:336-361) -- everything is equal.  Q3, where the project differs on purpose:
      tensor   the reference's plane stride is W * H_eff (removeMask is given the doubled-back dims), the project's W * H;
               plane c, row y < H_eff, column x hold the same half either way, and the reference writes nothing
               behind 5 * W * H_eff
      rows >= H_eff   the reference leaves depth and image as they were and has no mask; the project takes them through
               removeMask with mask = non-empty ? 255 : 0 (asserted on `o` in test_tail_rows_follow_design).
    -> list of the outputs that differ (empty = same)."""
    h_eff = (H >> LEVELS) << LEVELS
    assert r["mask"].shape == (h_eff, W) and r["tensor"].shape == (5, h_eff, W)
    bad = []
    if not np.array_equal(r["depth"][:h_eff].view(np.uint32), o["depth"][:h_eff].view(np.uint32)):
        bad.append("depth")
    if not np.array_equal(r["img"][:h_eff], o["img"][:h_eff]):
        bad.append("img")
    if not np.array_equal(r["mask"], o["mask"][:h_eff]):
        bad.append("mask")
    if not np.array_equal(r["tensor"], o["tensor"][:, :h_eff]):
        bad.append("tensor")
    if not np.array_equal(r["minmax"], o["minmax"]):
        bad.append("minmax")
    return bad


def test_filter_without_contraction_is_the_unfused_statement(ref, filter_inputs):
    for name, depth_bits, img in filter_inputs:
        H, W = depth_bits.shape
        r = ref["off_recip"].filter(depth_bits, img)
        assert same_filter_outputs(r, npfilter.apply_filter(depth_bits, img, blend="unfused"), W, H) == [], name
        r2 = ref["off_ieee"].filter(depth_bits, img)  # (no quotient in the filter: the same text, the same result)
        assert all(np.array_equal(r[k], r2[k]) for k in ("img", "mask", "minmax", "tensor_raw")), name


def test_filter_fused_by_the_host_compiler_is_the_oracle(orc, ref, filter_inputs):
    """... bit for bit on all 21 cases, although gcc fuses the blend the other way round than the contract does (next
    test): blended values reach the outputs only through comparisons.  Fused == unfused on at least 5 of every 6 cases
    (here: on all of them)."""
    agree = 0
    for name, depth_bits, img in filter_inputs:
        H, W = depth_bits.shape
        f = ref["fast_recip"].filter(depth_bits, img)
        assert same_filter_outputs(f, orc.filter(depth_bits, img), W, H) == [], name
        u = ref["off_recip"].filter(depth_bits, img)
        agree += all(np.array_equal(f[k], u[k]) for k in ("img", "mask", "minmax", "tensor_raw")) and \
            np.array_equal(f["depth"].view(np.uint32), u["depth"].view(np.uint32))
    print("fused == unfused reference outputs on %d of %d filter cases" % (agree, len(filter_inputs)))
    assert len(filter_inputs) == 21 and 6 * agree >= 5 * len(filter_inputs)


@pytest.mark.parametrize("oh,ow", [(2, 2), (6, 10), (30, 14), (64, 64)])
def test_blend_form_of_each_build(ref, oh, ow):
    """resizeKernel's own output (project_cloud.cu:157-160) on random levels, clamped borders included:
    contraction off == "unfused";  gcc's contraction == "fused_left", fma(1 - w, a, RN(w b)), and differs from the
    contract's "fused" form fma(w, b, RN((1 - w) a)) on a share of the pixels.  Which one nvcc picks stays unknown."""
    rng = np.random.default_rng(oh * 100 + ow)
    lo = rng.uniform(0.5, 8, (oh // 2, ow // 2)).astype(np.float32)
    hi = rng.uniform(0.5, 8, (oh, ow)).astype(np.float32)
    mask = np.where(rng.random((oh, ow)) < 0.3, 255, 0).astype(np.uint8)
    want = {}
    for blend in ("fused", "unfused", "fused_left"):
        want[blend] = hi.copy()
        npfilter.resize_into(lo, want[blend], mask, blend)
    off, fast = ref["off_recip"].resize(lo, hi, mask), ref["fast_recip"].resize(lo, hi, mask)
    assert np.array_equal(off.view(np.uint32), want["unfused"].view(np.uint32))
    assert np.array_equal(fast.view(np.uint32), want["fused_left"].view(np.uint32))
    assert np.array_equal(off[mask > 0], hi[mask > 0]) and (off[mask == 0] != hi[mask == 0]).any()
    if oh * ow >= 60:
        assert (fast.view(np.uint32) != want["fused"].view(np.uint32)).sum() > 0
        assert (off.view(np.uint32) != want["fused"].view(np.uint32)).sum() > 0


def test_tail_rows_follow_design(orc, ref, filter_inputs):
    """Q3 at H % 16 != 0 (16x31, 48x47, 160x120): what the reference does with rows >= H_eff and behind 5 W H_eff halves
    (nothing), and what the project does instead."""
    seen = 0
    for name, depth_bits, img in filter_inputs:
        H, W = depth_bits.shape
        h_eff = (H >> LEVELS) << LEVELS
        if h_eff == H:
            continue
        seen += 1
        r = ref["off_recip"].filter(depth_bits, img)
        assert np.array_equal(r["depth"][h_eff:].view(np.uint32), depth_bits[h_eff:]) and np.array_equal(r["img"][h_eff:], img[h_eff:])
        assert (r["tensor_raw"][5 * W * h_eff:] == orc.REF_POISON * 0x0101).all()
        o = orc.filter(depth_bits, img)
        filled = depth_bits[h_eff:] != EMPTY
        assert np.array_equal(o["mask"][h_eff:], np.where(filled, 255, 0))
        assert np.array_equal(o["depth"][h_eff:].view(np.uint32), np.where(filled, depth_bits[h_eff:], 0xBF800000))
        assert np.array_equal(o["img"][h_eff:], np.where(filled[..., None], img[h_eff:], 0))
        assert np.array_equal(o["tensor"][3, h_eff:], np.where(filled, 0x3C00, 0))
        assert np.array_equal(o["tensor"][4, h_eff:][~filled], np.full((~filled).sum(), 0xBC00))
        if "frame_cloud" in name and H - h_eff > 1:
            assert filled.any() and (~filled).any()
    assert seen == 6 + 2


@pytest.mark.parametrize("scene,W,H,pose,n", [("room_shell", 64, 48, 137, 12000), ("uniform_box", 160, 120, 500, 50000),
                                              ("room_shell", 320, 240, 500, 50000)])
def test_frame_is_project_then_filter(orc, pkg, ref, scene, W, H, pose, n):
    """End to end on one set of buffers (computeFilteredRGBD).  At 160x120 the unfiltered frame has eight undefined
    rows; the filter reads them (reduce, level 1) but nothing derived from them reaches an output below H_eff."""
    name, xyzw, rgba, P, W, H = ref_cases.scene_case(orc, pkg, scene, W, H, pose, n)
    h_eff = (H >> LEVELS) << LEVELS
    for v in ("off_recip", "fast_ieee"):
        lib = ref[v]
        u, f = lib.frame(xyzw, rgba, P, W, H)
        u2 = lib.project(xyzw, rgba, P, W, H)
        assert all(np.array_equal(u[k], u2[k]) for k in u)
        f2 = lib.filter(u2["depth_bits"], u2["img"])
        assert all(np.array_equal(f[k], f2[k]) for k in ("img", "mask", "minmax", "tensor_raw"))
        assert np.array_equal(f["depth"].view(np.uint32), f2["depth"].view(np.uint32))
        uo, fo = lib.frame(xyzw, rgba, P, W, H, poison=0x00)
        assert np.array_equal(f["depth"][:h_eff].view(np.uint32), fo["depth"][:h_eff].view(np.uint32))
        assert all(np.array_equal(f[k], fo[k]) for k in ("mask", "minmax", "tensor"))
        assert (f["mask"] > 0).sum() > 30


def test_reference_program_under_the_sanitizers(orc, tmp_path):
    """The driver's stand-alone main (one 160x120 frame through ref_frame) built with -fsanitize=address,undefined:
    a clean run and the same checksums as the plain build -- with one element of slack behind every buffer AND
    without: resolvePass tests `id > count` (render.cu:145), but its grid has at most W * H threads, so id == count
    never runs and the off-by-one is out of reach of the reference's own launch.  CPU only; nothing is loaded into
    Python under a sanitizer."""
    rb = orc.ref_builder()
    if not rb.have_reference():
        pytest.skip("needs the reference tree (it compiles the reference's sources)")
    san = rb.check_program(str(tmp_path / "ref_check_san"), sanitize=True)
    plain = rb.check_program(str(tmp_path / "ref_check"), sanitize=False)
    want = subprocess.check_output([plain], text=True)
    assert want.count("\n") == 2 and "mask 160x112" in want
    for args in (["1"], ["0"], ["0", "96"]):
        got = subprocess.run([san] + args, text=True, capture_output=True)
        assert got.returncode == 0 and got.stderr == "", (args, got.stderr[-2000:])
        assert got.stdout == want, args


def test_recipe_fails_loudly_on_a_tree_without_the_markers(orc, tmp_path, monkeypatch):
    """The kernel region is cut by markers; a tree whose project_cloud.cu lacks them, or has other text between them,
    must stop the build instead of compiling something else.  (Made-up files; nothing of the reference is needed.)"""
    rb = orc.ref_builder()
    src = tmp_path / "tree" / "src" / "RTRenderer" / "src"
    src.mkdir(parents=True)
    monkeypatch.setenv("RTR_REFERENCE_DIR", str(tmp_path / "tree"))
    (src / "render.cu").write_text("\n")
    for text, what in (("int x;\n", "markers"),
                       ("#define THREADS_PER_BLOCK 1024\n__global__ void reduce(float* a) {}\nProjectCloud::ProjectCloud(int) {}\n", "five filter kernels")):
        (src / "project_cloud.cu").write_text(text)
        assert rb.have_reference()
        with pytest.raises(RuntimeError, match=what):
            rb.cut_kernel_region(str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


# ---------------------------------------------------------------------------------------------------------------------
# reference-made fixtures: these two need neither the reference tree nor oracle/_ref

@pytest.mark.parametrize("case", ref_cases.GOLDEN_CASES, ids=[c[0] for c in ref_cases.GOLDEN_CASES])
def test_golden_reference_projection(orc, pkg, case):
    """oracle.project_variant(mm=2, dv) == the unfiltered frames the reference's contraction-off builds wrote down."""
    g = np.load(os.path.join(GOLDEN, case[0] + ".npz"))
    name, xyzw, rgba, P, W, H = ref_cases.scene_case(orc, pkg, *case[1:])
    assert np.array_equal(P, g["P"]) and (W, H) == (int(g["W"]), int(g["H"]))
    assert [zlib.crc32(xyzw.tobytes()), zlib.crc32(rgba.tobytes())] == g["cloud_crc32"].tolist()  # (the generator's cloud)
    n = written(W, H)
    assert n == int(g["written"])
    for dv, q in ((0, "recip"), (1, "ieee")):
        o = orc.project_variant(xyzw, rgba, P, W, H, 2, dv)
        for k in ("depth_bits", "acc", "img"):
            assert np.array_equal(o[k].reshape(W * H, -1)[:n], g["%s_%s" % (q, k)].reshape(W * H, -1)[:n]), (q, k)
        assert (g["%s_depth_bits" % q].reshape(-1)[:n] != EMPTY).sum() > 1000


@pytest.mark.parametrize("case", ref_cases.GOLDEN_CASES, ids=[c[0] for c in ref_cases.GOLDEN_CASES])
def test_golden_reference_filter(orc, case):
    """npfilter's unfused statement AND the oracle == the reference's recorded filter outputs of the recorded frame."""
    g = np.load(os.path.join(GOLDEN, case[0] + ".npz"))
    W, H = int(g["W"]), int(g["H"])
    r = {"depth": g["f_depth_bits"].view(np.float32), "img": g["f_img"], "mask": g["f_mask"], "tensor": g["f_tensor"],
         "minmax": g["f_minmax"]}
    assert same_filter_outputs(r, npfilter.apply_filter(g["in_depth_bits"], g["in_img"], blend="unfused"), W, H) == []
    assert same_filter_outputs(r, orc.filter(g["in_depth_bits"], g["in_img"]), W, H) == []
    assert (r["mask"] > 0).sum() > 100 and ((r["mask"] == 0) & (g["in_depth_bits"][:r["mask"].shape[0]] != EMPTY)).sum() > 100


