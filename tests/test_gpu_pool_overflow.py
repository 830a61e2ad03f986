"""Every frame consumer the library ships, on frames that overflow the adaptive extent pool (option "pool_worst_case"
= 0, the default; tests/pool_overflow_scenes.py builds the two scenarios).  Each consumer must return the oracle's
frame bit for bit -- depth bits, image, and the fp16 tensor / prefiltered depth where the path produces them -- or fail
loudly; and every test first checks that the pool really overflowed (it grew to the worst case between the calls), so
that none of them passes without testing anything."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import pool_overflow_scenes as sc

pytestmark = pytest.mark.gpu

W, H = sc.W, sc.H
SCENARIOS = ("first", "late")
# the four parity modes (test_gpu_parity.py), the fp32 cloud, the round-4 point kernel, non-lean frames, the second
# tile-store set, and a Morton-sorted cloud
CONFIGS = {
    "tile": {},
    "tile-split": {"split_threshold": 64, "split_slice": 48},
    "tile-packed": {"pack": 2},
    "two-pass": {"mode": 0},
    "pack0": {"pack": 0},
    "chunk_test0": {"chunk_test": 0},
    "lean0": {"lean": 0},
    "overlap": {"overlap": 1},
    "sorted": {},
}


@pytest.fixture(scope="module")
def world(pkg, orc):
    xyzw, rgba = sc.cloud(orc)
    sc.check_poses(pkg, orc, xyzw)
    refs = {}

    def ref(P, filtered):
        key = (P.tobytes(), filtered)
        if key not in refs:
            r = orc.project(xyzw, rgba, P, W, H)
            if filtered:
                f = orc.filter(r["depth_bits"], r["img"])
                r = {"depth_bits": f["depth"].view(np.uint32), "img": f["img"], "tensor": f["tensor"]}
            refs[key] = r
        return refs[key]

    P = sc.p_one(orc)[0]
    r = ref(P, False)
    assert (r["depth_bits"] != orc.EMPTY_DEPTH).sum() <= 9  # (the whole cloud on a handful of pixels)
    return xyzw, rgba, ref


def _projector(pkg, orc, world, scenario, config):
    xyzw, rgba, _ = world
    p = pkg.Projector(0)
    try:
        before = sc.prepare(pkg, orc, p, xyzw, rgba, scenario, CONFIGS[config], sort=config == "sorted")
    except BaseException:
        p.close()
        raise
    return p, before


def _overflowed(p, before, config, what):
    if config != "two-pass":
        sc.assert_overflowed(p, before, what)


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), (what, int((got != want).sum()))


# ---- 1. the synchronising calls ------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("consumer", ["project", "project_filtered", "render_synchronize", "render_download_views"])
def test_synchronising_calls_repair_the_frame(pkg, orc, world, scenario, config, consumer):
    import torch
    L = pkg._lib
    P = sc.p_one(orc)[0]
    ref = world[2]
    what = (scenario, config, consumer)
    p, before = _projector(pkg, orc, world, scenario, config)
    try:
        if consumer == "project":
            img, depth = p.project(P)
            _overflowed(p, before, config, what)
            _same(depth.view(np.uint32), ref(P, False)["depth_bits"], what)
            _same(img, ref(P, False)["img"], what)
        elif consumer == "project_filtered":
            img, depth = p.project(P, filtered=True)
            _overflowed(p, before, config, what)
            rf = ref(P, True)
            _same(depth.view(np.uint32), rf["depth_bits"], what)
            _same(img, rf["img"], what)
            _same(p.download(L.BUF_TENSOR).reshape(5, H, W), rf["tensor"], what)
        elif consumer == "render_synchronize":
            p.render(P, False)
            p.synchronize()
            _overflowed(p, before, config, what)
            _same(p.download(L.BUF_DEPTH), ref(P, False)["depth_bits"], what)
            _same(p.download(L.BUF_IMAGE), ref(P, False)["img"], what)
        else:  # a download repairs the frame; device-buffer views read after it show the same, repaired frame
            p.render(P, True)
            depth = p.download(L.BUF_DEPTH)
            _overflowed(p, before, config, what)
            rf = ref(P, True)
            _same(depth, rf["depth_bits"], what)
            dev = torch.device("cuda", 0)
            view = lambda which, ts=None: torch.as_tensor(p.device_buffer(which, ts), device=dev).cpu().numpy()  # noqa: E731
            torch.cuda.synchronize()
            _same(view(L.BUF_DEPTH, "<i4").view(np.uint32), rf["depth_bits"], what)
            _same(view(L.BUF_IMAGE), rf["img"], what)
            _same(view(L.BUF_TENSOR).view(np.uint16).reshape(5, H, W), rf["tensor"], what)
        sc.no_errors(p)
        # the frame after the repaired one is exact too
        P2 = pkg.orbit_projection(3, W, H)
        img, depth = p.project(P2)
        _same(depth.view(np.uint32), ref(P2, False)["depth_bits"], what + ("next",))
        _same(img, ref(P2, False)["img"], what + ("next",))
    finally:
        p.close()


# ---- 2. computeFull, Python and C++ -------------------------------------------------------------------------------

class _Planes:
    """The stand-in model of test_compute_full_handoff: the three colour planes (half(v / 255) * 255 rounds back to v),
    plus a copy of the tensor it was given."""

    def __init__(self):
        self.seen = []

    def __call__(self, x):
        self.seen.append(x.clone())
        return x[:, 0:3]


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_compute_full_hands_the_model_the_repaired_tensor(pkg, orc, world, scenario):
    xyzw, rgba, ref = world
    P, K, E = sc.p_one(orc)
    rf = ref(P, True)
    cal = pkg.CameraCalibration.pinhole(K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H)
    pc = pkg.ProjectCloud(xyzw, rgba)
    p = pc.projector
    try:
        if scenario == "late":
            ordinary = pkg.benchmark_calibration(W, H)
            for k in sc.ORDINARY:
                img = np.empty((H, W, 3), np.uint8)
                assert pc.computeRGBD(ordinary, pkg.orbit_pose(k), img, None) == 1
        before = sc.footprint(p)
        model = _Planes()
        pc.set_model(model)
        color = np.empty((H, W, 3), np.uint8)
        depth = np.empty((H, W), np.float32)
        assert pc.computeFull(cal, E, color, depth) == 1
        sc.assert_overflowed(p, before, scenario)
        assert len(model.seen) == 1
        _same(model.seen[0].cpu().numpy().view(np.uint16).reshape(5, H, W), rf["tensor"], "tensor the model saw")
        _same(color, rf["img"], "colour")
        _same(depth.view(np.uint32), rf["depth_bits"], "depth")
        sc.no_errors(p)
        color2 = np.empty((H, W, 3), np.uint8)  # again, colour only: the pool has grown, nothing to repair
        assert pc.computeFull(cal, E, color2, None) == 1
        _same(color2, rf["img"], "second call")
    finally:
        p.close()


def _cpp_compute_full_exe(tmp_path, pkg):
    import test_cpp_facade
    return test_cpp_facade._build_compute_full(tmp_path, pkg)


def test_cpp_compute_full_hands_the_model_the_repaired_tensor(tmp_path, pkg, orc, world):
    """tests/cpp/compute_full_check.cpp (RTR_WITH_TORCH) with the 2 M cloud and the P_one camera: its first
    computeFull is the cloud's first frame.  The program writes the footprint after the upload and after that call."""
    import torch
    exe = _cpp_compute_full_exe(tmp_path, pkg)
    xyzw, rgba, ref = world
    P, K, E = sc.p_one(orc)
    with open(tmp_path / "cloud.bin", "wb") as f:
        f.write(np.uint64(len(xyzw)).tobytes())
        f.write(np.ascontiguousarray(xyzw[:, :3]).tobytes())
        f.write(np.ascontiguousarray(rgba[:, :3]).tobytes())
    with open(tmp_path / "cam.bin", "wb") as f:
        f.write(np.ascontiguousarray(K, np.float64).tobytes())
        f.write(np.ascontiguousarray(E, np.float64).tobytes())

    class Planes(torch.nn.Module):
        def forward(self, x):
            return x[:, 0:3]

    (tmp_path / ".render_cache").mkdir()
    torch.jit.script(Planes()).save(str(tmp_path / ".render_cache" / "model.pt"))
    out = str(tmp_path / "out")
    env = dict(os.environ, HOME=str(tmp_path))
    res = subprocess.run([exe, str(tmp_path / "cloud.bin"), str(W), str(H), str(tmp_path / "cam.bin"), "model.pt", out,
                          "footprint"], capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    before, after = np.fromfile(out + ".footprint", np.int32)
    assert after >= sc.WORST_MB and after - before >= sc.JUMP_MB, (before, after)
    rf = ref(P, True)
    rd = lambda ext, dt: np.fromfile(out + ext, dtype=dt)  # noqa: E731
    _same(rd(".rgb", np.uint8), rf["img"].reshape(-1), "colour")
    _same(rd(".depth", np.uint32), rf["depth_bits"].reshape(-1), "depth")
    _same(rd(".tensor", np.uint16), rf["tensor"].reshape(-1), "tensor")


# ---- 3. asynchronous host outputs ---------------------------------------------------------------------------------

@pytest.mark.parametrize("config", ["tile", "overlap", "sorted"])
@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("form", ["one_slot", "two_slots", "wait_all"])
def test_async_slots_hold_their_own_repaired_frames(pkg, orc, world, scenario, config, form):
    """two_slots / wait_all: both slots are queued before the first wait, and both frames overflow (the second one's
    camera sits one pixel to the right).  Whichever wait reads the error word, each slot's buffers must hold the oracle's
    frame of the pose rendered into that slot; slot 1's is the filtered form."""
    ref = world[2]
    poses = [(sc.p_one(orc)[0], False), (sc.p_one(orc, cx=9.0)[0], True)]
    what = (scenario, config, form)
    p, before = _projector(pkg, orc, world, scenario, config)
    try:
        bufs = [p.host_output_buffers(s) for s in range(2)]
        slots = (0,) if form == "one_slot" else (0, 1)
        for s in slots:
            p.project_async(poses[s][0], s, filtered=poses[s][1])
        if form == "wait_all":
            p.wait_outputs(-1)
        else:
            for s in slots:
                p.wait_outputs(s)
        sc.assert_overflowed(p, before, what)
        for s in slots:
            r = ref(*poses[s])
            img, depth = bufs[s]
            _same(depth.view(np.uint32), r["depth_bits"], what + (s,))
            _same(img, r["img"], what + (s,))
        sc.no_errors(p)
        # the device buffers hold the last frame that was queued
        last = poses[slots[-1]]
        _same(p.download(pkg._lib.BUF_DEPTH), ref(*last)["depth_bits"], what + ("device",))
        # and the slots go on working with the grown pool
        P2 = pkg.orbit_projection(3, W, H)
        p.project_async(P2, 0)
        p.wait_outputs(0)
        _same(bufs[0][1].view(np.uint32), ref(P2, False)["depth_bits"], what + ("next",))
        _same(bufs[0][0], ref(P2, False)["img"], what + ("next",))
    finally:
        p.close()


# ---- 4. phase calls and the sharded collective form ---------------------------------------------------------------

@pytest.mark.parametrize("config", ["tile", "tile-split", "tile-packed", "two-pass", "pack0", "chunk_test0", "sorted"])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_phase_calls_are_exact(pkg, orc, world, scenario, config):
    """clear / min_depth_pass / accumulate_pass / resolve / filter, then the downloads.  Nothing can render a phase-call
    frame again, so a binned min_depth_pass sizes the pool for the worst case before the frame (the footprint still
    jumps to the worst case between the calls)."""
    L = pkg._lib
    P = sc.p_one(orc)[0]
    rf = world[2](P, True)
    what = (scenario, config)
    p, before = _projector(pkg, orc, world, scenario, config)
    try:
        p.clear()
        p.min_depth_pass(P)
        p.accumulate_pass(P)
        p.resolve()
        p.filter()
        _same(p.download(L.BUF_DEPTH), rf["depth_bits"], what)
        _overflowed(p, before, config, what)
        _same(p.download(L.BUF_IMAGE), rf["img"], what)
        _same(p.download(L.BUF_TENSOR).reshape(5, H, W), rf["tensor"], what)
        sc.no_errors(p)
    finally:
        p.close()


@pytest.mark.parametrize("colour", ["allreduce", "reduce_scatter"])
def test_sharded_collective_frame_is_exact(colour):
    """ShardedProjector(force_exchange=True) on a 1-rank RCCL group, both scenarios, in a child process (a second
    process group in this one would follow test_gpu_rccl.py's)."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pool_overflow_scenes.py"), "sharded", colour],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0 and ("sharded %s ok" % colour) in res.stdout, res.stdout[-4000:] + res.stderr[-4000:]
