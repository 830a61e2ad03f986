"""bench.py --dump-outputs: the frame of the last timed step as float32 .npy files.
CPU: the writer against a stand-in projector (full frames, the seeded pixel sample above 64 MB).
GPU: a small bench run, its dump against the oracle's frame of the last timed pose, and --steps
as the number of timed frames."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench_module():
    spec = importlib.util.spec_from_file_location("rtr_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # (defines functions only; main() runs under __main__)
    return mod


class _FakeProjector:
    """Frame buffers with the dtypes and shapes Projector.download returns, filled from a seed."""

    def __init__(self, pkg, W, H, seed):
        self.W, self.H, self.pkg = W, H, pkg
        rng = np.random.default_rng(seed)
        self.depth = rng.uniform(0.5, 9.0, (H, W)).astype(np.float32)
        self.depth[rng.random((H, W)) < 0.1] = -1.0
        self.img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        self.tensor = rng.uniform(-1.0, 1.0, (1, 5, H, W)).astype(np.float16)

    def download(self, which):
        L = self.pkg._lib
        return {L.BUF_DEPTH: self.depth.view(np.uint32), L.BUF_IMAGE: self.img,
                L.BUF_TENSOR: self.tensor.view(np.uint16)}[which].copy()


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


@pytest.mark.parametrize("with_filter", [True, False], ids=["filtered", "plain"])
def test_dump_small_frame_is_whole_and_exact(pkg, tmp_path, with_filter):
    b = _bench_module()
    fp = _FakeProjector(pkg, 320, 240, 1)
    b.dump_outputs(str(tmp_path), pkg, fp, with_filter)
    out = _load_dir(str(tmp_path))
    assert sorted(out) == (["depth", "image", "tensor"] if with_filter else ["depth", "image"])
    assert all(a.dtype == np.float32 for a in out.values())
    assert np.array_equal(out["depth"].view(np.uint32), fp.depth.view(np.uint32))
    assert np.array_equal(out["image"], fp.img.astype(np.float32))
    if with_filter:
        assert np.array_equal(out["tensor"], fp.tensor[0].astype(np.float32))


def test_dump_large_frame_is_a_fixed_sample_under_64mb(pkg, tmp_path):
    b = _bench_module()
    W, H = 1920, 1080
    fp = _FakeProjector(pkg, W, H, 2)
    a, c = tmp_path / "a", tmp_path / "b"
    b.dump_outputs(str(a), pkg, fp, True)
    b.dump_outputs(str(c), pkg, _FakeProjector(pkg, W, H, 3), True)
    assert _size(str(a)) <= 64_000_000
    out, other = _load_dir(str(a)), _load_dir(str(c))
    assert sorted(out) == ["depth", "image", "pixel_index", "tensor"]
    assert out["pixel_index"].dtype == np.float64 and all(out[k].dtype == np.float32 for k in ("depth", "image", "tensor"))
    assert np.array_equal(out["pixel_index"], other["pixel_index"])  # the same pixels whatever the frame
    idx = out["pixel_index"].astype(np.int64)
    k = len(idx)
    assert k > W * H // 2 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < W * H
    assert np.array_equal(out["depth"].view(np.uint32), fp.depth.view(np.uint32).reshape(-1)[idx])
    assert np.array_equal(out["image"], fp.img.reshape(-1, 3)[idx].astype(np.float32))
    assert np.array_equal(out["tensor"], fp.tensor.reshape(5, -1)[:, idx].astype(np.float32))
    assert out["tensor"].shape == (5, k)


def test_dump_refuses_multi_gpu_runs(tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert res.returncode != 0 and "--dump-outputs" in res.stderr
    assert not os.listdir(tmp_path)


@pytest.mark.gpu
def test_bench_dump_is_the_last_timed_frame(pkg, orc, tmp_path):
    n, W, H, steps, warmup = 300_000, 320, 240, 3, 2
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--points", str(n), "--width", str(W),
           "--height", str(H), "--steps", str(steps), "--warmup", str(warmup), "--time-every", "1", "--no-extra",
           "--no-cpu-baseline", "--no-parity", "--dump-outputs", str(tmp_path / "dump")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == steps and out["roofline"]["launches_timed"] == steps  # one point-kernel launch per step
    xyzw, rgba = orc.generate("room_shell", 0xC0FFEE03, 0, n, n)  # bench.py's SEEDS["C3"]
    ref = orc.project(xyzw, rgba, pkg.orbit_projection(warmup + steps - 1, W, H), W, H)
    f = orc.filter(ref["depth_bits"], ref["img"])
    d = _load_dir(str(tmp_path / "dump"))
    assert sorted(d) == ["depth", "image", "tensor"]
    assert np.array_equal(d["depth"].view(np.uint32), f["depth"].view(np.uint32))
    assert np.array_equal(d["image"], f["img"].astype(np.float32))
    assert np.array_equal(d["tensor"], f["tensor"].view(np.float16).reshape(5, H, W).astype(np.float32))
