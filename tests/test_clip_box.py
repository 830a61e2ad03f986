"""The clip planes' chunk-level rejection (csrc/rtr_chunk_box.h, clip_box_outside): a host build of the helper fuzzed
against the exact point test clip_keep -- no box it rejects may hold a corner or a sampled point the fp32 test keeps,
at huge and tiny magnitudes and on the boxes of packed chunk headers (tests/cpp/clip_box_check.cpp).  CPU only."""
import os
import subprocess

from conftest import ROOT


def test_clip_box_never_rejects_a_kept_point(tmp_path):
    exe = str(tmp_path / "clip_box_check")
    csrc = os.path.join(ROOT, "real-time-neural-rendering-of-lidar-point-clouds_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "clip_box_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True).split()
    assert out[0] == "ok", out
    boxes, rejected, points = (int(v) for v in out[1:4])
    assert boxes > 200000 and rejected > 20000 and points == rejected * 32
