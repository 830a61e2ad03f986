"""The two per-frame counters that wrap in a long-lived context, the part a CPU can check: the tile store's 24-bit frame
stamp (csrc/rtr_stamp_rule.h: next stamp, whether the directory must be cleared first, how many bytes) and the wait
condition of the peer-to-peer flag barrier (csrc/rtr_barrier_rule.h), each built with g++ and walked through its wrap
(tests/cpp/stamp_rule_check.cpp, tests/cpp/barrier_rule_check.cpp).  The barrier check is also built with the
comparison the kernels used before (`flag < seq`, -DBARRIER_RULE_OLD) and must then fail: that is where the old rule's
defect is demonstrated -- on the host, never on a GPU."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "real-time-neural-rendering-of-lidar-point-clouds_amd", "csrc")


def _build(tmp_path, name, *defines):
    exe = str(tmp_path / (name + "".join(defines).replace("-D", "_")))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, *defines,
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    return exe


def test_stamp_rule_through_the_wrap(tmp_path):
    out = subprocess.check_output([_build(tmp_path, "stamp_rule_check")], text=True).split()
    assert out[0] == "ok", out
    assert int(out[1]) >= 8 * (2 << 24)  # every step of eight walks of two full rounds was checked


def test_barrier_rule_across_the_wrap(tmp_path):
    out = subprocess.check_output([_build(tmp_path, "barrier_rule_check")], text=True).split()
    assert out[0] == "ok", out
    assert int(out[1]) >= 10_000


def test_barrier_check_fails_with_the_old_comparison(tmp_path):
    """`flag < seq` waits for nobody once seq has wrapped: the same program, built with it, must say so."""
    res = subprocess.run([_build(tmp_path, "barrier_rule_check", "-DBARRIER_RULE_OLD")], capture_output=True, text=True)
    assert res.returncode == 1 and res.stdout.startswith("FAIL"), (res.returncode, res.stdout)


def test_rule_headers_are_host_only_and_in_use():
    """The headers must stay free of HIP so that the checks above keep compiling them -- and the library must go on
    calling them: next_seq() the stamp rule, both barrier kernels the one wait condition."""
    for name in ("rtr_stamp_rule.h", "rtr_barrier_rule.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text, name
    api = open(os.path.join(CSRC, "rtr_api.hip")).read()
    body = api[api.index("int next_seq("):]
    body = body[:body.index("\n}\n")]
    assert "next_stamp(" in body and "dir_bytes(" in body and "hipMemsetAsync(" in body and "0xFFFFFF" not in body, body
    kern = open(os.path.join(CSRC, "rtr_kernels.hip")).read()
    for k in ("k_p2p_sync", "k_p2p_sync_gather"):
        src = kern[kern.index("__global__ void %s(" % k):]
        src = src[:src.index("\n}\n")]
        assert "barrier_not_arrived(" in src and "< seq" not in src, k
