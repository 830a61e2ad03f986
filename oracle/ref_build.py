"""Builds oracle/_ref/: the reference's own kernels compiled for the HOST (test infrastructure only).

    python oracle/ref_build.py [--force]          reference tree: $RTR_REFERENCE_DIR, default /root/reference

What is compiled is the reference's program text, unchanged:
  src/RTRenderer/src/render.cu            as it is
  src/RTRenderer/src/project_cloud.cu     its KERNEL REGION only -- from the line `#define THREADS_PER_BLOCK` up to the
                                          line that opens `ProjectCloud::ProjectCloud(`: constants, the five filter
                                          kernels and getPixelValue.  The rest of the file is host code bound to the
                                          CUDA runtime, OpenCV and torch; ref_host/ref_driver.cpp restates its launch
                                          sequence only.  The region is cut by these markers into
                                          oracle/_ref/project_cloud_kernels.cu at build time (and the five kernel
                                          signatures into project_cloud_kernels.h, which is how the driver declares
                                          them: none of the reference's text is kept in this repository); a reference whose text
                                          does not have them, or not these six functions between them, fails the build.
with ref_host/cuda_shim.h force-included, the glm stubs of ref_host/glm/ and c10/util/Half.h from the installed torch.
Nothing cut or compiled from the reference is committed: oracle/_ref/ is in .gitignore.

Four shared libraries, oracle/_ref/libref_<contraction>_<quotient>.so -- the two things a host build cannot decide:
  contraction   off   -ffp-contract=off -fno-fast-math      every fp32 operation rounded on its own
                fast  -ffp-contract=fast -mfma              the host compiler's own choice of fused multiply-adds
  quotient      recip __fdividef(x, z) = x * RN(1 / z)      ieee  __fdividef(x, z) = x / z
all -O2 otherwise.  `check_program()` builds the driver's stand-alone main (for the sanitizers).
"""
import importlib.util
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "ref_host")
OUT = os.path.join(HERE, "_ref")
CONTRACTION = {"off": ["-ffp-contract=off", "-fno-fast-math"], "fast": ["-ffp-contract=fast", "-mfma"]}
QUOTIENT = {"recip": [], "ieee": ["-DREF_FDIVIDEF_IEEE"]}
VARIANTS = ["%s_%s" % (c, q) for c in CONTRACTION for q in QUOTIENT]
CUT_NAME = "project_cloud_kernels.cu"
DECL_NAME = "project_cloud_kernels.h"
CUT_BEGIN = "#define THREADS_PER_BLOCK"
CUT_END = "ProjectCloud::ProjectCloud("
CUT_MUST_HOLD = ["void reduce(", "void laplacianKernel(", "float getPixelValue(", "void compareImgsKernel(",
                 "void resizeKernel(", "void removeMask(", "filterStrength", "gradientFilter", "laplaceKernel"]
CUT_MUST_NOT_HOLD = ["cudaMalloc", "cudaMemcpy", "<<<", "torch::", "cv::"]


def reference_dir():
    return os.environ.get("RTR_REFERENCE_DIR", "/root/reference")


def _ref_path(*parts):
    return os.path.join(reference_dir(), "src", "RTRenderer", *parts)


def have_reference():
    return os.path.isfile(_ref_path("src", "render.cu")) and os.path.isfile(_ref_path("src", "project_cloud.cu"))


def lib_path(variant):
    return os.path.join(OUT, "libref_%s.so" % variant)


def built():
    return all(os.path.isfile(lib_path(v)) for v in VARIANTS)


def torch_include():
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        raise RuntimeError("ref_build: torch (for c10/util/Half.h) is not installed")
    inc = os.path.join(list(spec.submodule_search_locations)[0], "include")
    if not os.path.isfile(os.path.join(inc, "c10", "util", "Half.h")):
        raise RuntimeError("ref_build: %s has no c10/util/Half.h" % inc)
    return inc


def cut_kernel_region(out_dir=OUT):
    """Writes the kernel region of project_cloud.cu, byte for byte, to <out_dir>/project_cloud_kernels.cu."""
    lines = open(_ref_path("src", "project_cloud.cu"), encoding="utf-8").read().splitlines(keepends=True)
    begin = [i for i, ln in enumerate(lines) if ln.startswith(CUT_BEGIN)]
    end = [i for i, ln in enumerate(lines) if ln.startswith(CUT_END)]
    if len(begin) != 1 or len(end) != 1 or not begin[0] < end[0]:
        raise RuntimeError("ref_build: project_cloud.cu does not have the markers %r ... %r exactly once, in this order "
                           "(found at lines %s and %s)" % (CUT_BEGIN, CUT_END, begin, end))
    text = "".join(lines[begin[0]:end[0]])
    missing = [s for s in CUT_MUST_HOLD if s not in text]
    stray = [s for s in CUT_MUST_NOT_HOLD if s in text]
    if missing or stray or text.count("__global__") != 5 or text.count("__device__") != 1:
        raise RuntimeError("ref_build: the region cut from project_cloud.cu is not the five filter kernels and getPixelValue "
                           "(missing %s, host code %s, %d kernels)" % (missing, stray, text.count("__global__")))
    protos = re.findall(r"__global__\s+void\s+\w+\s*\([^)]*\)", text)
    if len(protos) != 5:
        raise RuntimeError("ref_build: expected five kernel signatures in the cut region, found %d" % len(protos))
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, CUT_NAME)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write(text)
    with open(os.path.join(out_dir, DECL_NAME), "w", encoding="utf-8") as fh:  # the driver's declarations of the five kernels
        fh.write("#pragma once\n" + "".join(p + ";\n" for p in protos))
    return path


def _sources():
    own = [os.path.join(dp, f) for dp, _, fs in os.walk(HOST) for f in fs] + [os.path.abspath(__file__)]
    return own + [_ref_path("src", "render.cu"), _ref_path("src", "project_cloud.cu"), _ref_path("include", "render.cuh"),
                  _ref_path("include", "types.h")]


def _compile(flags, out, cut, extra=()):
    """One g++ call over the three translation units; -x c++ because two of them are named .cu."""
    base = ["g++", "-std=gnu++17", "-O2"] + list(flags) + ["-I", HOST, "-I", os.path.dirname(cut), "-I", _ref_path("include"), "-I", torch_include(),
                                                            "-include", os.path.join(HOST, "cuda_shim.h")]
    cmd = base + list(extra) + ["-x", "c++", _ref_path("src", "render.cu"),
                                "-include", os.path.join(HOST, "filter_prelude.h"), cut,
                                os.path.join(HOST, "ref_driver.cpp"), "-o", out]
    subprocess.check_call(cmd)


def build(force=False, verbose=False):
    """Builds the four libraries when the reference is there (and they are missing or older than a source).
    Without the reference an existing oracle/_ref is left alone.  -> True when all four libraries exist."""
    if not have_reference():
        return built()
    newest = max(os.path.getmtime(p) for p in _sources())
    if not force and built() and all(os.path.getmtime(lib_path(v)) >= newest for v in VARIANTS):
        return True
    cut = cut_kernel_region()
    for c, cflags in CONTRACTION.items():
        for q, qflags in QUOTIENT.items():
            out = lib_path("%s_%s" % (c, q))
            tmp = out + ".tmp%d" % os.getpid()
            _compile(cflags + qflags, tmp, cut, extra=["-fPIC", "-shared", "-Wl,-Bsymbolic"])
            os.replace(tmp, out)
            if verbose:
                print("ref_build:", os.path.relpath(out, HERE))
    return True


def check_program(out, sanitize, contraction="off", quotient="recip", out_dir=None):
    """The driver's stand-alone main (REF_HOST_MAIN) as a program of its own, optionally under the sanitizers."""
    cut = cut_kernel_region(out_dir or os.path.dirname(out))
    flags = CONTRACTION[contraction] + QUOTIENT[quotient] + ["-DREF_HOST_MAIN"]
    if sanitize:
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    _compile(flags, out, cut)
    return out


if __name__ == "__main__":
    if not have_reference():
        sys.exit("ref_build: no reference under %s (set RTR_REFERENCE_DIR)" % reference_dir())
    build(force="--force" in sys.argv[1:], verbose=True)
