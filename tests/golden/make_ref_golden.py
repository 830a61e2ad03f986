#!/usr/bin/env python3
"""Writes tests/golden/ref_*.npz: outputs of THE REFERENCE'S OWN KERNELS (oracle/_ref, the contraction-off host builds
of oracle/ref_build.py), so that a checkout without the reference tree still has reference-made fixtures -- every other
file in this directory was made by the oracle.  Inputs and recorded results only; needs the reference tree (or a built
oracle/_ref):  python tests/golden/make_ref_golden.py

Per case (tests/ref_cases.py GOLDEN_CASES; the cloud is the oracle generator's, recorded by its crc32):
  P, W, H, written            the matrix, the frame size, how many pixels (linear order) the reference's grids write
  recip_* / ieee_*            depth_bits, acc, img of ref_project under __fdividef = x * RN(1/z) and IEEE x / z;
                              pixels the reference never writes hold the poison byte 0xA5
  in_depth_bits, in_img       a given unfiltered frame (the oracle's contract frame of the same cloud)
  f_*                         ref_filter's outputs of that frame: depth bits, image, level-0 mask [H_eff, W], min/max,
                              fp16 tensor in the reference's layout [5, H_eff, W]"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import __graft_entry__ as entry  # noqa: E402
import ref_cases  # noqa: E402


def main():
    orc, pkg = entry.load_oracle(), entry.load_package()
    for case in ref_cases.GOLDEN_CASES:
        name, xyzw, rgba, P, W, H = ref_cases.scene_case(orc, pkg, *case[1:])
        out = {"P": P, "W": W, "H": H, "written": (W // 16) * (H // 16) * 256,
               "cloud_crc32": np.array([zlib.crc32(xyzw.tobytes()), zlib.crc32(rgba.tobytes())], np.uint64)}
        for q in ("recip", "ieee"):
            r = orc.ref("off_" + q).project(xyzw, rgba, P, W, H)
            for k in ("depth_bits", "acc", "img"):
                out["%s_%s" % (q, k)] = r[k]
        u = orc.project(xyzw, rgba, P, W, H)
        f = orc.ref("off_recip").filter(u["depth_bits"], u["img"])
        out.update(in_depth_bits=u["depth_bits"], in_img=u["img"], f_depth_bits=f["depth"].view(np.uint32), f_img=f["img"],
                   f_mask=f["mask"], f_minmax=f["minmax"], f_tensor=f["tensor"])
        path = os.path.join(HERE, case[0] + ".npz")
        np.savez_compressed(path, **out)
        print(case[0], "%d bytes" % os.path.getsize(path), "filled", int((u["depth_bits"] != orc.EMPTY_DEPTH).sum()),
              "kept", int((f["mask"] > 0).sum()))


if __name__ == "__main__":
    main()
