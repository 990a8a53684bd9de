#!/usr/bin/env python3
"""What the HIP runtime says of pt_camera_kernel's occupancy, per library variant: launches nothing.

  python tools/pt_occupancy.py base s30 ...     (variant "base" = libptgs.so, else libptgs_<variant>.so)

For each variant and each of the four untimed-statistics instantiations (plain, DEEP, TEX, TEX + DEEP) it asks
hipOccupancyMaxActiveBlocksPerMultiprocessor for the one-wave workgroup (ptgs_debug_pt_occupancy, pt_kernels.hip)
and prints the workgroups per CU the runtime would keep resident, the waves per SIMD that makes (4 SIMDs per CU),
the static LDS bytes, VGPRs and private bytes per lane, and the instantiation's LDS stack entries and launch bound. It
is the runtime's view of how the LDS is shared, e.g. build.build(defines=("PTGS_PT_STACK=32",), variant="s32")
beside the default 30. It answered 20 workgroups per CU for 8 192 B as for 7 680 B; the timings (tools/ab_pt.py,
profiles/r12_summary.md) did not bear the first out, so time a depth before trusting this number for it.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "plain", 1: "DEEP", 2: "TEX", 3: "TEX+DEEP"}


def main():
    for v in sys.argv[1:] or ["base"]:
        path = os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "libptgs.so" if v == "base" else f"libptgs_{v}.so")
        lib = C.CDLL(path)
        lib.ptgs_debug_pt_occupancy.restype = C.c_int
        lib.ptgs_debug_pt_occupancy.argtypes = [C.c_uint, C.POINTER(C.c_uint)]
        for inst, name in NAMES.items():
            out = (C.c_uint * 7)()
            rc = lib.ptgs_debug_pt_occupancy(inst, out)
            if rc:
                sys.exit(f"{v} {name}: hip error {rc}")
            blocks, lds, vgpr, priv, stack, minw, wg = list(out)
            print(f"{v:8s} {name:9s} LDS stack {stack}, launch bound {minw} waves per SIMD: {blocks} workgroups of {wg} per CU = "
                  f"{blocks * wg / 64 / 4:.2f} waves per SIMD; LDS {lds} B, {vgpr} VGPRs, {priv} B private per lane",
                  flush=True)


if __name__ == "__main__":
    main()
