#!/usr/bin/env python3
"""Static instruction counts of a kernel's loops in the gfx950 ISA (the loop tables of profiles/r09_summary.md).

  python tools/isa_loops.py [-DNAME=VALUE ...]

Compiles csrc/<ISA_SRC> (default pt_kernels.hip) for the device only with build.py's flags plus the given
defines, to assembly, and lists every loop (a backward branch to a label) of the kernel whose mangled name
starts with ISA_KERNEL (default: the timed pt_camera_kernel<false, false, false>), nested by containment:
all instructions, VALU, SALU (s_waitcnt and branches included), v_cvt_f32_ubyte (24 mark a compact-node box
test), pk (packed v_pk_ instructions: 12 v_pk_fma_f32 + 2 v_pk_mul_f32 mark a packed box test), LDS, vector-memory loads and scratch accesses between the loop's header and its back edge. Then the
kernel's resource usage (-Rpass-analysis=kernel-resource-usage). The assembly is left in ISA_OUT (default: a
temporary directory) as <ISA_TAG>.s.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from pathtracer_gaussiansplatting_amd import build as B
    defs = sys.argv[1:]
    kern = os.environ.get("ISA_KERNEL", "_ZN4ptgs16pt_camera_kernelILb0ELb0ELb0EE")
    src = os.environ.get("ISA_SRC", "pt_kernels.hip")
    out_dir = os.environ.get("ISA_OUT") or tempfile.mkdtemp(prefix="isa_loops_")
    out = os.path.join(out_dir, os.environ.get("ISA_TAG", "kernel") + ".s")
    cmd = [B._hipcc()] + B.COMMON + defs + B.EXTRA.get(src, []) + [
        f"--offload-arch={B.ARCH}", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
        os.path.join(B.CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-3000:])
    lines = open(out).read().split("\n")
    s = next(i for i, l in enumerate(lines) if l.startswith(kern) and ":" in l)
    e = next(i for i in range(s, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    body = lines[s:e + 1]
    lab = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            lab[m.group(1)] = i
    head = {}
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in lab and lab[m.group(1)] <= i:
            a = lab[m.group(1)]
            head[a] = max(head.get(a, i), i)  # (several back edges to one header: the widest)
    loops = sorted(head.items())

    def is_inst(l):
        t = l.strip()
        return bool(t) and not t.startswith((";", ".", "//")) and not t.endswith(":")

    for a, b in loops:
        ins = [x.strip().split()[0] for x in body[a:b + 1] if is_inst(x)]
        n = lambda *p: sum(1 for x in ins if x.startswith(p))
        depth = sum(1 for c, d in loops if c <= a and d >= b) - 1
        print(f"{'  ' * depth}loop {a}-{b}: all {len(ins)} VALU {n('v_')} SALU {n('s_')} cvt_ubyte {n('v_cvt_f32_ubyte')} "
              f"pk {n('v_pk_')} lds {n('ds_')} vmem_ld {n('global_load', 'buffer_load', 'flat_load')} scratch {n('scratch_')}")
    show = False
    for l in r.stderr.split("\n"):
        if "Function Name:" in l:
            show = kern in l
        if show and "remark:" in l:
            print(l.split("remark: ")[-1].split(" [-R")[0])
    print("assembly:", out)


if __name__ == "__main__":
    main()
