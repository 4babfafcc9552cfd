#!/usr/bin/env python3
"""Prints VGPR / SGPR / scratch / LDS / occupancy of every gfx950 kernel (hipcc -Rpass-analysis), compiled with the product's
flags and from the product's kernel sources (csrc/build.py: FLAGS, FILE_FLAGS, the k_* entries of SOURCES).

--isa DIR also writes every kernel's instruction stream (hipcc -S --cuda-device-only, same flags) to DIR/<demangled name>.txt:
instructions and labels only, comments and assembler directives stripped, so that `diff -r` of the dumps of two trees shows
exactly the kernels whose code a change touched.  --profiling adds -DGS_PROFILING (dump it into a directory of its own).
Usage: tools/kernel_resources.py [--isa DIR] [--profiling] [k_file.hip ...]"""
import argparse, os, re, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gaussian-splatting-wgpu_amd", "csrc"))
import build as B


def demangle(sym):
    return subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip().split("(")[0]


def dump_isa(asm, outdir):
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    cur = None
    for line in asm.splitlines():
        line = line.split(";")[0].rstrip()
        m = re.match(r"^([A-Za-z_$][\w$.]*):$", line)
        if m and m.group(1) in kernels:
            name = demangle(m.group(1)).replace("void ", "").replace(" ", "")
            cur = open(os.path.join(outdir, name + ".txt"), "w")
        elif cur and line.startswith(".Lfunc_end"):
            cur.close()
            cur = None
        elif cur and line.strip() and (not line.lstrip().startswith(".") or line.endswith(":")):
            # block labels carry the function's index in the file (.LBB<k>_<n>): not part of the kernel's code
            cur.write(re.sub(r"\.LBB\d+_", ".LBB_", line.strip() if line.endswith(":") else "\t" + " ".join(line.split())) + "\n")


ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--isa", metavar="DIR", help="write one instruction-stream file per kernel under DIR")
ap.add_argument("--profiling", action="store_true", help="compile with -DGS_PROFILING")
ap.add_argument("sources", nargs="*", help="kernel files (default: every k_* of the product)")
args = ap.parse_args()
if args.isa:
    os.makedirs(args.isa, exist_ok=True)
for src in args.sources or [s for s in B.SOURCES if s.startswith("k_")]:
    cmd = [B.HIPCC] + B.FLAGS + B.FILE_FLAGS.get(src, []) + (["-DGS_PROFILING"] if args.profiling else []) + [os.path.join(B.HERE, src)]
    out = subprocess.run(cmd + ["-c", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True).stderr
    cur = None
    for line in out.splitlines():
        m = re.search(r"remark: .*?(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "Function Name":
            if cur: print(cur)
            cur = "%-46s" % demangle(v)
        else:
            cur += " %s=%s" % (k.split(" ")[0], v)
    if cur: print(cur)
    if args.isa:
        dump_isa(subprocess.run(cmd + ["-S", "--cuda-device-only", "-o", "-"], capture_output=True, text=True, check=True).stdout, args.isa)
