#!/usr/bin/env python3
"""Prints VGPR / SGPR / scratch / LDS / occupancy of every gfx950 kernel (hipcc -Rpass-analysis), compiled with the product's
flags and from the product's kernel sources (csrc/build.py: FLAGS, FILE_FLAGS, the k_* entries of SOURCES)."""
import os, re, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "gaussian-splatting-wgpu_amd", "csrc"))
import build as B
for src in (s for s in B.SOURCES if s.startswith("k_")):
    out = subprocess.run([B.HIPCC] + B.FLAGS + B.FILE_FLAGS.get(src, []) + ["-c", os.path.join(B.HERE, src), "-o", "/dev/null",
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True).stderr
    cur = None
    for line in out.splitlines():
        m = re.search(r"remark: .*?(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "Function Name":
            if cur: print(cur)
            name = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip().split("(")[0]
            cur = "%-46s" % name[:46]
        else:
            cur += " %s=%s" % (k.split(" ")[0], v)
    if cur: print(cur)
