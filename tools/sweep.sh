#!/bin/bash
# usage: tools/sweep.sh "<bench args>" v1 v2 ...   -> runs bench.py with --blend-ablation v for each v
# (most ablation bits act only in the PROFILING build: python gaussian-splatting-wgpu_amd/csrc/build.py --profiling; used here when present)
PROF=$(dirname "$0")/../gaussian-splatting-wgpu_amd/lib/libgsplat_hip_prof.so
[ -f "$PROF" ] && export GSPLAT_LIB=$(cd "$(dirname "$PROF")" && pwd)/libgsplat_hip_prof.so
ARGS=$1; shift
J=$(mktemp)
for v in "$@"; do
  timeout -k 10 200 python bench.py --full --steps 60 --warmup 10 --no-cpu $ARGS --blend-ablation $v > "$J" 2>/dev/null || exit 1
  python - "$v" "$J" <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
print(sys.argv[1], round(d["value"], 1), {k: v["us"] for k, v in d["stages"].items()})
PY
done
rm -f "$J"
