#!/bin/bash
# Where a tile of the RTS smoother step spends its time (smoother): builds pb_smooth.hip and pb_smooth_wide.hip as
# shipped (`full`) and with the tile timeline (`timeline`: -DSML_TIMELINE=<tile>, shader-clock stamps of one tile's role waves
# behind the barriers, printed to stderr; rbis_smooth_lane.hpp, rbis_smooth_wide.hpp), links each variant against the other
# objects of the library and runs scripts/smooth_rate.py with it (PRONTO_BATCH_LIB).  The variants that compiled parts of the
# kernels out are gone with their flags; what they measured is in profiles/EXPERIMENTS.md and profiles/r0N_smoother_*.txt.
#   on the build host:  bash scripts/smooth_attribution.sh build
#   on the GPU box:     bash scripts/smooth_attribution.sh run > smooth_attribution.txt
set -u
cd "$(dirname "$0")/.."
V="full: timeline:-DSML_TIMELINE=0"
V=${SM_VARIANTS:-$V}   # e.g. SM_VARIANTS="timeline:-DSML_TIMELINE=255" (a tile of the last dispatch round)
D=gpurun_scratch/smooth_attr
if [ "${1:-}" = build ]; then
  mkdir -p $D
  # the library's other objects: the Makefile's own list (print-objs) without the two smoother objects
  OTHERS=$(make -s -C pronto_amd/csrc print-objs | tr ' ' '\n' | grep -v '/pb_smooth\(_wide\)\?\.o$' | sed 's|^\.\./lib/obj/|pronto_amd/lib/obj/|' | tr '\n' ' ')
  [ -n "$OTHERS" ] || { echo "no object list from the Makefile (make print-objs)" >&2; exit 1; }
  for v in $V; do
    n=${v%%:*}; fl=$(echo ${v#*:} | tr ',' ' ')
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -DPB_EXPERIMENTS -Ipronto_amd/csrc $fl -c -o $D/pb_smooth_$n.o pronto_amd/csrc/pb_smooth.hip || exit 1
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -DPB_EXPERIMENTS -mllvm -disable-machine-licm -Ipronto_amd/csrc $fl -c -o $D/pb_smooth_wide_$n.o pronto_amd/csrc/pb_smooth_wide.hip || exit 1
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared -o $D/lib_$n.so $OTHERS $D/pb_smooth_$n.o $D/pb_smooth_wide_$n.o || exit 1
    rm -f $D/pb_smooth_$n.o $D/pb_smooth_wide_$n.o
  done
  ls $D
  exit 0
fi
for v in $V; do
  n=${v%%:*}
  echo "== build: $n (${v#*:})"
  PRONTO_BATCH_LIB=$PWD/$D/lib_$n.so python3 scripts/smooth_rate.py 2>&1 | grep 'smoother\|timeline'
done
