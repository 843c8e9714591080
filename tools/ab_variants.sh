#!/bin/bash
# Twin builds of the rasterizer library with other values of its -D tunables (DGS_BWD_CHUNK, DGS_BWD_MINWAVES, DGS_FWD_MINWAVES,
# DGS_BIG_RECT), timed back to back on ONE lease (tools/quick_timing.py through DGS_SURFEL_LIB).
#   where hipcc is:    tools/ab_variants.sh build  name1:-DDGS_BWD_CHUNK=64 name2:"-DDGS_BWD_CHUNK=32 -DDGS_BWD_MINWAVES=6" ...
#                      (one library per name, ab_<name>.so next to the product library; earlier ab_*.so there are removed first)
#   on the GPU box:    tools/ab_variants.sh run [quick_timing args]      (tools/ab_check.sh: the parity file first, then the timing)
R=$(cd "$(dirname "$0")/.." && pwd)
D=$R/dynamic-2dgs_amd/csrc
if [ "$1" = build ]; then
  shift
  rm -f $D/ab_*.so
  for v in "$@"; do
    name=${v%%:*}; flags=${v#*:}
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -munsafe-fp-atomics -fno-slp-vectorize $flags $D/surfel_rasterizer.hip -o $D/ab_$name.so 2>&1 | grep -v warning | grep -v "^$" &
  done
  wait
  ls $D/ab_*.so
else
  shift
  for so in $D/ab_*.so; do
    printf "%-28s " $(basename $so .so)
    DGS_SURFEL_LIB=$so python $R/tools/quick_timing.py "$@" 2>&1 | tail -2 | tr '\n' ' '
    echo
  done
fi
