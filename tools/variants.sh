#!/bin/bash
# Build libbwrt.so variants for A/B timing: tools/variants.sh name "EXTRA FLAGS" ...
# -> bwidman-raytracer_amd/build/variants/<name>/libbwrt.so (what tools/ab.sh loads), built by
# the Makefile's own rules in a tree of its own (OUT=build/variants/<name>) with
# the extra flags after the tuning defines.  TUNE / BVHFLAGS override the Makefile's.
set -e
cd "$(dirname "$0")/../bwidman-raytracer_amd"
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  out=build/variants/$name
  make -j"${JOBS:-8}" OUT=$out TUNE="${TUNE:--DRT_WAVES_PER_EU=6 -DRT_SORTED_BLOCK=256} $flags" EXTRA="$flags" ${BVHFLAGS:+BVHFLAGS="$BVHFLAGS"} lib
  ln -sf lib/libbwrt.so $out/libbwrt.so
  make OUT=$out TUNE="${TUNE:--DRT_WAVES_PER_EU=6 -DRT_SORTED_BLOCK=256} $flags" $out/build/rt_kernels-gfx950.s > /dev/null
  grep -A8 "rt_render_kernelILi256ELb1ELb0" $out/build/resource-usage.txt | grep -oE " (VGPRs|TotalSGPRs|ScratchSize[^:]*|Occupancy[^:]*): [0-9]+" | tr -d '\n' | sed "s/^/$name:/; s/$/\n/" || true
done
