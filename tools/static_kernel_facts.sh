#!/bin/bash
# Register / LDS / scratch budget and the instruction mix of the final kernels, from the compiler (no GPU needed):
# writes profiles/r02_static_kernel_facts.md.  usage: tools/static_kernel_facts.sh
#        tools/static_kernel_facts.sh fast   writes profiles/fast_shade_static.txt instead: the fast-math shade kernels (tu_shade_f*.hip) beside their exact twins
set -eu
repo=$(cd "$(dirname "$0")/.." && pwd); work=$(mktemp -d)
F="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -I$repo/include --cuda-device-only"
FAST="-fno-hip-fp32-correctly-rounded-divide-sqrt -Xarch_device -fapprox-func"   # what csrc/Makefile adds for the tu_shade_f*.hip units (FAST_FLAGS) but the generic set's two
if [ "${1:-}" = fast ]; then
  cd $repo/rs_pbrt_amd/csrc
  one() { x=""; case $1 in tu_shade_fc|tu_shade_fmc) ;; tu_shade_f*) x=$FAST;; esac
          /opt/rocm/bin/hipcc $F $x -S $1.hip -o $work/$1.s && /opt/rocm/bin/hipcc $F $x -Rpass-analysis=kernel-resource-usage -c $1.hip -o /dev/null 2> $work/$1.ru; }
  export -f one; export F FAST work
  printf '%s\n' tu_shade_a tu_shade_b tu_shade_c tu_shade_h tu_shade_ma tu_shade_mb tu_shade_mc tu_shade_mh \
                tu_shade_fa tu_shade_fb tu_shade_fc tu_shade_fh tu_shade_fma tu_shade_fmb tu_shade_fmc tu_shade_fmh | xargs -P "${JOBS:-8}" -I{} bash -c 'one {}'
  cat $work/tu_shade_*.s > $work/shade.s; cat $work/tu_shade_*.ru > $work/ru.txt
  python3 $repo/tools/fast_shade_static.py $work $repo
  rm -rf $work
  exit 0
fi
# every translation unit of the library (rs_pbrt_amd/csrc/Makefile: librspt.hip + the tu_*.hip instantiation groups)
: > $work/final.s; : > $work/ru.txt
for tu in $repo/rs_pbrt_amd/csrc/*.hip; do
  x=""; case $tu in */tu_shade_fc.hip|*/tu_shade_fmc.hip) ;; */tu_shade_f*) x=$FAST;; esac
  /opt/rocm/bin/hipcc $F $x -S $tu -o $work/one.s && cat $work/one.s >> $work/final.s
  /opt/rocm/bin/hipcc $F $x -Rpass-analysis=kernel-resource-usage -c $tu -o $work/x.o 2>> $work/ru.txt
done
python3 $repo/tools/static_kernel_facts.py $work $repo
rm -rf $work
