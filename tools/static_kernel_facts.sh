#!/bin/bash
# Register / LDS / scratch budget and the instruction mix of the final kernels, from the compiler (no GPU needed):
# writes profiles/r02_static_kernel_facts.md.  usage: tools/static_kernel_facts.sh
#        tools/static_kernel_facts.sh fast   writes profiles/fast_shade_static.txt instead: the fast-math shade kernels (groups SHADE_F*) beside their exact twins
# The device assembly and the resource-usage remarks of a unit come from csrc/Makefile ($OBJDIR/<unit>.s, .ru), which alone knows each unit's flags.
set -eu
repo=$(cd "$(dirname "$0")/.." && pwd); work=$(mktemp -d); csrc=$repo/rs_pbrt_amd/csrc
if [ "${1:-}" = fast ]; then
  units=$(for g in A B C H MA MB MC MH FA FB FC FH FMA FMB FMC FMH; do echo tu_SHADE_$g; done)
  make -s -j"${JOBS:-8}" -C $csrc OBJDIR=$work $(for u in $units; do echo $work/$u.s $work/$u.ru; done)
  cat $work/tu_SHADE_*.s > $work/shade.s; cat $work/tu_SHADE_*.ru > $work/ru.txt
  python3 $repo/tools/fast_shade_static.py $work $repo
  rm -rf $work
  exit 0
fi
# every translation unit of the library (librspt.hip + tu.hip once per instantiation group)
make -s -j"${JOBS:-8}" -C $csrc OBJDIR=$work unit-asm unit-remarks
cat $work/*.s > $work/final.s; cat $work/*.ru > $work/ru.txt
python3 $repo/tools/static_kernel_facts.py $work $repo
rm -rf $work
