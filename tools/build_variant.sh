#!/bin/bash
# Build a variant of libpvamd for A/B timing or instrumentation.  A variant is one source file -- an edited copy, or the product
# source with a patch from tools/patches/ applied -- plus optional flags; every other object is the product's:
#   tools/build_variant.sh NAME SRC.hip [FLAGS...]     SRC's basename (mesh.hip, composed_x.hip, ...) says which object it replaces
# Unused parameters are errors, as in csrc/Makefile; a source from before that rule (an older commit's file as the `parent` of an
# A/B run) builds with -Wno-error=unused-parameter among FLAGS.
# -> tools/variants/libpvamd_NAME.so ; run a tool against it with PVAMD_LIB=tools/variants/libpvamd_NAME.so
set -e
name=$1; src=$2; shift 2
cd "$(dirname "$0")/.."
make -s -C pytorch_volumetric_amd/csrc
mkdir -p tools/variants
C=pytorch_volumetric_amd/csrc
base=$(basename "$src" .hip); which=""   # the longest object name that is `base` or a prefix of it up to a '_'
for o in $C/*.o; do
  n=$(basename $o .o)
  if { [ "$base" = "$n" ] || [ "${base#${n}_}" != "$base" ]; } && [ ${#n} -gt ${#which} ]; then which=$n; fi
done
[ -n "$which" ] || { echo "$src: no object of csrc/Makefile to replace" >&2; exit 1; }
extra=""; { [ "$which" = composed ] || [ "$which" = mesh ] || [ "$which" = mesh_ray ]; } && extra="-fno-slp-vectorize"   # as csrc/Makefile (FLAGS_*)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-fast-math -ffp-contract=off -Wno-unused-value -Werror=unused-parameter -I$C -Iinclude $extra "-DPVAMD_VARIANT=\"$name: $*\"" "$@" -c "$src" -o tools/variants/${which}_$name.o
objs=""
for o in $C/*.o; do   # every object the Makefile built, except the one being replaced
  [ "$(basename $o .o)" = "$which" ] || objs="$objs $o"
done
objs="$objs tools/variants/${which}_$name.o"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o tools/variants/libpvamd_$name.so $objs
echo tools/variants/libpvamd_$name.so
