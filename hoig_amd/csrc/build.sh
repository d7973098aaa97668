#!/bin/bash
# Builds libhoig_hip.so (gfx950 code objects) in-tree: hoig_amd/csrc/_build/libhoig_hip.so
#
# Sources are found, not listed: every *.hip of this directory (kernels and their launchers) and every *_host.cpp (the host halves:
# sizes, tables and CPU twins with no HIP call -- plain C++ through the same compiler driver, so that each also builds on its own
# under a host sanitizer).  Dependencies come from the compiler (-M): an object is rebuilt when it or its .d is missing, or when a
# file its .d names, or this script, is newer.  The library links the objects of the sources found and nothing else.
set -e
cd "$(dirname "$0")"
mkdir -p _build
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SELF=$(basename "$0")
JOBS=$(nproc); [ "$JOBS" -gt 16 ] && JOBS=16
HIP_FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -I../../include -I. -Wno-unused-result -Wno-c++20-designator"
HOST_FLAGS="-x c++ -O3 -std=c++17 -fPIC"
# The per-file exceptions.  -ffp-contract=off where results are pinned bit for bit: these kernels reproduce float->int truncations
# of the reference (see input_prep.hip's header) or round step by step like their CPU twins -- and so does every host half ...
HIP_NO_CONTRACT=" input_prep raster data_prep pil_resize fid_stats grad_guard ema d_augment feature_metrics swd region_metrics gan_loss region_loss style_loss "
# ... except these three
HOST_CONTRACT=" jpeg_host png_host png_decode_host "

stale() {   # $1 = object
  local d=_build/$(basename "$1" .o).d f
  [ -f "$1" ] && [ -f "$d" ] && [ ! "$SELF" -nt "$1" ] || return 0
  for f in $(sed -e 's/^[^:]*://' -e 's/\\$//' "$d"); do
    [ -e "$f" ] && [ ! "$f" -nt "$1" ] || return 0
  done
  return 1
}

objs=(); cmds=()
for src in *.hip *_host.cpp; do
  n=${src%.*}; o=_build/$n.o
  objs+=("$o")
  stale "$o" || continue
  if [ "$src" = "$n.hip" ]; then
    extra=""; [[ "$HIP_NO_CONTRACT" == *" $n "* ]] && extra="-ffp-contract=off"
    flags="$HIP_FLAGS $extra"
  else
    extra="-ffp-contract=off"; [[ "$HOST_CONTRACT" == *" $n "* ]] && extra=""
    flags="$HOST_FLAGS $extra -I../../include -I."
  fi
  # (the .d comes from a preprocessing pass of its own, which takes a fraction of a second: hipcc derives the compile unit's id, a
  # part of its symbol names, from the command line, so -MD on the compile itself would change every object that holds a kernel)
  cmds+=("$HIPCC $flags -M -MT $o -MF _build/$n.d $src && $HIPCC $flags -c $src -o $o")
  echo "compile $src"
done
if [ ${#cmds[@]} -gt 0 ]; then
  printf '%s\n' "${cmds[@]}" | xargs -P "$JOBS" -I{} sh -c '{}'
fi
$HIPCC --offload-arch=gfx950 -shared -fPIC -o _build/libhoig_hip.so $(printf '%s\n' "${objs[@]}" | LC_ALL=C sort)
echo built _build/libhoig_hip.so
