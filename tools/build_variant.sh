#!/bin/bash
# Builds variants/libtd_<name>.so: csrc/<file>.hip recompiled with extra flags, the other objects
# taken from the regular build (run `python -c "import __graft_entry__ as g; g.build()"` first).
#   tools/build_variant.sh <name> <file.hip> [flags...]      select it with TD_HOTPATH_LIB
# The way to A/B an edited source against the regular build in one GPU session.
set -eu
name=$1; src=$2; shift 2
root=$(cd "$(dirname "$0")/.." && pwd)
obj=$root/telluride_decoding_amd/csrc/_obj
mkdir -p $root/variants
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -fno-slp-vectorize -Wno-unused-result \
  -I$root/include -I$root/telluride_decoding_amd/csrc "$@" -c $root/telluride_decoding_amd/csrc/$src \
  -o $root/variants/$name.$src.o 2> $root/variants/$name.log
others=$(ls $obj/*.o | grep -v "/$src.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $root/variants/libtd_$name.so $root/variants/$name.$src.o $others
echo built variants/libtd_$name.so
